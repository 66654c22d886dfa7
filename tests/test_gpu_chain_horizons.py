"""The Newton step of the HIP kernel at the horizons around the unroll depths of the two sequential chains
(riccati.inc forward_chain, backward_chain), in the dense system of tests/newton.py exactly as test_gpu_newton.py
checks it at N = 50, 1, 2, 3, 7: same samples, same dumped iterations, same bounds.

Both chains run PF coefficient slots in a straight-line body of PF steps followed by up to PF - 1 remainder steps,
with the fetches PF - 1 stages ahead of the steps (past the horizon's end in forward_chain, below stage 0 in
backward_chain) and one counted wait per step whose count depends on the step's place in the body.  The horizons are
the ones at which that structure changes shape:

    forward_chain, PF = 6:   4, 5 remainder only; 6 exactly one body; 11 a body and the longest remainder; 12 two bodies
    backward_chain, PF = 4:  4 exactly one body; 5, 6 a body and a remainder; 8 two bodies; 11 two bodies and the longest
                             remainder; 12 three bodies  (3: remainder only and 7: a body and the longest remainder are
                             test_gpu_newton.py's)

The step is dumped before and after the refinement: the unrefined step runs forward_chain on the factorisation's
record, the refined one runs backward_chain and forward_chain on the refinement right-hand sides.  `ipm_kernel_dump`
instantiates the same linear_solve as the production kernel (see test_gpu_newton.py).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import newton  # noqa: E402
import newton_cases as NC  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0                       # test_gpu_newton.py's
HORIZONS = (4, 5, 6, 8, 11, 12)
_cache = {}
_engines = {}


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def engine(N):
    if N not in _engines:
        from learningagileflight_se3_amd.engine import Engine
        _engines[N] = Engine(horizon=N)
    return _engines[N]


def gpu_run(prob, N, k, after_refine, idx):
    e = engine(N)
    idx = np.asarray(idx)
    rec = torch.full((len(idx), newton.DUMP_W), NC.SENTINEL, dtype=torch.float64, device=e.device)
    tr = torch.zeros((len(idx), k + 1, 16), dtype=torch.float64, device=e.device)
    p = e.params
    saved = p.max_iter
    p.max_iter = k + 1
    e.set_params(p)
    e.debug_dump(rec, k, bool(after_refine))
    e.debug_trace(tr, k + 1)
    try:
        e.ocp_solve(prob["ini"][idx], prob["goal"][idx], prob["p"][idx], prob["a"][idx], prob["t"][idx],
                    u_last=prob["ulast"][idx])
        torch.cuda.synchronize()
        resto = e.last_resto_counters()["resto_entries"]
    finally:
        e.debug_dump(None)
        e.debug_trace(None)
        p.max_iter = saved
        e.set_params(p)
    return rec.cpu().numpy(), tr.cpu().numpy(), resto


def horizon(batch, N):
    """(problem, oracle cases, GPU cases) of horizon N; the dumped iterations come from the oracle's full solve."""
    if N not in _cache:
        prob = NC.problem(batch, N)
        iters = NC.oracle_full(prob, N)["iters"]
        _cache[N] = (prob, NC.collect(NC.oracle_run, prob, N, iters), NC.collect(gpu_run, prob, N, iters))
    return _cache[N]


@pytest.mark.parametrize("N", HORIZONS)
def test_step_solves_the_dense_system(batch, N):
    """The refined step has a residual ratio <= 1e-5 in every case, and the largest ratio of the refined and of the
    unrefined steps is at most MARGIN times the oracle's on the same cases."""
    prob, ocases, gcases = horizon(batch, N)
    assert set(ocases) == set(gcases)
    for (s, k), c in gcases.items():
        assert c["resto"] == [0, 0], (N, s, k, "restoration phase entered")
        assert np.all(c["trace"][:k + 1, 0] > 0.0), (N, s, k)
    g = NC.ratios("gpu-chain", prob, N, gcases)
    o = NC.ratios("oracle-chain", prob, N, ocases)
    gpre, gpost = max(v[0] for v in g.values()), max(v[1] for v in g.values())
    opre, opost = max(v[0] for v in o.values()), max(v[1] for v in o.values())
    print(f"N={N}: {len(g)} cases, largest residual ratio unrefined GPU {gpre:.3e} oracle {opre:.3e}, "
          f"refined GPU {gpost:.3e} oracle {opost:.3e}")
    assert all(v[1] <= 1e-5 for v in g.values()), g           # IPOPT's residual_ratio_singular
    assert gpost <= MARGIN * opost, (gpost, opost)
    assert gpre <= MARGIN * opre, (gpre, opre)


@pytest.mark.parametrize("N", HORIZONS)
def test_dump_structure(batch, N):
    """dx of stage 0 exactly 0, every entry up to N written and finite, the padding beyond N untouched."""
    prob, _, gcases = horizon(batch, N)
    NC.structure(prob, N, gcases)
