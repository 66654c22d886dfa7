"""The factorisation sweep's per-lane tables in LDS (riccati_mfma.inc init_mf_tables, Smem::mfo / Smem::mfp).

Run on an MI355X:  python -m pytest tests/test_gpu_sweep_tables.py -m gpu -q -s

Every solver kernel writes the tables once per workgroup, ahead of its instance loop, and every factorisation sweep of
every instance that the workgroup then takes from the queue reads them back.  They must therefore (a) survive whatever
an instance does to the LDS, (b) be there again in the next launch, whose LDS starts out undefined, and (c) be the same
offsets the sweep used to compute from the lane index, at every horizon.

 1. Workgroup reuse.  ocp_solve of B = 2 slots + 256 instances (slots = 4 x CUs: every workgroup takes at least two
    instances, some three) at N = 3 and N = 7 against the same instances solved in launches of at most `slots`
    instances, where each workgroup's only instance follows the table set-up directly: x, u, lam, cost, status and
    iters of every instance equal bit for bit.  Inputs: scenario.synthetic_batch(B, seed=47), t = 0.5 N dt, u_last = 1
    on the odd instances (newton_cases.problem's convention); at least 99 % of the instances must solve, so that the
    comparison is one of full solves.
 2. Horizons.  The dumped Newton step solves the dense system of tests/newton.py at N = 1, 2, 3, 7 and 50 under the
    bounds of test_gpu_chain_horizons.py (newton_gpu.py's helpers, the same samples); N = 1 and 2 take the peeled stage
    0 alone or after one pass of the stage loop.
 3. Both gradient kernels.  sol_gradient on 8 samples (synthetic_batch(8, seed=7)), FD and grad_mode = 1, twice on one
    context: out8, rewards9 and status9 of the second launch equal the first's bit for bit, and every solve converged.

The tables share no storage with another phase (the restoration phase's scratch is hv / hh / cc, untouched), so
there is no rebuild to test after a restoration entry.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import newton_cases as NC  # noqa: E402
from newton_gpu import horizon, step_solves_the_dense_system  # noqa: E402

pytestmark = pytest.mark.gpu

OUT = ("x", "u", "lam", "cost", "status", "iters")


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def _bits(a):
    return a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a


@pytest.mark.parametrize("N", (3, 7))
def test_workgroup_reuse(N):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(horizon=N)
    slots = 4 * torch.cuda.get_device_properties(e.device).multi_processor_count
    B = 2 * slots + 256
    sb = S.synthetic_batch(B, seed=47)
    d = sb["dnn_out"].astype(np.float64)
    ul = np.zeros((B, 4))
    ul[1::2] = 1.0
    args = (sb["ini"], sb["goal"], d[:, :3], d[:, 3:6], np.full(B, 0.5 * N * NC.DT))

    def solve(lo, hi):
        out = e.ocp_solve(*(a[lo:hi] for a in args), u_last=ul[lo:hi])
        torch.cuda.synchronize()
        return out

    big = solve(0, B)
    parts = [solve(lo, min(lo + slots, B)) for lo in range(0, B, slots)]
    assert len(parts) == 3 and all(len(p["status"]) <= slots for p in parts)
    solved = float((big["status"] <= 1).double().mean())
    print(f"N={N}: slots {slots}, B {B}, solved {solved:.4f}, iterations {int(big['iters'].sum())}")
    assert solved >= 0.99
    for k in OUT:
        small = torch.cat([p[k] for p in parts])
        assert small.shape == big[k].shape and small.dtype == big[k].dtype, k
        diff = _bits(small) != _bits(big[k])
        assert not bool(diff.any()), (N, k, int(diff.reshape(B, -1).any(dim=1).sum()), "instances differ")
    e.check_device()


@pytest.mark.parametrize("N", (1, 2, 3, 7, 50))
def test_horizons(batch, N):
    prob, ocases, gcases = horizon(batch, N)
    assert set(ocases) == set(gcases)
    step_solves_the_dense_system(f"N={N}", "-chain", prob, N, ocases, gcases)
    NC.structure(prob, N, gcases)


@pytest.mark.parametrize("grad_mode", (0, 1))
def test_gradient_kernels_launch_twice(grad_mode):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.engine import Engine
    sb = S.synthetic_batch(8, seed=7)
    e = Engine()
    runs = []
    for _ in range(2):
        runs.append(e.sol_gradient(sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"], want_rewards=True,
                                   grad_mode=grad_mode))
        torch.cuda.synchronize()
    (o1, r1, s1), (o2, r2, s2) = runs
    assert bool(torch.isfinite(o1).all()) and bool((s1 <= 1).all()), (o1, s1)
    assert torch.equal(_bits(o1), _bits(o2))
    assert torch.equal(_bits(r1), _bits(r2))
    assert torch.equal(s1, s2)
