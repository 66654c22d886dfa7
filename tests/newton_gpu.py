"""What the device tests of the Newton step and of the solver options share (test_gpu_newton.py,
test_gpu_chain_horizons.py, test_gpu_pass_folds.py, test_gpu_refine_steps.py, test_gpu_options.py): the engines, the
device backend of newton_cases.py, the bound on the residual ratios against the oracle's, and the oracle's traced solve
with the decision words of a trace."""
import numpy as np
import torch

import newton
import newton_cases as NC
from learningagileflight_se3_amd.engine import Engine, _param_override

MARGIN = 10.0      # GPU against oracle, largest residual ratio over the cases: a different summation order (MFMA
                   # k-steps, FMA contraction, the rsq-based pivot) shifts rounding by small factors; a wrong matrix
                   # entry leaves the ratio orders of magnitude higher
_engines = {}
_horizons = {}


def engine(N, fields=None):
    """One Engine per (horizon, parameter fields); ``fields``: a dict of Params fields, None or empty for the defaults."""
    key = (N, tuple(sorted((fields or {}).items())))
    if key not in _engines:
        _engines[key] = Engine(horizon=N, **dict(key[1]))
    return _engines[key]


def _engine_of(prob, N):
    prm = prob.get("prm")
    return engine(N, None if prm is None else prm.fields())


def _solve(e, prob, idx):
    out = e.ocp_solve(prob["ini"][idx], prob["goal"][idx], prob["p"][idx], prob["a"][idx], prob["t"][idx],
                      u_last=prob["ulast"][idx])
    torch.cuda.synchronize()
    return out


def gpu_solve(prob, N, idx, max_iter):
    """The samples idx of prob solved with at most max_iter iterations -> ocp_solve's outputs as numpy arrays."""
    e = _engine_of(prob, N)
    with _param_override(e, "max_iter", max_iter):
        out = _solve(e, prob, idx)
    return {k: v.cpu().numpy() for k, v in out.items()}


def gpu_run(prob, N, k, after_refine, idx):
    """newton_cases backend: the samples idx solved up to iteration k with the dump of iteration k and the trace armed."""
    e = _engine_of(prob, N)
    idx = np.asarray(idx)
    rec = torch.full((len(idx), newton.DUMP_W), NC.SENTINEL, dtype=torch.float64, device=e.device)
    tr = torch.zeros((len(idx), k + 1, 16), dtype=torch.float64, device=e.device)
    with _param_override(e, "max_iter", k + 1):
        e.debug_dump(rec, k, bool(after_refine))
        e.debug_trace(tr, k + 1)
        try:
            _solve(e, prob, idx)
            resto = e.last_resto_counters()["resto_entries"]
        finally:
            e.debug_dump(None)
            e.debug_trace(None)
    return rec.cpu().numpy(), tr.cpu().numpy(), resto


def horizon(batch, N):
    """(problem, oracle cases, GPU cases) of horizon N; the dumped iterations come from the oracle's full solve."""
    if N not in _horizons:
        prob = NC.problem(batch, N)
        iters = NC.oracle_full(prob, N)["iters"]
        _horizons[N] = (prob, NC.collect(NC.oracle_run, prob, N, iters), NC.collect(gpu_run, prob, N, iters))
    return _horizons[N]


def step_solves_the_dense_system(head, tag, prob, N, ocases, gcases):
    """No case in a restoration phase; the refined step has a residual ratio <= 1e-5 in every case, and the largest
    ratio of the refined and of the unrefined steps is at most MARGIN times the oracle's on the same cases.  ``head``
    starts the printed line, ``tag`` names the dense systems of the two sides in newton_cases' cache."""
    for (s, k), c in gcases.items():
        assert c["resto"] == [0, 0], (N, s, k, "restoration phase entered")
        assert np.all(c["trace"][:k + 1, 0] > 0.0), (N, s, k)
    g = NC.ratios("gpu" + tag, prob, N, gcases)
    o = NC.ratios("oracle" + tag, prob, N, ocases)
    gpre, gpost = max(v[0] for v in g.values()), max(v[1] for v in g.values())
    opre, opost = max(v[0] for v in o.values()), max(v[1] for v in o.values())
    print(f"{head}: {len(g)} cases, largest residual ratio unrefined GPU {gpre:.3e} oracle {opre:.3e}, "
          f"refined GPU {gpost:.3e} oracle {opost:.3e}")
    assert all(v[1] <= 1e-5 for v in g.values()), g           # IPOPT's residual_ratio_singular
    assert gpost <= MARGIN * opost, (gpost, opost)
    assert gpre <= MARGIN * opre, (gpre, opre)


def oracle_traced(prob, params, TI=None):
    """(solve, trace (B, TI, 16)) of the oracle's strict build; TI defaults to the longest solve + 1."""
    from oracle import oracle as O
    args = tuple(prob[k] for k in ("ini", "goal", "p", "q", "t"))
    r = O.solve(*args, params=params)
    TI = int(r["iters"].max()) + 1 if TI is None else TI
    buf = np.zeros((len(r["iters"]), TI, 16))
    O.debug_trace(buf, TI)
    try:
        O.solve(*args, params=params)
    finally:
        O.debug_trace(None, 0)
    return r, buf


def decisions(tr):
    """The decision words of a trace: mu, delta_w, accepted, filter size, number of step halvings."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(tr[:, :, 7] > 0, np.round(np.log2(tr[:, :, 5] / tr[:, :, 7])), -1.0)
    return np.concatenate([tr[:, :, [0, 8, 9, 10]], h[:, :, None]], axis=2)
