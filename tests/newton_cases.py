"""The cases of the Newton-step tests (test_newton_host.py on the oracle, test_gpu_newton.py on the HIP engine) and
the bookkeeping both share: which iterations of which solves are dumped, and how a dump is put into the dense system
of tests/newton.py.  A `backend` is a function

    run(prob, N, k, after_refine, idx) -> (records (n, DUMP_W), trace (n, k + 1, 16), restoration entries or None)

that solves the samples `idx` of `prob` with horizon N and max_iter = k + 1 (the solve stops after iteration k) with
the dump of iteration k and the trace armed.

Every helper takes an optional `prm` (kkt.Problem); None is the reference's problem, as before.  `prob` carries the
set it was made for under "prm" (absent: the reference's), so a backend reads the parameters from the problem it is
handed.
"""
from __future__ import annotations

import numpy as np

import kkt
import newton

DT = 0.1
SAMPLES = (0, 1, 2, 3)
HORIZONS = (50, 1, 2, 3, 7)
SENTINEL = -777.25        # fill of the dump buffers: entries the solver does not write keep it


def _prm(prm):
    return kkt.DEFAULT if prm is None else prm


def oracle_params(prm=None, **kw):
    """The oracle's parameter block for the set `prm` (None: the defaults) with the solver fields `kw`."""
    from oracle import oracle as O
    return O.default_params(**{**({} if prm is None else prm.fields()), **kw})


def problem(batch, N, prm=None, t_scale=1.0, samples=SAMPLES):
    """Samples 0..3 of scenario.synthetic_batch(64, seed=2025): at N = 50 with t_scale times their own t (1 for the
    reference's 5 s horizon), at the short horizons with t = 0.5 N dt (the traversal weight inside the horizon);
    u_last = 1 on the odd samples, 0 (none) on the even."""
    from oracle import oracle as O
    i = np.array(samples)
    dt = DT if prm is None else prm.dt
    d = batch["dnn_out"][i].astype(np.float64)
    ul = np.zeros((len(i), 4))
    ul[i % 2 == 1] = 1.0
    t = d[:, 6] * t_scale if N == 50 else np.full(len(i), 0.5 * N * dt)
    return {"prm": prm, "ini": batch["ini"][i], "goal": batch["goal"][i], "p": d[:, :3], "a": d[:, 3:6],
            "q": np.stack([O.rd2quat(a) for a in d[:, 3:6]]), "t": t, "ulast": ul}


def oracle_run(prob, N, k, after_refine, idx, fast=False):
    """The oracle's strict build, or with fast=True its -O3 / FMA build (the rounding yardstick's other side)."""
    from oracle import oracle as O
    idx = np.asarray(idx)
    rec = np.full((len(idx), newton.DUMP_W), SENTINEL)
    tr = np.zeros((len(idx), k + 1, 16))
    O.debug_dump(rec, k, after_refine, fast=fast)
    O.debug_trace(tr, k + 1, fast=fast)
    try:
        O.solve(prob["ini"][idx], prob["goal"][idx], prob["p"][idx], prob["q"][idx], prob["t"][idx],
                ulast=prob["ulast"][idx], params=oracle_params(prob.get("prm"), horizon=N, max_iter=k + 1), fast=fast)
    finally:
        O.debug_dump(None, fast=fast)
        O.debug_trace(None, 0, fast=fast)
    return rec, tr, None


def oracle_run_fma(prob, N, k, after_refine, idx):
    return oracle_run(prob, N, k, after_refine, idx, fast=True)


def oracle_full(prob, N):
    from oracle import oracle as O
    return O.solve(prob["ini"], prob["goal"], prob["p"], prob["q"], prob["t"], ulast=prob["ulast"],
                   params=oracle_params(prob.get("prm"), horizon=N))


def dump_iterations(N, iters):
    """Iterations dumped of a solve that took `iters` iterations: 0, 1, 3, 8 and the late iterate iters - 2 (small
    mu, large Sigma) at N = 50; 0, 1, 3 at the short horizons; each clipped below iters - 1."""
    ks = (0, 1, 3, 8, iters - 2) if N == 50 else (0, 1, 3)
    return sorted({max(0, min(k, iters - 2)) for k in ks})


def collect(run, prob, N, iters):
    """Every case of horizon N through backend `run`: one launch per (k, side) on the samples that dump k.
    Returns {(sample, k): case}, case = dict(pre, post: the steps; point; pad: the padding entries of both records;
    trace (k + 1, 16); resto: restoration entries of the two launches (None for the oracle))."""
    per_sample = [dump_iterations(N, int(it)) for it in iters]
    cases = {}
    for k in sorted({k for ks in per_sample for k in ks}):
        idx = [s for s, ks in enumerate(per_sample) if k in ks]
        side = {}
        for ar in (0, 1):
            rec, tr, resto = run(prob, N, k, ar, idx)
            side[ar] = (rec, tr, resto)
        for j, s in enumerate(idx):
            pre, pt0, pad0 = newton.split_record(side[0][0][j], N)
            post, pt1, pad1 = newton.split_record(side[1][0][j], N)
            for f in pt0:   # the iterate does not change between the two dump points
                assert np.array_equal(pt0[f], pt1[f]), (N, s, k, f)
            assert np.array_equal(side[0][1][j, :k], side[1][1][j, :k]), (N, s, k, "trace of the two launches")
            cases[(s, k)] = {"pre": pre, "post": post, "point": pt0, "pad": np.concatenate([pad0, pad1]),
                             "trace": side[1][1][j], "resto": [side[0][2], side[1][2]]}
    return cases


def collect_pairs(run, prob, N, cases, launch=4):
    """Iterations k and k + 1 of every (sample, k) of `cases` through backend `run`, refined steps: per k, launches of
    at most `launch` samples with max_iter k + 1 and k + 2.  Returns {(sample, k): dict(step, point: iteration k;
    next_step, next_point: iteration k + 1; pad: the padding entries of both records; first (k + 1, 16), trace
    (k + 2, 16): the traces of the two launches)}."""
    out = {}
    for k in sorted({k for _, k in cases}):
        idx = sorted(s for s, kk in cases if kk == k)
        for o in range(0, len(idx), launch):
            part = idx[o:o + launch]
            rec0, tr0, _ = run(prob, N, k, 1, part)
            rec1, tr1, _ = run(prob, N, k + 1, 1, part)
            for j, s in enumerate(part):
                step, point, pad0 = newton.split_record(rec0[j], N)
                nstep, npoint, pad1 = newton.split_record(rec1[j], N)
                out[(s, k)] = {"step": step, "point": point, "next_step": nstep, "next_point": npoint,
                               "pad": np.concatenate([pad0, pad1]), "first": tr0[j], "trace": tr1[j]}
    return out


_systems = {}


def system(tag, prob, N, s, k, case):
    """The dense Newton system at a case's dumped point (cached per backend tag: both sides and the inertia check
    share it)."""
    key = (tag, N, s, k)
    if key not in _systems:
        ul = prob["ulast"][s] if np.any(prob["ulast"][s]) else None
        _systems[key] = newton.NewtonSystem(case["point"], case["trace"][k, 0], prob["ini"][s], prob["goal"][s],
                                            prob["p"][s], prob["q"][s], prob["t"][s], ul, N, _prm(prob.get("prm")))
    return _systems[key]


def ratios(tag, prob, N, cases):
    """{(sample, k): (unrefined, refined)} residual ratios of the dumped steps in the dense system of their own point,
    with the delta_w of the trace."""
    out = {}
    for (s, k), c in cases.items():
        ns = system(tag, prob, N, s, k, c)
        dw = c["trace"][k, 8]
        out[(s, k)] = (ns.residual_ratio(c["pre"], dw), ns.residual_ratio(c["post"], dw))
    return out


def inertia(tag, prob, N, cases):
    """Checks the inertia verdict of every case against the eigenvalues of the dense K.  Returns (cases, left out):
    a delta_w == 0 case whose K(0) has smallest |eig| / largest |eig| below 1e-10 and an eigenvalue count other than
    13 N is left out (the sign of a numerically zero eigenvalue is not defined); every other miss is an assertion.
    Where delta_w > 0 came from a retry, the retry before it must have been rejected rightly (same singularity rule)."""
    left = 0
    for (s, k), c in cases.items():
        ns = system(tag, prob, N, s, k, c)
        dw = c["trace"][k, 8]
        n0, cond0 = ns.neg_eigs(0.0)
        if dw == 0.0:
            if n0 != ns.m:
                assert cond0 < 1e-10, (tag, N, s, k, "delta_w = 0 but K(0) has", n0, "negative eigenvalues, not", ns.m)
                left += 1
        else:
            assert n0 != ns.m, (tag, N, s, k, "delta_w =", dw, "but K(0) already has the right inertia")
            nd, _ = ns.neg_eigs(dw)
            assert nd == ns.m, (tag, N, s, k, "K(delta_w) has", nd, "negative eigenvalues, not", ns.m)
            # the retry before the accepted one was rejected rightly: IPOPT's sequence starts at 1e-4 and grows by
            # 100 while no iteration has been regularised yet, else at a third of the last delta_w, growing by 8
            prev = [d for d in c["trace"][:k, 8] if d > 0.0]
            first, grow = (1e-4, 100.0) if not prev else (max(1e-20, prev[-1] / 3.0), 8.0)
            if dw > first * (1.0 + 1e-12):
                npv, cpv = ns.neg_eigs(dw / grow)
                assert npv != ns.m or cpv < 1e-10, (tag, N, s, k, "delta_w =", dw, "but K(delta_w /", grow,
                                                    ") already has the right inertia")
    return len(cases), left


def structure(prob, N, cases):
    """dx of stage 0 exactly 0, the padding beyond N untouched, iteration 0 dumped at the stated initial point."""
    for (s, k), c in cases.items():
        for side in ("pre", "post"):
            assert np.all(c[side]["dx"][0] == 0.0), (N, s, k, side, "dx at stage 0")
            for f in c[side]:
                assert np.all(np.isfinite(c[side][f])) and not np.any(c[side][f] == SENTINEL), (N, s, k, side, f)
        assert np.all(c["pad"] == SENTINEL), (N, s, k, "padding beyond the horizon written")
        if k == 0:
            p0 = newton.initial_point(prob["ini"][s], N, _prm(prob.get("prm")))
            for f in p0:
                if f != "lam":   # lam of iteration 0 is the least-squares initialisation
                    assert np.array_equal(c["point"][f], p0[f]), (N, s, k, f)


def lam_deviation(lam, dense):
    return float(np.max(np.abs(lam - dense)) / (1.0 + np.max(np.abs(dense))))
