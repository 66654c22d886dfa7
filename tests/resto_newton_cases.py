"""The cases of the restoration-phase tests (test_resto_newton_host.py on the oracle, test_gpu_resto_newton.py and
the exits of test_gpu_resto.py on the HIP engine) and the bookkeeping they share, as newton_cases.py is for the main
phase.

The instance family: ini_state = 0 except z = 1, quaternion entry [6] = 1 and the body rate omega_0; goal (5, 0, 1),
p_tra (2.5, 0, 1.2), traversal attitude the identity, t = 0.05 N, no u_last.

  yaw     omega_0 = (0, 0, wz), wz in {4.8, 8, 25}: the yaw torque is too weak to bring the rate of stage 1 into its
          box, and the solve ends with status 9 at N = 50, 7, 3, 2, 1 (threshold between wz = 4.54, solved without
          restoration, and 4.56; swept 4.30 .. 4.90 in steps of 0.02 at N = 7, 3, 2, 1 and 1.6 .. 12 in steps of 0.4 at
          all five horizons).  Every one of these solves enters the phase two or three times (up to six at the generic
          parameter set): the first entries return to the original problem after one or two iterations (status 0 of
          the phase: the successful-return path, at every horizon), the last one converges to the infeasible point.
          ENTRIES records, per horizon and wz, (IPM iterations before the entry, restoration iterations of the entry)
          of every entry, measured with the oracle; test_resto_newton_host.py holds the oracle to it.
          With max_iter = 10, wz = 25 ends with status 2 after 10 iterations, inside its second entry (N = 50, N = 2).
  roll / pitch (N = 50)  omega_0 = (7.2, 0, 0), (7.6, 0, 0), (0, 8.0, 0): solved with status 0 after 81, 98 and 90
          iterations.  The oracle does NOT enter the restoration phase on them (nor at any of 6.0 .. 9.4 in steps of
          0.2 on either axis, nor with watchdog = 0, max_soc = 0 or lsq_mult_init = 0): their long tails are soft
          restoration and watchdog iterations of the main phase.  They are kept as solves that must agree with the
          oracle and pass the KKT certificate with entries == returns; the returns that are dumped and counted are
          the yaw family's.

  regularised  N = 50, wz = 11.2 (set name "reg"): the only inertia corrections the sweeps above met lie in the last
          entries of the N = 50 solves with wz = 10.6, 11.2, 11.8: here entry 1 (of 2), iterations 5 (delta_w 1e-2, after
          the rejected 1e-4), 6 (3.3e-3) and 8 (1.1e-3).  Dumped: iterations 0, 5 and 6 of that entry.

Dumped otherwise: entry 0 (iterations 0, 1, 3 clipped below the entry's count, which leaves iteration 0 and once iteration 1) and
the last entry (iterations 0, 1, 3: the barrier parameter has moved, lam is not the least-squares value any more).

A `backend` is a function

    run(prob, N, entry, k, after_refine, idx, max_iter) -> (records (n, resto_newton.DUMP_W), counters or None, outputs)

that solves the samples `idx` of `prob` with horizon N and the given max_iter (None: the default) with the dump of
restoration iteration k of the entry-th entry armed.
"""
from __future__ import annotations

import numpy as np

import newton_cases as NC
import resto_newton as RN

HORIZONS = (50, 7, 3, 2, 1)
GENERIC_HORIZONS = (50, 3)
YAW = (4.8, 8.0, 25.0)
ROLL_PITCH = ((7.2, 0.0, 0.0), (7.6, 0.0, 0.0), (0.0, 8.0, 0.0))   # N = 50: status 0, no restoration entry (oracle)
# (IPM iterations before the entry, restoration iterations of the entry) of every entry, per (set, N) and wz (oracle)
ENTRIES = {
    ("default", 50): (((7, 1), (9, 1), (11, 7)), ((5, 1), (7, 2), (11, 7)), ((4, 2), (7, 8))),
    ("default", 7): (((11, 1), (13, 1), (15, 16)), ((7, 1), (10, 11)), ((5, 1), (7, 9))),
    ("default", 3): (((6, 1), (8, 1), (10, 6)), ((4, 1), (6, 7)), ((4, 1), (6, 7))),
    ("default", 2): (((6, 1), (8, 3), (12, 5)), ((4, 1), (6, 7)), ((4, 1), (6, 7))),
    ("default", 1): (((6, 1), (8, 6)), ((6, 1), (8, 6)), ((5, 1), (7, 6))),
    ("generic", 50): (((8, 1), (11, 1), (14, 1), (16, 1), (19, 2), (22, 8)), ((6, 1), (9, 1), (11, 1), (14, 7)),
                      ((5, 1), (7, 1), (10, 1), (12, 7))),
    ("generic", 3): (((5, 1), (7, 1), (9, 8)), ((4, 1), (6, 8)), ((4, 1), (6, 9))),
    ("reg", 50): (((5, 1), (7, 9)),),
}
REG_WZ, REG_DUMPS = (11.2,), (((1, 0), (1, 5), (1, 6)),)
FAMILIES = [("default", N) for N in HORIZONS] + [("generic", N) for N in GENERIC_HORIZONS] + [("reg", 50)]
DUMP_KS = (0, 1, 3)
SENTINEL = NC.SENTINEL
MAXITER_WZ, MAXITER = 25.0, 10   # the iteration limit inside the phase


def problem(N, omegas, prm=None):
    """The family's instances with the given body rates, in the layout of newton_cases.problem."""
    w = np.asarray(omegas, dtype=np.float64).reshape(-1, 3)
    B = len(w)
    ini = np.zeros((B, 13))
    ini[:, 2] = 1.0
    ini[:, 6] = 1.0
    ini[:, 10:13] = w
    return {"prm": prm, "ini": ini, "goal": np.tile([5.0, 0.0, 1.0], (B, 1)), "p": np.tile([2.5, 0.0, 1.2], (B, 1)),
            "a": np.zeros((B, 3)), "q": np.tile([1.0, 0.0, 0.0, 0.0], (B, 1)), "t": np.full(B, 0.05 * N),
            "ulast": np.zeros((B, 4))}


def yaw(N, prm=None, wz=YAW):
    return problem(N, [(0.0, 0.0, w) for w in wz], prm)


def family(pset, N):
    """(problem, per-sample (entry, iteration) pairs to dump) of a member of FAMILIES."""
    if pset == "reg":
        return yaw(N, None, REG_WZ), REG_DUMPS
    import generic_params as GP
    return yaw(N, GP.SETS[pset][0]), tuple(dumped(en) for en in ENTRIES[(pset, N)])


def oracle_run(prob, N, entry, k, after_refine, idx, max_iter=None):
    from oracle import oracle as O
    idx = np.asarray(idx)
    rec = np.full((len(idx), RN.DUMP_W), SENTINEL)
    kw = {} if max_iter is None else {"max_iter": int(max_iter)}
    O.debug_dump_resto(rec, entry, k, after_refine)
    try:
        out = O.solve(prob["ini"][idx], prob["goal"][idx], prob["p"][idx], prob["q"][idx], prob["t"][idx],
                      params=NC.oracle_params(prob.get("prm"), horizon=N, **kw))
    finally:
        O.debug_dump_resto(None)
    return rec, None, out


_engines = {}


def engine(N, prm=None):
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    if (N, prm) not in _engines:
        from learningagileflight_se3_amd.engine import Engine
        _engines[(N, prm)] = Engine(horizon=N, **({} if prm is None else prm.fields()))
    return _engines[(N, prm)]


def gpu_run(prob, N, entry, k, after_refine, idx, max_iter=None):
    """The backend of the HIP engine (lafse3_ocp_solve with lafse3_debug_dump_resto armed)."""
    import torch
    e = engine(N, prob["prm"])
    idx = np.asarray(idx)
    rec = torch.full((len(idx), RN.DUMP_W), SENTINEL, dtype=torch.float64, device=e.device)
    p = e.params
    saved = p.max_iter
    if max_iter is not None:
        p.max_iter = int(max_iter)
        e.set_params(p)
    e.debug_dump_resto(rec, entry, k, bool(after_refine))
    try:
        out = e.ocp_solve(prob["ini"][idx], prob["goal"][idx], prob["p"][idx], prob["a"][idx], prob["t"][idx])
        torch.cuda.synchronize()
        cnt = e.last_resto_counters()
    finally:
        e.debug_dump_resto(None)
        p.max_iter = saved
        e.set_params(p)
    return rec.cpu().numpy(), cnt, {f: v.cpu().numpy() for f, v in out.items()}


def probe_entries(run, prob, N):
    """Every entry of every sample through backend `run`, by arming one (entry, iteration) after the other on the
    uncut solve: per sample a tuple of (IPM iterations before the entry, restoration iterations of the entry)."""
    B = len(prob["ini"])
    res = [[] for _ in range(B)]
    for e in range(16):
        cnt, k = np.zeros(B, int), 0
        while True:
            rec = run(prob, N, e, k, 0, np.arange(B), None)[0]
            parts = [RN.split_record(r, N) for r in rec]
            w = np.array([p[3]["written"] == 1.0 for p in parts])
            if not w.any():
                break
            cnt, k = cnt + w, k + 1
        entered = [p[4]["iters_before"] != SENTINEL for p in parts]
        if not any(entered):
            break
        for b in range(B):
            if entered[b]:
                res[b].append((int(parts[b][4]["iters_before"]), int(cnt[b])))
    return tuple(tuple(r) for r in res)


def dumped(entries):
    """The (entry, iteration) pairs dumped of a sample with the given entries: DUMP_KS, clipped below the entry's
    iteration count, of entry 0 and of the last entry."""
    return sorted({(e, min(k, entries[e][1] - 1)) for e in {0, len(entries) - 1} for k in DUMP_KS})


def collect(run, prob, N, entries, per_sample):
    """Every case of a problem through backend `run` (per_sample: the (entry, iteration) pairs dumped of each sample,
    as `family` gives them): one launch per (entry, iteration, side) on the samples that dump it, with max_iter just past the dumped iteration of the sample that gets there last.  Returns
    {(sample, entry, k): case}, case = dict(pre, post: the steps; point; ref; scal: the scalars; lsq; pad: the padding
    of both records)."""
    cases = {}
    for e, k in sorted({ek for eks in per_sample for ek in eks}):
        idx = [s for s, eks in enumerate(per_sample) if (e, k) in eks]
        max_iter = max(entries[s][e][0] for s in idx) + k + 1
        side = [run(prob, N, e, k, ar, idx, max_iter)[0] for ar in (0, 1)]
        for j, s in enumerate(idx):
            pre, pt0, rf0, sc0, lq0, pad0 = RN.split_record(side[0][j], N)
            post, pt1, rf1, sc1, lq1, pad1 = RN.split_record(side[1][j], N)
            assert sc0["written"] == 1.0 and sc1["written"] == 1.0, (N, s, e, k, "the iteration was not dumped")
            for a, b in ((pt0, pt1), (rf0, rf1), (lq0, lq1)):   # nothing but the step differs between the two
                for f in a:
                    assert np.array_equal(a[f], b[f]), (N, s, e, k, f)
            for f in ("mu", "eta", "delta_w", "ratio_pre", "ratio_post"):
                assert sc0[f] == sc1[f], (N, s, e, k, f, sc0[f], sc1[f])
            assert lq0["iters_before"] == entries[s][e][0], (N, s, e, k, lq0["iters_before"], entries[s][e])
            cases[(s, e, k)] = {"pre": pre, "post": post, "point": pt0, "ref": rf0, "scal": sc1, "lsq": lq0,
                                "pad": np.concatenate([pad0, pad1])}
    return cases


_systems = {}


def system(tag, prob, N, s, k, case):
    """The dense restoration system at a case's dumped point, k = (entry, iteration) (cached per backend tag)."""
    key = (tag, N, s) + tuple(k)
    if key not in _systems:
        _systems[key] = RN.RestoSystem(case["point"], case["ref"], case["scal"]["mu"], case["scal"]["eta"],
                                       prob["ini"][s], N, NC._prm(prob.get("prm")))
    return _systems[key]


def ratios(tag, prob, N, cases):
    """{(sample, k): (unrefined, refined)} residual ratios of the dumped steps in the dense system of their own
    point, with the dumped delta_w."""
    out = {}
    for (s, e, k), c in cases.items():
        rs = system(tag, prob, N, s, (e, k), c)
        dw = c["scal"]["delta_w"]
        out[(s, e, k)] = (rs.residual_ratio(c["pre"], dw), rs.residual_ratio(c["post"], dw))
    return out


def inertia(tag, prob, N, cases):
    """The inertia verdict of every case against the eigenvalues of the dense system: delta_w == 0 needs 13 N negative
    eigenvalues at 0, delta_w > 0 needs them at delta_w and not at 0.  A case whose matrix at 0 is numerically
    singular (smallest |eig| / largest |eig| below 1e-10) and misses is left out.  Returns (cases, left out)."""
    left = 0
    for (s, e, k), c in cases.items():
        rs = system(tag, prob, N, s, (e, k), c)
        dw = c["scal"]["delta_w"]
        n0, cond0 = rs.neg_eigs(0.0)
        if dw == 0.0:
            if n0 != rs.m:
                assert cond0 < 1e-10, (tag, N, s, k, "delta_w = 0 but K(0) has", n0, "negative eigenvalues, not", rs.m)
                left += 1
        else:
            if n0 == rs.m:
                assert cond0 < 1e-10, (tag, N, s, k, "delta_w =", dw, "but K(0) already has the right inertia")
                left += 1
            assert rs.neg_eigs(dw)[0] == rs.m, (tag, N, s, k, "K(delta_w) has the wrong inertia")
            # the smallest delta_w IPOPT's sequence tries is 1e-4 (first correction) or a third of the last one: a
            # larger one means a retry was rejected, rightly if K at the retry before it has the wrong inertia
            for grow in (100.0, 8.0):
                if abs(dw / grow - 1e-4) <= 1e-16:
                    npv, cpv = rs.neg_eigs(dw / grow)
                    assert npv != rs.m or cpv < 1e-10, (tag, N, s, k, "K(1e-4) already has the right inertia")
    return len(cases), left


def start_point_terms(tag, prob, N, s, ek, case):
    """(c, mu_R) at a case of iteration 0: the defects of the start point from the dense module and the barrier
    parameter the phase started with, read off z_p p."""
    rs = system(tag, prob, N, s, ek, case)
    return rs.c.reshape(N, 13), float(np.median(case["point"]["zp"] * case["point"]["p"]))


def structure(tag, prob, N, cases):
    """dx of stage 0 exactly 0; no entry inside the horizon left unwritten, none beyond it written; p, n and their
    duals positive.  At iteration 0: v_R is the dumped x and u, z_p p = z_n n = mu_R >= max|c| with the dumped mu not
    above it, p and n are RestoIterateInitializer's closed form for the start point's defects c,
        n = a + sqrt(a^2 + mu_R c / (2 rho)),  a = (mu_R - rho c) / (2 rho),  p = c + n,
    and lam is the least-squares value, or 0 where that exceeds 1e3."""
    for (s, e, k), c in cases.items():
        for side in ("pre", "post"):
            assert np.all(c[side]["dx"][0] == 0.0), (N, s, k, side, "dx at stage 0")
            for f in c[side]:
                assert np.all(np.isfinite(c[side][f])) and not np.any(c[side][f] == SENTINEL), (N, s, k, side, f)
        for grp in ("point", "ref"):
            for f in c[grp]:
                assert np.all(np.isfinite(c[grp][f])) and not np.any(c[grp][f] == SENTINEL), (N, s, k, f)
        assert np.all(c["pad"] == SENTINEL), (N, s, k, "padding beyond the horizon written")
        P = c["point"]
        for f in ("p", "n", "zp", "zn"):
            assert np.all(P[f] > 0.0), (N, s, k, f)
        assert np.array_equal(c["ref"]["xR"][0], prob["ini"][s]) and np.array_equal(P["x"][0], prob["ini"][s])
        assert c["lsq"]["lsq_ok"] == 1.0 and np.all(np.isfinite(c["lsq"]["lsq_lamp"])), (N, s, k)
        if k != 0:
            continue
        assert np.array_equal(c["ref"]["xR"], P["x"]) and np.array_equal(c["ref"]["uR"], P["u"]), (N, s, "v_R")
        cc, mu_r = start_point_terms(tag, prob, N, s, (e, k), c)
        for z, v in (("zp", "p"), ("zn", "n")):
            assert np.all(np.abs(P[z] * P[v] - mu_r) <= 1e-12 * mu_r), (N, s, z)
        cmax = float(np.max(np.abs(cc)))
        assert mu_r >= cmax * (1.0 - 1e-12) and c["scal"]["mu"] <= mu_r * (1.0 + 1e-12), (N, s, mu_r, cmax)
        assert c["scal"]["eta"] == np.sqrt(c["scal"]["mu"]), (N, s)
        a = (mu_r - RN.RHO * cc) / (2.0 * RN.RHO)
        n = a + np.sqrt(a * a + mu_r * cc / (2.0 * RN.RHO))
        # c carries the rounding of f_d (1e-16 of the state's scale); a and the root cancel where c > 0
        tol = 1e-9 * np.maximum(np.abs(n), 1e-6)
        assert np.all(np.abs(P["n"] - n) <= tol), (N, s, "n", float(np.max(np.abs(P["n"] - n) / tol)))
        assert np.all(np.abs(P["p"] - (cc + n)) <= 1e-9 * np.maximum(np.abs(cc + n), 1e-6)), (N, s, "p")
        lq = c["lsq"]["lsq_lamp"]
        cut = lq if np.max(np.abs(lq)) <= 1e3 else np.zeros_like(lq)
        assert np.array_equal(P["lam"], cut), (N, s, "lam of iteration 0 is not the cut least-squares value")


def lsq_deviation(tag, prob, N, cases):
    """Largest deviation (newton_cases.lam_deviation) of the dumped least-squares multipliers from the dense value,
    over the iteration-0 cases."""
    devs = []
    for (s, e, k), c in cases.items():
        if k == 0:
            devs.append(NC.lam_deviation(c["lsq"]["lsq_lamp"], system(tag, prob, N, s, (e, k), c).lsq_multipliers()))
    return max(devs)


def honoured(point, prm=None):
    """(x, u) of a dumped point as the solver returns it: the bounded entries projected onto the original, unrelaxed
    boxes (IPOPT's honor_original_bounds: an iterate may sit up to 1e-8 outside them)."""
    prm = NC._prm(prm)
    x, u = point["x"].copy(), np.clip(point["u"], prm.u_lb, prm.u_ub)
    x[1:, 10:13] = np.clip(x[1:, 10:13], prm.w_lb, prm.w_ub)
    return x, u
