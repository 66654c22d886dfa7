"""GPU tests of the warm start: lafse3_ocp_solve_warm (csrc/warm.inc, ipm_kernel_warm), Engine.ocp_solve_warm with its
cold retry, and moving_gate.run_episodes_device(..., warm=True).

Run on an MI355X:  python -m pytest tests/test_gpu_warm.py -m gpu -q -s

Inputs: tests/sens_w_cases.py's batch under the weight rows D and G as tests/test_gpu_vjp.py: horizon 50 (samples
0..15) and 20, 2, 1 (samples 0..7, that module's case_t; at horizon 1 the non-zero u_last of test_gpu_vjp.py): per
horizon one launch of 2 n instances, samples 0..n-1 under row D, then the same under row G.  The records come from one
cold ocp_solve_rec launch per horizon, solved once and never modified.

(1) The loaded iterate.  With max_iter = 0 the solve writes its initial iterate to rec_out, which is compared with a
numpy restatement of include/lafse3.h's rules (`expected_load`): shifts 0, 1, N-1, N, N+3, zero pushes and the
defaults.  Copied and pushed entries bit for bit; lam and the bound duals to 2^-51 relative (one product of two
correctly rounded factors: the ratio s_new / s_rec may be formed either side of the multiplication); stage-0 omega
duals 0; mu = opts.mu_init; x and u outputs = the record's blocks; s_new within 1e-10 relative of min(1, 100 / gmax),
gmax from autograd on tests/kkt.py's objective at the loaded point.
(2) Same problem from its own record, default opts, no retry: warm status <= 1 wherever the cold status is; the KKT
certificate of tests/kkt.py (primal <= 5e-7, dual <= 1e-4 s_d, compl <= 1e-6, no bound violation) on every such
solve; summed warm iterations <= half the cold sum at horizons 50 and 20; ocp_vjp on the warm rec_out: sens_status 0.
(3) Receding-horizon successor P1 of P0's cold optimum (ini_state = x*_1, u_last = u*_0, t - dt, same goal, p, a),
warm-started from P0's record with shift = 1: the same certificate and the same cap against P1's own cold solve.  No
equality with the cold optimum is asked: the NLP is nonconvex; the test prints how many instances agree with the cold
cost to 1e-6 relative.
(4) Fallbacks: records made unusable four ways (status word 2, horizon word of another horizon, a NaN in lam, s = 0)
among good ones in one launch: warm_status 1 and every output ocp_solve_rec's bit for bit; the good rows equal a
launch of the good rows alone.  Refusals are LAFSE3_EINVAL before a launch.  At the C boundary rec_out may be rec_in
(the records are overwritten with what a separate rec_out receives) or NULL.
(5) Retry: under a small max_iter some warm starts end with status 2 (both outcomes are asserted to occur); with
retry=True those rows are warm_status 2 and ocp_solve_rec's bit for bit, the others untouched; with retry=False they
keep status 2.
(6) Past one instance per wave (tests/test_gpu_sens_queue.py's scheme): B = 2 slots + 256 at horizon 20, every 7th
record unusable, so warm and cold starts alternate on a wave.  The launch repeated is bit-identical, a 64-row subset
alone equals its rows, >= 99 % of the rows end with status <= 1 (the cold launch that makes the records first),
check_device() passes.
(7) The moving-gate loop on tests/golden/moving.npz's two episodes x 120 plant steps, warm=False and warm=True: summed
IPM iterations of the control steps warm < cold; every warm-loop solve with status <= 1 passes the certificate on its
captured inputs; no more status > 1 solves than the cold loop; warm=False equals a call without the argument.

First GPU run (256 CUs; all 18 tests passed; IPM iterations summed over the instances whose cold solve converged):
    (1) largest relative |s_new - min(1, 100 / gmax)|: 1.1e-14 (horizon 50), 1.2e-14 (20), 1.4e-15 (2), 0 (1); every
        bit-for-bit and 2^-51 comparison held at every shift and both push settings.
    (2) horizon 50 (32 instances): cold 2012, warm 288 (5 .. 17 per instance); horizon 20 (16): 1428 -> 170 (8 .. 13);
        horizons 2 and 1 (16 each): 96 -> 48 (3 each).  Warm status 0 on all 80; all end at the cold cost to 1e-6.
    (3) successor: horizon 50 1876 -> 340, 28 of 32 agree with the cold cost and 4 differ (3 of them lower); horizon 20
        1261 -> 191, 14 of 16 agree, 2 differ (1 lower); horizon 2 96 -> 64, horizon 1 80 -> 64, all agree.
    (5) max_iter 12 (chosen from (2)'s counts at horizon 50: three instances need 13, 14 and 17): 3 of 32 warm starts
        end with status 2, 29 with status 0.
    (6) slots 1024, B 2304, 330 unusable records: status <= 1 on 100 % of the cold and of the warm launch; the 1974
        warm-started rows take 19752 iterations against 167551 cold.
    (7) 24 solves per loop: cold 1015 iterations, warm 661 (112 of them the cold first control step); status > 1 on
        none in either loop; warm_status 0 on all 22 warm calls; the final states differ by 2.7e-6.
    Certificates, largest over all checked solves: primal 2.0e-7 (the final clamp of a control at its relaxed
    bound, 2.4e-8, times dt l / (2 J) = 7.6; the cold solves show the same), dual / s_d 2.8e-5 (loop), compl 9.6e-7
    (horizon 20, both sets), bound violation 0.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import kkt
import sens_w_cases as C

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NSAMPLES = {50: 16, 20: 8, 2: 8, 1: 8}
REC_X, REC_U, REC_LAM, REC_ZLU, REC_ZUU, REC_ZLW, REC_ZUW = 0, 663, 863, 1513, 1713, 1913, 2066
REC_MU, REC_S, REC_STATUS, REC_N, REC_W = 2219, 2220, 2221, 2222, 2223
MAXN = 50
KKT_BARS = {"primal": 5e-7, "dual": 1e-4, "compl": 1e-6}   # dual relative to s_d (tests/kkt.py dual_scale)
RETRY_MAX_ITER = 12   # (5): between the fastest and the slowest warm solve of (2) at horizon 50 (FIRST_RUN)


def _np(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def sb():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    return C.batch()


_CASES = {}


def _problem(row):
    return dataclasses.replace(kkt.DEFAULT, **dict(zip(C.WEIGHT_NAMES, map(float, row))))


def _case(sb, horizon):
    """The instances of one horizon and their cold solve (never modified)."""
    if horizon not in _CASES:
        from learningagileflight_se3_amd.engine import Engine
        from oracle import oracle as O
        n = NSAMPLES[horizon]
        idx = np.concatenate([np.arange(n), np.arange(n)])
        t = C.case_t(sb, horizon)
        ul = np.tile([0.4, 0.9, 0.2, 1.3], (2 * n, 1)) if horizon == 1 else np.zeros((2 * n, 4))
        W = np.concatenate([np.tile(C.ROW_D, (n, 1)), np.tile(C.ROW_G, (n, 1))])
        args = tuple(v[idx].copy() for v in (sb["ini"], sb["goal"], sb["p"], sb["a"], t)) + (ul, W)
        eng = Engine(horizon=horizon)
        cold = eng.ocp_solve_rec(*args[:6], weights=W)
        torch.cuda.synchronize()
        _CASES[horizon] = {"eng": eng, "args": args, "cold": cold, "coldn": _np(cold), "B": 2 * n, "N": horizon,
                           "q": np.stack([O.rd2quat(a) for a in args[3]]),
                           "prm": [_problem(C.ROW_D)] * n + [_problem(C.ROW_G)] * n}
    return _CASES[horizon]


def _certificate(label, sol, args, q, prm, rows):
    """The suite's KKT certificate on the solves `rows` of `sol` against the inputs args (ini, goal, p, a, t, u_last).
    Prints the largest figures; returns the rows that miss a bar."""
    worst, bad = {"primal": 0.0, "dual": 0.0, "compl": 0.0, "bound_viol": 0.0}, []
    for i in rows:
        r = kkt.kkt_residual(sol["x"][i], sol["u"][i], sol["lam"][i], args[0][i], args[1][i], args[2][i], q[i],
                             args[4][i], args[5][i], prm[i])
        fig = {"primal": r["primal"], "dual": r["dual"] / r["s_d"], "compl": r["compl"]}
        if any(fig[k] > KKT_BARS[k] for k in fig) or r["bound_viol"] > 0.0:
            bad.append((int(i), r))
        worst = {k: max(worst[k], dict(fig, bound_viol=r["bound_viol"])[k]) for k in worst}
    print(f"{label}: certificate on {len(rows)} solves, largest primal {worst['primal']:.2e}, dual / s_d "
          f"{worst['dual']:.2e}, compl {worst['compl']:.2e}, bound violation {worst['bound_viol']:.1e}; "
          f"{len(bad)} miss a bar")
    return bad


# ---- (1) the loaded iterate -----------------------------------------------------------------------------------------

def expected_load(rec, ini, N, shift, o, prm):
    """include/lafse3.h's rules for a usable record, restated: the loaded x (B, N+1, 13), u (B, N, 4), and the record's
    lam and bound duals remapped (before the rescaling), as arrays."""
    B = rec.shape[0]
    relax = 1e-8

    def box(lb, ub):
        return lb - relax * max(1.0, abs(lb)), ub + relax * max(1.0, abs(ub))

    def push(v, lo, hi):
        pl = min(o.bound_push * max(1.0, abs(lo)), o.bound_frac * (hi - lo))
        pu = min(o.bound_push * max(1.0, abs(hi)), o.bound_frac * (hi - lo))
        return np.minimum(np.maximum(v, lo + pl), hi - pu)

    blk = lambda off, rows, w: rec[:, off:off + rows * w].reshape(B, rows, w)   # noqa: E731
    kx = np.minimum(np.arange(1, N + 1) + shift, N)
    ku = np.minimum(np.arange(N) + shift, N - 1)
    x = np.zeros((B, N + 1, 13))
    x[:, 0] = ini
    x[:, 1:] = blk(REC_X, MAXN + 1, 13)[:, kx]
    x[:, 1:, 10:13] = push(x[:, 1:, 10:13], *box(prm.w_lb, prm.w_ub))
    u = push(blk(REC_U, MAXN, 4)[:, ku], *box(prm.u_lb, prm.u_ub))
    zlw, zuw = np.zeros((B, N + 1, 3)), np.zeros((B, N + 1, 3))
    zlw[:, 1:] = blk(REC_ZLW, MAXN + 1, 3)[:, kx]
    zuw[:, 1:] = blk(REC_ZUW, MAXN + 1, 3)[:, kx]
    return {"x": x, "u": u, "lam": blk(REC_LAM, MAXN, 13)[:, ku], "zlu": blk(REC_ZLU, MAXN, 4)[:, ku],
            "zuu": blk(REC_ZUU, MAXN, 4)[:, ku], "zlw": zlw, "zuw": zuw, "copied": x[:, :, :10]}


def _gmax(x, u, args, q, prm, i):
    """max |dJ/dx_k| (k >= 1), |dJ/du| of tests/kkt.py's objective at (x, u), by autograd."""
    f64 = torch.float64
    X = torch.tensor(x, dtype=f64, requires_grad=True)
    U = torch.tensor(u, dtype=f64, requires_grad=True)
    tens = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=f64) for a in (args[0][i], args[1][i], args[2][i], q[i])]
    J, _ = kkt.objective_and_defects(X, U, tens[0], tens[1], tens[2], tens[3], torch.tensor(float(args[4][i]), dtype=f64),
                                     torch.tensor(args[5][i], dtype=f64), prm)
    gX, gU = torch.autograd.grad(J, [X, U])
    return max(float(gX[1:].abs().max()), float(gU.abs().max()))


@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_loaded_iterate_equals_the_restated_rules(sb, horizon):
    from learningagileflight_se3_amd import _lib
    from learningagileflight_se3_amd.engine import Engine
    c = _case(sb, horizon)
    N, B, args = c["N"], c["B"], c["args"]
    rec = c["coldn"]["rec"]
    assert np.all(c["coldn"]["status"] <= 1)
    eng0 = Engine(horizon=N, max_iter=0)
    rel = 2.0 ** -51
    worst_s = 0.0
    for shift in sorted({0, 1, max(N - 1, 0), N, N + 3}):
        for pushes in (0.0, 1e-3):
            o = _lib.default_warm_opts(bound_push=pushes, bound_frac=pushes, mult_bound_push=pushes, mu_init=3e-3)
            out = _np(eng0.ocp_solve_warm(*args[:6], weights=args[6], rec=c["cold"]["rec"], shift=shift, mu_init=3e-3,
                                          opts=o, retry=False))
            tag = f"horizon {N}, shift {shift}, pushes {pushes}"
            assert np.all(out["warm_status"] == 0), tag
            assert np.all(out["iters"] == 0) and np.all(out["status"] <= 2), tag
            ro = out["rec"]
            exp = expected_load(rec, args[0], N, shift, o, kkt.DEFAULT)
            got = lambda off, rows, w: ro[:, off:off + rows * w].reshape(B, -1, w)[:, :rows]   # noqa: E731
            # copied and pushed entries, and the outputs against the record's blocks
            assert _same(got(REC_X, N + 1, 13), exp["x"]), tag
            assert _same(got(REC_U, N, 4), exp["u"]), tag
            assert _same(out["x"], exp["x"]) and _same(out["u"], exp["u"]), tag
            if pushes == 0.0:   # nothing to push: the record's own clamped values
                assert _same(exp["u"], rec[:, REC_U:REC_U + MAXN * 4].reshape(B, MAXN, 4)[:, np.minimum(
                    np.arange(N) + shift, N - 1)]), tag
            # scalars
            assert np.all(ro[:, REC_MU] == 3e-3) and np.all(ro[:, REC_N] == N), tag
            assert np.array_equal(ro[:, REC_STATUS], out["status"].astype(np.float64)), tag
            s_new = ro[:, REC_S]
            for i in range(B):
                g = _gmax(exp["x"][i], exp["u"][i], args, c["q"], c["prm"][i], i)
                s_ref = min(1.0, 100.0 / g)
                worst_s = max(worst_s, abs(s_new[i] - s_ref) / s_ref)
            # rescaled multipliers
            r = (s_new / rec[:, REC_S])[:, None, None]
            pairs = [("lam", got(REC_LAM, N, 13), exp["lam"] * r),
                     ("zLu", got(REC_ZLU, N, 4), np.maximum(exp["zlu"] * r, pushes)),
                     ("zUu", got(REC_ZUU, N, 4), np.maximum(exp["zuu"] * r, pushes)),
                     ("zLw", got(REC_ZLW, N + 1, 3), np.maximum(exp["zlw"] * r, pushes)),
                     ("zUw", got(REC_ZUW, N + 1, 3), np.maximum(exp["zuw"] * r, pushes))]
            for name, a, b in pairs:
                if name in ("zLw", "zUw"):
                    assert np.all(a[:, 0] == 0.0), (tag, name)
                    a, b = a[:, 1:], b[:, 1:]
                assert np.all(np.abs(a - b) <= rel * np.abs(b)), (tag, name, float(np.abs(a - b).max()))
            # the lam output is lam / s
            assert np.all(np.abs(out["lam"] - got(REC_LAM, N, 13) / s_new[:, None, None])
                          <= rel * np.abs(out["lam"])), tag
    print(f"horizon {N}: largest relative |s_new - min(1, 100 / gmax)| {worst_s:.3e}")
    assert worst_s <= 1e-10


# ---- (2) the same problem from its own record -----------------------------------------------------------------------

def _warm_same(c):
    if "warm" not in c:
        c["warm"] = c["eng"].ocp_solve_warm(*c["args"][:6], weights=c["args"][6], rec=c["cold"]["rec"], retry=False)
        torch.cuda.synchronize()
        c["warmn"] = _np(c["warm"])
    return c["warmn"]


@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_same_problem_from_its_own_record(sb, horizon):
    c = _case(sb, horizon)
    cold, warm = c["coldn"], _warm_same(c)
    ok = cold["status"] <= 1
    print(f"horizon {horizon}: cold status {np.bincount(cold['status'], minlength=3).tolist()}, warm status "
          f"{np.bincount(warm['status'], minlength=3).tolist()}; iterations cold {int(cold['iters'][ok].sum())} warm "
          f"{int(warm['iters'][ok].sum())}; warm per instance {warm['iters'].tolist()}")
    same = np.abs(warm["cost"] - cold["cost"]) <= 1e-6 * np.abs(cold["cost"])
    print(f"horizon {horizon}: {int(same[ok].sum())} of {int(ok.sum())} instances end at the cold cost to 1e-6 "
          f"relative, {int((~same)[ok].sum())} elsewhere")
    assert np.all(warm["warm_status"] == 0)
    assert ok.sum() >= 0.9 * c["B"]                      # the comparison has a subject
    assert np.all(warm["status"][ok] <= 1), np.flatnonzero(ok & (warm["status"] > 1))
    bad = _certificate(f"horizon {horizon}, same problem", warm, c["args"], c["q"], c["prm"], np.flatnonzero(ok))
    assert not bad, bad
    if horizon in (50, 20):
        assert 2 * warm["iters"][ok].sum() <= cold["iters"][ok].sum()
    # the warm solve's record is a valid input of ocp_vjp
    rng = np.random.default_rng(7)
    v = _np(c["eng"].ocp_vjp(*c["args"], c["warm"]["rec"], rng.standard_normal((c["B"], horizon + 1, 13)),
                             rng.standard_normal((c["B"], horizon, 4))))
    assert np.all(v["sens_status"][ok] == 0), v["sens_status"]
    assert np.all(np.isfinite(v["grad"])) and np.all(np.abs(v["grad"][ok]).max(1) > 0)


# ---- (3) the receding-horizon successor -----------------------------------------------------------------------------

def _successor(c):
    """P1 of P0's cold optimum, P1's own cold solve and its warm start from P0's record with shift = 1."""
    if "succ" not in c:
        a, cold = c["args"], c["coldn"]
        args1 = (cold["x"][:, 1].copy(), a[1], a[2], a[3], a[4] - kkt.DT, cold["u"][:, 0].copy(), a[6])
        cold1 = c["eng"].ocp_solve_rec(*args1[:6], weights=args1[6])
        warm1 = c["eng"].ocp_solve_warm(*args1[:6], weights=args1[6], rec=c["cold"]["rec"], shift=1, retry=False)
        torch.cuda.synchronize()
        c["succ"] = (args1, _np(cold1), _np(warm1))
    return c["succ"]


@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_receding_horizon_successor(sb, horizon):
    c = _case(sb, horizon)
    args1, cold1, warm1 = _successor(c)
    ok = (c["coldn"]["status"] <= 1) & (cold1["status"] <= 1)
    same = np.abs(warm1["cost"] - cold1["cost"]) <= 1e-6 * np.abs(cold1["cost"])
    print(f"horizon {horizon}, successor: cold status {np.bincount(cold1['status'], minlength=3).tolist()}, warm "
          f"status {np.bincount(warm1['status'], minlength=3).tolist()}; iterations cold "
          f"{int(cold1['iters'][ok].sum())} warm {int(warm1['iters'][ok].sum())}; {int(same[ok].sum())} of "
          f"{int(ok.sum())} instances agree with the cold cost to 1e-6 relative, {int((~same)[ok].sum())} differ "
          f"(lower cost on {int(((warm1['cost'] < cold1['cost']) & ~same & ok).sum())})")
    assert np.all(warm1["warm_status"] == 0)
    assert ok.sum() >= 0.9 * c["B"]
    assert np.all(warm1["status"][ok] <= 1), np.flatnonzero(ok & (warm1["status"] > 1))
    bad = _certificate(f"horizon {horizon}, successor", warm1, args1, c["q"], c["prm"], np.flatnonzero(ok))
    assert not bad, bad
    if horizon in (50, 20):
        assert 2 * warm1["iters"][ok].sum() <= cold1["iters"][ok].sum()


# ---- (4) fallbacks --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20])
def test_unusable_records_start_cold_and_leave_their_neighbours_alone(sb, horizon):
    c = _case(sb, horizon)
    N, B, args = c["N"], c["B"], c["args"]
    rec = c["cold"]["rec"].clone()
    rec[1, REC_STATUS] = 2.0
    rec[3, REC_N] = 20.0 if N == 50 else 50.0
    rec[5, REC_LAM + (N - 1) * 13 + 2] = float("nan")
    rec[6, REC_S] = 0.0
    badrows = np.array([1, 3, 5, 6])
    good = np.setdiff1d(np.arange(B), badrows)
    keep = rec.clone()
    mixed = _np(c["eng"].ocp_solve_warm(*args[:6], weights=args[6], rec=rec, retry=False))
    assert torch.equal(rec.view(torch.int64), keep.view(torch.int64))          # rec_in is read only
    expect = np.zeros(B, dtype=np.int32)
    expect[badrows] = 1
    assert np.array_equal(mixed["warm_status"], expect)
    for k in ("x", "u", "lam", "cost", "status", "iters", "rec"):
        assert _same(mixed[k][badrows], c["coldn"][k][badrows]), k
    alone = _np(c["eng"].ocp_solve_warm(*(v[good] for v in args[:6]), weights=args[6][good],
                                        rec=c["cold"]["rec"][torch.as_tensor(good, device=rec.device)], retry=False))
    for k in ("x", "u", "lam", "cost", "status", "iters", "rec", "warm_status"):
        assert _same(mixed[k][good], alone[k]), k
    # a shift moves the entries read: the NaN at stage N-1 of lam is read at every shift (the tail repeats it), one at
    # stage 0 of u only at shift 0
    rec2 = c["cold"]["rec"].clone()
    rec2[2, REC_U + 1] = float("inf")
    for shift, ws in ((0, 1), (1, 0 if N > 1 else 1)):
        w = _np(c["eng"].ocp_solve_warm(*args[:6], weights=args[6], rec=rec2, shift=shift, retry=False))
        assert w["warm_status"][2] == ws and np.all(np.delete(w["warm_status"], 2) == 0), (shift, w["warm_status"])
    c["eng"].check_device()


def test_rec_out_may_alias_rec_in_or_be_null(sb):
    """At the C boundary: rec_out == rec_in overwrites the records with what a separate rec_out receives (each
    instance reads its record before it writes), and rec_out == NULL changes no other output."""
    c = _case(sb, 20)
    eng, args, B, N = c["eng"], c["args"], c["B"], c["N"]
    d = eng.device
    inp = [torch.as_tensor(np.ascontiguousarray(v), device=d) for v in args]
    p = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())   # noqa: E731
    base = c["cold"]["rec"].clone()
    base[4, REC_STATUS] = 2.0            # one cold start among them

    def call(rec_in, rec_out):
        o = {"x": torch.empty(B, N + 1, 13, dtype=torch.float64, device=d),
             "u": torch.empty(B, N, 4, dtype=torch.float64, device=d),
             "lam": torch.empty(B, N, 13, dtype=torch.float64, device=d),
             "cost": torch.empty(B, dtype=torch.float64, device=d),
             "status": torch.empty(B, dtype=torch.int32, device=d), "iters": torch.empty(B, dtype=torch.int32, device=d),
             "warm_status": torch.empty(B, dtype=torch.int32, device=d)}
        rc = eng._L.lafse3_ocp_solve_warm(eng._ctx, B, *(p(v) for v in inp), p(rec_in), None, p(o["x"]), p(o["u"]),
                                          p(o["lam"]), p(o["cost"]), p(o["status"]), p(o["iters"]),
                                          p(o["warm_status"]), p(rec_out), eng._stream())
        assert rc == 0, eng._L.lafse3_last_error()
        torch.cuda.synchronize()
        return _np(o)

    separate = torch.zeros_like(base)
    ref = call(base.clone(), separate)
    aliased = base.clone()
    ali = call(aliased, aliased)
    none = call(base.clone(), None)
    for k in ref:
        assert _same(ref[k], ali[k]) and _same(ref[k], none[k]), k
    assert ref["warm_status"][4] == 1 and ref["warm_status"].sum() == 1
    assert torch.equal(aliased.view(torch.int64), separate.view(torch.int64))
    assert not torch.equal(aliased, base)


def test_refusals_come_before_any_launch(sb):
    from learningagileflight_se3_amd import _lib
    c = _case(sb, 20)
    eng, args = c["eng"], c["args"]
    eng.ocp_solve_rec(*(v[:2] for v in args[:6]))     # a launch of two instances: what the counters must keep showing
    before = eng.last_counters()
    kw = dict(weights=args[6], rec=c["cold"]["rec"], retry=False)
    for opt in (dict(shift=-1), dict(shift=-(2 ** 31)), dict(bound_push=-1e-3), dict(bound_frac=-1.0),
                dict(mult_bound_push=-1e-9), dict(mu_init=float("nan")), dict(bound_push=float("inf")),
                dict(mult_bound_push=float("nan"))):
        o = _lib.default_warm_opts(**{k: v for k, v in opt.items() if k not in ("shift", "mu_init")})
        with pytest.raises(_lib.Lafse3Error, match="rc=-1"):
            eng.ocp_solve_warm(*args[:6], shift=opt.get("shift", 0), mu_init=opt.get("mu_init"), opts=o, **kw)
    with pytest.raises(ValueError, match="rec"):
        eng.ocp_solve_warm(*args[:6], weights=args[6], rec=None)
    with pytest.raises(ValueError, match="rec"):
        eng.ocp_solve_warm(*args[:6], weights=args[6], rec=c["cold"]["rec"][:3])
    # NULL rec_in at the C boundary, with every other pointer valid
    d = eng.device
    t = [torch.as_tensor(v, device=d).contiguous() for v in args[:5]]
    st = torch.empty(c["B"], dtype=torch.int32, device=d)
    p = lambda v: ctypes.c_void_p(v.data_ptr())   # noqa: E731
    rc = eng._L.lafse3_ocp_solve_warm(eng._ctx, c["B"], *(p(v) for v in t), None, None, None, None, None, None, None,
                                      None, p(st), None, None, None, None)
    assert rc == -1 and b"rec_in" in eng._L.lafse3_last_error()
    assert eng.last_counters() == before          # none of the refused calls was a solver launch
    # mu_init <= 0 is no refusal: it stands for the context's mu_init
    w = _np(eng.ocp_solve_warm(*args[:6], mu_init=0.0, **kw))
    assert np.all(w["warm_status"] == 0) and eng.last_counters() != before


# ---- (5) retry ------------------------------------------------------------------------------------------------------

def test_failed_warm_starts_are_solved_again_cold(sb):
    from learningagileflight_se3_amd.engine import Engine
    c = _case(sb, 50)
    args, B = c["args"], c["B"]
    eng = Engine(horizon=50, max_iter=RETRY_MAX_ITER)
    kw = dict(weights=args[6], rec=c["cold"]["rec"])
    plain = _np(eng.ocp_solve_warm(*args[:6], retry=False, **kw))
    failed = plain["status"] > 1
    print(f"max_iter {RETRY_MAX_ITER}: {int(failed.sum())} of {B} warm starts end with status > 1 "
          f"({np.bincount(plain['status'], minlength=3).tolist()})")
    assert failed.any() and (~failed).any()
    assert np.all(plain["status"][failed] == 2) and np.all(plain["warm_status"] == 0)
    launches = []
    retried = _np(eng.ocp_solve_warm(*args[:6], retry=True, counters=launches, **kw))
    assert len(launches) == 2
    assert np.array_equal(retried["warm_status"], np.where(failed, 2, 0).astype(np.int32))
    coldn = _np(eng.ocp_solve_rec(*args[:6], weights=args[6]))
    for k in ("x", "u", "lam", "cost", "status", "iters", "rec"):
        assert _same(retried[k][failed], coldn[k][failed]), k
        assert _same(retried[k][~failed], plain[k][~failed]), k
    # nothing failed: no second launch
    easy = np.flatnonzero(~failed)
    launches = []
    one = _np(eng.ocp_solve_warm(*(v[easy] for v in args[:6]), weights=args[6][easy],
                                 rec=c["cold"]["rec"][torch.as_tensor(easy, device=eng.device)], retry=True,
                                 counters=launches))
    assert len(launches) == 1 and np.all(one["warm_status"] == 0)
    eng.check_device()


# ---- (6) past one instance per wave ---------------------------------------------------------------------------------

def test_warm_launch_does_not_depend_on_batch_position_or_size():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.engine import Engine
    eng = Engine(horizon=20)
    dev = eng.device
    slots = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    B = 2 * slots + 256
    sb = S.synthetic_batch(B, seed=31)
    b = np.arange(B)
    t = np.clip(0.5 * sb["dnn_out"][:, 6].astype(np.float64), 0.3, 1.5)
    W = np.where((b % 2 == 0)[:, None], C.ROW_D, C.ROW_G)
    dt = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)   # noqa: E731
    args = [dt(sb["ini"]), dt(sb["goal"]), dt(sb["dnn_out"][:, :3].astype(np.float64)),
            dt(sb["dnn_out"][:, 3:6].astype(np.float64)), dt(t)]
    Wt = dt(W)
    cold = eng.ocp_solve_rec(*args, weights=Wt)
    cold_ok = float((cold["status"] <= 1).double().mean())
    print(f"slots {slots}, B {B}: cold status <= 1 on {100 * cold_ok:.2f} %, iterations {int(cold['iters'].sum())}")
    assert cold_ok >= 0.99
    rec = cold["rec"].clone()
    unusable = torch.as_tensor(b % 7 == 0, device=dev)
    rec[unusable, REC_STATUS] = 2.0

    def launch(sel):
        if sel is None:
            return eng.ocp_solve_warm(*args, weights=Wt, rec=rec, retry=False)
        return eng.ocp_solve_warm(*(v[sel] for v in args), weights=Wt[sel], rec=rec[sel], retry=False)

    def tbits(a):
        return a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a

    big, again = launch(None), launch(None)
    for k in big:
        assert torch.equal(tbits(big[k]), tbits(again[k])), ("the launch repeated", k)
    del again
    idx = set(np.random.default_rng(8).choice(B, 64, replace=False).tolist())
    idx = torch.as_tensor(sorted(idx), device=dev)
    sub = launch(idx)
    for k in big:
        assert torch.equal(tbits(big[k][idx]), tbits(sub[k])), ("the subset alone against its rows", k)
    assert torch.equal(big["warm_status"], unusable.to(torch.int32))
    # an unusable record's row is the cold launch's, wherever it ran
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert torch.equal(tbits(big[k][unusable]), tbits(cold[k][unusable])), k
    warm_ok = float((big["status"] <= 1).double().mean())
    started = ~unusable
    print(f"warm status <= 1 on {100 * warm_ok:.2f} % ({100 * float((big['status'][started] <= 1).double().mean()):.2f} "
          f"% of the warm-started rows); iterations of the warm-started rows: cold {int(cold['iters'][started].sum())} "
          f"warm {int(big['iters'][started].sum())}; status histogram {torch.bincount(big['status']).tolist()}")
    assert warm_ok >= 0.99
    eng.check_device()


# ---- (7) the moving-gate loop ---------------------------------------------------------------------------------------

def test_moving_gate_loop_warm(golden):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import moving_gate as MG
    from learningagileflight_se3_amd.engine import Engine
    from oracle import oracle as O
    from moving_cases import dnn2_from_fixture, fixture_episodes
    g = golden("moving")
    n_ep, steps = g["t"].shape
    assert (n_ep, steps) == (2, 120)
    samples, noise = fixture_episodes(g)
    net = dnn2_from_fixture(golden("dnn2_nn3_1")).cuda()
    eng = Engine()
    plain = MG.run_episodes_device(eng, net, samples, noise, steps=steps)
    cc, wc, cap = [], [], []
    cold = MG.run_episodes_device(eng, net, samples, noise, steps=steps, counters=cc, warm=False)
    warm = MG.run_episodes_device(eng, net, samples, noise, steps=steps, counters=wc, capture=cap, warm=True)
    for k in ("states", "t", "status"):
        assert torch.equal(plain[k], cold[k]), k
    assert plain["solves"] == cold["solves"] == warm["solves"] == n_ep * (steps // MG.CTRL_EVERY)
    assert len(cc) == len(wc) == len(cap) == steps // MG.CTRL_EVERY
    it_cold, it_warm = sum(r["iterations"] for r in cc), sum(r["iterations"] for r in wc)
    bad_cold, bad_warm = int((cold["status"] > 1).sum()), int((warm["status"] > 1).sum())
    ws = torch.stack([e["warm_status"] for e in cap[1:]], 1).cpu().numpy()
    print(f"moving-gate loop, {n_ep} episodes x {steps} plant steps: IPM iterations cold {it_cold} warm {it_warm} "
          f"(first control step {wc[0]['iterations']}); status > 1: cold {bad_cold} warm {bad_warm}; warm_status "
          f"histogram of the {ws.size} warm calls {np.bincount(ws.ravel(), minlength=3).tolist()}; final state "
          f"difference {float((warm['states'][:, -1] - cold['states'][:, -1]).abs().max()):.3e}")
    assert it_warm < it_cold
    assert bad_warm <= bad_cold
    assert cap[0].get("warm_status") is None and np.all(ws != 1)
    prm = [kkt.DEFAULT] * n_ep
    checked = 0
    for e in cap:
        e = _np(e)
        d64 = e["dnn_out"].astype(np.float64)
        args = (e["ini"], e["goal"], d64[:, 0:3], d64[:, 3:6], d64[:, 6], e["u_last"])
        q = np.stack([O.rd2quat(a) for a in args[3]])
        rows = np.flatnonzero(e["status"] <= 1)
        bad = _certificate(f"plant step {e['step']}", e, args, q, prm, rows)
        assert not bad, bad
        checked += len(rows)
    assert checked >= 0.9 * warm["solves"]
    eng.check_device()
