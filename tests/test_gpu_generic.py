"""The HIP engine at the generic parameter set (generic_params.py) against the CPU oracle given the same parameters
and against the parameterised autograd restatement (tests/kkt.py): solve parity with the KKT certificate, both
sol_gradient modes, the iteration-0 NLP inputs and the PMP costates.  The rules, tolerances and helper functions are
those of tests/test_gpu_parity.py; only the parameters differ.  The Newton step at this set is in test_gpu_newton.py
(test_set_*), the sensitivities in test_gpu_generic_sens.py.

Run on an MI355X:  python -m pytest tests/test_gpu_generic.py -m gpu -q -s

Why: at the reference's constants Model::az is 0 (Jx == Jy), every `wqf != 0` branch is dead, the bound midpoints are
u_ub / 2 and 0 and the lower relaxation acts on a zero bound; every other GPU test runs there.

Problems: generic_params.problem: synthetic_batch(64, seed=2025), t = 0.8 of the sample's own at N = 50 and 0.5 N dt
below, u_last = 1 on the odd samples (the solve tests).  sol_gradient takes the first 16 samples' float32 DNN outputs
unchanged and no u_last (its IFT mode refuses one).

Measured on the CPU with the oracle alone (before any device value; the `oracle_*` functions below):
    statuses        0 on every solve, N = 50 (16 samples), 20, 7, 3, 2, 1 (8 each);
    yardstick       solve_decisions keeps 15 of 16 at N = 50 and 7 of 8 at N = 20, 8 of 8 below: 54 of 56; the FMA build
                    follows the strict build's path on all 54 kept;
    KKT residuals of the oracle's own optima under the parameterised kkt_residual, largest over the 56 solves:
                    primal 1.382e-07 (bar 5e-7), dual / s_d 4.835e-06 (bar 1e-4), complementarity 4.899e-07 (bar 1e-6):
                    the oracle passes the thresholds of test_shorter_horizon, so they are used unchanged (the figures
                    are asserted again in test_solve_parity_and_kkt_certificate, on the oracle before the device);
    active bounds   the oracle's N = 50 optima: 930 of 3 200 control entries at a bound (100 at u_lb = 0.1), 796 of
                    2 400 rate entries;
    sol_gradient    both grad_modes: status 0 on all 144 solves, 110 of 112 gradient entries non-zero (96 of 96 p / a
                    entries); the FMA build follows the strict build on all 16 nominal solves;
    PMP costates    the recursion without the wqf gradient differs from the one with it by up to 5.3e+01 relative.

First run on an MI355X:
    solve parity    53 of the 54 kept solves on the oracle's path (yardstick 54 of 54; the bar is 54 - 2 % of 54): at
                    N = 50 sample 6 takes 208 iterations for the oracle's 206; sample 0 (not kept) 66 for 67; N = 20 and
                    below 8 of 8.  KKT residuals of the device's optima: primal 1.382e-07, dual / s_d 4.835e-06,
                    complementarity 4.899e-07: the oracle's figures to four digits.  930 control and 796 rate entries
                    at a bound, 100 controls at u_lb.
    FD mode         16 of 16 converged, 16 on the oracle's 9-solve path, largest relative difference 4.0e-10 against the
                    bound 1e-5.
    NLP inputs      J, barrier log sum and theta of iteration 0 within 1e-13 on all 144 solves.
    PMP costates    within 1e-11 on 8 samples.
    IFT mode        all 16 nominal solves on the oracle's path (yardstick 16); out8[:, :6] within 2.099e-08 (bound 1e-7 on
                    equal paths, 1e-5 everywhere), probe rewards within 3.0e-09 relative; the oracle's own FMA build
                    differs from its strict build by up to 3.3e-08 on the same samples (printed by the test).

The sol_gradient tests take the batch's DNN outputs as they are.  With the DNN's t multiplied by 0.8 as well (rounded
t 1.6 .. 3.0 s) the oracle gives 109 non-zero entries instead of 110, and one sample becomes badly conditioned: the
oracle's FMA build then differs from its strict build by 4.986e-07 in out8 of sample 0 on the same iteration path
(next sample 5.0e-08), and the device by 2.882e-07, above the 1e-7 bound; every other sample stays below 1.0e-07.
test_sol_gradient_ift_mode_matches_oracle_scaled_t runs those inputs under the same bounds on the 15 samples where the
oracle's two builds agree within 1e-7 (an admission decided from the oracle alone), and under the 1e-5 bound on all 16.
On the device those 15 are within 9.1e-08 (sample 5) and their probe rewards within 2.9e-08 relative.

Mutation check (builds not kept, see test_gpu_newton.py for the three mutations): (a) az = 0 in the G table fails the
parity test (status 6 on sample 0 at N = 50), both sol_gradient tests and the PMP costates; (b) the wqf block dropped
from the Hxx table passes this file except the IFT test (13 of 16 nominal paths) and is caught by the Newton-step and
sensitivity tests; (c) umid = u_ub / 2 fails the NLP inputs (J off by 3.4e-04), the parity test (cost off by 1.1e-03)
and both sol_gradient tests.  No test of test_gpu_parity.py failed under any of them.
"""
import numpy as np
import pytest
import yardstick

torch = pytest.importorskip("torch")

import generic_params as GP  # noqa: E402
import kkt  # noqa: E402
import newton_cases as NC  # noqa: E402
from parity_ref import grad_parity, pmp_reference  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = GP.GENERIC
SOLVES = ((50, 16), (20, 8), (7, 8), (3, 8), (2, 8), (1, 8))     # (horizon, samples)
KKT_BARS = {"primal": 5e-7, "dual": 1e-4, "compl": 1e-6}         # test_shorter_horizon's; dual is relative to s_d
_engines = {}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def engine(N=50):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    if N not in _engines:
        from learningagileflight_se3_amd.engine import Engine
        _engines[N] = Engine(horizon=N, **GENERIC.fields())
    return _engines[N]


def oracle_params(**kw):
    return NC.oracle_params(GENERIC, **kw)


def kkt_figures(sol, prob):
    """Largest (primal, dual / s_d, compl) of kkt.kkt_residual at the generic set over the solves of `sol`, and the
    list of solves that miss KKT_BARS."""
    worst, bad = {"primal": 0.0, "dual": 0.0, "compl": 0.0}, []
    for i in range(len(sol["cost"])):
        r = kkt.kkt_residual(sol["x"][i], sol["u"][i], sol["lam"][i], prob["ini"][i], prob["goal"][i], prob["p"][i],
                             prob["q"][i], prob["t"][i], prob["ulast"][i], GENERIC)
        fig = {"primal": r["primal"], "dual": r["dual"] / r["s_d"], "compl": r["compl"]}
        assert r["bound_viol"] <= 1e-7, (i, r)          # bound_relax 1e-8 max(1, |bound|), honor_original_bounds
        if any(fig[k] > KKT_BARS[k] for k in fig):
            bad.append((i, r))
        worst = {k: max(worst[k], fig[k]) for k in fig}
    return worst, bad


def oracle_solves(batch, N, n):
    """The oracle's side of one horizon, decided without the device: (problem, strict solve, solves whose decisions
    rounding leaves alone, how many of those the FMA build solves on the strict build's path)."""
    from oracle import oracle as O
    prob = GP.problem(batch, N, range(n))
    args = GP.solve_args(prob)
    kw = {"ulast": prob["ulast"], "params": oracle_params(horizon=N)}
    ref = O.solve(*args, **kw)
    kept = yardstick.solve_decisions(args, kw, ref)
    yard = yardstick.solve_paths(tuple(v[kept] for v in args), {"ulast": prob["ulast"][kept], "params": kw["params"]},
                                 {k: v[kept] for k, v in ref.items()})
    return prob, ref, kept, yard


def test_solve_parity_and_kkt_certificate(batch):
    """test_shorter_horizon's comparison at the generic set, N = 50 (16 samples) and 20, 7, 3, 2, 1 (8 each): statuses
    <= 1 on both sides; x, u within 1e-6, cost within 1e-10 and lam within 1e-6 relative on equal iteration paths; cost
    within 1e-6 on every solve; equal paths >= yardstick - 2 % over the solves solve_decisions keeps, kept >= 90 %; the
    KKT certificate of every device optimum under the thresholds the oracle's own optima pass."""
    n_same = n_yard = n_kept = n_all = 0
    for N, B in SOLVES:
        prob, ref, kept, yard = oracle_solves(batch, N, B)
        assert np.all(ref["status"] <= 1), (N, ref["status"])
        oworst, obad = kkt_figures(ref, prob)
        print(f"N={N}: oracle's own optima: KKT residuals {oworst}, decisions stable under rounding on "
              f"{kept.astype(int).tolist()}, yardstick {yard}/{int(kept.sum())}")
        assert not obad, (N, "the oracle's optimum misses the certificate", obad)
        out = engine(N).ocp_solve(prob["ini"], prob["goal"], prob["p"], prob["a"], prob["t"], u_last=prob["ulast"])
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in out.items()}
        assert g["x"].shape == (B, N + 1, 13) and g["u"].shape == (B, N, 4) and g["lam"].shape == (B, N, 13), N
        assert np.all(g["status"] <= 1), (N, g["status"])
        same = g["iters"] == ref["iters"]
        ns = int(same.sum())
        n_all, n_kept, n_yard, n_same = n_all + B, n_kept + int(kept.sum()), n_yard + yard, n_same + int((same & kept).sum())
        print(f"N={N}: same iteration path {ns}/{B}, iterations {g['iters'].tolist()} (oracle {ref['iters'].tolist()})")
        if ns:
            for k in ("x", "u"):
                d = np.abs(g[k][same] - ref[k][same]) / (1 + np.abs(ref[k][same]))
                assert d.max() < 1e-6, (N, k, d.max())
            assert np.max(np.abs(g["cost"][same] - ref["cost"][same]) / np.abs(ref["cost"][same])) < 1e-10, N
            dl = np.abs(g["lam"][same] - ref["lam"][same]).reshape(ns, -1).max(1)
            assert np.max(dl / (1 + np.abs(ref["lam"][same]).reshape(ns, -1).max(1))) < 1e-6, N
        assert np.max(np.abs(g["cost"] - ref["cost"]) / np.abs(ref["cost"])) < 1e-6, N
        gworst, gbad = kkt_figures(g, prob)
        print(f"N={N}: device optima: KKT residuals {gworst}")
        assert not gbad, (N, gbad)
        # the boxes themselves: the final clamp to the original (asymmetric) bounds
        assert g["u"].min() >= GENERIC.u_lb and g["u"].max() <= GENERIC.u_ub, N
        assert g["x"][:, 1:, 10:13].min() >= GENERIC.w_lb and g["x"][:, 1:, 10:13].max() <= GENERIC.w_ub, N
        if N == 50:
            at_u = int(np.sum((g["u"] <= GENERIC.u_lb + 1e-6) | (g["u"] >= GENERIC.u_ub - 1e-6)))
            w = g["x"][:, 1:, 10:13]
            at_w = int(np.sum((w <= GENERIC.w_lb + 1e-6) | (w >= GENERIC.w_ub - 1e-6)))
            lo_u = int(np.sum(g["u"] <= GENERIC.u_lb + 1e-6))
            print(f"N=50: {at_u} of {g['u'].size} control entries at a bound ({lo_u} at the lower), {at_w} of {w.size} "
                  "rate entries")
            assert lo_u > 0 and at_u > lo_u and at_w > 0        # both sides of the control box are active
    print(f"same iteration path {n_same}/{n_kept} (rounding yardstick {n_yard}/{n_kept}) of {n_all} solves")
    assert n_kept >= 0.9 * n_all, n_kept
    assert n_same >= n_yard - 0.02 * n_kept, f"iteration paths differ on {n_kept - n_same} of {n_kept}; yardstick {n_yard}"


def grad_args(batch, B=16):
    """sol_gradient inputs of the first B samples: the batch's float32 DNN outputs as they are, as test_gpu_parity.py
    passes them (the rounded traversal times, 2.0 .. 3.8 s, lie inside the 4 s horizon)."""
    return batch["ini"][:B], batch["goal"][:B], batch["gate12"][:B], batch["dnn_out"][:B]


def test_sol_gradient_fd_mode_matches_oracle(batch):
    """grad_mode 0 on 16 samples at N = 50 against the oracle's sol_gradient under parity_ref.grad_parity."""
    eng = engine()
    args = grad_args(batch)
    it = torch.full((16, 9), -1, dtype=torch.int32, device=eng.device)
    eng.record_iters(it)
    try:
        o8, R9, s9 = eng.sol_gradient(*args, want_rewards=True, grad_mode=0)
        torch.cuda.synchronize()
    finally:
        eng.record_iters(None)
    o8, s9, it = o8.cpu().numpy(), s9.cpu().numpy(), it.cpu().numpy()
    assert np.all(s9 <= 1), s9
    assert np.count_nonzero(o8[:, :7]) >= 0.75 * o8[:, :7].size     # a gradient, not clipped-away zeros
    grad_parity(o8, s9, it, args, "generic set, FD mode", params=oracle_params(grad_mode=0))


def _ift_mode_against_oracle(args, label, resolvable_only=False):
    """grad_mode 1 under test_gpu_parity.py's test_sol_gradient_ift_mode_matches_oracle bounds: out8[:, :6] within 1e-7
    where the nominal solve took the oracle's iteration path, 1e-5 everywhere, probe rewards 1e-6 relative on equal
    paths; the count of equal nominal paths held to the rounding yardstick less 2 %.  resolvable_only: the 1e-7 and
    1e-6 bounds are held on the samples where the oracle's own two builds (strict, FMA) agree within 1e-7 in out8,
    which is decided from the oracle alone and must leave at least 90 % of the samples; where they do not agree the
    yardstick cannot resolve 1e-7."""
    from oracle import oracle as O
    eng = engine()
    B = len(args[0])
    it = torch.zeros((B, 9), dtype=torch.int32, device=eng.device)
    eng.record_iters(it)
    try:
        g8, gR, gS = eng.sol_gradient(*args, want_rewards=True, grad_mode=1)
        torch.cuda.synchronize()
    finally:
        eng.record_iters(None)
    g8, gR, gS, it = g8.cpu().numpy(), gR.cpu().numpy(), gS.cpu().numpy(), it.cpu().numpy()
    r8, rR, rS = O.sol_gradient(*args, params=oracle_params(grad_mode=1))
    assert np.all(rS <= 1) and np.array_equal(gS <= 1, rS <= 1), (gS, rS)
    pp, qq, tt, _ = O.grad_params(args[3], params=oracle_params())               # job 0 = the nominal solve
    nominal = (args[0], args[1], pp[:, 0], qq[:, 0], tt[:, 0])
    ref = O.solve(*nominal, params=oracle_params())
    yard = yardstick.solve_paths(nominal, {"params": oracle_params()}, ref)
    same = it[:, 0] == ref["iters"]
    d = np.abs(g8[:, :6] - r8[:, :6])
    dR = np.abs(gR[:, 1:7] - rR[:, 1:7]) / np.abs(rR[:, 1:7])
    f8, _, _ = O.sol_gradient(*args, params=oracle_params(grad_mode=1), fast=True)
    own = np.abs(f8[:, :6] - r8[:, :6]).max(1)
    res = own <= 1e-7 if resolvable_only else np.ones(B, bool)
    tight = same & res
    stats = dict(same=int(same.sum()), yardstick=yard, resolvable=int(res.sum()), d_tight=d[tight].max(), d_all=d.max(),
                 dR_tight=dR[tight].max(), nonzero=int(np.count_nonzero(r8[:, :6])), d_per_sample=d.max(1).tolist(),
                 oracle_fma_vs_strict_per_sample=own.tolist())
    print(f"{label}, IFT HIP vs oracle:", stats)
    assert res.sum() >= 0.9 * B, stats
    assert same.sum() >= yard - 0.02 * B, stats
    assert stats["nonzero"] >= 0.75 * r8[:, :6].size, stats
    assert d[tight].max() <= 1e-7, stats
    assert d.max() <= 1e-5, stats
    assert dR[tight].max() <= 1e-6, stats


def test_sol_gradient_ift_mode_matches_oracle(batch):
    """grad_mode 1 on the same 16 samples, every one of them under every bound."""
    _ift_mode_against_oracle(grad_args(batch), "generic set")


def test_sol_gradient_ift_mode_matches_oracle_scaled_t(batch):
    """The same with the DNN's t output multiplied by 0.8 (float32), the rule of the solve problems at N = 50.  The
    oracle alone leaves out sample 0: its FMA build differs from its strict build by 5.0e-07 there, on one iteration
    path; the 1e-5 bound still covers it."""
    ini, goal, gate12, dnn = grad_args(batch)
    dnn = dnn.astype(np.float32).copy()
    dnn[:, 6] = (dnn[:, 6] * np.float32(GP.T_SCALE)).astype(np.float32)
    _ift_mode_against_oracle((ini, goal, gate12, dnn), "generic set, t scaled", resolvable_only=True)


def test_sol_gradient_nlp_inputs_match_oracle(batch):
    """Iteration 0 of the 9 x 16 sol_gradient NLPs: J, the barrier log sum and theta (trace words 14, 15, 2) agree with
    the oracle's to 1e-13 relative.  At this set the initial point is (u_lb + u_ub) / 2 and w = (w_lb + w_ub) / 2 = 0.1
    inside asymmetric relaxed boxes, J carries the goal-attitude term and every model constant."""
    from oracle import oracle as O
    eng = engine()
    args = grad_args(batch)
    B, TI = 16, 2
    tr = torch.zeros((9 * B, TI, 16), dtype=torch.float64, device=eng.device)   # instance = probe * B + sample
    eng.debug_trace(tr, TI)
    try:
        eng.sol_gradient(*args, want_rewards=True, grad_mode=0)
        torch.cuda.synchronize()
    finally:
        eng.debug_trace(None)
    td = tr.cpu().numpy()[:, 0, :].reshape(9, B, 16)
    pp, qq, tt, _ = O.grad_params(args[3], params=oracle_params())
    for j in range(9):
        buf = np.zeros((B, TI, 16))
        O.debug_trace(buf, TI)
        try:
            O.solve(args[0], args[1], pp[:, j], qq[:, j], tt[:, j], params=oracle_params())
        finally:
            O.debug_trace(None, 0)
        for w, name in ((14, "J"), (15, "barrier log sum"), (2, "theta")):
            d = np.abs(td[j, :, w] - buf[:, 0, w]) / np.maximum(np.abs(buf[:, 0, w]), 1e-300)
            assert d.max() < 1e-13, (j, name, int(d.argmax()), d.max())


def test_pmp_costates_match_reference_recursion(batch):
    """costate_option = 1 at the generic set against parity_ref.pmp_reference on the oracle's derivatives
    with the same parameters, 8 samples, 1e-11: the recursion's dc/dx carries the goal-attitude gradient (wqf) and its
    A_k^T the az terms."""
    eng = engine()
    B = 8
    prob = GP.problem(batch, 50, range(B))
    a = (prob["ini"], prob["goal"], prob["p"], prob["a"], prob["t"])
    o0 = eng.ocp_solve(*a, u_last=prob["ulast"])
    o1 = eng.ocp_solve(*a, u_last=prob["ulast"], costate_option=1)
    assert eng.params.costate_option == 0
    x, u, lam = (o1[k].cpu().numpy() for k in ("x", "u", "lam"))
    assert np.array_equal(x, o0["x"].cpu().numpy()) and np.array_equal(u, o0["u"].cpu().numpy())
    assert np.all(o1["status"].cpu().numpy() <= 1)
    # the goal-attitude gradient is part of what is compared: the recursion without it is another vector
    far = 0.0
    for b in range(B):
        ref = pmp_reference(x[b], u[b], prob["goal"][b], prob["p"][b], prob["q"][b], params=oracle_params())
        assert np.max(np.abs(lam[b] - ref) / (1.0 + np.abs(ref))) < 1e-11, b
        no_q = pmp_reference(x[b], u[b], prob["goal"][b], prob["p"][b], prob["q"][b], params=oracle_params(wqf=0.0))
        far = max(far, float(np.max(np.abs(no_q - ref) / (1.0 + np.abs(ref)))))
    print(f"PMP costates: the recursion without the wqf gradient differs by up to {far:.3e}")
    assert far > 1e-3
