"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle and the reference fixtures.

Run on an MI355X:  python -m pytest tests -m gpu -x -q

Tolerances (fp64 everywhere):
  * trajectories / controls of the NLP optimum: 1e-6 relative, cost 1e-10 relative, for instances whose
    IPM took the same number of iterations on both sides (identical decision path; the final iterate is
    determined only to IPOPT's 1e-8 KKT tolerance, observed <= 5e-8 on x), and the optimum
    KKT-certified (tests/kkt.py) for every GPU instance;
  * rewards: 1e-9 on the reference's own scored trajectories (no solver involved);
  * sol_gradient out8: 1e-6 absolute (entries are clipped differences scaled by <= 0.2) for samples
    whose 9 solves followed the oracle's iteration path; every sample within 1e-3 (a different
    accept/reject decision at IPOPT's 1e-8 tolerance moves the reward by up to ~1e-4).
"""
import numpy as np
import pytest
import yardstick

torch = pytest.importorskip("torch")

from parity_ref import grad_parity, pmp_reference  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def _loaded_native():
    import learningagileflight_se3_amd._lib as L
    return L._lib is not None and L._lib._name.endswith("liblafse3.so")


def test_native_library_is_the_hip_build(eng):
    assert _loaded_native()
    import learningagileflight_se3_amd._lib as L
    assert b"gfx950" in L.load().lafse3_version()


def test_reward_matches_reference_fixture(eng, golden):
    g = golden("policy")
    B = g["x_calls"].shape[0]
    x = g["x_calls"].reshape(B * 9, 51, 13)
    R = eng.reward(x, np.repeat(g["goal"], 9, 0), np.repeat(g["gate12"], 9, 0)).cpu().numpy()
    assert np.max(np.abs(R - g["rewards"].reshape(-1))) < 1e-9


def test_ocp_solve_matches_oracle_and_is_kkt(eng, batch):
    from oracle import oracle as O
    import kkt
    sb = batch
    p = sb["dnn_out"][:, :3].astype(np.float64)
    a = sb["dnn_out"][:, 3:6].astype(np.float64)
    t = sb["dnn_out"][:, 6].astype(np.float64)
    out = eng.ocp_solve(sb["ini"], sb["goal"], p, a, t)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in out.items()}
    q = np.stack([O.rd2quat(ai) for ai in a])
    ref = O.solve(sb["ini"], sb["goal"], p, q, t)
    assert np.all(g["status"] <= 1) and np.all(ref["status"] <= 1)
    same = g["iters"] == ref["iters"]
    # exact iteration paths against the rounding yardstick (tests/yardstick.py: the oracle's FMA build against its
    # strict build on the same 64 solves), less 2 % of the solves
    yard = yardstick.solve_paths((sb["ini"], sb["goal"], p, q, t), {}, ref)
    print(f"same iteration path {int(same.sum())}/64 (rounding yardstick {yard}/64)")
    assert same.sum() >= yard - 0.02 * same.size, f"iteration paths differ on {np.sum(~same)} of {len(same)}; yardstick {yard}"
    for k in ("x", "u"):
        d = np.abs(g[k][same] - ref[k][same]) / (1 + np.abs(ref[k][same]))
        assert d.max() < 1e-6, k
    assert np.max(np.abs(g["cost"][same] - ref["cost"][same]) / np.abs(ref["cost"][same])) < 1e-10
    # multipliers are determined only to the dual tolerance: compare relative to each instance's scale
    dl = np.abs(g["lam"][same] - ref["lam"][same]).reshape(int(same.sum()), -1).max(1)
    assert np.max(dl / (1 + np.abs(ref["lam"][same]).reshape(int(same.sum()), -1).max(1))) < 1e-6
    # all instances: same optimum up to the IPOPT tolerance
    assert np.max(np.abs(g["cost"] - ref["cost"]) / np.abs(ref["cost"])) < 1e-6
    # KKT certificate of every GPU optimum from an independent torch-autograd restatement (tests/kkt.py):
    # bound_relax = 1e-8 + honor_original_bounds (IPOPT defaults) leave ~2e-7 defects after projection; the
    # dual bound carries IPOPT's multiplier scaling s_d = max(1, mean|lam| / 100) (kkt.dual_scale)
    bad = []
    for i in range(64):
        r = kkt.kkt_residual(g["x"][i], g["u"][i], g["lam"][i], sb["ini"][i], sb["goal"][i], p[i], q[i], t[i])
        if not (r["primal"] <= 5e-7 and r["dual"] <= 1e-4 * r["s_d"] and r["compl"] <= 1e-6):
            bad.append((i, r))
    assert not bad, bad


def test_sol_gradient_matches_oracle(eng, batch):
    from oracle import oracle as O
    sb = batch
    B = 64
    args = (sb["ini"][:B], sb["goal"][:B], sb["gate12"][:B], sb["dnn_out"][:B])
    out8, R9, S9 = eng.sol_gradient(*args, want_rewards=True)
    torch.cuda.synchronize()
    out8, R9, S9 = out8.cpu().numpy(), R9.cpu().numpy(), S9.cpu().numpy()
    r8, rR, rS = O.sol_gradient(*args)
    assert np.all(S9 <= 1) and np.all(rS <= 1)
    # The IPM's iteration path is sensitive to last-bit rounding (the oracle built with FMA contraction
    # differs from itself built without it on ~12 % of the 9-solve groups, rewards by up to ~1e-5), so
    # the criterion is the gradient itself (north_star: <= 1e-5 relative), not reward equality.
    d8 = np.abs(out8[:, :7] - r8[:, :7]) / (1.0 + np.abs(r8[:, :7]))
    per = d8.max(1)
    assert per.max() < 1e-5, per
    assert np.mean(per < 1e-6) >= 0.9, per
    # rewards (every solve converged on both sides): north_star's 1e-5 relative
    assert np.max(np.abs(R9 - rR) / np.maximum(1.0, np.abs(rR))) < 1e-5
    assert np.max(np.abs(out8[:, 7] - r8[:, 7]) / np.maximum(1.0, np.abs(r8[:, 7]))) < 1e-5


def test_sol_gradient_nlp_inputs_match_oracle(eng, batch):
    """Every one of the 9 x 64 sol_gradient NLPs starts from the oracle's problem: at iteration 0 (the same initial
    point) the objective J, the barrier log sum and theta agree to 1e-13 relative (debug trace words 14, 15, 2).  This
    pins the float32 input semantics (round1_f32, magni_f32 -> the traversal attitude, the probes' p / a / t, SURVEY
    A10): a one-ulp float32 sqrt on the device moved J by 1.2e-7 relative on 18 of the resto fixture's solves (round
    4) and every iterate after it."""
    from oracle import oracle as O
    sb = batch
    B, TI = 64, 2
    args = (sb["ini"][:B], sb["goal"][:B], sb["gate12"][:B], sb["dnn_out"][:B])
    tr = torch.zeros((9 * B, TI, 16), dtype=torch.float64, device=eng.device)   # instance = probe * B + sample
    eng.debug_trace(tr, TI)
    try:
        eng.sol_gradient(*args, want_rewards=True)
        torch.cuda.synchronize()
    finally:
        eng.debug_trace(None)
    td = tr.cpu().numpy()[:, 0, :].reshape(9, B, 16)
    pp, qq, tt, _ = O.grad_params(sb["dnn_out"][:B])
    for j in range(9):
        buf = np.zeros((B, TI, 16))
        O.debug_trace(buf, TI)
        try:
            O.solve(sb["ini"][:B], sb["goal"][:B], pp[:, j], qq[:, j], tt[:, j])
        finally:
            O.debug_trace(None, 0)
        for w, name in ((14, "J"), (15, "barrier log sum"), (2, "theta")):
            d = np.abs(td[j, :, w] - buf[:, 0, w]) / np.maximum(np.abs(buf[:, 0, w]), 1e-300)
            assert d.max() < 1e-13, (j, name, int(d.argmax()), d.max())


def test_ocp_solve_fp32_twin(eng, batch):
    """lafse3_ocp_solve_f32: float32 buffers at the boundary, the fp64 solve inside -> exactly the fp64
    entry point on the widened inputs, rounded to float32."""
    sb = batch
    B = 16
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    ini, goal = f32(sb["ini"][:B]), f32(sb["goal"][:B])
    p, a, t = f32(sb["dnn_out"][:B, :3]), f32(sb["dnn_out"][:B, 3:6]), f32(sb["dnn_out"][:B, 6])
    r32 = eng.ocp_solve(ini, goal, p, a, t, dtype=torch.float32)
    r64 = eng.ocp_solve(*(v.astype(np.float64) for v in (ini, goal, p, a, t)))
    torch.cuda.synchronize()
    assert np.array_equal(r32["status"].cpu().numpy(), r64["status"].cpu().numpy())
    for k in ("x", "u", "lam", "cost"):
        assert r32[k].dtype == torch.float32
        assert np.array_equal(r32[k].cpu().numpy(), r64[k].cpu().numpy().astype(np.float32)), k


def test_sol_gradient_ift_mode_against_fd(eng, batch):
    """grad_mode 1 (IFT, lafse3.h) against the reference's FD semantics (grad_mode 0, itself pinned to the
    oracle above) on the same 64 samples.  The nominal and t-probe solves are the same computations, so
    out8[:, 6:8] must be identical.  The p/a entries replace R(theta + 1e-3 e_i) by R(x* + 1e-3 dx*/dtheta_i):
    they agree to the second-order term of the solution map (measured on 4096 samples: median |diff| 5e-7
    for p, 4e-6..9e-6 for a; 90th percentile relative 1e-3 for p, 3-6 % for a) except where the reward is
    non-smooth along the probe (a rotor track crossing a gate edge, or an FD re-solve landing on another
    local optimum: ~1 % of probes), which the FD difference straddles and the linearisation cannot."""
    sb = batch
    args = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    fd, _, sf = eng.sol_gradient(*args, want_rewards=True, grad_mode=0)
    ift, R9, si = eng.sol_gradient(*args, want_rewards=True, grad_mode=1)
    torch.cuda.synchronize()
    fd, ift, sf, si = fd.cpu().numpy(), ift.cpu().numpy(), sf.cpu().numpy(), si.cpu().numpy()
    assert eng.params.grad_mode == 0                      # the override is restored
    assert np.array_equal(sf[:, [0, 7, 8]], si[:, [0, 7, 8]])
    assert np.array_equal(fd[:, 6:], ift[:, 6:])
    # the factorisation at z* (delta_w = 0) failing marks the six p/a probe statuses 6 and leaves their rewards at R0
    # (a zero p/a gradient that is not a measurement): counted, and bounded
    fb = (si[:, 0] <= 1) & np.all(si[:, 1:7] == 6, axis=1)
    print(f"IFT z* factorisation fallbacks: {int(fb.sum())} of {len(fb)} samples")
    assert np.all(ift[fb, :6] == 0.0) and fb.mean() <= 0.05
    d = np.abs(fd[:, :6] - ift[:, :6])
    assert np.all(np.median(d, axis=0) < 2e-5), np.median(d, axis=0)
    close = d <= 1e-4 + 0.1 * np.abs(fd[:, :6])
    assert np.all(close.mean(axis=0) >= 0.85), close.mean(axis=0)
    with pytest.raises(Exception):                        # IFT linearises the nominal solve (u_last = 0)
        eng.sol_gradient(*[a[:2] for a in args], u_last=np.zeros((2, 4)), grad_mode=1)


def test_sol_gradient_ift_mode_matches_oracle(eng, batch):
    """grad_mode 1 against its oracle counterpart (oracle/lafse3_oracle.c orc_ift_probes: one Newton-system
    factorisation at the optimum z*, delta_w = 0, and one solve per parameter with right-hand side
    dF/dtheta_i by central differences of the cost gradient) on the same 64 samples: out8[:, :6] within
    1e-7 absolute where the nominal solve took the oracle's iteration path, within 1e-5 everywhere.  The
    floor is z* itself: on the same iteration path the two optima still differ by up to ~5e-8 in x
    (different rounding through ~60 IPM iterations, test_ocp_solve_matches_oracle_and_is_kkt), which
    moves R(x* + 1e-3 dx*) by ~1e-7 relative and out8 by up to ~6e-8 (measured); the FD mode agrees only
    to 1e-6 on the same samples for the same reason.  IFT is an
    approximation of the reference's FD gradient (first order in the 1e-3 probe), not the same number."""
    from oracle import oracle as O
    sb = batch
    args = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    it = torch.zeros((64, 9), dtype=torch.int32, device=eng.device)
    eng.record_iters(it)
    try:
        g8, gR, gS = eng.sol_gradient(*args, want_rewards=True, grad_mode=1)
        torch.cuda.synchronize()
    finally:
        eng.record_iters(None)
    g8, gR, gS, it = g8.cpu().numpy(), gR.cpu().numpy(), gS.cpu().numpy(), it.cpu().numpy()
    r8, rR, rS = O.sol_gradient(*args, params=O.default_params(grad_mode=1))
    assert np.array_equal(gS <= 1, rS <= 1)
    pp, qq, tt, _ = O.grad_params(sb["dnn_out"])                 # job 0 = the nominal solve
    ref = O.solve(sb["ini"], sb["goal"], pp[:, 0], qq[:, 0], tt[:, 0])
    same = it[:, 0] == ref["iters"]
    d = np.abs(g8[:, :6] - r8[:, :6])
    dR = np.abs(gR[:, 1:7] - rR[:, 1:7]) / np.abs(rR[:, 1:7])
    stats = dict(same=same.mean(), d_same=d[same].max(), d_all=d.max(), dR_same=dR[same].max(),
                 R0_same=np.max(np.abs(gR[same, 0] - rR[same, 0]) / np.abs(rR[same, 0])))
    print("IFT HIP vs oracle:", stats)
    assert same.mean() >= 0.85, stats
    assert d[same].max() <= 1e-7, stats
    assert d.max() <= 1e-5, stats
    # probe rewards: the nominal reward R0 already differs by up to ~3e-7 relative (measured) on these paths
    assert dR[same].max() <= 1e-6, stats


def test_objective_and_get_input(eng, batch):
    from oracle import oracle as O
    sb = batch
    B = 8
    p = sb["dnn_out"][:B, :3].astype(np.float64)
    a = sb["dnn_out"][:B, 3:6].astype(np.float64)
    t = sb["dnn_out"][:B, 6].astype(np.float64) + 0.04     # objective rounds t (quad_policy.py:70)
    R, st = eng.objective(sb["ini"][:B], sb["goal"][:B], sb["gate12"][:B], p, a, t)
    R = R.cpu().numpy()
    q = np.stack([O.rd2quat(ai) for ai in a])
    tr = np.round(t * 10) / 10
    ref = O.solve(sb["ini"][:B], sb["goal"][:B], p, q, tr)
    rR, _ = O.reward(ref["x"], sb["goal"][:B], sb["gate12"][:B])
    assert np.max(np.abs(R - rR)) < 1e-6
    # get_input: first control of the solve on float32 DNN outputs, t unrounded
    u0, x, st = eng.get_input(sb["ini"][:B], sb["goal"][:B], sb["dnn_out"][:B], want_x=True)
    u0 = u0.cpu().numpy()
    dn = sb["dnn_out"][:B]
    nrm = [np.float64(np.sqrt(np.float32(sum(np.float64(np.float32(c * c)) for c in v)))) for v in dn[:, 3:6]]
    q32 = np.stack([O.rd2quat(v.astype(np.float64), n) for v, n in zip(dn[:, 3:6], nrm)])
    ref = O.solve(sb["ini"][:B], sb["goal"][:B], dn[:, :3].astype(np.float64), q32, dn[:, 6].astype(np.float64))
    assert np.max(np.abs(u0 - ref["u"][:, 0, :])) < 1e-6
    assert np.max(np.abs(x.cpu().numpy() - ref["x"])) < 1e-5


def test_edge_cases(eng, batch):
    sb = batch
    # empty batch
    out = eng.ocp_solve(np.zeros((0, 13)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    assert out["status"].numel() == 0
    # Ulast given (only the six pose perturbations receive it)
    from oracle import oracle as O
    ul = np.full((4, 4), 1.0)
    o8, _, s9 = eng.sol_gradient(sb["ini"][:4], sb["goal"][:4], sb["gate12"][:4], sb["dnn_out"][:4], u_last=ul,
                                 want_rewards=True)
    o8, s9 = o8.cpu().numpy(), s9.cpu().numpy()
    r8, _, rs = O.sol_gradient(sb["ini"][:4], sb["goal"][:4], sb["gate12"][:4], sb["dnn_out"][:4], ulast=ul)
    assert np.all(s9 <= 1) and np.all(rs <= 1)
    assert np.max(np.abs(o8[:, :7] - r8[:, :7]) / (1.0 + np.abs(r8[:, :7]))) < 1e-5
    assert np.max(np.abs(o8[:, 7] - r8[:, 7]) / np.maximum(1.0, np.abs(r8[:, 7]))) < 1e-5
    # invalid horizon is rejected with an error code, not a crash
    from learningagileflight_se3_amd import _lib
    p = _lib.default_params(horizon=64)
    with pytest.raises(_lib.Lafse3Error):
        eng.set_params(p)


def test_shorter_horizon(batch):
    """Horizons 1, 2, 3, 7, 20, 49 (the lane-per-stage guards lane < N, lane <= N, min(k + 1, N - 1), max(k - 1, 0) at
    their edges), 8 samples each, t = 0.5 N dt so that the traversal weight lies inside the horizon: the comparison of
    test_ocp_solve_matches_oracle_and_is_kkt, same rule and tolerances, the count of equal iteration paths held to
    the rounding yardstick less 2 % over the 48 solves together.  The count is taken over the solves that the oracle's
    own FMA build solves with its strict build's decisions (yardstick.solve_decisions: mu, delta_w, accepted, filter
    size, step halvings of every iteration): where rounding alone moves a decision of the oracle, the device's path is
    not held to it.  That leaves out one solve, N = 20, sample 6, and this is what was measured on it (debug traces of
    all three, strict oracle 141 iterations ending acceptable, FMA build 141, device 161):
      * the continuous trace words (E0, theta, phi, grad phi.d, alpha_max, alpha_z, J, log sum) of the device and of
        the FMA build leave the strict build's at the same rate: 4e-15 at iteration 0, 6e-13 at 10, 5e-11 at 40, 5e-8 at
        70, 9e-7 at 90 (90 iterations at mu = 0.1 with steps of 1e-3 .. 1e-1 and delta_w of 10 .. 300), the device
        within a factor of 1.5 of the FMA build's figure at every one of them; every decision agrees up to iteration 125;
      * at mu = 2.5e-9, theta = 7e-9 the inertia verdict on K(0) is a near tie: the device regularises
        (delta_w = 113.8) at iteration 126, the strict build at 127, the FMA build at 128, one after the other.
        From there the three paths are different solves; the FMA build happens to end after 141 iterations too, which
        is why status and iteration count (yardstick.solve_paths) do not show its flip.
    The N = 20 cost assertion of this test has always contained that sample, and every other assertion here (statuses,
    cost to 1e-6, KKT certificate) still covers it.  First run: 47 of 47 paths equal, yardstick 47 of 47.
    The oracle converges (status <= 1) on all 48, N = 1 included, so no sample was replaced."""
    from learningagileflight_se3_amd.engine import Engine
    from oracle import oracle as O
    import kkt
    sb = batch
    B = 8
    p = sb["dnn_out"][:B, :3].astype(np.float64)
    a = sb["dnn_out"][:B, 3:6].astype(np.float64)
    q = np.stack([O.rd2quat(ai) for ai in a])
    n_same = n_yard = n_kept = 0
    for N in (1, 2, 3, 7, 20, 49):
        e = Engine(horizon=N)
        t = np.full(B, 0.5 * N * 0.1)
        out = e.ocp_solve(sb["ini"][:B], sb["goal"][:B], p, a, t)
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in out.items()}
        ref = O.solve(sb["ini"][:B], sb["goal"][:B], p, q, t, params=O.default_params(horizon=N))
        assert g["x"].shape == (B, N + 1, 13) and g["u"].shape == (B, N, 4) and g["lam"].shape == (B, N, 13), N
        assert np.all(g["status"] <= 1) and np.all(ref["status"] <= 1), (N, g["status"], ref["status"])
        if N == 20:
            assert out["x"].shape == (B, 21, 13)
            assert np.max(np.abs(out["cost"].cpu().numpy() - ref["cost"]) / ref["cost"]) < 1e-6
        same = g["iters"] == ref["iters"]
        ns = int(same.sum())
        yargs, ykw = (sb["ini"][:B], sb["goal"][:B], p, q, t), {"params": O.default_params(horizon=N)}
        kept = yardstick.solve_decisions(yargs, ykw, ref)
        n_kept += int(kept.sum())
        n_same += int((same & kept).sum())
        n_yard += yardstick.solve_paths(tuple(v[kept] for v in yargs), ykw, {k: v[kept] for k, v in ref.items()})
        print(f"N={N}: same iteration path {ns}/{B}, iterations {g['iters'].tolist()}, oracle's decisions stable "
              f"under rounding on {kept.astype(int).tolist()}")
        if ns:
            for k in ("x", "u"):
                d = np.abs(g[k][same] - ref[k][same]) / (1 + np.abs(ref[k][same]))
                assert d.max() < 1e-6, (N, k)
            assert np.max(np.abs(g["cost"][same] - ref["cost"][same]) / np.abs(ref["cost"][same])) < 1e-10, N
            dl = np.abs(g["lam"][same] - ref["lam"][same]).reshape(ns, -1).max(1)
            assert np.max(dl / (1 + np.abs(ref["lam"][same]).reshape(ns, -1).max(1))) < 1e-6, N
        assert np.max(np.abs(g["cost"] - ref["cost"]) / np.abs(ref["cost"])) < 1e-6, N
        bad = []
        for i in range(B):
            r = kkt.kkt_residual(g["x"][i], g["u"][i], g["lam"][i], sb["ini"][i], sb["goal"][i], p[i], q[i], t[i])
            if not (r["primal"] <= 5e-7 and r["dual"] <= 1e-4 * r["s_d"] and r["compl"] <= 1e-6):
                bad.append((i, r))
        assert not bad, (N, bad)
    print(f"same iteration path {n_same}/{n_kept} (rounding yardstick {n_yard}/{n_kept})")
    assert n_kept >= 0.9 * 48, n_kept
    assert n_same >= n_yard - 0.02 * n_kept, f"iteration paths differ on {n_kept - n_same} of {n_kept}; yardstick {n_yard}"


def test_dropin_run_quad_and_ocsys(eng, batch):
    """quad_policy.run_quad / OCSys mirror (reference method names) against the batched engine + oracle."""
    from learningagileflight_se3_amd.quad_policy import OCSys, run_quad
    from oracle import oracle as O
    sb = batch
    i = 3
    rq = run_quad(goal_pos=sb["goal"][i].tolist(), ini_r=sb["ini"][i, :3].tolist(), engine=eng)
    rq.init_obstacle(sb["gate12"][i])
    o = sb["dnn_out"][i]
    # float32 DNN outputs -> the fused 9-solve kernel; must equal the batched call bit for bit
    g = rq.sol_gradient(sb["ini"][i], o[0:3], o[3:6], o[6])
    gb = eng.sol_gradient(sb["ini"][i:i + 1], sb["goal"][i:i + 1], sb["gate12"][i:i + 1],
                          sb["dnn_out"][i:i + 1]).cpu().numpy()[0]
    assert g.shape == (8,) and np.array_equal(g, gb)
    # float64 inputs -> 9 objective evaluations composed as quad_policy.py:94-112
    p64, a64, t64 = o[0:3].astype(np.float64), o[3:6].astype(np.float64), 3.0
    g64 = rq.sol_gradient(sb["ini"][i], p64, a64, t64)
    j = rq.objective(sb["ini"][i], p64, a64, t64)
    assert abs(g64[7] - j) < 1e-12
    q = O.rd2quat(a64)
    ref = O.solve(sb["ini"][i:i + 1], sb["goal"][i:i + 1], p64[None], q[None], np.array([3.0]))
    rR, _ = O.reward(ref["x"], sb["goal"][i:i + 1], sb["gate12"][i:i + 1])
    assert abs(j - rR[0]) < 1e-6
    # OCSys.ocSolver returns the reference dict layout
    oc = OCSys(goal_pos=sb["goal"][i], engine=eng)
    oc.setTraCost(p64, a64, 3.0)
    sol = oc.ocSolver(ini_state=sb["ini"][i], horizon=50, dt=0.1)
    assert sol["state_traj_opt"].shape == (51, 13) and sol["control_traj_opt"].shape == (50, 4)
    assert sol["costate_traj_opt"].shape == (50, 13) and sol["cost"].shape == (1, 1)
    assert np.max(np.abs(sol["state_traj_opt"] - ref["x"][0])) < 1e-6
    u0 = rq.get_input(sb["ini"][i], None, p64, a64, 3.0)
    assert np.max(np.abs(u0 - ref["u"][0, 0])) < 1e-6


def test_pmp_costates_match_reference_recursion(eng, batch):
    """costate_option=1 (quad_OC.py:188-201): the GPU recursion on the GPU optimum equals the reference's
    recursion evaluated with the oracle's Jacobians on the same trajectory; x, u are unchanged."""
    from oracle import oracle as O
    sb = batch
    B = 8
    p = sb["dnn_out"][:B, :3].astype(np.float64)
    a = sb["dnn_out"][:B, 3:6].astype(np.float64)
    t = sb["dnn_out"][:B, 6].astype(np.float64)
    o0 = eng.ocp_solve(sb["ini"][:B], sb["goal"][:B], p, a, t)
    o1 = eng.ocp_solve(sb["ini"][:B], sb["goal"][:B], p, a, t, costate_option=1)
    assert eng.params.costate_option == 0                      # per-call override is restored
    x, u, lam = (o1[k].cpu().numpy() for k in ("x", "u", "lam"))
    assert np.array_equal(x, o0["x"].cpu().numpy()) and np.array_equal(u, o0["u"].cpu().numpy())
    for b in range(B):
        ref = pmp_reference(x[b], u[b], sb["goal"][b], p[b], O.rd2quat(a[b]))
        assert np.max(np.abs(lam[b] - ref) / (1.0 + np.abs(ref))) < 1e-11, b
    # OCSys mirror passes the option through
    from learningagileflight_se3_amd.quad_policy import OCSys
    oc = OCSys(goal_pos=sb["goal"][0], engine=eng)
    oc.setTraCost(p[0], a[0], t[0])
    sol = oc.ocSolver(ini_state=sb["ini"][0], costate_option=1)
    assert np.max(np.abs(sol["costate_traj_opt"] - lam[0])) < 1e-12


def test_full_size_properties(eng):
    """configs[2] size (B = 4096 samples, 36 864 solves) through size-independent properties: the launch is
    deterministic (bit-identical out8 on a rerun: no cross-instance races in the shared workspace), a
    sample's result does not depend on its batch position or batch size (a 32-sample subset re-solved
    alone gives the identical rows), and >= 99 % of the solves converge."""
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(4096, seed=77)
    args = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    o1, _, s1 = eng.sol_gradient(*args, want_rewards=True)
    o2 = eng.sol_gradient(*args)
    torch.cuda.synchronize()
    o1, o2, s1 = o1.cpu().numpy(), o2.cpu().numpy(), s1.cpu().numpy()
    assert np.array_equal(o1, o2)
    assert np.mean(s1 <= 1) >= 0.99
    idx = np.random.default_rng(0).choice(4096, 32, replace=False)
    o3 = eng.sol_gradient(*(a[idx] for a in args)).cpu().numpy()
    assert np.array_equal(o3, o1[idx])


def test_ift_mode_full_size_properties(eng):
    """configs[2] size in IFT mode (grad_mode 1: 4096 samples = 12 288 NLP solves + 24 576 sensitivity sweeps) through
    size-independent properties: a rerun is bit-identical, a seeded 32-sample subset solved alone reproduces its
    rows, >= 99 % of the nominal and t-probe solves converge, the z* factorisation fallback stays rare (<= 5 %),
    and the t entries (out8[:, 6:8]: the same nominal / t-probe solves as FD) equal FD mode's on a 256-sample
    subset bit for bit."""
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(4096, seed=5)
    args = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    o1, _, s1 = eng.sol_gradient(*args, want_rewards=True, grad_mode=1)
    o2 = eng.sol_gradient(*args, grad_mode=1)
    torch.cuda.synchronize()
    o1, o2, s1 = o1.cpu().numpy(), o2.cpu().numpy(), s1.cpu().numpy()
    assert np.all(np.isfinite(o1)) and np.array_equal(o1, o2)
    assert np.mean(s1[:, [0, 7, 8]] <= 1) >= 0.99
    fb = (s1[:, 0] <= 1) & np.all(s1[:, 1:7] == 6, axis=1)
    assert fb.mean() <= 0.05, fb.mean()
    rng = np.random.default_rng(11)
    idx = np.sort(rng.choice(4096, 32, replace=False))
    alone = eng.sol_gradient(*(a[idx] for a in args), grad_mode=1).cpu().numpy()
    assert np.array_equal(alone, o1[idx])
    sub = np.sort(rng.choice(4096, 256, replace=False))
    fd = eng.sol_gradient(*(a[sub] for a in args), grad_mode=0).cpu().numpy()
    assert np.array_equal(fd[:, 6:], o1[sub, 6:])


def test_fp32_twin_full_size(eng):
    """The fp32 twin at configs[2]'s batch size (SURVEY config 3 names fp32 buffers): 4096 float32 forward solves,
    every output equal to the fp64 entry point on the widened inputs rounded to float32 (statuses identical)."""
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(4096, seed=21)
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    ins = (f32(sb["ini"]), f32(sb["goal"]), f32(sb["dnn_out"][:, :3]), f32(sb["dnn_out"][:, 3:6]),
           f32(sb["dnn_out"][:, 6]))
    r32 = eng.ocp_solve(*ins, dtype=torch.float32)
    r64 = eng.ocp_solve(*(v.astype(np.float64) for v in ins))
    torch.cuda.synchronize()
    st = r32["status"].cpu().numpy()
    assert np.array_equal(st, r64["status"].cpu().numpy()) and np.mean(st <= 1) >= 0.99
    for k in ("x", "u", "lam", "cost"):
        assert np.array_equal(r32[k].cpu().numpy(), r64[k].cpu().numpy().astype(np.float32)), k


def test_configs3_shard_8192_samples(eng):
    """configs[3]'s per-GPU shard (65 536 episodes / 8 GPUs = 8 192 samples = 73 728 NLP solves) in one launch:
    every out8 finite, >= 99 % of the solves solved/acceptable, the seeded 64-sample subset re-solved alone
    reproduces its rows of the full launch bit for bit (no dependence on batch position or size), and the subset
    against the CPU oracle under grad_parity's bound (north_star: <= 1e-5 relative)."""
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(8192, seed=3)
    args = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    it = torch.full((8192, 9), -1, dtype=torch.int32, device=eng.device)
    eng.record_iters(it)
    try:
        o8, R9, s9 = eng.sol_gradient(*args, want_rewards=True)
        torch.cuda.synchronize()
    finally:
        eng.record_iters(None)
    o8, R9, s9, it = o8.cpu().numpy(), R9.cpu().numpy(), s9.cpu().numpy(), it.cpu().numpy()
    assert o8.shape == (8192, 8) and np.all(np.isfinite(o8))
    assert np.mean(s9 <= 1) >= 0.99, np.mean(s9 <= 1)
    assert np.all(it >= 0)
    idx = np.sort(np.random.default_rng(8).choice(8192, 64, replace=False))
    sub = tuple(a[idx] for a in args)
    alone = eng.sol_gradient(*sub).cpu().numpy()
    assert np.array_equal(alone, o8[idx])
    grad_parity(o8[idx], s9[idx], it[idx], sub, "configs[3] shard subset")


def test_last_inputs_scenario(eng, golden):
    """The scenario the reference ships in gym_pybullet_drone/last_inputs.npy (start, goal, yaw, gate width and
    pitch) through the GPU sol_gradient and get_input, against the oracle, with the trained DNN2's outputs
    on that scenario (moving.npz episode 0, nn3_1.pth; 12 from the episode + 52 on perturbed inputs) as the
    traversal parameters, under grad_parity's bound."""
    from learningagileflight_se3_amd import scenario as S
    from oracle import oracle as O
    s = golden("last_inputs")["inputs"]
    g = golden("moving")
    assert g["source"][0] == 0 and np.array_equal(g["inputs"][0], s)
    outs = np.ascontiguousarray(g["outs"][0], dtype=np.float32)          # (12, 7) DNN2 outputs, float32
    # 52 more traversal parameters: the trained DNN2 on the episode's 18-dim gate-frame inputs perturbed by
    # N(0, 0.05) (seeded), so that the oracle comparison covers 64 samples of this scenario
    from learningagileflight_se3_amd.policy_net import Network
    net = Network(18, 128, 128, 7)
    net.load_state_dict({k: torch.as_tensor(g[k.replace(".", "_")]) for k in net.state_dict()})
    rng = np.random.default_rng(64)
    ins = g["ins18"][0][rng.integers(0, 12, 52)] + rng.normal(0.0, 0.05, (52, 18))
    with torch.no_grad():
        more = net(torch.as_tensor(ins, dtype=torch.float32)).numpy()
    outs = np.ascontiguousarray(np.concatenate([outs, more]), dtype=np.float32)
    B = outs.shape[0]
    ini = np.repeat(S.initial_state(s[0:3], s[6]), B, 0)
    goal = np.repeat(s[None, 3:6], B, 0)
    gate12 = np.repeat(S.gate_corners(np.array([s[7]]), np.array([s[8]])), B, 0)
    it = torch.full((B, 9), -1, dtype=torch.int32, device=eng.device)
    eng.record_iters(it)
    try:
        o8, R9, S9 = eng.sol_gradient(ini, goal, gate12, outs, want_rewards=True)
        torch.cuda.synchronize()
    finally:
        eng.record_iters(None)
    o8, R9, S9, it = o8.cpu().numpy(), R9.cpu().numpy(), S9.cpu().numpy(), it.cpu().numpy()
    r8, rR, rS = O.sol_gradient(ini, goal, gate12, outs)
    assert np.array_equal(S9 <= 1, rS <= 1) and np.mean(S9 <= 1) >= 0.9
    ok = (S9 <= 1).all(1) & (rS <= 1).all(1)
    grad_parity(o8, S9, it, (ini, goal, gate12, outs), "last_inputs scenario (64 DNN2 outputs)")
    assert np.max(np.abs(o8[ok, 7] - r8[ok, 7]) / np.abs(r8[ok, 7])) < 1e-6
    # get_input on the scenario's initial state (float32 DNN outputs, t unrounded; quad_policy.py:202-211)
    u0, _ = eng.get_input(ini[:1], goal[:1], outs[:1])
    u0 = u0.cpu().numpy()
    nrm = np.float64(np.sqrt(np.float32(sum(np.float64(np.float32(c * c)) for c in outs[0, 3:6]))))
    q32 = O.rd2quat(outs[0, 3:6].astype(np.float64), nrm)[None]
    ref = O.solve(ini[:1], goal[:1], outs[:1, :3].astype(np.float64), q32, outs[:1, 6].astype(np.float64))
    assert np.max(np.abs(u0 - ref["u"][:, 0, :])) < 1e-6
