"""GPU tests of the restoration phase (ipm_kernel.hip / resto.inc) against the oracle (oracle/lafse3_oracle.c
orc_restoration) on tests/golden/resto.npz: the NLP instances whose filter line search fails -- 18 samples of the
configs[2] bench batch (synthetic_batch(4096, seed 1000); 162 sol_gradient solves) and 64 moving-gate MPC solves
of configs[4] (lafse3_get_input, quad_policy.py:202-211).

  * restoration = 0 (the 0.4 solver) reproduces the oracle's line-search failures on the device;
  * restoration = 1 (default): no instance ends in a line-search failure, the restoration counters report the
    phase's entries and returns, statuses / iteration counts agree with the oracle's, and where both took the
    same iteration path the rewards / trajectories agree to the A5 tolerances.
The restored solves are certified as KKT points of the reference NLP by tests/test_restoration_host.py (oracle
side); here the device has to follow the oracle onto them.

The exits of the phase (test_infeasible_exit and below) run on the yaw family of resto_newton_cases.py at N = 50, 7, 3,
2, 1: statuses 9 and "max_iter inside the phase" (2), the rule that the outputs then hold the point where the phase
started, the successful return at every horizon (the first entries of the same solves), and the other entry points.
Two things are not as the issue that asked for these tests assumed, both established with the oracle
(test_resto_newton_host.py):
  * a yaw solve enters the phase two or three times, the first entries returning after one or two iterations, so
    `last_resto_counters` must report the oracle's entries (7, 7, 7, 7, 6 for the three instances at N = 50, 7, 3, 2, 1)
    and entries - 3 returns, not 3 and 0; the start point the outputs hold is the last entry's, and it is compared
    after the projection onto the original bounds that every output gets (honor_original_bounds);
  * the N = 50 roll / pitch instances (7.2, 0, 0), (7.6, 0, 0), (0, 8.0, 0) are solved with status 0 without entering
    the phase at all, so `entries >= 1` cannot be asked of them: they are held to status <= 1, returns == entries, the
    KKT certificate and the oracle's result, and returns >= 1 is asserted where returns exist, on the yaw family.
Searched for and not found (oracle, CPU, about ten minutes of sweeps): status 8 (none among the yaw sweeps above, the
roll and pitch sweeps 6.0 .. 9.4 in steps of 0.2 at N = 50, nor with watchdog = 0, max_soc = 0 or lsq_mult_init = 0 on
the roll / pitch instances).  A short-horizon instance whose SOLVE ends solved after a restoration phase was not
searched further: the phase's successful-return path itself runs at every horizon, in the first entries of the yaw
solves.  No solver constant was changed to make a case.
"""
import numpy as np
import pytest
import yardstick

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("resto")


def _engine(**overrides):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import _lib
    from learningagileflight_se3_amd.engine import Engine
    e = Engine()
    if overrides:
        e.set_params(_lib.default_params(**overrides))
    return e


def _bench_args(g):
    return (g["bench_ini"], g["bench_goal"], g["bench_gate12"], g["bench_dnn_out"])


def test_without_restoration_the_failures_reproduce(g):
    """restoration = 0: the device ends the oracle's line-search failures (restoration = 0) in line-search failures
    too, at least as many of them as the oracle's own FMA-contracted build does (the rounding yardstick,
    tests/yardstick.py: 8 of the 10).  Round 4's VALU stage reproduced 10 of 10, the MFMA stage 9 or 10: a
    line-search failure is the end of a long ill-conditioned path whose near-tie decisions rounding moves."""
    from oracle import oracle as O
    e = _engine(restoration=0)
    _, _, S9 = e.sol_gradient(*_bench_args(g), want_rewards=True)
    e.close()
    S9 = S9.cpu().numpy()
    prm = O.default_params(restoration=0)
    _, _, so = O.sol_gradient(*_bench_args(g), params=prm)
    _, _, sf = O.sol_gradient(*_bench_args(g), params=prm, fast=True)
    fail_o = so == 3
    yard = int((fail_o & (sf == 3)).sum())
    print(f"restoration=0: oracle ls_fail {fail_o.sum()}, device ls_fail {(S9 == 3).sum()}, "
          f"both {(fail_o & (S9 == 3)).sum()} (rounding yardstick: oracle FMA build {yard})")
    assert fail_o.sum() >= 10
    assert (fail_o & (S9 == 3)).sum() >= yard
    # regression bar: the count this kernel measured (9 of 10 since the MFMA stage, profiles/r05_*), so that a
    # drift towards the yardstick's floor shows up as a failure instead of passing silently
    assert (fail_o & (S9 == 3)).sum() >= 9, (fail_o & (S9 == 3)).sum()


def test_bench_failures_restored_on_device(g):
    """restoration = 1 on the 162 bench-fixture solves: every status solved/acceptable (the oracle's are), the
    restoration counters show entries == returns >= 10, and on the solves that take the oracle's iteration count the
    nine rewards agree to 1e-6 (relative).  How many solves take the oracle's exact iteration path is judged against
    the rounding yardstick (tests/yardstick.py): the oracle built with FMA contraction against its strict build on
    the same jobs (157 / 162 measured round 4) -- the device must reach that count minus 2 % of the jobs.  Every
    remaining divergence is preceded by rounding-level drift of theta / phi (tools/resto_diverge.py,
    profiles/r04_resto_diverge.log), so a fixed fraction would judge the rounding, not the solver."""
    from oracle import oracle as O
    e = _engine()
    it = torch.full((18, 9), -1, dtype=torch.int32, device=e.device)
    e.record_iters(it)
    o8, R9, S9 = e.sol_gradient(*_bench_args(g), want_rewards=True)
    rc = e.last_resto_counters()
    e.record_iters(None)
    e.check_device()
    R9, S9, it = R9.cpu().numpy(), S9.cpu().numpy(), it.cpu().numpy()
    e.close()
    ito = np.zeros((18, 9), np.int32)
    o8o, Ro, So = O.sol_gradient(*_bench_args(g), iters=ito)
    same = (S9 == So) & (it == ito)
    yard = yardstick.grad_paths(_bench_args(g), So, ito)
    print(f"device statuses {dict(zip(*np.unique(S9, return_counts=True)))}, resto {rc}, "
          f"same status+iterations {same.sum()}/162 (rounding yardstick: oracle FMA build {yard}/162)")
    _, _, s0 = O.sol_gradient(*_bench_args(g), params=O.default_params(restoration=0))
    restored = s0 == 3
    print(f"restored jobs: device iterations {it[restored].tolist()}, oracle {ito[restored].tolist()}")
    assert np.all(S9 <= 1), dict(zip(*np.unique(S9, return_counts=True)))
    assert np.all(np.isfinite(R9)) and np.all(np.isfinite(o8.cpu().numpy()))
    assert rc["resto_entries"] >= 10 and rc["resto_returns"] == rc["resto_entries"], rc
    assert same.sum() >= yard - 0.02 * same.size, (same.sum(), yard)
    d = np.abs(R9[same] - Ro[same]) / (1.0 + np.abs(Ro[same]))
    assert d.max() < 1e-6, d.max()


def test_moving_gate_failures_restored_on_device(g):
    """The 64 configs[4] get_input solves: restoration = 1 leaves no line-search failure (the round-2 solver failed
    >= 90 % of them); every device trajectory matches the oracle's KKT-certified one to 1e-5 (relative) whatever
    the iteration path, and the count that takes the oracle's iteration path exactly reaches the rounding yardstick
    minus 2 % of the solves (tests/yardstick.py).  These solves run 30-440 iterations through one or more restoration
    phases, and rounding alone moves their paths: the oracle built with FMA contraction takes its own strict build's
    path on only 42 / 64 (tools/resto_diverge.py); the device, with the oracle's float32 input semantics and mu
    sequence bit for bit since round 4, on 40 / 64 (round 3: 36), each divergence after a drift that starts at the
    rounding level (profiles/r04_resto_diverge.log)."""
    from oracle import oracle as O
    e = _engine()
    B = len(g["moving_ini"])
    it = torch.full((B,), -1, dtype=torch.int32, device=e.device)
    e.record_iters(it)
    _, x, st = e.get_input(g["moving_ini"], g["moving_goal"], g["moving_dnn_out"], u_last=g["moving_u_last"],
                           want_x=True)
    rc = e.last_resto_counters()
    e.record_iters(None)
    x, st, it = x.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    e.close()
    dn = g["moving_dnn_out"]
    nrm = [np.float64(np.sqrt(np.float32(sum(np.float64(np.float32(c * c)) for c in v)))) for v in dn[:, 3:6]]
    q32 = np.stack([O.rd2quat(v.astype(np.float64), n) for v, n in zip(dn[:, 3:6], nrm)])
    ref = O.solve(g["moving_ini"], g["moving_goal"], dn[:, :3].astype(np.float64), q32, dn[:, 6].astype(np.float64),
                  ulast=g["moving_u_last"])
    same = (st == ref["status"]) & (it == ref["iters"])
    yard = yardstick.solve_paths((g["moving_ini"], g["moving_goal"], dn[:, :3].astype(np.float64), q32,
                                  dn[:, 6].astype(np.float64)), dict(ulast=g["moving_u_last"]), ref)
    print(f"moving: device statuses {dict(zip(*np.unique(st, return_counts=True)))}, resto {rc}, "
          f"same path {same.sum()}/{B} (rounding yardstick: oracle FMA build {yard}/{B})")
    assert np.all(st <= 1), dict(zip(*np.unique(st, return_counts=True)))
    assert rc["resto_entries"] >= 0.5 * B and rc["resto_returns"] == rc["resto_entries"], rc
    assert same.sum() >= yard - 0.02 * B, (same.sum(), yard)
    d = np.abs(x - ref["x"]) / (1.0 + np.abs(ref["x"]))
    assert d.max() < 1e-5, d.max()


# ---- the exits of the phase on the yaw family (resto_newton_cases.py)
import resto_newton as RN  # noqa: E402
import resto_newton_cases as RC  # noqa: E402


def _oracle_full(prob, N, **kw):
    from oracle import oracle as O
    return O.solve(prob["ini"], prob["goal"], prob["p"], prob["q"], prob["t"], params=O.default_params(horizon=N, **kw))


def _start_point_outputs(prob, N, entries, max_iter=None):
    """Every sample solved with the dump of (its last entry, iteration 0) armed: (outputs, start points as returned,
    counters of the launch with every sample in it)."""
    B = len(entries)
    outs, pts = {}, {}
    for e in sorted({len(en) - 1 for en in entries}):
        rec, cnt, out = RC.gpu_run(prob, N, e, 0, 0, np.arange(B), max_iter)
        for s in range(B):
            if len(entries[s]) - 1 == e:
                sc = RN.split_record(rec[s], N)
                assert sc[3]["written"] == 1.0 and sc[4]["iters_before"] == entries[s][e][0], (N, s, e, sc[4])
                outs[s] = {k: v[s] for k, v in out.items()}
                pts[s] = RC.honoured(sc[1])
    return outs, pts, cnt


@pytest.mark.parametrize("N", RC.HORIZONS)
def test_infeasible_exit(N):
    """Status 9 on the device: iteration counts and restoration counters as the oracle's, finite outputs equal to the
    oracle's to 1e-9, and x, u bit for bit the point where the (last) entry into the phase started."""
    prob, entries = RC.yaw(N), RC.ENTRIES[("default", N)]
    B = len(entries)
    ref = _oracle_full(prob, N)
    outs, pts, cnt = _start_point_outputs(prob, N, entries)
    st = np.array([outs[s]["status"] for s in range(B)])
    it = np.array([outs[s]["iters"] for s in range(B)])
    print(f"N={N}: status {st.tolist()} iters {it.tolist()} oracle {ref['iters'].tolist()} counters {cnt}")
    assert np.all(st == 9) and np.all(ref["status"] == 9), (st, ref["status"])
    n_ent = sum(len(en) for en in entries)
    assert cnt == {"resto_entries": n_ent, "resto_returns": n_ent - B} and n_ent - B >= B, (cnt, n_ent)
    same = it == ref["iters"]
    if N <= 7:
        assert np.all(same), (it, ref["iters"])      # solves of at most 31 iterations
    else:
        yard = yardstick.solve_paths(tuple(prob[k] for k in ("ini", "goal", "p", "q", "t")), {}, ref)
        assert same.sum() >= yard - 0.02 * B, (it, ref["iters"], yard)
    for s in range(B):
        o = outs[s]
        for f in ("x", "u", "lam"):
            assert np.all(np.isfinite(o[f])), (N, s, f)
            if same[s]:
                d = np.max(np.abs(o[f] - ref[f][s])) / max(1.0, np.max(np.abs(ref[f][s])))
                assert d <= 1e-9, (N, s, f, d)
        assert np.isfinite(o["cost"])
        assert np.array_equal(o["x"], pts[s][0]) and np.array_equal(o["u"], pts[s][1]), (N, s, "start point")


@pytest.mark.parametrize("N", (50, 2))
def test_iteration_limit_inside_the_phase(N):
    """max_iter = 10 with wz = 25: the limit falls inside the last entry; status 2 after 10 iterations, the outputs
    the point where that entry started."""
    i = RC.YAW.index(RC.MAXITER_WZ)
    prob, entries = RC.yaw(N, wz=(RC.MAXITER_WZ,)), (RC.ENTRIES[("default", N)][i],)
    assert entries[0][-1][0] < RC.MAXITER < sum(entries[0][-1])
    ref = _oracle_full(prob, N, max_iter=RC.MAXITER)
    outs, pts, cnt = _start_point_outputs(prob, N, entries, RC.MAXITER)
    o = outs[0]
    assert o["status"] == 2 and o["iters"] == RC.MAXITER and ref["status"][0] == 2 and ref["iters"][0] == RC.MAXITER
    assert cnt == {"resto_entries": len(entries[0]), "resto_returns": len(entries[0]) - 1}, cnt
    assert np.array_equal(o["x"], pts[0][0]) and np.array_equal(o["u"], pts[0][1])
    for f in ("x", "u", "lam"):
        d = np.max(np.abs(o[f] - ref[f][0])) / max(1.0, np.max(np.abs(ref[f][0])))
        assert d <= 1e-9, (N, f, d)


def test_roll_pitch_instances_are_solved():
    """N = 50, omega_0 = (7.2, 0, 0), (7.6, 0, 0), (0, 8.0, 0): status <= 1, every entry into the phase returned (the
    oracle enters it on none of them), the result passes the KKT certificate at test_restoration_host.py's thresholds
    and agrees with the oracle to 1e-5 relative."""
    import kkt
    prob = RC.problem(50, RC.ROLL_PITCH)
    ref = _oracle_full(prob, 50)
    _, cnt, out = RC.gpu_run(prob, 50, 0, 0, 0, np.arange(len(RC.ROLL_PITCH)))
    print(f"roll / pitch: status {out['status'].tolist()} iters {out['iters'].tolist()} oracle "
          f"{ref['iters'].tolist()} counters {cnt}")
    assert np.all(out["status"] <= 1) and cnt["resto_returns"] == cnt["resto_entries"], (out["status"], cnt)
    for s in range(len(RC.ROLL_PITCH)):
        k = kkt.kkt_residual(out["x"][s], out["u"][s], out["lam"][s], prob["ini"][s], prob["goal"][s], prob["p"][s],
                             prob["q"][s], prob["t"][s])
        assert k["primal"] <= 5e-7 and k["dual"] <= 1e-4 * k["s_d"] and k["compl"] <= 1e-6 and k["bound_viol"] <= 0, k
        for f in ("x", "u"):
            d = np.max(np.abs(out[f][s] - ref[f][s]) / (1.0 + np.abs(ref[f][s])))
            assert d <= 1e-5, (s, f, d)


@pytest.mark.parametrize("N", RC.HORIZONS)
def test_infeasible_exit_through_the_other_entry_points(N):
    """The yaw instances through lafse3_ocp_sensitivity_ex: status 9, sens_status 1, dx, du and gain zero; through
    lafse3_ocp_solve_f32: status 9."""
    prob = RC.yaw(N)
    e = RC.engine(N)
    args = tuple(prob[k] for k in ("ini", "goal", "p", "a", "t"))
    r = e.ocp_sensitivity_ex(*args)
    assert np.all(r["status"].cpu().numpy() == 9) and np.all(r["sens_status"].cpu().numpy() == 1)
    for f in ("dx", "du", "gain"):
        assert not np.any(r[f].cpu().numpy()), (N, f)
    r32 = e.ocp_solve(*args, dtype=torch.float32)
    assert np.all(r32["status"].cpu().numpy() == 9), r32["status"]
    assert all(np.all(np.isfinite(r32[f].cpu().numpy())) for f in ("x", "u", "lam"))
