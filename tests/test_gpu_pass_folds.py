"""The stage-parallel passes around the Newton sweeps after their folds (ipm_kernel.hip): what each fold can break, at
the smallest shapes where it can.

Run on an MI355X:  python -m pytest tests/test_gpu_pass_folds.py -m gpu -q -s

1. Terminal rows of kkt_residual.  Lanes 1..N share one instruction stream; lane N reads u, lambda and lambda+ at a
   clamped stage index, drops the stage Hessian and A^T lambda+ it forms from them and keeps its own diagonal, the wqf
   block and g - lambda+_{N-1} + o.  The residual steers the refinement, so a wrong terminal row shows in the refined
   step: at N = 1, 2 and 3 lane N's rows are a half to a quarter of the x rows.  Samples 4..11 of
   synthetic_batch(64, seed=2025) (test_gpu_newton.py holds samples 0..3), iterations 0, 1 and 3, both parameter sets
   (wqf != 0 only at the generic one), the dense system of tests/newton.py at the kernel's own dumped point, and
   test_gpu_newton.py's assertions and margin: every refined ratio <= 1e-5, the largest refined and unrefined ratio at
   most MARGIN times the oracle's on the same cases.  At N = 50 the same check on the same 8 samples, iterations 1 and 3.

2. kkt_residual with soc = 1, where the defect loads are live (one uniform branch now): solves that take a second-order
   correction.  Chosen on the CPU from the oracle's trace: max_soc = 0 changes the trace of 15 of the 64 samples
   (1, 5, 14, 21, 22, 24, 34, 35, 49, 50, 51, 53, 54, 59, 62; the sweep counter, word 11, counts a correction's sweep
   whether or not its point is accepted); the test takes the first eight and asserts the change on every one of them.

3. The line search's powers pow(-gBD, 2.3) and pow(theta, 1.1), formed once per iteration at the reference point and
   again only on a watchdog trial.  watchdog = 1 and watchdog = 3 (default 10) on samples of the same batch.  Chosen on
   the CPU from the oracle's traces: against watchdog = 0 the trace changes (the watchdog started) on samples 5, 14, 22,
   24, 34, 53, 54 at watchdog = 1 and on 34, 54 at watchdog = 3; at watchdog = 1 every trial is accepted (the watchdog
   stops by acceptance, judged at the stored reference point); at watchdog = 3 sample 34 is twice back at its stored
   point (StopWatchDog: words theta, phi, gBD of iterations 76 and 91 are those of 73 and 88), where the powers of the
   stored point carry over to the line search.  The test asserts both kinds of coverage on the oracle before it looks
   at the device.

Items 2 and 3 compare with the oracle under the criteria of test_gpu_parity.py's
test_ocp_solve_matches_oracle_and_is_kkt: status <= 1 on both sides, exact iteration paths on at least the rounding
yardstick's count less 2 % of the solves, x and u within 1e-6 and the cost within 1e-10 on equal paths, multipliers
within 1e-6 of each instance's scale, every cost within 1e-6, and the KKT certificate of tests/kkt.py for every device
optimum.  On top of that, on the solves the yardstick admits (yardstick.solve_decisions; all of the listed ones when
they were chosen) the device takes the oracle's decisions at every iteration (mu, delta_w, accepted, filter size,
step halvings: test_gpu_options.py's comparison).

First run (MI355X): every device solve on the oracle's iteration path (8/8, 8/8, 4/4; the yardstick the same), the
decisions compared on all 20 solves; largest residual ratios of the terminal-row cases, GPU / oracle:

    set      N    cases   unrefined                refined
    default  1    24      4.232e-16 / 2.742e-16    5.869e-17 / 8.556e-17
    default  2    24      5.049e-16 / 3.395e-16    5.049e-16 / 3.395e-16
    default  3    24      5.451e-16 / 4.520e-16    5.474e-16 / 5.091e-16
    default  50   16      3.008e-15 / 3.051e-13    8.878e-16 / 8.817e-16
    generic  1    24      1.198e-16 / 1.008e-16    9.179e-17 / 1.008e-16
    generic  2    24      6.896e-16 / 4.284e-16    6.896e-16 / 4.284e-16
    generic  3    24      6.365e-16 / 5.058e-16    5.015e-16 / 4.130e-16
    generic  50   16      1.505e-14 / 5.183e-13    4.520e-16 / 3.781e-16

Mutation check (builds not kept, each run once on the tests named).  Lane N run as a stage lane (`term` always
false): all eight terminal-row tests fail.  delta_w dropped from the terminal diagonal of rows 0..2: both N = 50 tests
fail, the six short-horizon ones pass (no dumped iteration there needs a delta_w).  The defect loads skipped with
soc = 1: the second-order-correction test fails.  The powers of a watchdog trial left at zero: both watchdog tests
fail, and only on the filter size among the decision words; the iteration counts stay the oracle's, so the criteria
of test_ocp_solve_matches_oracle_and_is_kkt alone had passed that build.
"""
import numpy as np
import pytest
import yardstick

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import generic_params as GP  # noqa: E402
import newton_cases as NC  # noqa: E402
from newton_gpu import decisions, engine, gpu_run, oracle_traced, step_solves_the_dense_system  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLES = tuple(range(4, 12))         # 8 instances per launch
SOC_SAMPLES = (1, 5, 14, 21, 22, 24, 34, 35)
WATCHDOG = {1: (5, 14, 22, 24, 34, 53, 54, 0), 3: (34, 54, 5, 14)}   # option value -> samples


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def dense_check(batch, N, pset, last_iteration):
    """test_gpu_newton.py's test_step_solves_the_dense_system on SAMPLES; `last_iteration` + 2 stands in for the
    solve's length in newton_cases.dump_iterations (iterations 0, 1, 3 at the short horizons, 1 and 3 at N = 50)."""
    prob = GP.problem(batch, N, SAMPLES, pset)
    full = NC.oracle_full(prob, N)["iters"]
    assert np.all(full >= last_iteration + 2), (N, pset, full)   # every dumped iteration is one the solve takes
    iters = np.full(len(SAMPLES), last_iteration + 2)
    ocases = NC.collect(NC.oracle_run, prob, N, iters)
    gcases = NC.collect(gpu_run, prob, N, iters)
    if N == 50:   # iteration 0 is the least-squares start on every side: one launch pair less
        ocases = {c: v for c, v in ocases.items() if c[1] > 0}
        gcases = {c: v for c, v in gcases.items() if c[1] > 0}
    assert set(ocases) == set(gcases) and len(gcases) >= 2 * len(SAMPLES)
    step_solves_the_dense_system(f"{pset} N={N}", f"/folds/{pset}", prob, N, ocases, gcases)
    NC.structure(prob, N, gcases)


@pytest.mark.parametrize("pset", list(GP.SETS))
@pytest.mark.parametrize("N", (1, 2, 3))
def test_terminal_rows_at_short_horizons(batch, N, pset):
    dense_check(batch, N, pset, 3)


@pytest.mark.parametrize("pset", list(GP.SETS))
def test_terminal_rows_at_the_full_horizon(batch, pset):
    dense_check(batch, 50, pset, 3)


# ---- items 2 and 3: whole solves against the oracle -------------------------------------------------------------
def problem(batch, idx):
    from oracle import oracle as O
    i = np.asarray(idx)
    d = batch["dnn_out"][i].astype(np.float64)
    return {"ids": i, "ini": batch["ini"][i], "goal": batch["goal"][i], "p": d[:, :3], "a": d[:, 3:6],
            "q": np.stack([O.rd2quat(a) for a in d[:, 3:6]]), "t": d[:, 6].copy()}


def option_changes(prob, opts, other):
    """Oracle alone: (solve with opts, its trace, per sample whether the trace differs from the solve with `other`)."""
    from oracle import oracle as O
    ref, tr = oracle_traced(prob, O.default_params(horizon=50, **opts))
    ro, _ = oracle_traced(prob, O.default_params(horizon=50, **other))
    TI = max(tr.shape[1], int(ro["iters"].max()) + 1)
    _, tr = oracle_traced(prob, O.default_params(horizon=50, **opts), TI)
    _, tro = oracle_traced(prob, O.default_params(horizon=50, **other), TI)
    return ref, tr, np.any(tr != tro, axis=(1, 2))


def back_at_stored_point(tr, iters):
    """Iterations j of one solve's trace whose reference point (theta, phi, gBD: words 2..4) is exactly that of an
    iteration i < j - 1: the watchdog gave up its trial steps and resumed the point it had stored."""
    return [j for j in range(2, int(iters)) if any(np.array_equal(tr[j, 2:5], tr[i, 2:5]) for i in range(j - 1))]


def solve_matches_oracle(label, prob, opts, ref, otr):
    """The criteria of test_gpu_parity.py's test_ocp_solve_matches_oracle_and_is_kkt on the solves of prob, and on the
    solves that the rounding yardstick admits (the oracle's FMA build takes its strict build's decisions) also the
    decision words of every iteration, as test_gpu_options.py compares them: the switching condition decides
    whether an accepted step enters the filter, which the iteration count alone need not show (with the watchdog
    trial's powers left at zero the oracle's filter size changes on samples 5, 14, 24, 34, 53, 54 at watchdog = 1 and
    on 54 at watchdog = 3, and no iteration count does)."""
    from oracle import oracle as O
    import kkt
    e = engine(50, opts)
    gtr = torch.zeros((len(prob["ids"]), otr.shape[1], 16), dtype=torch.float64, device=e.device)
    e.debug_trace(gtr, otr.shape[1])
    try:
        out = e.ocp_solve(*(prob[k] for k in ("ini", "goal", "p", "a", "t")))
        torch.cuda.synchronize()
    finally:
        e.debug_trace(None)
    g = {k: v.cpu().numpy() for k, v in out.items()}
    gtr = gtr.cpu().numpy()
    n = len(prob["ids"])
    args = tuple(prob[k] for k in ("ini", "goal", "p", "q", "t"))
    params = O.default_params(horizon=50, **opts)
    assert np.all(g["status"] <= 1) and np.all(ref["status"] <= 1), (label, g["status"], ref["status"])
    same = g["iters"] == ref["iters"]
    yard = yardstick.solve_paths(args, {"params": params}, ref)
    kept = yardstick.solve_decisions(args, {"params": params}, ref)
    print(f"{label}: samples {prob['ids'].tolist()}, oracle iterations {ref['iters'].tolist()}, device "
          f"{g['iters'].tolist()}; same iteration path {int(same.sum())}/{n} (rounding yardstick {yard}/{n}); "
          f"decisions compared on {prob['ids'][kept].tolist()}")
    assert same.sum() >= yard - 0.02 * n, (label, "iteration paths differ", g["iters"], ref["iters"], yard)
    assert kept.sum() >= n // 2, (label, "the yardstick admits too few of the listed samples", kept)
    dg, do = decisions(gtr), decisions(otr)
    for j in np.nonzero(kept)[0]:
        m = int(ref["iters"][j])
        assert g["status"][j] == ref["status"][j] and g["iters"][j] == m, (label, int(prob["ids"][j]))
        bad = np.argwhere(dg[j, :m] != do[j, :m])
        assert bad.size == 0, (label, int(prob["ids"][j]), "first differing (iteration, word)", bad[0].tolist(),
                               dg[j, bad[0][0]].tolist(), do[j, bad[0][0]].tolist())
    for k in ("x", "u"):
        d = np.abs(g[k][same] - ref[k][same]) / (1 + np.abs(ref[k][same]))
        assert d.max() < 1e-6, (label, k, d.max())
    assert np.max(np.abs(g["cost"][same] - ref["cost"][same]) / np.abs(ref["cost"][same])) < 1e-10, label
    dl = np.abs(g["lam"][same] - ref["lam"][same]).reshape(int(same.sum()), -1).max(1)
    assert np.max(dl / (1 + np.abs(ref["lam"][same]).reshape(int(same.sum()), -1).max(1))) < 1e-6, label
    assert np.max(np.abs(g["cost"] - ref["cost"]) / np.abs(ref["cost"])) < 1e-6, label
    bad = []
    for i in range(n):
        r = kkt.kkt_residual(g["x"][i], g["u"][i], g["lam"][i], prob["ini"][i], prob["goal"][i], prob["p"][i],
                             prob["q"][i], prob["t"][i])
        if not (r["primal"] <= 5e-7 and r["dual"] <= 1e-4 * r["s_d"] and r["compl"] <= 1e-6):
            bad.append((int(prob["ids"][i]), r))
    assert not bad, (label, bad)


def test_second_order_correction_solves_match_the_oracle(batch):
    prob = problem(batch, SOC_SAMPLES)
    ref, tr, changed = option_changes(prob, {}, {"max_soc": 0})
    print(f"second-order corrections: max_soc = 0 changes the oracle's trace on samples {prob['ids'][changed].tolist()}")
    assert np.all(changed), ("a listed sample takes no second-order correction any more", prob["ids"][~changed])
    solve_matches_oracle("soc", prob, {}, ref, tr)


@pytest.mark.parametrize("wd", list(WATCHDOG))
def test_watchdog_solves_match_the_oracle(batch, wd):
    prob = problem(batch, WATCHDOG[wd])
    ref, tr, started = option_changes(prob, {"watchdog": wd}, {"watchdog": 0})
    back = [len(back_at_stored_point(tr[b], ref["iters"][b])) for b in range(len(started))]
    print(f"watchdog = {wd}: it starts on samples {prob['ids'][started].tolist()}; returns to the stored point per "
          f"sample {dict(zip(prob['ids'].tolist(), back))}")
    if wd == 1:     # seven solves in which it starts, and every trial accepted at the stored reference point
        assert started.sum() >= 7 and sum(back) == 0, (started, back)
    else:           # a solve that gives up its trials and resumes the stored point, more than once
        assert started.sum() >= 2 and max(back) >= 2, (started, back)
    solve_matches_oracle(f"watchdog={wd}", prob, {"watchdog": wd}, ref, tr)
