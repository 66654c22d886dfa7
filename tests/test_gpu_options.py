"""The solver options of lafse3_params on the device, one changed at a time at the reference's model, against the CPU
oracle given the same option.  Before this file only horizon, max_iter, grad_mode, costate_option and restoration had
reached a kernel at a non-default value.

Run on an MI355X:  python -m pytest tests/test_gpu_options.py -m gpu -q -s

Admission, decided from the oracle alone: an option is tested on the samples where it changes the oracle's own solve
relative to the default options (another status, iteration count or debug trace) and where the oracle's FMA build takes
the strict build's decisions with that option set (yardstick.solve_decisions).  On those samples the device must give
the oracle's status and iteration count, its trace words 0 (mu), 8 (delta_w), 9 (accepted), 10 (filter size) and its
number of step halvings at every iteration, x and u within 1e-6 and the cost within 1e-10 (test_gpu_parity.py's bounds
on equal paths).  Every case needs at least MIN_SAMPLES admitted samples: a case that admits fewer fails instead of
passing on nothing.

Inputs: scenario.synthetic_batch(64, seed=2025) with its own t at N = 50 and t = 0.5 N dt at N = 20, u_last none; for the
watchdog solves of tests/golden/resto.npz (18 samples x 9 probes), where test_restoration_host.py shows that it
matters.  Each case lists its candidate samples; the test decides admission among them and prints it.

Found on the CPU with the oracle (positions in the 64-sample batch; "changes" = another status, iteration count or trace):
    lsq_mult_init = 0   changes 8 of the first 8 at N = 50 and N = 20; N = 20 sample 6 fails the yardstick: 8 and 7 admitted
    max_soc = 0         N = 50: changes 15 of 64 (1, 5, 14, 21, 22, 24, 34, 35, 49, 50, 51, 53, 54, 59, 62), all kept;
                        N = 20: changes 14 of 64 (0, 6, 7, 18, 21, 25, 28, 31, 33, 40, 45, 55, 57, 61), 12 kept (not 6,
                        45); the first eight of each list are the candidates: 8 and 7 admitted
    mu_init = 1, bound_relax = 1e-6, tol = 1e-6 with acceptable_tol = 1e-4: each changes 8 of 8 (bound_relax moves the
                        decision words on 2 of them, the continuous words on all), 8 admitted
    acceptable_iter = 3 with tol = 1e-13: status 1 on all 8, 6 admitted (3 and 4 fail the yardstick)
    watchdog = 0        changes 1 of 64 batch samples (34) but 58 of the fixture's 162 solves, 47 of them kept; the
                        candidates are the eight shortest of those (73 .. 87 iterations)
"""
import numpy as np
import pytest
import yardstick

torch = pytest.importorskip("torch")

from newton_gpu import decisions, oracle_traced  # noqa: E402

pytestmark = pytest.mark.gpu

MIN_SAMPLES = 2
WATCHDOG_JOBS = (13, 35, 40, 111, 113, 116, 143, 159)
FIRST8 = tuple(range(8))
# name -> (horizon, option fields, candidate samples)
CASES = {
    "lsq_mult_init=0 N=50": (50, {"lsq_mult_init": 0}, FIRST8),
    "lsq_mult_init=0 N=20": (20, {"lsq_mult_init": 0}, FIRST8),
    "max_soc=0 N=50": (50, {"max_soc": 0}, (1, 5, 14, 21, 22, 24, 34, 35)),
    "max_soc=0 N=20": (20, {"max_soc": 0}, (0, 6, 7, 18, 21, 25, 28, 31)),
    "mu_init=1": (50, {"mu_init": 1.0}, FIRST8),
    "bound_relax=1e-6": (50, {"bound_relax": 1e-6}, FIRST8),
    "tol=1e-6 acceptable_tol=1e-4": (50, {"tol": 1e-6, "acceptable_tol": 1e-4}, FIRST8),
    "acceptable_iter=3 tol=1e-13": (50, {"acceptable_iter": 3, "tol": 1e-13}, FIRST8),
}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def problem(batch, N, idx):
    from oracle import oracle as O
    i = np.asarray(idx)
    d = batch["dnn_out"][i].astype(np.float64)
    t = d[:, 6].copy() if N == 50 else np.full(len(i), 0.5 * N * 0.1)
    return {"ids": i, "ini": batch["ini"][i], "goal": batch["goal"][i], "p": d[:, :3], "a": d[:, 3:6],
            "q": np.stack([O.rd2quat(a) for a in d[:, 3:6]]), "t": t}


def admit(prob, N, opts):
    """Oracle alone: (option solve, its trace, admitted samples, samples the option changes, samples kept by the
    yardstick)."""
    from oracle import oracle as O
    args = tuple(prob[k] for k in ("ini", "goal", "p", "q", "t"))
    base = O.solve(*args, params=O.default_params(horizon=N))
    popt = O.default_params(horizon=N, **opts)
    ref, tr = oracle_traced(prob, popt)
    _, tr0 = oracle_traced(prob, O.default_params(horizon=N), TI=tr.shape[1])
    changed = (base["status"] != ref["status"]) | (base["iters"] != ref["iters"]) | np.any(tr != tr0, axis=(1, 2))
    kept = yardstick.solve_decisions(args, {"params": popt}, ref)
    return ref, tr, changed & kept, changed, kept


def device_traced(prob, N, opts, idx, TI):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(horizon=N, **opts)
    tr = torch.zeros((len(idx), TI, 16), dtype=torch.float64, device=e.device)
    e.debug_trace(tr, TI)
    try:
        out = e.ocp_solve(*(prob[k][idx] for k in ("ini", "goal", "p", "a", "t")))
        torch.cuda.synchronize()
    finally:
        e.debug_trace(None)
    return {k: v.cpu().numpy() for k, v in out.items()}, tr.cpu().numpy()


def compare(label, prob, N, opts, ref, otr, idx):
    """The assertions of this file on the admitted samples idx (positions in prob)."""
    assert len(idx) >= MIN_SAMPLES, (
        label, "the oracle admits", len(idx), "of the candidate samples listed in this file: the oracle's paths have "
        "changed since they were chosen, so derive the candidates again (solve the whole batch / fixture with and "
        "without the option on the CPU, as the docstring describes) before looking at the device")
    g, gtr = device_traced(prob, N, opts, idx, otr.shape[1])
    print(f"{label}: {len(idx)} solves ({prob['ids'][idx].tolist()}), oracle status {ref['status'][idx].tolist()} iterations "
          f"{ref['iters'][idx].tolist()}; device status {g['status'].tolist()} iterations {g['iters'].tolist()}")
    assert np.array_equal(g["status"], ref["status"][idx]), label
    assert np.array_equal(g["iters"], ref["iters"][idx]), label
    dg, do = decisions(gtr), decisions(otr[idx])
    for j in range(len(idx)):
        n = int(ref["iters"][idx[j]])
        bad = np.argwhere(dg[j, :n] != do[j, :n])
        assert bad.size == 0, (label, int(prob["ids"][idx[j]]), "first differing (iteration, word)", bad[0].tolist(),
                               dg[j, bad[0][0]].tolist(), do[j, bad[0][0]].tolist())
    for k in ("x", "u"):
        d = np.abs(g[k] - ref[k][idx]) / (1 + np.abs(ref[k][idx]))
        assert d.max() < 1e-6, (label, k, d.max())
    dc = np.max(np.abs(g["cost"] - ref["cost"][idx]) / np.abs(ref["cost"][idx]))
    print(f"{label}: largest relative cost difference {dc:.3e}")
    assert dc < 1e-10, (label, dc)


@pytest.mark.parametrize("case", list(CASES))
def test_option_on_the_device_follows_the_oracle(batch, case):
    N, opts, cand = CASES[case]
    prob = problem(batch, N, cand)
    ref, tr, adm, changed, kept = admit(prob, N, opts)
    print(f"{case}: the option changes {int(changed.sum())} of {len(changed)} oracle solves "
          f"(samples {prob['ids'][changed].tolist()}), the yardstick keeps {int(kept.sum())}; admitted samples "
          f"{prob['ids'][adm].tolist()}")
    if case.startswith("acceptable_iter"):
        assert np.all(ref["status"] == 1), ref["status"]        # the option is what ends these solves
    idx = np.nonzero(adm)[0][:8]                                # eight solves are enough for one launch
    compare(case, prob, N, opts, ref, tr, idx)


def resto_fixture_problems(g):
    """The 18 x 9 sol_gradient jobs of the restoration fixture as plain solves: p and t of each probe as the oracle's
    grad_params gives them, the probe's angle vector widened to float64 (+ 1e-3 on one entry for probes 4..6) and
    its quaternion from the float64 norm, which is how lafse3_ocp_solve reads an angle vector."""
    from oracle import oracle as O
    dnn = g["bench_dnn_out"]
    B = dnn.shape[0]
    pp, _, tt, _ = O.grad_params(dnn)
    a = np.repeat(dnn[:, None, 3:6].astype(np.float64), 9, axis=1)
    for j in (4, 5, 6):
        a[:, j, j - 4] += 1e-3
    a = a.reshape(B * 9, 3)
    return {"ini": np.repeat(g["bench_ini"], 9, axis=0), "goal": np.repeat(g["bench_goal"], 9, axis=0),
            "p": pp.reshape(B * 9, 3), "a": a, "q": np.stack([O.rd2quat(v) for v in a]), "t": tt.reshape(B * 9)}


def test_watchdog_off_on_the_device_follows_the_oracle(golden):
    """watchdog = 0 on solves of the restoration fixture (job = 9 sample + probe) that it changes."""
    prob = resto_fixture_problems(golden("resto"))
    prob = {k: v[list(WATCHDOG_JOBS)] for k, v in prob.items()}
    prob["ids"] = np.array(WATCHDOG_JOBS)
    ref, tr, adm, changed, kept = admit(prob, 50, {"watchdog": 0})
    print(f"watchdog=0: the option changes {int(changed.sum())} of {len(changed)} oracle solves "
          f"(jobs {prob['ids'][changed].tolist()}), the yardstick keeps {int(kept.sum())}; admitted jobs "
          f"{prob['ids'][adm].tolist()}")
    idx = np.nonzero(adm)[0]
    compare("watchdog=0", prob, 50, {"watchdog": 0}, ref, tr, idx)
