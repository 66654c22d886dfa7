"""The weight columns of lafse3_ocp_sensitivity_w (csrc/sens.inc, csrc/weight_columns.hpp) and the adjoint sweep of
lafse3_ocp_vjp (csrc/vjp.inc) at the generic parameter set (generic_params.py).  tests/test_gpu_sens_w.py and
tests/test_gpu_vjp.py take only the ten weights from that set: dt, the model and the bounds stay the reference's, a
non-zero u_last appears at horizon 1 alone, and vjp.inc's hand-written copy of run_instance's prologue (relaxed bounds,
make_model, S.wk from prm.dt) has run only where u_lb = 0 and w_lb = -w_ub hide a wrong bound.  Here dt = 0.08,
Jx != Jy, u_lb = 0.1, w_lb = -1.2, w_ub = 1.4, wqf = 2, and u_last = 1 on the odd samples at every horizon, so the
u_{-1} = u_last term of the du_weight column at k = 0 is compared with finite differences at N > 1.

Run on an MI355X:  python -m pytest tests/test_gpu_generic_sens_w.py -m gpu -q -s

Engine(horizon=N, **GENERIC.fields()); problems generic_params.problem(batch, N, range(8)) (t = 0.5 N dt); the weight
row is GENERIC's own ten weights (sens_w_cases.ROW_G).  Every test asserts sens_status 0 on all eight instances.

(1) Weight columns against central differences of the CPU oracle's solve with params = GENERIC and weight j moved, at
h_j = 1e-4 max(|w_j|, 1) and 2 h_j, u_last passed.  Admission and bound are sens_yardstick's / test_gpu_sens_w.py's: four
solves with status <= 1 and e = max|J_h - J_2h| / max|J_h| <= 1e-3; err = max|J_gpu - J_h| / max|J_h| <= 10 e + F; at
most 15 % of the pairs left out.  Oracle admission counts (CPU, decided before any GPU value is looked at):
    horizon 20, all ten columns             69 of 80
    horizon  7, all ten columns             80 of 80
    horizon  2, six non-traversal columns   48 of 48   (the traversal columns' J_h is exactly 0 there: (3) covers them)
Horizon 50 is not compared: the tight boxes of this set kink the solution map (the oracle admits 52 of 80 pairs), as
tests/test_gpu_generic_sens.py explains.  F is the first GPU run's largest err - 10 e rounded up to the next power of
ten, never above the admission threshold 1e-3.  First GPU run (sens_status 0 on every instance), largest err - 10 e:
    horizon 20  5.380e-04 (sample 6, wqf: err 5.395e-04, e 1.495e-07), median err 2.988e-06, max err 9.335e-04
                (a pair whose own e carries it); du_weight 1.33e-05, tra_w_decay 6.51e-06           F = 1e-3
    horizon  7  8.213e-06 (sample 7, wqt: err 8.366e-06, e 1.533e-08), median err 3.084e-07;
                du_weight 3.81e-06, tra_w_decay 2.32e-06                                             F = 1e-5
    horizon  2  7.736e-09 (sample 6, wrf: err 7.920e-09, e 1.842e-11), median err 3.790e-09          F = 1e-8
The du_weight column must have admitted pairs on the odd samples (u_last = 1), or its u_{-1} term would go unseen:
the oracle admits 3 of 4 at horizon 20 and 4 of 4 at horizons 7 and 2, and the test asserts at least 3.

(2) The row handed over in the ``weights`` array equals the same row read from the context's params (weights=None)
bit for bit on every output, horizons 20 and 7 (test_gpu_sens_w.py's test of that name at a non-default model).

(3) Adjoint identities at horizons 20, 7, 2 and 1, all 33 columns:
    gain == du[:, :, 0, :] under sens_yardstick.ADJ_BAR_WEIGHTS on the weight columns and ADJ_BAR on all 33;
    ocp_vjp on ocp_solve_rec's record against dx, du of the same inputs contracted with standard normal g_x, g_u
    (np.random.default_rng(7)), then each alone with the other None, under sens_yardstick.VJP_BAR on vjp_relative's scale;
    ocp_solve_rec's outputs equal ocp_sensitivity_w's bit for bit.
With (1) this ties the adjoint sweep at this set to the oracle; at horizons 2 and 1, where finite differences say
nothing about the traversal columns, the identity is what covers them.
First GPU run, largest relative differences (ADJ_FIRST_RUN; those above rounding are in the ini_state group, whose
contraction passes through lam+_0, as in the sibling modules):
    horizon   gain, weight columns   gain, all 33   ocp_vjp (worst of the three right-hand sides)
      20          1.382e-14           2.337e-08      6.735e-10 (g_u alone)
       7          2.259e-15           5.007e-09      2.876e-09 (g_u alone)
       2          3.866e-16           4.396e-16      3.393e-15 (g_x alone)
       1          3.414e-16           1.210e-15      1.720e-14 (g_x alone)
No kernel or host-layer bug came to light.

What the module sees, tried on scratch builds (nothing of them is committed):
  - prm.dt replaced by 0.1 in the forward route's sens_w_column call: (1) fails at horizons 20 and 7 in tra_w_peak and
    tra_w_decay (err - 10 e 5.5 and 17.3, 1.8 and 3.2) and both identities of (3) fail there (gain 0.94 and 0.47,
    ocp_vjp 0.16 and 0.045 in the weights group);
  - the u_last term of the du_weight column dropped at k = 0 (um = 0 in sens_w_column): (1) fails in du_weight at
    every horizon (err - 10 e 1.9e-03, 2.6e-02, 3.7), while (2), (3) and every test of tests/test_gpu_sens_w.py and
    tests/test_gpu_vjp.py pass: all routes share the column, only the oracle tells.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import generic_params as GP  # noqa: E402
import newton_cases as NC  # noqa: E402
import sens_w_cases as C  # noqa: E402
import sens_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = GP.GENERIC
NAMES = C.WEIGHT_NAMES
ROW = np.array([getattr(GENERIC, k) for k in NAMES])
ADMIT = Y.ADMIT
NS = 8
WCOLS = Y.SL["weights"]
WANT = ("x", "u", "lam", "cost", "dx", "du", "gain")
FD_COLS = {20: tuple(range(10)), 7: tuple(range(10)), 2: C.NON_TRAVERSAL}
ADMITTED = {20: (69, 80), 7: (80, 80), 2: (48, 48)}
# largest err - 10 e on the first GPU run, per horizon, and the bar: rounded up to the next power of ten (<= ADMIT)
F_MEASURED = {20: 5.380e-04, 7: 8.213e-06, 2: 7.736e-09}
F = {20: 1e-3, 7: 1e-5, 2: 1e-8}
# first GPU run, horizon -> (gain vs du_0 on the weight columns, on all 33 columns, vjp vs contracted Jacobians); the
# bars are the sibling modules' (sens_yardstick's ADJ_BAR_WEIGHTS, ADJ_BAR, VJP_BAR), not derived from these
ADJ_FIRST_RUN = {20: (1.382e-14, 2.337e-08, 6.735e-10), 7: (2.259e-15, 5.007e-09, 2.876e-09),
                 2: (3.866e-16, 4.396e-16, 3.393e-15), 1: (3.414e-16, 1.210e-15, 1.720e-14)}
_runs = {}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def gpu_run(batch, horizon):
    """The eight instances of the horizon solved once by every route (shared, never modified): ocp_sensitivity_w with
    the row in the weights array (all four groups, every output), the same with weights=None, and ocp_solve_rec."""
    Y.require_gpu()
    if horizon not in _runs:
        from learningagileflight_se3_amd.engine import Engine
        e = Engine(horizon=horizon, **GENERIC.fields())
        assert np.array_equal(e.weights().cpu().numpy(), ROW) and np.array_equal(ROW, C.ROW_G)
        prob = GP.problem(batch, horizon, range(NS))
        assert np.any(prob["ulast"] != 0.0)
        W = np.tile(ROW, (NS, 1))
        args = (prob["ini"], prob["goal"], prob["p"], prob["a"], prob["t"], prob["ulast"])
        arr = Y.to_numpy(e.ocp_sensitivity_w(*args, weights=W, want=WANT))
        ctx = Y.to_numpy(e.ocp_sensitivity_w(*args, weights=None, want=WANT))
        rec = e.ocp_solve_rec(*args, weights=W)
        torch.cuda.synchronize()
        e.check_device()
        print(f"generic set, horizon {horizon}: status {arr['status'].tolist()}; sens_status histogram "
              f"{np.bincount(arr['sens_status'], minlength=3).tolist()}")
        _runs[horizon] = {"eng": e, "prob": prob, "args": args, "W": W, "arr": arr, "ctx": ctx, "rec": rec}
    return _runs[horizon]


def _live(g):
    assert np.all(g["status"] <= 1), g["status"]
    assert np.all(g["sens_status"] == 0), g["sens_status"]


def oracle_fd(prob, n, horizon, cols):
    """sens_yardstick.oracle_fd_weights at the generic set: GENERIC's row with weight j moved, u_last passed."""
    return Y.oracle_fd_weights(prob, n, ROW, cols, lambda row: NC.oracle_params(
        GENERIC, horizon=horizon, **dict(zip(NAMES, map(float, row)))))


# ---- (1) weight columns against the oracle's finite differences -------------------------------------------------

@pytest.mark.parametrize("horizon", [20, 7, 2])
def test_weight_columns_against_oracle_finite_differences(batch, horizon):
    r = gpu_run(batch, horizon)
    g, cols = r["arr"], list(FD_COLS[horizon])
    fd = oracle_fd(r["prob"], NS, horizon, cols)
    _live(g)
    assert g["columns"][23:] == list(NAMES) and g["dx"].shape == (NS, 33, horizon + 1, 13)
    assert np.all(g["dx"][:, WCOLS, 0, :] == 0.0) and np.all(np.isfinite(g["dx"])) and np.all(np.isfinite(g["du"]))
    J = Y.traj(g["dx"][:, WCOLS][:, cols], g["du"][:, WCOLS][:, cols])
    assert F[horizon] <= ADMIT
    names = [NAMES[j] for j in cols]
    _, excess, _ = Y.check_against_fd(J, g["sens_status"], fd, f"horizon {horizon}", F[horizon], names=names)
    adm = fd["admitted"]
    print(f"horizon {horizon}: max(err - 10 e) per column "
          f"{dict(zip(names, (f'{v:.2e}' for v in excess.max(0))))}")
    assert (int(adm.sum()), adm.size) == ADMITTED[horizon]
    # the u_last term of the du_weight column is under test: admitted pairs of it on samples with u_last != 0
    odd = np.any(r["prob"]["ulast"] != 0.0, axis=1)
    assert adm[odd][:, cols.index(9)].sum() >= 3


# ---- (2) the weights array against the context's row --------------------------------------------------------------

@pytest.mark.parametrize("horizon", [20, 7])
def test_the_row_through_the_weights_array_equals_the_contexts_own_row(batch, horizon):
    r = gpu_run(batch, horizon)
    _live(r["arr"])
    assert r["ctx"]["columns"] == r["arr"]["columns"]
    for k in WANT + ("status", "iters", "sens_status"):
        assert np.array_equal(r["arr"][k], r["ctx"][k]), k
    assert np.any(r["arr"]["du"][:, WCOLS] != 0.0)


# ---- (3) adjoint identities -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [20, 7, 2, 1])
def test_adjoint_gain_equals_forward_du0(batch, horizon):
    g = gpu_run(batch, horizon)["arr"]
    _live(g)
    assert g["du"].shape == (NS, 33, horizon, 4) and g["gain"].shape == (NS, 4, 33)
    assert np.all(np.isfinite(g["du"])) and np.all(np.isfinite(g["gain"]))
    assert Y.ADJ_BAR_WEIGHTS <= 1e-5 and Y.ADJ_BAR <= 1e-5
    label = f"generic set, horizon {horizon}"
    assert Y.adjoint_difference(g, label, {"weights": WCOLS}, Y.ADJ_BAR_WEIGHTS) <= Y.ADJ_BAR_WEIGHTS
    assert Y.adjoint_difference(g, label + ", all 33 columns", {"all": slice(0, 33)}, Y.ADJ_BAR) <= Y.ADJ_BAR
    # the du_weight column moves u_0 through its u_last term on the odd samples, at one stage through nothing else
    odd = np.any(gpu_run(batch, horizon)["prob"]["ulast"] != 0.0, axis=1)
    assert np.all(np.abs(g["du"][odd][:, 32, 0, :]).max(-1) > 0)


@pytest.mark.parametrize("horizon", [20, 7, 2, 1])
def test_adjoint_sweep_equals_the_contracted_forward_jacobians(batch, horizon):
    r = gpu_run(batch, horizon)
    e, fwd = r["eng"], r["arr"]
    _live(fwd)
    assert bool((r["rec"]["status"] <= 1).all())
    rng = np.random.default_rng(7)
    g_x = rng.standard_normal((NS, horizon + 1, 13))
    g_u = rng.standard_normal((NS, horizon, 4))
    for label, gx, gu in (("g_x and g_u", g_x, g_u), ("g_x alone", g_x, None), ("g_u alone", None, g_u)):
        out = Y.to_numpy(e.ocp_vjp(*r["args"], r["W"], r["rec"]["rec"], gx, gu))
        assert out["grad"].shape == (NS, 33) and np.all(np.isfinite(out["grad"]))
        assert out["columns"] == fwd["columns"] and np.all(out["sens_status"] == 0), out["sens_status"]
        ref, scale = Y.vjp_reference(fwd, np.zeros_like(g_x) if gx is None else gx, np.zeros_like(g_u) if gu is None else gu)
        assert np.all(scale[:, 3] > 0) and np.any(out["grad"][:, WCOLS] != 0.0)
        worst = Y.vjp_relative(out["grad"], ref, scale, f"generic set, horizon {horizon}, {label}")
        assert Y.VJP_BAR <= 1e-5 and worst <= Y.VJP_BAR
    e.check_device()


@pytest.mark.parametrize("horizon", [20, 7, 2, 1])
def test_solve_rec_outputs_equal_those_of_ocp_sensitivity_w(batch, horizon):
    r = gpu_run(batch, horizon)
    _live(r["arr"])
    rec = Y.to_numpy(r["rec"])
    assert set(rec) == {"x", "u", "lam", "cost", "status", "iters", "rec"}
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert np.array_equal(rec[k], r["arr"][k]), k
    assert np.all(rec["rec"][:, Y.REC_N] == horizon)
