"""GPU tests of lafse3_ocp_sensitivity_w (csrc/sens.inc): per-instance cost weights, the sensitivities of the optimum
to the ten weights, and the autograd layers' ``weights=`` (diff_mpc.mpc_layer, diff_mpc.mpc_policy).

Run on an MI355X:  python -m pytest tests/test_gpu_sens_w.py -m gpu -q -s

Inputs and weight rows D and G: tests/sens_w_cases.py; the finite-difference yardstick: tests/sens_yardstick.py.

(a) Weight columns against central differences of the CPU oracle's solve at h_j = 1e-4 max(|w_j|, 1) and 2 h_j.  A
(sample, weight) pair is admitted from the oracle alone (four solves with status <= 1, e = max|J_h - J_2h| / max|J_h|
<= 1e-3); on admitted pairs of instances with sens_status 0, err = max|J_gpu - J_h| / max|J_h| <= 10 e + F; at most
15 % of the pairs may be left out.  Oracle admission counts (CPU, decided before any GPU value is looked at):
    N = 50, row D, samples 0..15, t as given                       148 of 160
    N = 50, row G, samples 0..7                                      73 of  80
    N = 20, row G, samples 0..7, t := clip(0.5 t, 0.3, 1.5)          72 of  80
    N =  2, row G, samples 0..3, t := 0.1, six non-traversal columns 24 of  24
(at N = 2 the traversal columns' J_h is at rounding level, exactly zero for tra_w_decay at t = dt k: (c) covers them).
The N = 50 check is one launch of 24 instances, 16 under row D and 8 under row G, both through the weights array.
F is the largest err - 10 e of the first GPU run rounded up to the next power of ten, never above the admission
threshold 1e-3 (above it the test could not tell a right column from a wrong one).  First GPU run (sens_status 0 on
every instance of every case), largest err - 10 e:
    N = 50 D  6.046e-04 (sample 13, wwf: err 6.259e-04, e 2.131e-06), median err 1.459e-06            F = 1e-3
    N = 50 G  4.242e-04 (sample 2, wqf: err 4.245e-04, e 2.995e-08), median err 2.783e-06, max err
              1.734e-03 (a pair whose own e carries it)                                                F = 1e-3
    N = 20 G  7.078e-05 (sample 6, du_weight: err 3.758e-04, e 3.050e-05), median err 3.248e-06        F = 1e-4
    N =  2 G  2.240e-09 (sample 0, wrf: err 2.293e-09, e 5.339e-12), median err 4.046e-09              F = 1e-8

(b) One heterogeneous launch (samples 0..7 under D, G, D with wqf = 2, G with wqf = 0: 32 instances) equals the four
ocp_sensitivity_ex launches on engines whose params carry those rows, bit for bit, in x, u, lam, cost, status, iters
and the 23 theta / ini_state / goal columns of dx, du and gain: equal doubles go through the same code, so a difference
means some read of a weight still goes to the context's params.  weights=None and the context's own row equal
ocp_sensitivity_ex on every output.

(c) Adjoint against forward: gain[:, :, weight columns] against du[:, weight columns, 0, :] of the same launch at
horizons 50, 20, 2 and 1 under row G (N = 1: t = 0.1 and a non-zero u_last, the only term of its du_weight column),
relative to the largest |du[b, weight columns, 0, :]| of the instance (test_gpu_sens_ex.py's rule).  The bar is the
first run's largest difference rounded up to a power of ten, at most 1e-5.  First GPU run, weight columns:
    horizon 50: 2.539e-14;  horizon 20: 1.225e-13;  horizon 2: 3.669e-16;  horizon 1: 1.893e-16.
So the bar is 1e-12.  Over all 33 columns of the same launches the largest difference was 3.190e-07 (horizon 20, an
ini_state column): those keep test_gpu_sens_ex.py's bar, 1e-6.

(d) also: a non-finite weight ends its instance with status 4 and leaves the other instances of the launch alone.

(e) Autograd: the gradient of ``weights`` equals the einsum of the returned Jacobians (first GPU run: 2.8e-16 for
mpc_layer, 2.2e-16 for mpc_policy), the (10,) gradient is the batch sum of the (B, 10) one (equal to the bit on that
run), and one descent step lowers the re-solved loss.  The step, 0.1, was fixed on the oracle alone: with the
finite-difference gradient of the batch-mean loss |x_N[:3] - goal|^2 over samples 0..7 at N = 50 under a shared row G,
w - 0.1 g keeps every weight positive (w - g does not: wthrust) and the oracle's re-solved loss falls from 6.5625 to
3.2189.  That gradient's wrf entry, -34.8, is carried by sample 1, whose wrf pair the oracle does not admit (a jump
inside +-h: e = 1); the layer's analytic entry is -1.33, the other nine agree to the digits printed.  At the layer's
own gradient the oracle's re-solve gives 6.5625 -> 6.1408, and the first GPU run 6.562482 -> 6.140534.
"""
import ctypes

import numpy as np
import pytest

import sens_w_cases as C
import sens_yardstick as Y

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ADMIT = Y.ADMIT
# largest err - 10 e on the first GPU run, per case, and the bar: rounded up to the next power of ten (<= ADMIT)
F_MEASURED = {"50D": 6.046e-04, "50G": 4.242e-04, "20G": 7.078e-05, "2G": 2.240e-09}
F = {"50D": 1e-3, "50G": 1e-3, "20G": 1e-4, "2G": 1e-8}
ADMITTED = {"50D": (148, 160), "50G": (73, 80), "20G": (72, 80), "2G": (24, 24)}
ADJ_MEASURED = 1.225e-13   # largest |gain - du_0| / scale over the weight columns on the first GPU run
ADJ_BAR = Y.ADJ_BAR_WEIGHTS   # ADJ_MEASURED rounded up to the next power of ten, at most 1e-5
ADJ_BAR_ALL = Y.ADJ_BAR       # all 33 columns: tests/test_gpu_sens_ex.py's bar (first run here 3.190e-07)
ETA = 0.1                # the descent step, fixed on the oracle alone (module docstring)
_np = Y.to_numpy
NAMES = C.WEIGHT_NAMES
WCOLS = Y.SL["weights"]
ROWS4 = {"D": C.ROW_D, "G": C.ROW_G, "D+wqf": np.where(np.arange(10) == 5, 2.0, C.ROW_D),
         "G-wqf": np.where(np.arange(10) == 5, 0.0, C.ROW_G)}


@pytest.fixture(scope="module")
def eng():
    Y.require_gpu()
    from learningagileflight_se3_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def sb():
    return Y.batch()


def _args(sb, idx, t=None):
    t = sb["t"] if t is None else t
    return tuple(v[idx] for v in (sb["ini"], sb["goal"], sb["p"], sb["a"], t))


IDX24 = np.concatenate([np.arange(16), np.arange(8)])
W24 = np.concatenate([np.tile(C.ROW_D, (16, 1)), np.tile(C.ROW_G, (8, 1))])


@pytest.fixture(scope="module")
def full24(eng, sb):
    """One launch, every group and output: samples 0..15 under row D, then 0..7 under row G (never modified)."""
    out = eng.ocp_sensitivity_w(*_args(sb, IDX24), weights=W24, want=("x", "u", "lam", "cost", "dx", "du", "gain"))
    torch.cuda.synchronize()
    return _np(out)


@pytest.fixture(scope="module")
def fd50(sb):
    """The oracle side of the N = 50 cases (about 13 s of CPU), computed once."""
    prob = {**sb, "t": C.case_t(sb, 50)}
    return {"50D": Y.oracle_fd_weights(prob, 16, C.ROW_D, range(10), C.params_for(50)),
            "50G": Y.oracle_fd_weights(prob, 8, C.ROW_G, range(10), C.params_for(50))}


def _check_against_fd(J_gpu, sens_status, fd, case, cols=range(10)):
    """sens_yardstick.check_against_fd under the case's F, and the oracle's admission count of the module docstring."""
    assert F[case] <= ADMIT
    Y.check_against_fd(J_gpu, sens_status, fd, case, F[case], names=[NAMES[j] for j in cols])
    assert (int(fd["admitted"].sum()), fd["admitted"].size) == ADMITTED[case]


# ---- (a) weight columns against the oracle's finite differences -----------------------------------------------

def test_weight_columns_against_oracle_finite_differences_horizon_50(full24, fd50):
    assert np.all(full24["status"] <= 1) and np.all(full24["sens_status"] != 1)
    assert full24["columns"][23:] == list(NAMES) and full24["dx"].shape == (24, 33, 51, 13)
    J = Y.traj(full24["dx"][:, WCOLS], full24["du"][:, WCOLS])
    _check_against_fd(J[:16], full24["sens_status"][:16], fd50["50D"], "50D")
    _check_against_fd(J[16:], full24["sens_status"][16:], fd50["50G"], "50G")


@pytest.mark.parametrize("horizon", [20, 2])
def test_weight_columns_against_oracle_finite_differences_short(sb, horizon):
    from learningagileflight_se3_amd.engine import Engine
    n = 8 if horizon == 20 else 4
    cols = list(range(10)) if horizon == 20 else list(C.NON_TRAVERSAL)
    t = C.case_t(sb, horizon)
    fd = Y.oracle_fd_weights({**sb, "t": t}, n, C.ROW_G, cols, C.params_for(horizon))
    e = Engine(horizon=horizon)
    g = _np(e.ocp_sensitivity_w(*_args(sb, slice(0, n), t), weights=np.tile(C.ROW_G, (n, 1)), groups=("weights",),
                                want=("x", "u", "dx", "du")))
    assert g["dx"].shape == (n, 10, horizon + 1, 13) and g["du"].shape == (n, 10, horizon, 4)
    assert np.all(g["dx"][:, :, 0, :] == 0.0) and np.all(np.isfinite(g["dx"])) and np.all(np.isfinite(g["du"]))
    _check_against_fd(Y.traj(g["dx"][:, cols], g["du"][:, cols]), g["sens_status"], fd, f"{horizon}G", cols)


# ---- (b) heterogeneous launch equals per-set launches ------------------------------------------------------------

def test_heterogeneous_launch_equals_per_set_launches_bit_for_bit(eng, sb):
    from learningagileflight_se3_amd.engine import Engine
    n = 8
    idx = np.tile(np.arange(n), 4)
    W = np.concatenate([np.tile(r, (n, 1)) for r in ROWS4.values()])
    want = ("x", "u", "lam", "cost", "dx", "du", "gain")
    het = _np(eng.ocp_sensitivity_w(*_args(sb, idx), weights=W, want=want))
    ms_het = eng.last_kernel_ms()
    ms_sets = []
    for r, (name, row) in enumerate(ROWS4.items()):
        e = Engine(**dict(zip(NAMES, map(float, row))))
        assert np.array_equal(e.weights().cpu().numpy(), row)
        ref = _np(e.ocp_sensitivity_ex(*_args(sb, slice(0, n)), want=want))
        ms_sets.append(e.last_kernel_ms())
        sl = slice(r * n, (r + 1) * n)
        for k in ("x", "u", "lam", "cost", "status", "iters", "sens_status"):
            assert np.array_equal(het[k][sl], ref[k]), (name, k)
        assert np.array_equal(het["dx"][sl, :23], ref["dx"]), name
        assert np.array_equal(het["du"][sl, :23], ref["du"]), name
        assert np.array_equal(het["gain"][sl][:, :, :23], ref["gain"]), name
    print(f"kernel time (information only): one launch of 32 instances {ms_het:.2f} ms; the four launches of 8 "
          f"it replaces {' + '.join(f'{m:.2f}' for m in ms_sets)} = {sum(ms_sets):.2f} ms")
    # the rows differ where they should: the heterogeneous launch is no copy of one solve
    assert not np.array_equal(het["x"][:n], het["x"][n:2 * n]) and not np.array_equal(het["x"][:n], het["x"][2 * n:3 * n])
    eng.check_device()


def test_no_weights_and_the_contexts_own_row_equal_the_ex_launch(eng, sb):
    n = 8
    want = ("x", "u", "lam", "cost", "dx", "du", "gain")
    ref = _np(eng.ocp_sensitivity_ex(*_args(sb, slice(0, n)), want=want))
    assert np.array_equal(eng.weights().cpu().numpy(), C.ROW_D)
    for w in (None, eng.weights(), np.tile(C.ROW_D, (n, 1))):
        out = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=w, groups=("theta", "ini", "goal"), want=want))
        assert out["columns"] == ref["columns"]
        for k in want + ("status", "iters", "sens_status"):
            assert np.array_equal(out[k], ref[k]), k
    # no sensitivity output: a plain solve, under the instance's weights when they are given
    plain = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), want=("x",)))
    assert set(plain) == {"x", "status", "iters", "columns"} and np.array_equal(plain["x"], ref["x"])
    solved = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=C.ROW_G, groups=0, want=("x", "cost")))
    gref = _np(type(eng)(**dict(zip(NAMES, map(float, C.ROW_G)))).ocp_solve(*_args(sb, slice(0, n))))
    assert np.array_equal(solved["x"], gref["x"]) and np.array_equal(solved["cost"], gref["cost"])
    assert np.array_equal(solved["iters"], gref["iters"])


# ---- (c) adjoint against forward ------------------------------------------------------------------------------------

W_ONLY, ALL33 = {"weights": WCOLS}, {"all": slice(0, 33)}      # the column groups of the identity's two bars


def test_adjoint_gain_equals_forward_du0_horizon_50(eng, sb, full24):
    g = {k: (v[16:] if isinstance(v, np.ndarray) else v) for k, v in full24.items()}      # the row G instances
    assert Y.adjoint_difference(g, "horizon 50", W_ONLY, ADJ_BAR) <= ADJ_BAR
    only = _np(eng.ocp_sensitivity_w(*_args(sb, IDX24), weights=W24, want=("gain",)))
    assert set(only) == {"gain", "status", "iters", "sens_status", "columns"}
    assert np.array_equal(only["gain"], full24["gain"]) and np.array_equal(only["sens_status"], full24["sens_status"])


@pytest.mark.parametrize("horizon", [20, 2, 1])
def test_adjoint_gain_equals_forward_du0_short(sb, horizon):
    from learningagileflight_se3_amd.engine import Engine
    n = 8
    e = Engine(horizon=horizon)
    t = C.case_t(sb, horizon)
    ul = np.tile([0.4, 0.9, 0.2, 1.3], (n, 1)) if horizon == 1 else None
    W = np.tile(C.ROW_G, (n, 1))
    g = _np(e.ocp_sensitivity_w(*_args(sb, slice(0, n), t), ul, weights=W, want=("u", "du", "gain")))
    assert g["du"].shape == (n, 33, horizon, 4) and g["gain"].shape == (n, 4, 33)
    assert np.all(np.isfinite(g["du"])) and np.all(np.isfinite(g["gain"]))
    assert Y.adjoint_difference(g, f"horizon {horizon}", W_ONLY, ADJ_BAR) <= ADJ_BAR
    assert Y.adjoint_difference(g, f"horizon {horizon}, all 33 columns", ALL33, ADJ_BAR_ALL) <= ADJ_BAR_ALL
    if horizon == 1:
        # one stage: the du_weight column is its u_last term alone, and it moves u_0
        live = g["sens_status"] == 0
        assert np.all(np.abs(g["du"][live][:, 32, 0, :]).max(-1) > 0)
    only = _np(e.ocp_sensitivity_w(*_args(sb, slice(0, n), t), ul, weights=W, want=("gain",)))
    assert np.array_equal(only["gain"], g["gain"])


# ---- (d) column selection and refusals ------------------------------------------------------------------------------

def test_group_subsets_select_the_columns_of_the_full_launch(eng, sb, full24):
    from learningagileflight_se3_amd import _lib
    n = 4
    G = ("theta", "ini", "goal", "weights")
    assert full24["columns"] == [c for g in G for c in _lib.SENS_COLUMNS_W[g]]
    assert np.all(full24["dx"][:, WCOLS, 0, :] == 0.0)                          # x_0 does not move with a weight
    ref = {k: full24[k][16:16 + n] for k in ("dx", "du", "gain")}                # row G, samples 0..3
    W = np.tile(C.ROW_G, (n, 1))
    for sel in (("weights",), ("weights", "theta"), ("weights", "ini"), ("goal", "weights"), G):
        out = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=W, groups=sel))
        cols = np.concatenate([np.arange(33)[Y.SL[g]] for g in G if g in sel])
        assert out["columns"] == [full24["columns"][c] for c in cols]
        assert out["dx"].shape == (n, len(cols), 51, 13) and out["gain"].shape == (n, 4, len(cols))
        assert np.array_equal(out["dx"], ref["dx"][:, cols]), sel
        assert np.array_equal(out["du"], ref["du"][:, cols]), sel
        assert np.array_equal(out["gain"], ref["gain"][:, :, cols]), sel
        mask = sum(_lib.SENS_GROUPS_W[g] for g in sel)
        same = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=W, groups=mask, want=("gain",)))
        assert np.array_equal(same["gain"], out["gain"])
    # a (10,) row is broadcast over the batch
    one = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=C.ROW_G, groups="weights", want=("du",)))
    assert np.array_equal(one["du"], ref["du"][:, WCOLS])


def test_bad_groups_and_weight_shapes_are_refused(eng, sb):
    from learningagileflight_se3_amd import _lib
    a2 = _args(sb, slice(0, 2))
    for bad in (0, (), 16, 8 | 32):
        with pytest.raises(ValueError, match="groups"):
            eng.ocp_sensitivity_w(*a2, groups=bad)
    with pytest.raises(ValueError, match="groups"):
        eng.ocp_sensitivity_w(*a2, groups=("weights", "u_last"))
    for shape in ((2, 9), (3, 10), (9,), (2, 10, 1)):
        with pytest.raises(ValueError, match="weights"):
            eng.ocp_sensitivity_w(*a2, weights=np.ones(shape))
    # the C entry point itself: refused before any launch (the output pointer is never used)
    L = _lib.load()
    buf = torch.zeros(8, dtype=torch.float64, device=eng.device)
    ptr = ctypes.c_void_p(buf.data_ptr())
    for bad in (0, 16, 1 | 32):
        for which in range(3):
            outs = [ptr if i == which else None for i in range(3)]
            rc = L.lafse3_ocp_sensitivity_w(eng._ctx, 2, *([ptr] * 5), None, None, *([None] * 6), bad, *outs, None, None)
            assert rc == -1 and b"groups" in L.lafse3_last_error()
    assert torch.all(buf == 0.0)
    # lafse3_ocp_sensitivity_ex keeps refusing the weights bit
    with pytest.raises(ValueError):
        eng.ocp_sensitivity_ex(*a2, groups=8)


def test_unconverged_solves_give_zero_outputs(sb):
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(max_iter=3)
    out = e.ocp_sensitivity_w(*_args(sb, slice(0, 2)), weights=np.stack([C.ROW_D, C.ROW_G]))
    torch.cuda.synchronize()
    assert out["status"].tolist() == [2, 2] and out["sens_status"].tolist() == [1, 1]
    assert out["dx"].shape == (2, 33, 51, 13)
    assert torch.all(out["dx"] == 0.0) and torch.all(out["du"] == 0.0) and torch.all(out["gain"] == 0.0)
    e.check_device()                                     # no device error word


def test_a_non_finite_weight_ends_its_instance_as_non_finite(eng, sb, full24):
    n = 4
    ref = {k: full24[k][16:16 + n] for k in ("x", "status", "iters", "dx", "gain", "sens_status")}
    for j, bad in ((0, np.nan), (3, np.inf), (8, np.nan), (9, -np.inf)):
        W = np.tile(C.ROW_G, (n, 1))
        W[1, j] = bad
        out = _np(eng.ocp_sensitivity_w(*_args(sb, slice(0, n)), weights=W, want=("x", "dx", "gain")))
        assert out["status"][1] == 4 and out["sens_status"][1] == 1, (NAMES[j], out["status"].tolist())
        assert np.all(out["dx"][1] == 0.0) and np.all(out["gain"][1] == 0.0)
        for k, v in ref.items():                           # the other instances of the launch are what they were
            assert np.array_equal(out[k][[0, 2, 3]], v[[0, 2, 3]]), (NAMES[j], k)
    eng.check_device()


# ---- (e) autograd ------------------------------------------------------------------------------------------------------

def test_autograd_through_mpc_layer_to_the_weights(eng, sb, full24):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    n, dev = 24, eng.device
    rng = np.random.default_rng(2025)
    W_x, W_u = rng.standard_normal((n, 51, 13)), rng.standard_normal((n, 50, 4))
    w = torch.tensor(W24, dtype=torch.float64, device=dev, requires_grad=True)
    x, u, status = mpc_layer(eng, *_args(sb, IDX24), weights=w)
    assert x.dtype == torch.float64 and not status.requires_grad
    assert np.array_equal(x.detach().cpu().numpy(), full24["x"])
    ((torch.as_tensor(W_x, device=dev) * x).sum() + (torch.as_tensor(W_u, device=dev) * u).sum()).backward()
    assert w.grad.shape == (n, 10) and w.grad.dtype == torch.float64
    dx, du = full24["dx"][:, WCOLS], full24["du"][:, WCOLS]
    live = (full24["sens_status"] == 0)[:, None]
    Jw = live * (np.einsum("bqki,bki->bq", dx, W_x) + np.einsum("bqka,bka->bq", du, W_u))
    mag = np.einsum("bqki,bki->bq", np.abs(dx), np.abs(W_x)) + np.einsum("bqka,bka->bq", np.abs(du), np.abs(W_u))
    rel = np.abs(w.grad.cpu().numpy() - Jw) / mag
    print(f"mpc_layer autograd vs einsum of the Jacobian: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    # a (10,) row: the batch sum of the (B, 10) gradient of the same launch; float32: widened, float32 gradient
    m = 8
    Wx8, Wu8 = torch.as_tensor(W_x[16:], device=dev), torch.as_tensor(W_u[16:], device=dev)
    wB = torch.tensor(W24[16:], dtype=torch.float64, device=dev, requires_grad=True)
    w1 = torch.tensor(C.ROW_G, dtype=torch.float64, device=dev, requires_grad=True)
    w32 = torch.tensor(C.ROW_G, dtype=torch.float32, device=dev, requires_grad=True)
    for leaf in (wB, w1, w32):
        x, u, _ = mpc_layer(eng, *_args(sb, slice(0, m)), weights=leaf)
        ((Wx8 * x).sum() + (Wu8 * u).sum()).backward()
    assert w1.grad.shape == (10,) and wB.grad.shape == (m, 10) and w32.grad.dtype == torch.float32
    assert np.array_equal(wB.grad.cpu().numpy(), w.grad.cpu().numpy()[16:])
    tot, mag1 = wB.grad.sum(0).cpu().numpy(), wB.grad.abs().sum(0).cpu().numpy()
    rel1 = np.abs(w1.grad.cpu().numpy() - tot) / mag1
    print(f"(10,) gradient vs the batch sum of the (B, 10) gradient: max relative difference {rel1.max():.3e}")
    assert rel1.max() <= 1e-12
    # the float32 row widens to other doubles (0.15, 0.7 are not float32 numbers): compared at float32 resolution
    assert w32.grad.shape == (10,) and bool(torch.all(torch.isfinite(w32.grad)))


def test_autograd_through_mpc_policy_to_the_weights(eng, sb, full24):
    from learningagileflight_se3_amd.diff_mpc import mpc_policy
    n, dev = 24, eng.device
    c = np.random.default_rng(7).standard_normal((n, 4))
    w = torch.tensor(W24, dtype=torch.float64, device=dev, requires_grad=True)
    t = torch.tensor(sb["t"][IDX24], dtype=torch.float64, device=dev, requires_grad=True)
    ini, goal, p, a, _ = _args(sb, IDX24)
    u0, status = mpc_policy(eng, ini, goal, p, a, t, weights=w)
    assert u0.shape == (n, 4) and not status.requires_grad
    assert np.array_equal(u0.detach().cpu().numpy(), full24["u"][:, 0])
    (torch.as_tensor(c, device=dev) * u0).sum().backward()
    live = (full24["sens_status"] == 0)[:, None]
    ref = live * np.einsum("baq,ba->bq", full24["gain"], c)
    mag = np.einsum("baq,ba->bq", np.abs(full24["gain"]), np.abs(c))
    got = np.concatenate([t.grad.cpu().numpy()[:, None], w.grad.cpu().numpy()], axis=1)
    cols = [6] + list(range(23, 33))
    rel = np.abs(got - ref[:, cols]) / np.where(mag[:, cols] > 0, mag[:, cols], 1.0)
    print(f"mpc_policy autograd vs gain contracted with c: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    w1 = torch.tensor(C.ROW_G, dtype=torch.float64, device=dev, requires_grad=True)
    u0, _ = mpc_policy(eng, *_args(sb, slice(0, 8)), weights=w1)
    (torch.as_tensor(c[16:], device=dev) * u0).sum().backward()
    tot, mag1 = ref[16:, 23:].sum(0), np.abs(ref[16:, 23:]).sum(0)
    assert w1.grad.shape == (10,) and np.max(np.abs(w1.grad.cpu().numpy() - tot) / mag1) <= 1e-12


def test_one_descent_step_on_the_weights_lowers_the_resolved_loss(eng, sb):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    n, dev = 8, eng.device
    args = _args(sb, slice(0, n))
    goal = torch.as_tensor(sb["goal"][:n], device=dev)
    loss = lambda x: (x[:, -1, :3] - goal).square().sum(1).mean()
    w = torch.tensor(C.ROW_G, dtype=torch.float64, device=dev, requires_grad=True)
    x, _, status = mpc_layer(eng, *args, weights=w)
    L0 = loss(x)
    L0.backward()
    assert int(status.max()) <= 1
    w1 = (w - ETA * w.grad).detach()
    x1, _, status1 = mpc_layer(eng, *args, weights=w1)
    L1 = loss(x1)
    L0, L1 = L0.detach(), L1.detach()
    print(f"descent: loss {float(L0):.6e} -> {float(L1):.6e} (decrease {float(L0 - L1):.3e}) with step {ETA}; gradient "
          f"{dict(zip(NAMES, (f'{v:.2e}' for v in w.grad.tolist())))}")
    assert int(status1.max()) <= 1 and float(L1) < float(L0)


def test_instances_without_sensitivity_contribute_zero_gradient(sb):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer, mpc_policy
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(max_iter=3)
    args = _args(sb, slice(0, 2))
    w = torch.tensor(np.stack([C.ROW_D, C.ROW_G]), dtype=torch.float64, device=e.device, requires_grad=True)
    u0, status = mpc_policy(e, *args, weights=w)
    assert status.tolist() == [2, 2]
    x, u, _ = mpc_layer(e, *args, weights=w)
    (u0.sum() + x.sum() + u.sum()).backward()
    assert bool(torch.all(w.grad == 0.0))
