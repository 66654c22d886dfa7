"""GPU tests of lafse3_ocp_sensitivity_ex (csrc/sens.inc): the sensitivities to ini_state and goal, the MPC
feedback gain from the adjoint use of the factorisation, and the autograd layers built on them (diff_mpc.mpc_layer
with ini_state / goal leaves, diff_mpc.mpc_policy).

Run on an MI355X:  python -m pytest tests/test_gpu_sens_ex.py -m gpu -q -s

Inputs: scenario.synthetic_batch(64, seed=2025) with p, a, t widened to float64 and u_last = None, as
tests/test_gpu_sens.py.

(a) Forward columns against central finite differences of the CPU oracle's solve at h = 1e-4 and 2h over the whole
trajectory, for the 13 ini_state and 3 goal parameters.  Admission, bound and printing are those of
tests/test_gpu_sens.py: a (sample, parameter) pair is admitted from the oracle alone when its four solves end with
status <= 1 and e = max|J_h - J_2h| / max|J_h| <= 1e-3; on admitted pairs of instances with sens_status 0,
err = max|J_gpu - J_h| / max|J_h| <= 10 e + F with F = 1e-3 (that file's, where it equals the admission threshold).
At most 15 % of the pairs may be left out.  Horizons 50 (first 8 samples), 20 and 2 (first 4); at horizon 2 only the
ini_state columns are compared (position cannot respond to goal x / y within two steps: J_h is exactly zero there),
the goal columns are covered by (b).  Largest err - 10 e on the first GPU run (sens_status 0 on every instance):
    horizon 50, 112 of 128 pairs (ini 90 of 104, goal 22 of 24): 3.866e-05 (sample 7, ini_state[5]: err 3.891e-05,
                e 2.569e-08), median err 2.283e-06, max err 1.196e-04 (a pair whose own e carries it);
    horizon 20,  64 of  64 pairs: 7.800e-06 (sample 1, ini_state[10]), median err 7.575e-07;
    horizon  2,  52 of  52 ini_state pairs: 7.572e-12, median err 2.331e-12.

(b) Adjoint against forward, the identity K^-T = K^-1: gain[b, a, q] against du[b, q, 0, a] of the same launch, all
23 columns of every instance with sens_status 0, horizons 50 (16 samples), 20, 2 and 1 (8 samples each), relative to
the largest |du[b, :, 0, :]| of the instance's parameter group.  The bar is the largest difference of the first GPU
run rounded up to the next power of ten, never above 1e-5 (the project's parity scale, IFT_BAR of
tests/test_gpu_sens.py): a larger difference is a wrong sign, row block or stage-0 contraction, not a bar to raise.
First GPU run, per horizon the largest difference (always in the ini_state group; theta and goal stay below 3e-13):
    horizon 50: 1.600e-07 (sample 7);  horizon 20: 8.574e-08;  horizon 2: 7.430e-16;  horizon 1: 8.701e-16.
So the bar is 1e-6.  On that run the autograd gradients matched the einsum of the returned Jacobians to 4.7e-16
(mpc_layer) and 2.1e-16 (mpc_policy).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sens_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

F = Y.F              # tests/test_gpu_sens.py's F (= ADMIT)
# largest err - 10 e per horizon on the first GPU run (admitted pairs with sens_status 0)
MEASURED = {50: 3.866e-05, 20: 7.800e-06, 2: 7.572e-12}
ADJ_MEASURED = 1.600e-07   # largest |gain - du_0| / group scale on the first GPU run (horizons 50, 20, 2, 1)
ADJ_BAR = Y.ADJ_BAR  # ADJ_MEASURED rounded up to the next power of ten, at most 1e-5
NFD = 8              # samples of the horizon-50 finite-difference comparison
NS = 16              # samples of the shared horizon-50 launch
_np = Y.to_numpy
GROUPS = ("theta", "ini", "goal")
SL = {g: Y.SL[g] for g in GROUPS}
INI_GOAL = range(7, 23)                  # the ini_state and goal columns of sens_yardstick.oracle_fd's z


@pytest.fixture(scope="module")
def eng():
    Y.require_gpu()
    from learningagileflight_se3_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def batch():
    return Y.batch()


def _args(sb, n):
    return tuple(sb[k][:n] for k in ("ini", "goal", "p", "a", "t"))


@pytest.fixture(scope="module")
def full16(eng, batch):
    """One launch with all three groups and every output on the first 16 samples (never modified)."""
    out = eng.ocp_sensitivity_ex(*_args(batch, NS), want=("x", "u", "lam", "cost", "dx", "du", "gain"))
    torch.cuda.synchronize()
    return _np(out)


# ---- (a) forward columns against the oracle's finite differences ---------------------------------------------

def _check_against_fd(J_gpu, sens_status, fd, label):
    ini, goal = fd["admitted"][:, :13], fd["admitted"][:, 13:]
    print(f"{label}: oracle admits ini {int(ini.sum())} of {ini.size}, goal {int(goal.sum())} of {goal.size}")
    Y.check_against_fd(J_gpu, sens_status, fd, label, F)


def test_forward_columns_against_oracle_finite_differences_horizon_50(batch, full16):
    fd = Y.oracle_fd(batch, NFD, 50, INI_GOAL)
    st = full16["sens_status"][:NFD]
    assert np.all(full16["status"][:NFD] <= 1) and np.all(st != 1)
    J = Y.traj(full16["dx"][:NFD, 7:], full16["du"][:NFD, 7:])
    _check_against_fd(J, st, fd, "horizon 50")


@pytest.mark.parametrize("horizon", [20, 2])
def test_forward_columns_against_oracle_finite_differences_short(batch, horizon):
    from learningagileflight_se3_amd.engine import Engine
    n = 4
    e = Engine(horizon=horizon)
    fd = Y.oracle_fd(batch, n, horizon, INI_GOAL if horizon != 2 else range(7, 20))
    g = _np(e.ocp_sensitivity_ex(*_args(batch, n), groups=("ini", "goal"), want=("x", "u", "dx", "du")))
    assert g["dx"].shape == (n, 16, horizon + 1, 13) and g["du"].shape == (n, 16, horizon, 4)
    Q = fd["J"].shape[1]
    _check_against_fd(Y.traj(g["dx"][:, :Q], g["du"][:, :Q]), g["sens_status"], fd, f"horizon {horizon}")


# ---- (b) adjoint against forward ------------------------------------------------------------------------------

def test_adjoint_gain_equals_forward_du0_horizon_50(eng, batch, full16):
    assert Y.adjoint_difference(full16, "horizon 50", SL, ADJ_BAR) <= ADJ_BAR
    # a gain-only call (dx = du = NULL) returns the same gain bit for bit
    only = _np(eng.ocp_sensitivity_ex(*_args(batch, NS), want=("gain",)))
    assert set(only) == {"gain", "status", "iters", "sens_status", "columns"}
    assert np.array_equal(only["gain"], full16["gain"])
    assert np.array_equal(only["sens_status"], full16["sens_status"])


@pytest.mark.parametrize("horizon", [20, 2, 1])
def test_adjoint_gain_equals_forward_du0_short(batch, horizon):
    from learningagileflight_se3_amd.engine import Engine
    n = 8
    e = Engine(horizon=horizon)
    g = _np(e.ocp_sensitivity_ex(*_args(batch, n), want=("du", "gain")))
    assert g["du"].shape == (n, 23, horizon, 4) and g["gain"].shape == (n, 4, 23)
    assert np.all(np.isfinite(g["du"])) and np.all(np.isfinite(g["gain"]))
    assert Y.adjoint_difference(g, f"horizon {horizon}", SL, ADJ_BAR) <= ADJ_BAR
    only = _np(e.ocp_sensitivity_ex(*_args(batch, n), want=("gain",)))
    assert np.array_equal(only["gain"], g["gain"])


# ---- (c) nothing existing moves -------------------------------------------------------------------------------

def test_outputs_are_the_plain_solves_and_theta_columns_bit_for_bit(eng, batch, full16):
    sb = batch
    args = _args(sb, NS)
    gargs = (sb["ini"][:NS], sb["goal"][:NS], sb["gate12"][:NS], sb["dnn_out"][:NS])
    e2 = type(eng)()                                  # a context that never ran the new kernel
    ref = _np(e2.ocp_solve(*args))
    old = _np(e2.ocp_sensitivity(*args))
    g_ref = [v.cpu().numpy() for v in e2.sol_gradient(*gargs, want_rewards=True, grad_mode=1)]
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert np.array_equal(full16[k], ref[k]), k
    assert np.array_equal(full16["sens_status"], old["sens_status"])
    # the theta columns: of the full launch and of a launch with groups = THETA alone
    th = _np(eng.ocp_sensitivity_ex(*args, groups=("theta",), want=("dx", "du")))
    assert th["dx"].shape == old["dx"].shape and th["du"].shape == old["du"].shape
    assert np.array_equal(th["dx"], old["dx"]) and np.array_equal(th["du"], old["du"])
    assert np.array_equal(full16["dx"][:, :7], old["dx"]) and np.array_equal(full16["du"][:, :7], old["du"])
    # workspace reuse: launches that follow a new-kernel launch on the same context are what a fresh context gives
    eng.ocp_sensitivity_ex(*args)
    after = _np(eng.ocp_solve(*args))
    g_after = [v.cpu().numpy() for v in eng.sol_gradient(*gargs, want_rewards=True, grad_mode=1)]
    for k in ref:
        assert np.array_equal(after[k], ref[k]), k
    for a, b in zip(g_after, g_ref):
        assert np.array_equal(a, b)
    # no sensitivity output: the call is the plain solve
    plain = eng.ocp_sensitivity_ex(*_args(sb, 4), want=("x",))
    assert set(plain) == {"x", "status", "iters", "columns"} and np.array_equal(plain["x"].cpu().numpy(), ref["x"][:4])
    eng.check_device()


# ---- (d) shapes and statuses ----------------------------------------------------------------------------------

def test_group_subsets_select_columns_in_the_fixed_order(eng, batch, full16):
    from learningagileflight_se3_amd import _lib
    n = 4
    names = {g: list(_lib.SENS_COLUMNS[g]) for g in GROUPS}
    assert full16["columns"] == names["theta"] + names["ini"] + names["goal"]
    assert full16["dx"].shape == (NS, 23, 51, 13) and full16["du"].shape == (NS, 23, 50, 4)
    assert full16["gain"].shape == (NS, 4, 23) and full16["sens_status"].dtype == np.int32
    # dx at stage 0: the identity in the ini_state columns, zero in the others
    live = full16["sens_status"] == 0
    assert np.all(full16["dx"][live][:, SL["ini"], 0, :] == np.eye(13))
    assert np.all(full16["dx"][:, SL["theta"], 0, :] == 0.0) and np.all(full16["dx"][:, SL["goal"], 0, :] == 0.0)
    for mask in range(1, 8):
        sel = [g for i, g in enumerate(GROUPS) if mask >> i & 1]
        # given in reverse: the column order does not follow the order of the argument
        out = _np(eng.ocp_sensitivity_ex(*_args(batch, n), groups=tuple(reversed(sel))))
        cols = np.concatenate([np.arange(23)[SL[g]] for g in sel])
        P = len(cols)
        assert P == sum({"theta": 7, "ini": 13, "goal": 3}[g] for g in sel)
        assert out["columns"] == [full16["columns"][c] for c in cols]
        assert out["dx"].shape == (n, P, 51, 13) and out["du"].shape == (n, P, 50, 4) and out["gain"].shape == (n, 4, P)
        assert np.array_equal(out["dx"], full16["dx"][:n, cols]), mask
        assert np.array_equal(out["du"], full16["du"][:n, cols]), mask
        assert np.array_equal(out["gain"], full16["gain"][:n][:, :, cols]), mask
        same = _np(eng.ocp_sensitivity_ex(*_args(batch, n), groups=mask, want=("gain",)))   # the bit mask itself
        assert np.array_equal(same["gain"], out["gain"])
    one = _np(eng.ocp_sensitivity_ex(*_args(batch, 1)))
    assert one["dx"].shape == (1, 23, 51, 13) and one["du"].shape == (1, 23, 50, 4) and one["gain"].shape == (1, 4, 23)
    assert np.array_equal(one["dx"][0], full16["dx"][0]) and np.array_equal(one["gain"][0], full16["gain"][0])


def test_unconverged_solves_give_zero_outputs(batch):
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(max_iter=3)
    out = e.ocp_sensitivity_ex(*_args(batch, 2))
    torch.cuda.synchronize()
    assert out["status"].tolist() == [2, 2] and out["sens_status"].tolist() == [1, 1]
    assert torch.all(out["dx"] == 0.0) and torch.all(out["du"] == 0.0) and torch.all(out["gain"] == 0.0)
    e.check_device()                                     # no device error word


def test_no_groups_with_outputs_is_refused(eng, batch):
    from learningagileflight_se3_amd import _lib
    for bad in (0, (), 8, 15):
        with pytest.raises(ValueError):
            eng.ocp_sensitivity_ex(*_args(batch, 2), groups=bad)
    with pytest.raises(ValueError):
        eng.ocp_sensitivity_ex(*_args(batch, 2), groups=("theta", "u_last"))
    # the C entry point itself: refused before any launch (the output pointer is never used)
    L = _lib.load()
    buf = torch.zeros(8, dtype=torch.float64, device=eng.device)
    ptr = ctypes.c_void_p(buf.data_ptr())
    for bad in (0, 8, 1 | 16):
        for which in range(3):
            outs = [ptr if i == which else None for i in range(3)]
            rc = L.lafse3_ocp_sensitivity_ex(eng._ctx, 2, *([ptr] * 5), None, *([None] * 6), bad, *outs, None, None)
            assert rc == -1 and b"groups" in L.lafse3_last_error()
    assert torch.all(buf == 0.0)


# ---- (e) autograd ----------------------------------------------------------------------------------------------

def test_autograd_through_mpc_layer_to_ini_state_and_goal(eng, batch, full16):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    sb, n, dev = batch, NS, eng.device
    rng = np.random.default_rng(2025)
    W_x, W_u = rng.standard_normal((n, 51, 13)), rng.standard_normal((n, 50, 4))
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True)
    ini, goal = leaf(sb["ini"][:n]), leaf(sb["goal"][:n])
    x, u, status = mpc_layer(eng, ini, goal, sb["p"][:n], sb["a"][:n], sb["t"][:n])
    assert x.dtype == torch.float64 and not status.requires_grad
    assert np.array_equal(x.detach().cpu().numpy(), full16["x"])
    ((torch.as_tensor(W_x, device=dev) * x).sum() + (torch.as_tensor(W_u, device=dev) * u).sum()).backward()
    assert ini.grad.dtype == goal.grad.dtype == torch.float64
    assert ini.grad.shape == (n, 13) and goal.grad.shape == (n, 3)
    got = np.concatenate([ini.grad.cpu().numpy(), goal.grad.cpu().numpy()], axis=1)
    dx, du = full16["dx"][:, 7:], full16["du"][:, 7:]
    live = (full16["sens_status"] == 0)[:, None]
    Jw = live * (np.einsum("bqki,bki->bq", dx, W_x) + np.einsum("bqka,bka->bq", du, W_u))
    mag = np.einsum("bqki,bki->bq", np.abs(dx), np.abs(W_x)) + np.einsum("bqka,bka->bq", np.abs(du), np.abs(W_u))
    rel = np.abs(got - Jw) / mag
    print(f"mpc_layer autograd vs einsum of the Jacobian: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    # a float32 goal leaf alone: only its group is asked for, and the gradient comes back in float32
    g32 = torch.tensor(sb["goal"][:4], dtype=torch.float32, device=dev, requires_grad=True)
    x4, _, _ = mpc_layer(eng, sb["ini"][:4], g32, sb["p"][:4], sb["a"][:4], sb["t"][:4])
    x4.sum().backward()
    assert g32.grad.dtype == torch.float32 and g32.grad.shape == (4, 3) and bool(torch.all(torch.isfinite(g32.grad)))


def test_autograd_through_mpc_policy(eng, batch, full16):
    from learningagileflight_se3_amd.diff_mpc import mpc_policy
    sb, n, dev = batch, NS, eng.device
    rng = np.random.default_rng(7)
    w = rng.standard_normal((n, 4))
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True)
    ini, goal, p, a, t = (leaf(sb[k][:n]) for k in ("ini", "goal", "p", "a", "t"))
    u0, status = mpc_policy(eng, ini, goal, p, a, t)
    assert u0.shape == (n, 4) and u0.dtype == torch.float64 and not status.requires_grad
    assert np.array_equal(u0.detach().cpu().numpy(), full16["u"][:, 0])
    (torch.as_tensor(w, device=dev) * u0).sum().backward()
    got = np.concatenate([v.grad.cpu().numpy().reshape(n, -1) for v in (p, a, t, ini, goal)], axis=1)   # column order
    live = (full16["sens_status"] == 0)[:, None]
    ref = live * np.einsum("baq,ba->bq", full16["gain"], w)
    mag = np.einsum("baq,ba->bq", np.abs(full16["gain"]), np.abs(w))
    rel = np.abs(got - ref) / np.where(mag > 0, mag, 1.0)
    print(f"mpc_policy autograd vs gain contracted with w: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    assert t.grad.shape == (n,) and ini.grad.shape == (n, 13)


def test_closed_loop_of_two_steps_backpropagates_to_the_first_state(eng, batch):
    from learningagileflight_se3_amd.diff_mpc import mpc_policy
    sb, n, dev = batch, 4, eng.device
    Wf = torch.as_tensor(np.random.default_rng(11).standard_normal((4, 13)) * 0.1, device=dev)
    x0 = torch.tensor(sb["ini"][:n], dtype=torch.float64, device=dev, requires_grad=True)
    rest = (sb["goal"][:n], sb["p"][:n], sb["a"][:n], sb["t"][:n])
    u0, st0 = mpc_policy(eng, x0, *rest)
    x1 = x0 + 0.1 * torch.tanh(u0 @ Wf)                  # a fixed differentiable stand-in for the plant
    u1, st1 = mpc_policy(eng, x1, *rest)
    u1.square().sum().backward()
    assert int(st0.max()) <= 1 and int(st1.max()) <= 1
    g = x0.grad.cpu().numpy()
    print(f"closed loop: |dL/dx0| max {np.abs(g).max():.3e}")
    assert g.shape == (n, 13) and np.all(np.isfinite(g)) and np.all(np.abs(g).max(axis=1) > 0)


def test_instances_without_sensitivity_contribute_zero_gradient(batch):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer, mpc_policy
    from learningagileflight_se3_amd.engine import Engine
    sb, n = batch, 2
    e = Engine(max_iter=3)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device=e.device, requires_grad=True)
    ini, goal, t = leaf(sb["ini"][:n]), leaf(sb["goal"][:n]), leaf(sb["t"][:n])
    u0, status = mpc_policy(e, ini, goal, sb["p"][:n], sb["a"][:n], t)
    assert status.tolist() == [2, 2]
    x, u, _ = mpc_layer(e, ini, goal, sb["p"][:n], sb["a"][:n], t)
    (u0.sum() + x.sum() + u.sum()).backward()
    for v in (ini, goal, t):
        assert bool(torch.all(v.grad == 0.0))
