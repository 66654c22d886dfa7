"""GPU tests of the analytic trajectory sensitivities (lafse3_ocp_sensitivity, csrc/sens.inc) and of the
differentiable MPC layer built on them (learningagileflight_se3_amd/diff_mpc.py).

Run on an MI355X:  python -m pytest tests/test_gpu_sens.py -m gpu -q

Inputs: scenario.synthetic_batch(64, seed=2025), the batch of tests/test_gpu_parity.py, with p, a, t widened to
float64.  The independent reference is a central finite difference of the CPU oracle's solve (oracle.solve; a_tra
through oracle.rd2quat) at h = 1e-4 and 2h for each of the 7 parameters theta = (p_tra[3], a_tra[3], t).

Admission.  A (sample, parameter) pair is admitted when its four perturbed oracle solves end with status <= 1 and
e = max|J_h - J_2h| / max|J_h| <= 1e-3 over the (N+1) 13 + N 4 trajectory entries (863 at N = 50): the finite
difference is then a usable yardstick there (no other local optimum, no active-set change inside +-2h).  It is
decided from the oracle alone, before any GPU value is looked at; at most 15 % of the pairs may be left out (the
oracle admits 103 of the first 16 samples' 112 pairs; the short-horizon test states its own count).

Bound.  For admitted pairs on instances with sens_status 0:  err = max|J_gpu - J_h| / max|J_h| <= 10 e + F.
10 e covers the finite difference's own truncation / solver noise (its h-versus-2h disagreement); F covers what is
not the finite difference's fault: the barrier smoothing at the final mu and the 1e-8 KKT tolerance of both optima.
F was MEASURED on the first GPU run as the largest err - 10 e and committed rounded up to the next power of ten,
never above the admission threshold 1e-3 (above it the test could not tell a right column from a wrong one):
    horizon 50, 103 pairs: max(err - 10 e) = 3.914e-04 (sample 13, a_tra[2]: err 4.321e-04, e 4.068e-06), median err
                           1.302e-06, max err 1.578e-03 (a pair whose own e carries it);
    horizon 20,  21 pairs: max(err - 10 e) = 2.230e-06, median err 1.305e-06.
So F = 1e-3.  On that run: sens_status 0 on all 16 + 4 instances; the IFT-mode consistency below 3.856e-07; the
autograd gradient against the einsum of the Jacobian 8.2e-16; dL/dtheta against the oracle's finite difference at
1.1e-03 of its bound.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sens_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

F = Y.F              # the bound's F, measured on this file's first GPU run (module docstring)
NS = 16              # samples of the finite-difference comparison
THETA = range(0, 7)  # the columns of sens_yardstick.oracle_fd's z that are theta


@pytest.fixture(scope="module")
def eng():
    Y.require_gpu()
    from learningagileflight_se3_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def batch():
    return Y.batch()


@pytest.fixture(scope="module")
def fd16(batch):
    return Y.oracle_fd(batch, NS, 50, THETA)


@pytest.fixture(scope="module")
def sens64(eng, batch):
    """One ocp_sensitivity launch on the 64 samples, shared by the tests below (never modified)."""
    sb = batch
    out = eng.ocp_sensitivity(sb["ini"], sb["goal"], sb["p"], sb["a"], sb["t"], want=("x", "u", "lam", "cost", "dx", "du"))
    torch.cuda.synchronize()
    return Y.to_numpy(out)


def test_outputs_are_the_plain_solves_bit_for_bit(eng, batch, sens64):
    sb = batch
    args = (sb["ini"], sb["goal"], sb["p"], sb["a"], sb["t"])
    gargs = (sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    e2 = type(eng)()                                  # a context that never ran the sensitivity kernel
    ref = {k: v.cpu().numpy() for k, v in e2.ocp_solve(*args).items()}
    g_ref = [v.cpu().numpy() for v in e2.sol_gradient(*gargs, want_rewards=True, grad_mode=1)]
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert np.array_equal(sens64[k], ref[k]), k
    assert sens64["dx"].shape == (64, 7, 51, 13) and sens64["du"].shape == (64, 7, 50, 4)
    assert sens64["sens_status"].dtype == np.int32
    assert np.all(sens64["dx"][:, :, 0, :] == 0.0)
    assert np.all(np.isfinite(sens64["dx"])) and np.all(np.isfinite(sens64["du"]))
    # workspace reuse: launches that follow a sensitivity launch on the same context are what they were
    eng.ocp_sensitivity(*args)
    after = {k: v.cpu().numpy() for k, v in eng.ocp_solve(*args).items()}
    g_after = [v.cpu().numpy() for v in eng.sol_gradient(*gargs, want_rewards=True, grad_mode=1)]
    for k in ref:
        assert np.array_equal(after[k], ref[k]), k
    for a, b in zip(g_after, g_ref):
        assert np.array_equal(a, b)
    # dx / du alone, and neither (then the call is the plain solve)
    only = eng.ocp_sensitivity(*(v[:4] for v in args), want=("du",))
    assert set(only) == {"du", "status", "iters", "sens_status"}
    assert np.array_equal(only["du"].cpu().numpy(), sens64["du"][:4])
    plain = eng.ocp_sensitivity(*(v[:4] for v in args), want=("x",))
    assert set(plain) == {"x", "status", "iters"} and np.array_equal(plain["x"].cpu().numpy(), ref["x"][:4])


def test_against_oracle_finite_differences(sens64, fd16):
    st = sens64["sens_status"][:NS]
    assert np.sum(st == 2) <= 1, st
    assert np.all(sens64["status"][:NS] <= 1) and np.all(st != 1)
    Y.check_against_fd(Y.traj(sens64["dx"][:NS], sens64["du"][:NS]), st, fd16, "horizon 50", F)


def test_short_horizon(batch):
    """horizon 20: the lane <= N guards and the output strides of another N; B = 1 for shapes and status.
    The 15 % admission condition is stated for the 112 pairs of horizon 50.  Here the oracle alone admits 21 of the 28
    pairs: sample 1's traversal time (3.7 s) lies outside the 2 s horizon, so its trajectory does not depend on theta
    (max|J_h| ~ 4e-8, finite-difference noise) and none of its 7 pairs can be admitted; that count is the condition."""
    from learningagileflight_se3_amd.engine import Engine
    sb = batch
    e = Engine(horizon=20)
    n = 4
    t = sb["t"][:n]
    fd = Y.oracle_fd(sb, n, 20, THETA)
    out = e.ocp_sensitivity(sb["ini"][:n], sb["goal"][:n], sb["p"][:n], sb["a"][:n], t)
    g = {k: v.cpu().numpy() for k, v in out.items()}
    assert g["dx"].shape == (n, 7, 21, 13) and g["du"].shape == (n, 7, 20, 4)
    assert np.all(g["dx"][:, :, 0, :] == 0.0)
    ref = e.ocp_solve(sb["ini"][:n], sb["goal"][:n], sb["p"][:n], sb["a"][:n], t)
    assert np.array_equal(g["x"], ref["x"].cpu().numpy()) and np.array_equal(g["u"], ref["u"].cpu().numpy())
    Y.check_against_fd(Y.traj(g["dx"], g["du"]), g["sens_status"], fd, "horizon 20", F, max_left_out=7 / 28)
    one = e.ocp_sensitivity(sb["ini"][:1], sb["goal"][:1], sb["p"][:1], sb["a"][:1], t[:1])
    assert one["dx"].shape == (1, 7, 21, 13) and one["du"].shape == (1, 7, 20, 4)
    assert int(one["status"][0]) <= 1 and int(one["sens_status"][0]) == int(g["sens_status"][0])
    assert np.array_equal(one["dx"].cpu().numpy()[0], g["dx"][0])


def _round1_f32(t32):
    """round(t, 1) as MODE_GRAD takes it from a float32 DNN output (ipm_kernel.hip round1_f32)."""
    y = (np.asarray(t32, np.float32) * np.float32(10.0)).astype(np.float32)
    return (np.rint(y).astype(np.float64) / 10.0).astype(np.float32).astype(np.float64)


IFT_BAR = 1e-5       # the project's parity scale (tests/test_gpu_parity.py)


def test_consistent_with_the_ift_gradient_mode(eng, batch):
    """R(x* + 1e-3 dx*/dtheta_q), q < 6, against the six probe rewards of sol_gradient's IFT mode: the same
    factorisation and sweeps, reached through MODE_SOLVE instead of MODE_GRAD.  The nominal problems are made equal
    (t rounded to one decimal as MODE_GRAD does); what is left is MODE_GRAD's float32 angle norm (magni_f32)."""
    sb = batch
    _, R9, S9 = eng.sol_gradient(sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"], want_rewards=True, grad_mode=1)
    R9, S9 = R9.cpu().numpy(), S9.cpu().numpy()
    out = eng.ocp_sensitivity(sb["ini"], sb["goal"], sb["p"], sb["a"], _round1_f32(sb["dnn_out"][:, 6]))
    st, ss = out["status"].cpu().numpy(), out["sens_status"].cpu().numpy()
    both = (ss == 0) & (st <= 1) & np.all(S9[:, :7] <= 1, axis=1)
    print(f"IFT consistency: {int(both.sum())} of 64 samples on both paths")
    assert both.mean() >= 0.9
    worst = 0.0
    for q in range(6):
        Rq = eng.reward(out["x"] + 1e-3 * out["dx"][:, q], sb["goal"], sb["gate12"]).cpu().numpy()
        d = np.abs(Rq - R9[:, 1 + q]) / np.maximum(1.0, np.abs(R9[:, 1 + q]))
        worst = max(worst, float(d[both].max()))
    print(f"IFT consistency: max relative reward difference {worst:.3e} (bar {IFT_BAR:.0e})")
    assert worst <= IFT_BAR


def test_unconverged_solves_give_zero_sensitivity(batch):
    from learningagileflight_se3_amd.engine import Engine
    sb = batch
    e = Engine(max_iter=3)
    out = e.ocp_sensitivity(sb["ini"][:2], sb["goal"][:2], sb["p"][:2], sb["a"][:2], sb["t"][:2])
    torch.cuda.synchronize()
    assert out["status"].tolist() == [2, 2] and out["sens_status"].tolist() == [1, 1]
    assert torch.all(out["dx"] == 0.0) and torch.all(out["du"] == 0.0)
    e.check_device()                                     # no device error word


def test_autograd_through_mpc_layer(eng, batch, sens64, fd16):
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    sb = batch
    n = NS
    dev = eng.device
    rng = np.random.default_rng(2025)
    W_x, W_u = rng.standard_normal((n, 51, 13)), rng.standard_normal((n, 50, 4))
    leaf = lambda v: torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True)
    p, a, t = leaf(sb["dnn_out"][:n, :3]), leaf(sb["dnn_out"][:n, 3:6]), leaf(sb["dnn_out"][:n, 6])
    x, u, status = mpc_layer(eng, sb["ini"][:n], sb["goal"][:n], p, a, t)
    assert x.dtype == torch.float64 and not status.requires_grad
    assert np.array_equal(x.detach().cpu().numpy(), sens64["x"][:n])          # float32 leaves widen to the same inputs
    L = (torch.as_tensor(W_x, device=dev) * x).sum() + (torch.as_tensor(W_u, device=dev) * u).sum()
    L.backward()
    assert p.grad.dtype == a.grad.dtype == t.grad.dtype == torch.float32
    assert p.grad.shape == (n, 3) and a.grad.shape == (n, 3) and t.grad.shape == (n,)
    cat = lambda gp, ga, gt: np.concatenate([gp.cpu().numpy(), ga.cpu().numpy(), gt.cpu().numpy()[:, None]], axis=1)
    got = cat(p.grad, a.grad, t.grad)
    # The gradient is formed in float64 and rounded once to the leaves' dtype, so the 1e-12 comparison with the
    # einsum of the returned Jacobian is made on float64 leaves of the same values (relative to sum |J| |W|, the
    # scale of the sum's rounding), and the float32 gradients must be exactly those rounded to float32.
    p64, a64, t64 = (v.detach().double().requires_grad_() for v in (p, a, t))
    x64, u64, _ = mpc_layer(eng, sb["ini"][:n], sb["goal"][:n], p64, a64, t64)
    ((torch.as_tensor(W_x, device=dev) * x64).sum() + (torch.as_tensor(W_u, device=dev) * u64).sum()).backward()
    got64 = cat(p64.grad, a64.grad, t64.grad)
    assert got64.dtype == np.float64 and np.array_equal(got, got64.astype(np.float32))
    live = (sens64["sens_status"][:n] == 0)[:, None]
    Jw = live * (np.einsum("bqki,bki->bq", sens64["dx"][:n], W_x) + np.einsum("bqka,bka->bq", sens64["du"][:n], W_u))
    mag = np.einsum("bqki,bki->bq", np.abs(sens64["dx"][:n]), np.abs(W_x)) + \
        np.einsum("bqka,bka->bq", np.abs(sens64["du"][:n]), np.abs(W_u))
    rel = np.abs(got64 - Jw) / mag
    print(f"autograd vs einsum of the Jacobian: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    # against the oracle's finite difference of L on the admitted pairs: |sum W (J_gpu - J_h)| <= sum|W| max|J_gpu -
    # J_h| <= sum|W| (10 e + F) max|J_h| (Hoelder), plus the float32 rounding of the returned gradient
    W = Y.traj(W_x, W_u)                                                      # (n, E)
    L_fd = np.einsum("bqe,be->bq", fd16["J"], W)
    use = fd16["admitted"] & (sens64["sens_status"][:n] == 0)[:, None]
    bound = np.abs(W).sum(-1)[:, None] * (10 * fd16["e"] + F) * fd16["scale"] + 2.0 ** -23 * np.abs(L_fd)
    ratio = np.abs(got - L_fd)[use] / bound[use]
    print(f"dL/dtheta vs oracle finite difference: {int(use.sum())} pairs, max |diff| / bound {ratio.max():.3e}")
    assert ratio.max() <= 1.0
