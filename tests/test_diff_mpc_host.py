"""CPU checks of the differentiable MPC layer's backward arithmetic (learningagileflight_se3_amd/diff_mpc.py):
the vector-Jacobian product against a naive loop, the zero rows of instances without a sensitivity, the dtypes of
the returned gradients, and the autograd plumbing of MPCFunction on a stand-in engine (no device calls)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

B, N, NX, NU = 3, 5, 13, 4


def _random(seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return r(B, 7, N + 1, NX), r(B, 7, N, NU), r(B, N + 1, NX), r(B, N, NU)


def _naive(dx, du, g_x, g_u):
    out = np.zeros((B, 7))
    for b in range(B):
        for q in range(7):
            s = 0.0
            for k in range(N + 1):
                for i in range(NX):
                    s += float(dx[b, q, k, i]) * float(g_x[b, k, i])
            for k in range(N):
                for a in range(NU):
                    s += float(du[b, q, k, a]) * float(g_u[b, k, a])
            out[b, q] = s
    return out


def test_backward_equals_naive_loop():
    from learningagileflight_se3_amd.diff_mpc import mpc_backward
    dx, du, g_x, g_u = _random()
    gp, ga, gt = mpc_backward(dx, du, torch.zeros(B, dtype=torch.int32), g_x, g_u)
    ref = _naive(dx, du, g_x, g_u)
    assert gp.shape == (B, 3) and ga.shape == (B, 3) and gt.shape == (B,)
    got = np.concatenate([gp.numpy(), ga.numpy(), gt.numpy()[:, None]], axis=1)
    assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(np.abs(ref))
    # one of the two incoming gradients missing (autograd passes None for an unused output)
    gp, ga, gt = mpc_backward(dx, du, torch.zeros(B, dtype=torch.int32), g_x, None)
    ref_x = _naive(dx, du, g_x, torch.zeros_like(g_u))
    got = np.concatenate([gp.numpy(), ga.numpy(), gt.numpy()[:, None]], axis=1)
    assert np.max(np.abs(got - ref_x)) <= 1e-13 * np.max(np.abs(ref_x))


def test_rows_without_sensitivity_give_zero():
    from learningagileflight_se3_amd.diff_mpc import mpc_backward
    dx, du, g_x, g_u = _random(1)
    st = torch.tensor([0, 1, 2], dtype=torch.int32)
    gp, ga, gt = mpc_backward(dx, du, st, g_x, g_u)
    ref = _naive(dx, du, g_x, g_u)
    assert np.all(gp.numpy()[1:] == 0.0) and np.all(ga.numpy()[1:] == 0.0) and np.all(gt.numpy()[1:] == 0.0)
    assert np.max(np.abs(np.concatenate([gp[0].numpy(), ga[0].numpy(), gt[0:1].numpy()]) - ref[0])) <= 1e-13 * np.max(np.abs(ref))
    # a NaN Jacobian of a masked row must not leak through (0 * NaN)
    dx[1] = float("nan")
    gp, ga, gt = mpc_backward(dx, du, st, g_x, g_u)
    assert np.all(gp.numpy()[1] == 0.0) and float(gt[1]) == 0.0


def test_gradients_in_the_inputs_dtypes():
    from learningagileflight_se3_amd.diff_mpc import mpc_backward
    dx, du, g_x, g_u = _random(2)
    st = torch.zeros(B, dtype=torch.int32)
    f32 = (torch.float32,) * 3
    gp, ga, gt = mpc_backward(dx, du, st, g_x.float(), g_u.float(), dtypes=f32)
    assert gp.dtype == ga.dtype == gt.dtype == torch.float32
    ref = _naive(dx, du, g_x.float(), g_u.float())          # accumulated in float64, rounded once at the end
    got = np.concatenate([gp.numpy(), ga.numpy(), gt.numpy()[:, None]], axis=1)
    assert np.array_equal(got, ref.astype(np.float32)) or np.max(np.abs(got - ref)) <= 2.0 ** -23 * np.max(np.abs(ref))
    gp, ga, gt = mpc_backward(dx, du, st, g_x, g_u, dtypes=(torch.float64, torch.float32, torch.float64))
    assert (gp.dtype, ga.dtype, gt.dtype) == (torch.float64, torch.float32, torch.float64)


class _StubEngine:
    """ocp_sensitivity of a linear 'solver': x = X0 + sum_q dx_q theta_q, so the layer's gradient is exact."""

    def __init__(self, seed=3, sens_status=(0, 0, 0)):
        self.dx, self.du, _, _ = _random(seed)
        self.st = torch.tensor(sens_status, dtype=torch.int32)

    def ocp_sensitivity(self, ini_state, goal, p_tra, a_tra, t, u_last=None, want=()):
        th = torch.cat([p_tra.double(), a_tra.double(), t.double().reshape(-1, 1)], dim=1)
        return {"x": torch.einsum("bqki,bq->bki", self.dx, th), "u": torch.einsum("bqka,bq->bka", self.du, th),
                "dx": self.dx, "du": self.du, "sens_status": self.st,
                "status": torch.zeros(B, dtype=torch.int32), "iters": torch.zeros(B, dtype=torch.int32)}


def test_autograd_through_the_layer_float32_leaves():
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    eng = _StubEngine(sens_status=(0, 2, 0))
    g = torch.Generator().manual_seed(5)
    p = torch.randn(B, 3, generator=g).requires_grad_()
    a = torch.randn(B, 3, generator=g).requires_grad_()
    t = torch.randn(B, generator=g).requires_grad_()
    _, _, W_x, W_u = _random(4)
    x, u, status = mpc_layer(eng, torch.zeros(B, NX), torch.zeros(B, 3), p, a, t)
    assert x.dtype == torch.float64 and x.requires_grad and u.requires_grad and not status.requires_grad
    ((W_x * x).sum() + (W_u * u).sum()).backward()
    assert p.grad.dtype == a.grad.dtype == t.grad.dtype == torch.float32
    assert p.grad.shape == (B, 3) and a.grad.shape == (B, 3) and t.grad.shape == (B,)
    ref = _naive(eng.dx, eng.du, W_x, W_u)
    ref[1] = 0.0                                             # sens_status 2: no gradient from that instance
    got = np.concatenate([p.grad.numpy(), a.grad.numpy(), t.grad.numpy()[:, None]], axis=1)
    assert np.max(np.abs(got - ref)) <= 2.0 ** -23 * np.max(np.abs(ref))
    assert np.all(got[1] == 0.0)
