"""CPU checks of the autograd functions built on Engine.ocp_sensitivity_ex (diff_mpc.MPCFunctionEx through mpc_layer,
diff_mpc.mpc_policy) on a stand-in engine: the parameter groups asked for follow needs_input_grad, the gradients come
back in the inputs' dtypes and shapes, a t of one element is summed back, and instances without a sensitivity give
zero.  Also lafse3_sens_columns for all 8 masks (no device calls)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

B, N, NX, NU = 3, 4, 13, 4
NCOL = {"theta": 7, "ini": 13, "goal": 3}
ORDER = ("theta", "ini", "goal")


class _StubEngine:
    """ocp_sensitivity_ex of a linear 'solver' z = J [p, a, t, ini, goal]: the layer's gradient is exact.  Records
    the groups and outputs each call asked for."""

    def __init__(self, seed=0, sens_status=(0, 0, 0)):
        g = torch.Generator().manual_seed(seed)
        self.dx = torch.randn(B, 23, N + 1, NX, dtype=torch.float64, generator=g)
        self.du = torch.randn(B, 23, N, NU, dtype=torch.float64, generator=g)
        self.st = torch.tensor(sens_status, dtype=torch.int32)
        self.calls = []

    def ocp_sensitivity_ex(self, ini_state, goal, p_tra, a_tra, t, u_last=None, groups=ORDER, want=()):
        self.calls.append((tuple(groups), tuple(want)))
        f = lambda v: torch.as_tensor(v).detach().double()
        th = torch.cat([f(p_tra), f(a_tra), f(t).reshape(-1, 1).expand(B, 1), f(ini_state), f(goal)], dim=1)
        cols = [c for g, lo in (("theta", 0), ("ini", 7), ("goal", 20)) if g in groups for c in range(lo, lo + NCOL[g])]
        out = {"x": torch.einsum("bqki,bq->bki", self.dx, th), "u": torch.einsum("bqka,bq->bka", self.du, th),
               "dx": self.dx[:, cols], "du": self.du[:, cols], "gain": self.du[:, cols, 0, :].transpose(1, 2),
               "sens_status": self.st}
        out = {k: v for k, v in out.items() if k in want or k == "sens_status"}
        out["status"] = torch.zeros(B, dtype=torch.int32)
        return out


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return r(B, NX), r(B, 3), r(B, 3), r(B, 3), r(B)


def _weights(seed=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N + 1, NX, dtype=torch.float64, generator=g),
            torch.randn(B, N, NU, dtype=torch.float64, generator=g))


def _full_gradient(eng, W_x, W_u):
    """d(sum W_x x + sum W_u u) / d(column q) of every instance, (B, 23)."""
    return torch.einsum("bqki,bki->bq", eng.dx, W_x) + torch.einsum("bqka,bka->bq", eng.du, W_u)


def test_layer_asks_only_for_the_groups_that_need_a_gradient():
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    ini, goal, p, a, t = _inputs()
    W_x, W_u = _weights()
    for need_ini, need_goal, need_t in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)):
        eng = _StubEngine(sens_status=(0, 2, 0))
        leaves = [v.clone().requires_grad_(bool(n)) for v, n in ((ini, need_ini), (goal, need_goal), (t, need_t))]
        x, u, status = mpc_layer(eng, leaves[0], leaves[1], p, a, leaves[2])
        groups = tuple(g for g, n in zip(ORDER, (need_t, need_ini, need_goal)) if n)
        assert eng.calls == [(groups, ("x", "u", "dx", "du"))]
        assert x.requires_grad and u.requires_grad and not status.requires_grad
        ((W_x * x).sum() + (W_u * u).sum()).backward()
        ref = _full_gradient(eng, W_x, W_u)
        ref[1] = 0.0                                        # sens_status 2: no gradient from that instance
        for leaf, need, sl in zip(leaves, (need_ini, need_goal, need_t), (slice(7, 20), slice(20, 23), 6)):
            if not need:
                assert leaf.grad is None
                continue
            assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype
            want = ref[:, sl]
            assert torch.allclose(leaf.grad, want, rtol=1e-13, atol=1e-13 * float(ref.abs().max()))
            assert bool(torch.all(leaf.grad[1] == 0.0))


def test_layer_without_state_or_goal_gradient_keeps_the_theta_only_function():
    """mpc_layer goes through ocp_sensitivity_ex only when ini_state or goal needs a gradient: an engine that has
    ocp_sensitivity alone (tests/test_diff_mpc_host.py) keeps working for theta."""
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    ini, goal, p, a, t = _inputs()

    class ThetaOnly:
        def ocp_sensitivity(self, *args, **kw):
            raise KeyError("theta-only path")

    with pytest.raises(KeyError, match="theta-only path"):
        mpc_layer(ThetaOnly(), ini, goal, p.clone().requires_grad_(), a, t)
    with pytest.raises(AttributeError):
        mpc_layer(ThetaOnly(), ini.clone().requires_grad_(), goal, p, a, t)


def test_dtypes_shapes_and_a_broadcast_t():
    from learningagileflight_se3_amd.diff_mpc import mpc_layer, mpc_policy
    ini, goal, p, a, t = _inputs(3)
    W_x, W_u = _weights(4)
    eng = _StubEngine(seed=5)
    ini32 = ini.float().requires_grad_()
    goal64 = goal.clone().requires_grad_()
    p32 = p.float().requires_grad_()
    t1 = torch.tensor(0.7, dtype=torch.float32, requires_grad=True)      # one element, broadcast over the batch
    x, u, _ = mpc_layer(eng, ini32, goal64, p32, a, t1)
    assert eng.calls[-1][0] == ORDER
    ((W_x * x).sum() + (W_u * u).sum()).backward()
    ref = _full_gradient(eng, W_x, W_u)
    assert (ini32.grad.dtype, goal64.grad.dtype, p32.grad.dtype, t1.grad.dtype) == \
        (torch.float32, torch.float64, torch.float32, torch.float32)
    assert ini32.grad.shape == (B, NX) and goal64.grad.shape == (B, 3) and p32.grad.shape == (B, 3) and t1.grad.shape == ()
    tol = 2.0 ** -22 * float(ref.abs().max())
    assert float((ini32.grad.double() - ref[:, 7:20]).abs().max()) <= tol
    assert float((p32.grad.double() - ref[:, 0:3]).abs().max()) <= tol
    assert torch.allclose(goal64.grad, ref[:, 20:23], rtol=1e-13, atol=1e-13 * float(ref.abs().max()))
    assert abs(float(t1.grad) - float(ref[:, 6].sum())) <= 3 * tol
    # the policy: gain alone, and only the groups in use
    eng = _StubEngine(seed=6, sens_status=(0, 0, 1))
    w = torch.randn(B, NU, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    ini64 = ini.clone().requires_grad_()
    u0, status = mpc_policy(eng, ini64, goal, p, a, t)
    assert eng.calls == [(("ini",), ("u", "gain"))] and u0.shape == (B, NU) and not status.requires_grad
    (w * u0).sum().backward()
    ref = torch.einsum("bqa,ba->bq", eng.du[:, 7:20, 0, :], w)
    ref[2] = 0.0
    assert torch.allclose(ini64.grad, ref, rtol=1e-13, atol=1e-13 * float(ref.abs().max()))
    # no input needs a gradient: no sensitivity output is asked for
    eng = _StubEngine(seed=8)
    u0, _ = mpc_policy(eng, ini, goal, p, a, t)
    assert eng.calls[-1][1] == ("u",) and not u0.requires_grad


def test_sens_columns_for_all_masks():
    from learningagileflight_se3_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("liblafse3.so not built: run python -c 'import __graft_entry__ as g; g.build()'")
    L = _lib.load()
    for mask in range(8):
        P = 7 * (mask & 1) + 13 * (mask >> 1 & 1) + 3 * (mask >> 2 & 1)
        assert L.lafse3_sens_columns(mask) == P
        assert sum(len(_lib.SENS_COLUMNS[g]) for g, bit in _lib.SENS_GROUPS.items() if mask & bit) == P
    assert L.lafse3_sens_columns(8) == -1 and b"lafse3_sens_columns" in L.lafse3_last_error()
    assert list(_lib.SENS_GROUPS.items()) == [("theta", 1), ("ini", 2), ("goal", 4)]
