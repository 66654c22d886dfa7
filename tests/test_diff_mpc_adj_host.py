"""CPU checks of the adjoint route of the MPC layer (diff_mpc.MPCFunctionAdj, mpc_layer(..., backward="adjoint")) on a
stand-in engine with a linear 'solver': the forward pass is one ocp_solve_rec call that keeps the record and the inputs
and no Jacobian, backward() is one ocp_vjp call for the groups that need a gradient, every gradient comes back in its
input's dtype and shape (a broadcast t and a (10,) weights row summed over the batch), and the default ``backward=``
still reaches the existing engine methods with the existing arguments (no device calls)."""
import pytest

torch = pytest.importorskip("torch")

B, N, NX, NU = 3, 4, 13, 4
NCOL = {"theta": 7, "ini": 13, "goal": 3, "weights": 10}
LO = {"theta": 0, "ini": 7, "goal": 20, "weights": 23}
ORDER = ("theta", "ini", "goal", "weights")
REC_W = 5


class _StubEngine:
    """z = J [p, a, t, ini, goal, weights] with a fixed random J: ocp_solve_rec returns z and a record that names the
    instance, ocp_vjp contracts J's selected columns with (g_x, g_u).  It has no ocp_sensitivity* method at all."""

    def __init__(self, seed=0, sens_status=(0, 0, 0)):
        g = torch.Generator().manual_seed(seed)
        self.dx = torch.randn(B, 33, N + 1, NX, dtype=torch.float64, generator=g)
        self.du = torch.randn(B, 33, N, NU, dtype=torch.float64, generator=g)
        self.st = torch.tensor(sens_status, dtype=torch.int32)
        self.solves, self.vjps = [], []

    @staticmethod
    def _theta(ini_state, goal, p_tra, a_tra, t, weights):
        f = lambda v: torch.as_tensor(v).detach().double()
        w = torch.zeros(10, dtype=torch.float64) if weights is None else f(weights)
        w = w.unsqueeze(0).expand(B, 10) if w.dim() == 1 else w
        return torch.cat([f(p_tra), f(a_tra), f(t).reshape(-1, 1).expand(B, 1), f(ini_state), f(goal), w], dim=1)

    def ocp_solve_rec(self, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None, want=()):
        self.solves.append((tuple(want), weights is not None))
        th = self._theta(ini_state, goal, p_tra, a_tra, t, weights)
        return {"x": torch.einsum("bqki,bq->bki", self.dx, th), "u": torch.einsum("bqka,bq->bka", self.du, th),
                "status": torch.zeros(B, dtype=torch.int32), "iters": torch.zeros(B, dtype=torch.int32),
                "rec": torch.arange(B * REC_W, dtype=torch.float64).reshape(B, REC_W)}

    def ocp_vjp(self, ini_state, goal, p_tra, a_tra, t, u_last, weights, rec, g_x=None, g_u=None, groups=ORDER):
        assert torch.equal(rec, torch.arange(B * REC_W, dtype=torch.float64).reshape(B, REC_W))
        self.vjps.append((tuple(groups), [None if v is None else (v.dtype, tuple(v.shape))
                                          for v in (ini_state, goal, p_tra, a_tra, t, u_last, weights)]))
        cols = [c for g in ORDER if g in groups for c in range(LO[g], LO[g] + NCOL[g])]
        grad = torch.einsum("bqki,bki->bq", self.dx[:, cols], g_x) + torch.einsum("bqka,bka->bq", self.du[:, cols], g_u)
        grad = torch.where((self.st != 0).unsqueeze(1), torch.zeros_like(grad), grad)
        return {"grad": grad, "sens_status": self.st, "columns": cols}


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return r(B, NX), r(B, 3), r(B, 3), r(B, 3), r(B), r(B, 10)


def _cotangents(seed=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N + 1, NX, dtype=torch.float64, generator=g),
            torch.randn(B, N, NU, dtype=torch.float64, generator=g))


def _full_gradient(eng, W_x, W_u):
    return torch.einsum("bqki,bki->bq", eng.dx, W_x) + torch.einsum("bqka,bka->bq", eng.du, W_u)


def _same(got, want):
    """Equal up to the summation order of the two einsums (float64) or one float32 rounding."""
    tol = 1e-13 if got.dtype == torch.float64 else 2.0 ** -22
    return torch.allclose(got.double(), want.double(), rtol=tol, atol=tol * float(want.abs().max()))


SLICES = (slice(7, 20), slice(20, 23), slice(0, 3), slice(3, 6), 6, slice(23, 33))   # ini goal p a t weights


def test_forward_keeps_the_record_and_backward_asks_for_the_needed_groups():
    from learningagileflight_se3_amd.diff_mpc import MPCFunctionAdj, mpc_layer
    ini, goal, p, a, t, w = _inputs()
    W_x, W_u = _cotangents()
    eng = _StubEngine(sens_status=(0, 2, 0))
    gl, wl = goal.clone().requires_grad_(), w.clone().requires_grad_()
    x, u, status = mpc_layer(eng, ini, gl, p, a, t, weights=wl, backward="adjoint")
    assert eng.solves == [(("x", "u"), True)] and eng.vjps == []          # one solve, no dx / du, nothing else yet
    assert type(x.grad_fn).__name__.startswith(MPCFunctionAdj.__name__)
    assert x.requires_grad and u.requires_grad and not status.requires_grad
    # what the node keeps: the record and the six tensor inputs, never a Jacobian (B x P x 863 here B x P x 36)
    saved = x.grad_fn.saved_tensors
    assert sum(v.numel() for v in saved) == B * REC_W + sum(v.numel() for v in (ini, goal, p, a, t, w))
    loss = (W_x * x).sum() + (W_u * u).sum()
    loss.backward(retain_graph=True)
    assert [c[0] for c in eng.vjps] == [("goal", "weights")]              # only the groups that need a gradient
    assert eng.vjps[0][1][5] is None and eng.vjps[0][1][6] == (torch.float64, (B, 10))
    ref = _full_gradient(eng, W_x, W_u)
    ref[1] = 0.0                                                          # sens_status 2: a zero row
    assert _same(wl.grad, ref[:, 23:]) and _same(gl.grad, ref[:, 20:23])
    # backward() again on the retained graph: one more ocp_vjp, the same gradients accumulated once more
    loss.backward()
    assert len(eng.vjps) == 2 and _same(wl.grad, 2 * ref[:, 23:])
    # every input a leaf, weights None: three groups, weights passed through as None
    eng = _StubEngine(seed=3)
    leaves = [v.clone().requires_grad_() for v in (ini, goal, p, a, t)]
    x, u, _ = mpc_layer(eng, *leaves, backward="adjoint")
    ((W_x * x).sum() + (W_u * u).sum()).backward()
    assert eng.solves == [(("x", "u"), False)] and eng.vjps[0][0] == ("theta", "ini", "goal")
    assert eng.vjps[0][1][6] is None
    ref = _full_gradient(eng, W_x, W_u)
    for leaf, sl in zip(leaves, SLICES):
        assert leaf.grad.shape == leaf.shape and _same(leaf.grad, ref[:, sl])
    # nothing needs a gradient: a plain solve, and no ocp_vjp can follow
    eng = _StubEngine()
    x, u, _ = mpc_layer(eng, ini, goal, p, a, t, weights=w, backward="adjoint")
    assert eng.solves == [(("x", "u"), True)] and not x.requires_grad and not u.requires_grad


def test_gradients_come_back_in_the_inputs_dtypes_and_shapes():
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    ini, goal, p, a, t, w = _inputs(4)
    W_x, W_u = _cotangents(5)
    eng = _StubEngine(seed=6, sens_status=(0, 0, 1))
    ref = _full_gradient(eng, W_x, W_u)
    ref[2] = 0.0
    # float32 DNN outputs, a t of one element and a (10,) weights row
    p32, a32 = p.float().requires_grad_(), a.float().requires_grad_()
    t1 = t[:1].float().requires_grad_()
    w1 = w[0].clone().requires_grad_()
    il = ini.clone().requires_grad_()
    x, u, _ = mpc_layer(eng, il, goal, p32, a32, t1, None, w1, backward="adjoint")
    assert x.dtype == torch.float64 and u.dtype == torch.float64
    ((W_x * x).sum() + (W_u * u).sum()).backward()
    assert eng.vjps[0][0] == ("theta", "ini", "weights")
    assert eng.vjps[0][1][2] == (torch.float32, (B, 3)) and eng.vjps[0][1][4] == (torch.float32, (1,))
    assert p32.grad.dtype == torch.float32 and p32.grad.shape == (B, 3) and _same(p32.grad, ref[:, 0:3].float())
    assert a32.grad.dtype == torch.float32 and _same(a32.grad, ref[:, 3:6].float())
    assert t1.grad.dtype == torch.float32 and t1.grad.shape == (1,)
    assert _same(t1.grad, ref[:, 6].sum(0, keepdim=True).float())      # broadcast over the batch: summed back
    assert w1.grad.dtype == torch.float64 and w1.grad.shape == (10,) and _same(w1.grad, ref[:, 23:].sum(0))
    assert il.grad.shape == (B, NX) and _same(il.grad, ref[:, 7:20])
    # a float32 (B, 10) weights tensor and a 0-dim t
    w32 = w.float().requires_grad_()
    t0 = t[0].clone().requires_grad_()
    x, u, _ = mpc_layer(eng, ini, goal, p, a, t0, weights=w32, backward="adjoint")
    ((W_x * x).sum() + (W_u * u).sum()).backward()
    assert w32.grad.dtype == torch.float32 and _same(w32.grad, ref[:, 23:].float())
    assert t0.grad.shape == () and _same(t0.grad, ref[:, 6].sum())


def test_the_default_route_is_unchanged_and_a_wrong_keyword_is_refused():
    """backward="jacobian", given or not, reaches the existing engine methods with the existing arguments; the stand-in
    of the adjoint route has none of them."""
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    ini, goal, p, a, t, w = _inputs()

    class Earlier:
        def __init__(self):
            self.calls = []

        def _record(self, name, args, kw):
            self.calls.append((name, len(args), {k: v for k, v in kw.items() if k in ("groups", "want")}))
            raise KeyError(name)

        def ocp_sensitivity(self, *args, **kw):
            self._record("ocp_sensitivity", args, kw)

        def ocp_sensitivity_ex(self, *args, **kw):
            self._record("ocp_sensitivity_ex", args, kw)

        def ocp_sensitivity_w(self, *args, **kw):
            self._record("ocp_sensitivity_w", args, kw)

    for kw in ({}, {"backward": "jacobian"}):
        e = Earlier()
        with pytest.raises(KeyError, match="ocp_sensitivity"):
            mpc_layer(e, ini, goal, p.clone().requires_grad_(), a, t, **kw)
        with pytest.raises(KeyError, match="ocp_sensitivity_ex"):
            mpc_layer(e, ini.clone().requires_grad_(), goal, p, a, t, **kw)
        with pytest.raises(KeyError, match="ocp_sensitivity_w"):
            mpc_layer(e, ini, goal, p, a, t, weights=w.clone().requires_grad_(), **kw)
        assert e.calls == [("ocp_sensitivity", 6, {"want": ("x", "u", "dx", "du")}),
                           ("ocp_sensitivity_ex", 6, {"groups": ("ini",), "want": ("x", "u", "dx", "du")}),
                           ("ocp_sensitivity_w", 6, {"groups": ("weights",), "want": ("x", "u", "dx", "du")})]
    with pytest.raises(AttributeError):                                  # the adjoint route's engine has no such method
        mpc_layer(_StubEngine(), ini, goal, p.clone().requires_grad_(), a, t)
    with pytest.raises(ValueError, match="backward"):
        mpc_layer(_StubEngine(), ini, goal, p, a, t, backward="forward")
