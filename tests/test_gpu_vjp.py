"""GPU tests of the adjoint backward from a saved optimum: lafse3_ocp_solve_rec / lafse3_ocp_vjp (csrc/vjp.inc) and
diff_mpc.mpc_layer(..., backward="adjoint").

Run on an MI355X:  python -m pytest tests/test_gpu_vjp.py -m gpu -q -s

Inputs: tests/sens_w_cases.py's batch under the weight rows D and G, horizons 50 (samples 0..15) and 20, 2, 1 (samples
0..7, that module's case_t; at horizon 1 the non-zero u_last of tests/test_gpu_sens_w.py): per horizon one launch of
2 n instances, samples 0..n-1 under row D, then the same samples under row G.  Every test asserts sens_status 0 of both
routes on all of them.

(1) Adjoint against forward.  grad = lafse3_ocp_vjp on standard normal g_x, g_u (np.random.default_rng(7)) against
dx, du of lafse3_ocp_sensitivity_w contracted in numpy, relative to, per instance and parameter group, the largest
sum|dx||g_x| + sum|du||g_u| over the group's columns.  The bar follows tests/test_gpu_sens_ex.py's rule for this
identity: the first GPU run's largest value rounded up to the next power of ten, never above 1e-5.  First GPU run,
largest relative difference per horizon and group (sens_status 0 on every instance of both routes):
    horizon 50 (32 instances)  theta 2.969e-15  ini 3.253e-09  goal 7.274e-16  weights 1.583e-15
    horizon 20 (16)            theta 1.500e-15  ini 4.008e-08  goal 1.724e-15  weights 9.157e-15
    horizon  2 (16)            theta 1.464e-15  ini 3.741e-16  goal 1.976e-15  weights 7.801e-16
    horizon  1 (16)            theta 0          ini 1.015e-15  goal 0          weights 6.309e-16
and with one of the two gradients NULL the largest was 1.753e-07 (horizon 20, g_u alone, ini_state group; horizon 50:
1.304e-08).  As with the gain, only the ini_state group, whose contraction passes through lam+_0, is above rounding.
So ADJ_MEASURED = 1.753e-07 and the bar is 1e-6.
(2) Unit right-hand sides g_u = e_(u_0, a), g_x = 0 reproduce gain[b, a, :] under the same bar (first GPU run: equal
to the bit at every horizon, the two kernels run the same sweep and contraction).
(3) g_x at stage 0 only: the ini_state columns are g_x[:, 0, :] and every other column 0, exactly.
(4) Every subset of groups (names and masks) returns the full call's columns bit for bit; a repeated call is identical.
(5) The record: the outputs of ocp_solve_rec equal ocp_sensitivity_w's bit for bit, its x and u blocks the outputs.
(6) Refusals (LAFSE3_EINVAL before any launch), unconverged records (sens_status 1) and a record of another horizon
(sens_status 3): zero rows.
(7) mpc_layer(backward="adjoint") gives the default route's gradients under the bar of (1) (first GPU run: 4.349e-09,
ini_state group; float32 p, a, t receive float32 gradients, equal to the default route's on that run).
"""
import ctypes
import itertools

import numpy as np
import pytest

import sens_w_cases as C
import sens_yardstick as Y
from sens_yardstick import REC_N, REC_STATUS, REC_U, REC_W, REC_X

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ADJ_MEASURED = 1.753e-07   # largest relative |grad - reference| of (1) on the first GPU run
ADJ_BAR = Y.VJP_BAR         # ADJ_MEASURED rounded up to the next power of ten, at most 1e-5
GROUPS, SL = Y.GROUPS, Y.SL
BIT = {"theta": 1, "ini": 2, "goal": 4, "weights": 8}
NSAMPLES = {50: 16, 20: 8, 2: 8, 1: 8}
_np, _reference, _relative = Y.to_numpy, Y.vjp_reference, Y.vjp_relative


@pytest.fixture(scope="module")
def sb():
    Y.require_gpu()
    return Y.batch()


_CASES = {}


def _case(sb, horizon):
    """The instances of one horizon, solved once by both routes (never modified): the engine, the nine solve arguments,
    ocp_sensitivity_w's outputs with all 33 columns (the reference, from the existing kernel) and ocp_solve_rec's."""
    if horizon not in _CASES:
        from learningagileflight_se3_amd.engine import Engine
        n = NSAMPLES[horizon]
        idx = np.concatenate([np.arange(n), np.arange(n)])
        t = C.case_t(sb, horizon)
        ul = np.tile([0.4, 0.9, 0.2, 1.3], (2 * n, 1)) if horizon == 1 else None
        W = np.concatenate([np.tile(C.ROW_D, (n, 1)), np.tile(C.ROW_G, (n, 1))])
        args = tuple(v[idx] for v in (sb["ini"], sb["goal"], sb["p"], sb["a"], t)) + (ul, W)
        eng = Engine(horizon=horizon)
        fwd = _np(eng.ocp_sensitivity_w(*args[:6], weights=W, want=("x", "u", "lam", "cost", "dx", "du", "gain")))
        rec = eng.ocp_solve_rec(*args[:6], weights=W)
        torch.cuda.synchronize()
        rng = np.random.default_rng(7)
        g_x = rng.standard_normal((2 * n, horizon + 1, 13))
        g_u = rng.standard_normal((2 * n, horizon, 4))
        _CASES[horizon] = {"eng": eng, "args": args, "fwd": fwd, "rec": rec, "recn": _np(rec), "g_x": g_x, "g_u": g_u,
                           "B": 2 * n, "N": horizon}
    return _CASES[horizon]


def _vjp(c, g_x, g_u, groups=GROUPS, rec=None):
    out = _np(c["eng"].ocp_vjp(*c["args"], c["rec"]["rec"] if rec is None else rec, g_x, g_u, groups=groups))
    torch.cuda.synchronize()
    return out


def _all_live(c, out):
    assert np.all(c["fwd"]["sens_status"] == 0), c["fwd"]["sens_status"]
    assert np.all(out["sens_status"] == 0), out["sens_status"]
    assert np.all(c["fwd"]["status"] <= 1) and np.all(c["recn"]["status"] <= 1)


# ---- (1) adjoint against forward ------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_adjoint_sweep_equals_the_contracted_forward_jacobians(sb, horizon):
    c = _case(sb, horizon)
    out = _vjp(c, c["g_x"], c["g_u"])
    assert out["grad"].shape == (c["B"], 33) and np.all(np.isfinite(out["grad"]))
    assert out["columns"] == c["fwd"]["columns"]
    _all_live(c, out)
    ref, scale = _reference(c["fwd"], c["g_x"], c["g_u"])
    worst = _relative(out["grad"], ref, scale, f"horizon {horizon}, {c['B']} instances")
    assert ADJ_BAR <= 1e-5 and worst <= ADJ_BAR
    # one of the two gradients alone: the other is NULL, not a zero array
    only_x = _vjp(c, c["g_x"], None)
    only_u = _vjp(c, None, c["g_u"])
    rx, sx = _reference(c["fwd"], c["g_x"], np.zeros_like(c["g_u"]))
    ru, su = _reference(c["fwd"], np.zeros_like(c["g_x"]), c["g_u"])
    assert _relative(only_x["grad"], rx, sx, f"horizon {horizon}, g_x alone") <= ADJ_BAR
    assert _relative(only_u["grad"], ru, su, f"horizon {horizon}, g_u alone") <= ADJ_BAR


# ---- (2) unit right-hand sides --------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_unit_right_hand_sides_reproduce_the_gain(sb, horizon):
    c = _case(sb, horizon)
    worst = 0.0
    for a in range(4):
        g_u = np.zeros_like(c["g_u"])
        g_u[:, 0, a] = 1.0
        out = _vjp(c, None, g_u)
        _all_live(c, out)
        _, scale = _reference(c["fwd"], np.zeros_like(c["g_x"]), g_u)
        worst = max(worst, _relative(out["grad"], c["fwd"]["gain"][:, a, :], scale, f"horizon {horizon}, e_(u_0, {a})"))
    assert worst <= ADJ_BAR


# ---- (3) stage 0 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_a_gradient_at_stage_0_goes_to_the_ini_state_columns_alone(sb, horizon):
    c = _case(sb, horizon)
    g_x = np.zeros_like(c["g_x"])
    g_x[:, 0, :] = c["g_x"][:, 0, :]
    for g_u in (None, np.zeros_like(c["g_u"])):
        out = _vjp(c, g_x, g_u)
        _all_live(c, out)
        expect = np.zeros((c["B"], 33))
        expect[:, SL["ini"]] = g_x[:, 0, :]
        assert np.array_equal(out["grad"], expect)


# ---- (4) subsets and repeatability ----------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_group_subsets_and_repeated_calls_are_bit_identical(sb, horizon):
    c = _case(sb, horizon)
    full = _vjp(c, c["g_x"], c["g_u"])
    _all_live(c, full)
    again = _vjp(c, c["g_x"], c["g_u"])
    assert np.array_equal(again["grad"], full["grad"]) and np.array_equal(again["sens_status"], full["sens_status"])
    for r in range(1, 5):
        for sel in itertools.combinations(GROUPS, r):
            cols = np.concatenate([np.arange(33)[SL[g]] for g in sel])
            by_name = _vjp(c, c["g_x"], c["g_u"], groups=sel[::-1])           # the order given does not matter
            by_mask = _vjp(c, c["g_x"], c["g_u"], groups=sum(BIT[g] for g in sel))
            assert by_name["columns"] == [full["columns"][q] for q in cols]
            assert by_name["grad"].shape == (c["B"], len(cols))
            assert np.array_equal(by_name["grad"], full["grad"][:, cols]), sel
            assert np.array_equal(by_mask["grad"], full["grad"][:, cols]), sel
            assert np.all(by_name["sens_status"] == 0)


# ---- (5) the record -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("horizon", [50, 20, 2, 1])
def test_solve_rec_is_the_plain_solve_and_its_record_carries_the_outputs(sb, horizon):
    from learningagileflight_se3_amd import _lib
    c = _case(sb, horizon)
    N, B, r, f = c["N"], c["B"], c["recn"], c["fwd"]
    assert _lib.load().lafse3_rec_width() == REC_W == c["eng"].rec_width() and r["rec"].shape == (B, REC_W)
    assert set(r) == {"x", "u", "lam", "cost", "status", "iters", "rec"}
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert np.array_equal(r[k], f[k]), k
    assert np.array_equal(r["rec"][:, REC_X:REC_X + (N + 1) * 13].reshape(B, N + 1, 13), r["x"])
    assert np.array_equal(r["rec"][:, REC_U:REC_U + N * 4].reshape(B, N, 4), r["u"])
    assert np.array_equal(r["rec"][:, REC_STATUS], r["status"].astype(np.float64))
    assert np.all(r["rec"][:, REC_N] == N) and np.all(r["rec"][:, REC_STATUS - 2] > 0)          # mu
    # without weights: the context's weights, as ocp_sensitivity_w's plain solve without them
    n = 4
    ul = None if c["args"][5] is None else c["args"][5][:n]
    plain = _np(c["eng"].ocp_sensitivity_w(*(v[:n] for v in c["args"][:5]), ul, want=("x", "u", "lam", "cost")))
    none = _np(c["eng"].ocp_solve_rec(*(v[:n] for v in c["args"][:5]), ul, weights=None))
    for k in ("x", "u", "lam", "cost", "status", "iters"):
        assert np.array_equal(none[k], plain[k]), k
    for k in ("x", "u", "lam", "cost", "status", "iters", "rec"):      # the context's row is row D
        assert np.array_equal(none[k], r[k][:n]), k
    only = _np(c["eng"].ocp_solve_rec(*c["args"][:6], weights=c["args"][6], want=("cost",)))
    assert set(only) == {"cost", "status", "iters", "rec"} and np.array_equal(only["rec"], r["rec"])


# ---- (6) refusals and bad records -----------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(sb):
    from learningagileflight_se3_amd import _lib
    c = _case(sb, 20)
    eng = c["eng"]
    L = _lib.load()
    buf = torch.zeros(2 * REC_W, dtype=torch.float64, device=eng.device)
    ptr = ctypes.c_void_p(buf.data_ptr())
    ok = dict(groups=15, rec=ptr, grad=ptr)
    for bad in (dict(groups=0), dict(groups=16), dict(groups=1 | 32), dict(groups=-1), dict(rec=None), dict(grad=None)):
        k = {**ok, **bad}
        rc = L.lafse3_ocp_vjp(eng._ctx, 2, *([ptr] * 5), None, None, k["rec"], None, None, k["groups"], k["grad"], None,
                              None)
        assert rc == -1 and b"lafse3_ocp_vjp" in L.lafse3_last_error(), bad
    rc = L.lafse3_ocp_solve_rec(eng._ctx, 2, *([ptr] * 5), None, None, *([None] * 6), None, None)
    assert rc == -1 and b"rec is required" in L.lafse3_last_error()
    assert torch.all(buf == 0.0)
    a2 = tuple(None if v is None else v[:2] for v in c["args"])
    rec2 = c["rec"]["rec"][:2]
    for bad in (0, (), 16, ("weights", "u_last")):
        with pytest.raises(ValueError, match="groups"):
            eng.ocp_vjp(*a2, rec2, c["g_x"][:2], c["g_u"][:2], groups=bad)
    with pytest.raises(ValueError, match="rec"):
        eng.ocp_vjp(*a2, rec2[:, :-1], c["g_x"][:2], c["g_u"][:2])
    with pytest.raises(ValueError, match="g_x"):
        eng.ocp_vjp(*a2, rec2, c["g_x"][:2, :-1], c["g_u"][:2])


def test_unconverged_records_give_zero_rows(sb):
    from learningagileflight_se3_amd.engine import Engine
    e = Engine(max_iter=3)
    a2 = tuple(v[:2] for v in (sb["ini"], sb["goal"], sb["p"], sb["a"], sb["t"])) + (None, np.stack([C.ROW_D, C.ROW_G]))
    r = e.ocp_solve_rec(*a2[:6], weights=a2[6])
    rng = np.random.default_rng(7)
    out = e.ocp_vjp(*a2, r["rec"], rng.standard_normal((2, 51, 13)), rng.standard_normal((2, 50, 4)))
    torch.cuda.synchronize()
    assert r["status"].tolist() == [2, 2] and out["sens_status"].tolist() == [1, 1]
    assert out["grad"].shape == (2, 33) and torch.all(out["grad"] == 0.0)
    e.check_device()


def test_a_record_of_another_horizon_is_refused_per_instance(sb):
    c20, c50 = _case(sb, 20), _case(sb, 50)
    n = 2
    a50 = tuple(None if v is None else v[:n] for v in c50["args"])
    # samples 0, 1 under row D in both cases; the kernel reads the record's horizon before anything else of it
    out = _np(c50["eng"].ocp_vjp(*a50, c20["rec"]["rec"][:n], c50["g_x"][:n], c50["g_u"][:n]))
    assert out["sens_status"].tolist() == [3, 3] and np.all(out["grad"] == 0.0)
    mixed = torch.cat([c50["rec"]["rec"][:1], c20["rec"]["rec"][1:2]])
    out = _np(c50["eng"].ocp_vjp(*a50, mixed, c50["g_x"][:n], c50["g_u"][:n]))
    good = _vjp(c50, c50["g_x"], c50["g_u"])
    assert out["sens_status"].tolist() == [0, 3] and np.all(out["grad"][1] == 0.0)
    assert np.array_equal(out["grad"][0], good["grad"][0])
    c50["eng"].check_device()


# ---- (7) autograd ---------------------------------------------------------------------------------------------------

def test_mpc_layer_adjoint_route_gives_the_default_routes_gradients(sb):
    """All five inputs and the weights as leaves; loss = a fixed random linear form in x and u plus |x_N - goal|^2.
    The two routes' gradients agree under the bar of (1), on its scale, with float64 leaves and with float32 p, a, t,
    whose gradients come back in float32."""
    from learningagileflight_se3_amd.diff_mpc import mpc_layer
    c = _case(sb, 50)
    eng, dev = c["eng"], c["eng"].device
    sel = [0, 1, 2, 3, 16, 17, 18, 19]                       # samples 0..3 under row D, then under row G
    n = len(sel)
    ini, goal, p, a, t = (v[sel] for v in c["args"][:5])
    W = c["args"][6][sel]
    rng = np.random.default_rng(7)
    W_x, W_u = rng.standard_normal((n, 51, 13)), rng.standard_normal((n, 50, 4))
    T_x, T_u = torch.as_tensor(W_x, device=dev), torch.as_tensor(W_u, device=dev)

    def run(route, theta_dtype):
        dt = [torch.float64] * 2 + [theta_dtype] * 3 + [torch.float64]
        lv = [torch.tensor(v, dtype=d, device=dev, requires_grad=True) for v, d in zip((ini, goal, p, a, t, W), dt)]
        x, u, status = mpc_layer(eng, *lv[:5], None, lv[5], backward=route)
        loss = (T_x * x).sum() + (T_u * u).sum() + ((x[:, -1, :3] - lv[1]) ** 2).sum()
        first = torch.autograd.grad(loss, lv, retain_graph=True)
        second = torch.autograd.grad(loss, lv, retain_graph=True)
        assert all(torch.equal(g1, g2) for g1, g2 in zip(first, second))       # backward() again: the same gradients
        for v, g in zip(lv, first):
            assert g.dtype == v.dtype and g.shape == v.shape and bool(torch.isfinite(g).all())
        assert bool((status <= 1).all())
        return lv, x.detach(), u.detach(), first

    def columns(g):   # the six gradients in column order, (n, 33) float64
        return torch.cat([g[2].double(), g[3].double(), g[4].double().reshape(-1, 1), g[0], g[1], g[5]], 1).cpu().numpy()

    for theta_dtype in (torch.float64, torch.float32):
        lv_j, x_j, u_j, g_j = run("jacobian", theta_dtype)
        lv_a, x_a, u_a, g_a = run("adjoint", theta_dtype)
        assert torch.equal(x_j, x_a) and torch.equal(u_j, u_a)
        assert [g.dtype for g in g_a[2:5]] == [theta_dtype] * 3
        # the scale of (1): the Jacobians at these inputs and the loss's own gradients in x and u
        fwd = _np(eng.ocp_sensitivity_w(*(v.detach() for v in lv_a[:5]), weights=lv_a[5].detach(), want=("dx", "du")))
        assert np.all(fwd["sens_status"] == 0)
        g_x = W_x.copy()
        g_x[:, -1, :3] += 2.0 * (x_a[:, -1, :3].cpu().numpy() - goal)
        _, scale = _reference(fwd, g_x, W_u)
        worst = _relative(columns(g_a), columns(g_j), scale, f"mpc_layer with {theta_dtype} p, a, t: adjoint against jacobian")
        assert worst <= ADJ_BAR
