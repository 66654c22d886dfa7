"""CPU checks of the C-ABI library: it loads, exports every entry point include/lafse3.h declares,
and its parameter struct / defaults match the reference constants (no device calls)."""
import ctypes
import os
import re

import pytest

from learningagileflight_se3_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lafse3.h")


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(lafse3_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("liblafse3.so not built: run python -c 'import __graft_entry__ as g; g.build()'")
    return _lib.load()


def test_header_symbols_exported(lib):
    names = _declared()
    assert len(names) >= 15 and "lafse3_debug_dump" in names and "lafse3_debug_dump_resto" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in lafse3.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in _lib.SIGNATURES"


def test_version_names_gfx950(lib):
    assert b"gfx950" in lib.lafse3_version()


def test_params_struct_matches_header_and_reference(lib):
    p = _lib.default_params()
    # sizes: 24 doubles, then the solver block (int32 padding rules identical on both sides)
    assert ctypes.sizeof(_lib.Params) == ctypes.sizeof(p)
    # reference constants: quad_policy.py:37-51, quad_model.py:37, quad_OC.py:145
    assert (p.mass, p.Jx, p.Jy, p.Jz, p.arm_l, p.c_tau, p.grav, p.dt) == (0.5, 0.0023, 0.0023, 0.004, 0.35,
                                                                           0.0245, 9.78, 0.1)
    assert (p.wrt, p.wqt, p.wthrust, p.wrf, p.wvf, p.wqf, p.wwf) == (5, 80, 0.1, 5, 5, 0, 3)
    assert p.horizon == 50 and p.u_lb == 0.0 and abs(p.u_ub - 2.44) < 1e-15
    assert abs(p.w_ub - 3.141592653589793 / 2) < 1e-15 and p.tol == 1e-8
    assert p.costate_option == 0          # IPOPT lam_g, the reference's default (quad_OC.py:104)
    assert p.grad_mode == 0               # FD, the reference's sol_gradient (quad_policy.py:94-112)


def test_workspace_size_positive(lib):
    assert lib.lafse3_workspace_bytes_per_instance() > 0


def test_engine_rejects_mismatched_batch():
    """Every per-sample argument must have ini_state's batch (the kernels read row b < B of each); only u_last
    broadcasts from one row (out-of-bounds device reads otherwise)."""
    import torch
    from learningagileflight_se3_amd.engine import _same_batch
    B = 4
    goal = torch.zeros(B, 3)
    ul1 = torch.ones(1, 4)
    g, ul = _same_batch(B, goal=goal, u_last=ul1)
    assert ul.shape == (B, 4) and g is goal
    with pytest.raises(ValueError, match="gate12"):
        _same_batch(B, goal=goal, gate12=torch.zeros(1, 12))
    with pytest.raises(ValueError, match="dnn_out"):
        _same_batch(B, dnn_out=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="u_last"):
        _same_batch(B, u_last=torch.zeros(2, 4))


def test_stream_create_rejects_null_arguments(lib):
    """lafse3_stream_create / _destroy validate their pointers before any HIP call (LAFSE3_EINVAL, message set)."""
    assert lib.lafse3_stream_create(0, None) == -1
    assert b"null stream" in lib.lafse3_last_error()
    assert lib.lafse3_stream_destroy(None) == -1


def _takes_context(name):
    """Whether include/lafse3.h declares `name` with a lafse3_ctx parameter."""
    m = re.search(r"^[a-z][\w \*]*\b%s\s*\(([^;]*?)\)\s*;" % name, open(HEADER).read(), re.M | re.S)
    assert m, f"{name} has a ctypes signature but no declaration in lafse3.h"
    return "lafse3_ctx" in m.group(1)


def test_null_context_is_rejected_by_every_entry_point(lib):
    """Every entry point that takes a context answers a NULL one with LAFSE3_EINVAL and a message, before any HIP
    call (this test runs without a device).  Driven from _lib.SIGNATURES, so a new entry point is covered without
    being named here.  The two exceptions: lafse3_destroy(NULL) is a no-op, lafse3_last_kernel_ms(NULL) is -1."""
    names = [n for n in _lib.SIGNATURES if _takes_context(n)]
    assert len(names) >= 20 and "lafse3_create" in names and "lafse3_ocp_sensitivity" in names
    for n in names:
        res, argtypes = _lib.SIGNATURES[n]
        zeros = [0.0 if a is ctypes.c_double else 0 if a in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64) else None
                 for a in argtypes[1:]]
        assert lib.lafse3_stream_create(0, None) == -1      # a known message to tell this call's from
        rc = getattr(lib, n)(None, *zeros)
        if n == "lafse3_destroy":
            assert rc == 0
        elif n == "lafse3_last_kernel_ms":
            assert rc == -1.0
        else:
            assert rc == -1, n
            msg = lib.lafse3_last_error()
            assert msg and b"null stream" not in msg, (n, msg)


def test_solve_input_marshalling_on_cpu_tensors():
    """engine._solve_inputs / _dnn_inputs: a wrong trailing shape or batch raises ValueError naming the argument,
    a one-row u_last broadcasts to the batch and a scalar t expands to (B,)."""
    import torch
    from learningagileflight_se3_amd.engine import _dnn_inputs, _solve_inputs
    B, f64 = 4, torch.float64
    ini, goal, p, a = torch.zeros(B, 13), torch.zeros(B, 3), torch.ones(B, 3), torch.ones(B, 3)
    out = _solve_inputs("cpu", f64, ini, goal, p, a, 1.5, u_last=torch.ones(1, 4))
    assert out[0] == B and [tuple(v.shape) for v in out[1:7]] == [(B, 13), (B, 3), (B, 3), (B, 3), (B,), (B, 4)]
    assert out[7] is None and all(v.dtype == f64 and v.is_contiguous() for v in out[1:7])
    assert torch.equal(out[5], torch.full((B,), 1.5, dtype=f64)) and torch.equal(out[6], torch.ones(B, 4, dtype=f64))
    assert _solve_inputs("cpu", f64, ini, goal, p, a, 1.5)[6] is None                      # u_last stays optional
    g12 = _solve_inputs("cpu", f64, ini, goal, p, a, 1.5, None, torch.zeros(B, 12), True)[7]
    assert tuple(g12.shape) == (B, 12)
    with pytest.raises(ValueError, match="goal"):
        _solve_inputs("cpu", f64, ini, torch.zeros(B, 2), p, a, 1.5)                      # trailing shape
    with pytest.raises(ValueError, match="p_tra"):
        _solve_inputs("cpu", f64, ini, goal, torch.ones(3, 3), a, 1.5)                    # batch
    with pytest.raises(ValueError, match="u_last"):
        _solve_inputs("cpu", f64, ini, goal, p, a, 1.5, u_last=torch.ones(2, 4))
    with pytest.raises(ValueError, match="gate12"):
        _solve_inputs("cpu", f64, ini, goal, p, a, 1.5, None, None, True)                 # required when asked for
    n, i2, g2, dnn, ul, gate = _dnn_inputs("cpu", ini, goal, torch.zeros(B, 7), torch.ones(1, 4))
    assert n == B and dnn.dtype == torch.float32 and tuple(ul.shape) == (B, 4) and gate is None
    with pytest.raises(ValueError, match="dnn_out"):
        _dnn_inputs("cpu", ini, goal, torch.zeros(B, 6))
    with pytest.raises(ValueError, match="dnn_out"):
        _dnn_inputs("cpu", ini, goal, torch.zeros(3, 7))


def test_param_override_restores_when_the_body_raises():
    """engine._param_override sets one Params field and pushes it, and puts the old value back and pushes again on
    exit, also when the body raises; None or the current value pushes nothing."""
    import types
    from learningagileflight_se3_amd.engine import _param_override

    class StandIn:
        def __init__(self):
            self.params = types.SimpleNamespace(grad_mode=0, costate_option=1)
            self.pushed = []

        def set_params(self, p):
            self.pushed.append((p.grad_mode, p.costate_option))

    e = StandIn()
    with pytest.raises(KeyError):
        with _param_override(e, "grad_mode", 1):
            assert e.params.grad_mode == 1 and e.pushed == [(1, 1)]
            raise KeyError("body")
    assert e.params.grad_mode == 0 and e.pushed == [(1, 1), (0, 1)]
    with _param_override(e, "costate_option", 0):
        assert e.params.costate_option == 0
    assert e.params.costate_option == 1 and e.pushed[2:] == [(0, 0), (0, 1)]
    for same in (None, 1):
        with _param_override(e, "costate_option", same):
            pass
    assert len(e.pushed) == 4
