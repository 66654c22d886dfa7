"""Batched MPC solve / objective / gradient on MI355X through liblafse3.so.

``Engine`` owns one C-ABI context (device workspace + parameters) and takes torch tensors that
already live in HBM.  Every method is asynchronous on the current torch stream and returns tensors
allocated on the same device.  Host numpy inputs are accepted for convenience (copied to the device).

Reference interfaces mirrored (yanrui89/LearningAgileFlight_SE3):
  Engine.ocp_solve     OCSys.ocSolver          quad_OC.py:104-212
  Engine.objective     run_quad.objective      quad_policy.py:67-91
  Engine.sol_gradient  run_quad.sol_gradient   quad_policy.py:94-112
  Engine.get_input     run_quad.get_input      quad_policy.py:202-211
  Engine.ocp_sensitivity  ocSolver + dx*/dtheta, du*/dtheta (the PDP auxiliary system sketched in quad_OC.py:214-306)
  Engine.ocp_sensitivity_ex  the same with ini_state and goal columns and the MPC feedback gain du*_0/dx_0
  Engine.ocp_sensitivity_w   the same with per-instance cost weights and the columns of the ten weights
  Engine.ocp_solve_rec / ocp_vjp   the solve that saves its optimum, and a loss's gradients from it in one adjoint sweep
  Engine.ocp_solve_warm  the solve started from a saved optimum (same problem, or the receding-horizon successor)
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import NU, NX, Params, check, load


def _dev_tensor(a, shape_tail, dtype, device, name, allow_none=False):
    if a is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is required")
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    t = t.to(device=device, dtype=dtype)
    if t.dim() == len(shape_tail):
        t = t.unsqueeze(0)
    if tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name}: expected (B, {', '.join(map(str, shape_tail))}), got {tuple(t.shape)}")
    return t.contiguous()


def _same_batch(B, **named):
    """Every per-sample argument must carry the batch of ini_state (the kernels index row b < B of each);
    u_last alone may be one row, broadcast to the batch.  Returns the (possibly expanded) tensors."""
    out = []
    for name, v in named.items():
        if v is not None and v.shape[0] != B:
            if name == "u_last" and v.shape[0] == 1:
                v = v.expand(B, *v.shape[1:]).contiguous()
            else:
                raise ValueError(f"{name}: batch {v.shape[0]} != {B} (the batch of ini_state)")
        out.append(v)
    return out


def _solve_inputs(device, dtype, ini_state, goal, p_tra, a_tra, t, u_last=None, gate12=None, with_gate=False):
    """The solve inputs as ``dtype`` tensors on ``device`` with the batch B of ini_state (a scalar ``t`` expands
    to (B,), a one-row ``u_last`` to B rows): (B, ini, goal, p_tra, a_tra, t, u_last, gate12), gate12 None unless
    ``with_gate``.  A wrong trailing shape or batch raises ValueError naming the argument."""
    ini = _dev_tensor(ini_state, (NX,), dtype, device, "ini_state")
    B = ini.shape[0]
    named = {"goal": _dev_tensor(goal, (3,), dtype, device, "goal"),
             "p_tra": _dev_tensor(p_tra, (3,), dtype, device, "p_tra"),
             "a_tra": _dev_tensor(a_tra, (3,), dtype, device, "a_tra"),
             "u_last": _dev_tensor(u_last, (NU,), dtype, device, "u_last", allow_none=True),
             "gate12": _dev_tensor(gate12, (12,), dtype, device, "gate12") if with_gate else None}
    tt = torch.as_tensor(t, dtype=dtype).to(device).reshape(-1).expand(B).contiguous()
    goal, p, a, ul, g12 = _same_batch(B, **named)
    return B, ini, goal, p, a, tt, ul, g12


def _dnn_inputs(device, ini_state, goal, dnn_out, u_last=None, gate12=None, with_gate=False):
    """As _solve_inputs for the calls that take DNN1's output (B, 7) float32 in place of p_tra / a_tra / t:
    (B, ini, goal, dnn_out, u_last, gate12)."""
    f64 = torch.float64
    ini = _dev_tensor(ini_state, (NX,), f64, device, "ini_state")
    B = ini.shape[0]
    named = {"goal": _dev_tensor(goal, (3,), f64, device, "goal"),
             "dnn_out": _dev_tensor(dnn_out, (7,), torch.float32, device, "dnn_out"),
             "u_last": _dev_tensor(u_last, (NU,), f64, device, "u_last", allow_none=True),
             "gate12": _dev_tensor(gate12, (12,), f64, device, "gate12") if with_gate else None}
    return (B, ini, *_same_batch(B, **named))


@contextlib.contextmanager
def _param_override(eng, field, value):
    """Run the body with ``eng.params.<field> = value`` pushed through ``eng.set_params``; the saved value is put
    back and pushed again on exit, also when the body raises.  ``value`` None or equal to the field: nothing."""
    saved = getattr(eng.params, field)
    if value is None or int(value) == int(saved):
        yield
        return
    try:
        setattr(eng.params, field, int(value))
        eng.set_params(eng.params)
        yield
    finally:
        setattr(eng.params, field, saved)
        eng.set_params(eng.params)


def _parse_groups(groups, table, required=True):
    """``groups`` (names of ``table``, one name, or the LAFSE3_SENS_* bit mask) -> (mask, column names in the fixed
    order); ``table`` is _lib.SENS_GROUPS or, for the calls with the weights group, _lib.SENS_GROUPS_W.  ``required``:
    an empty selection or a bit outside the table raises ValueError."""
    if isinstance(groups, str):
        groups = (groups,)
    if isinstance(groups, int):
        mask = int(groups)
    else:
        unknown = [g for g in groups if g not in table]
        if unknown:
            raise ValueError(f"groups: unknown {unknown}; expected any of {list(table)}")
        mask = sum(bit for g, bit in table.items() if g in groups)
    if required and (mask == 0 or mask & ~sum(table.values())):
        raise ValueError(f"groups: {groups!r} selects no column or a bit outside {table}")
    return mask, [c for g, bit in table.items() if mask & bit for c in _lib.SENS_COLUMNS_W[g]]


def _weight_rows(weights, B, device):
    """``weights`` (B, 10) or (10,) (broadcast over the batch) as a contiguous (B, 10) float64 tensor on ``device``;
    None stays None (the context's weights)."""
    if weights is None:
        return None
    w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
    w = w.detach().to(device=device, dtype=torch.float64)
    given = tuple(w.shape)
    if given == (_lib.NW,):
        w = w.unsqueeze(0).expand(B, _lib.NW)
    if tuple(w.shape) != (B, _lib.NW):
        raise ValueError(f"weights: expected ({B}, {_lib.NW}) or ({_lib.NW},), got {given}")
    return w.contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _solve_outputs(B, N, want, dtype, device, **extra):
    """The outputs every solve entry point has, in the order the results are returned in: x, u, lam, cost and the
    ``extra`` name=shape ones as uninitialised ``dtype`` tensors, None for one not in ``want``, then status and iters
    (B,) int32."""
    shapes = {"x": (B, N + 1, NX), "u": (B, N, NU), "lam": (B, N, NX), "cost": (B,), **extra}
    out = {k: torch.empty(s, dtype=dtype, device=device) if k in want else None for k, s in shapes.items()}
    out["status"] = torch.empty((B,), dtype=torch.int32, device=device)
    out["iters"] = torch.empty((B,), dtype=torch.int32, device=device)
    return out


class QueueStream:
    """A torch stream (``.stream``, a torch.cuda.ExternalStream) on a hardware queue of its own
    (lafse3_stream_create): for contexts whose launches are meant to overlap, e.g. the episode groups of the
    moving-gate loop.  Two ordinary torch streams can share one of HIP's pooled hardware queues and then run
    their kernels back to back (profiles/r05_moving_trace.log).  ``close()`` synchronizes and destroys the stream;
    the solver contexts that launched on it stay usable (their counters are read on a stream of their own after the
    launch's end event, api.hip read_counters)."""

    def __init__(self, device=None):
        d = torch.device("cuda") if device is None else torch.device(device)
        # a device without an index ("cuda") is the current device, as torch reads it
        self.device = torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)
        self._L = load()
        self._h = ctypes.c_void_p()
        check(self._L.lafse3_stream_create(self.device.index, ctypes.byref(self._h)), "lafse3_stream_create")
        self.stream = torch.cuda.ExternalStream(self._h.value, device=self.device)

    def close(self):
        if self._h.value:
            self.stream.synchronize()
            check(self._L.lafse3_stream_destroy(self._h), "lafse3_stream_destroy")
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One solver context on one HIP device (``device=None``: torch's current device)."""

    def __init__(self, params: Params | None = None, device=None, **overrides):
        if not torch.cuda.is_available():
            raise _lib.Lafse3Error("no HIP device visible: the MI355X engine has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self._L = load()
        self._ctx = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._L.lafse3_create(ctypes.byref(self._ctx), self.device.index), "lafse3_create")
        p = params if params is not None else _lib.default_params()
        for k, v in overrides.items():
            setattr(p, k, v)
        self.set_params(p)

    # ------------------------------------------------------------------ params / resources
    def set_params(self, p: Params):
        check(self._L.lafse3_set_params(self._ctx, ctypes.byref(p)), "lafse3_set_params")
        self.params = p

    @property
    def horizon(self) -> int:
        return int(self.params.horizon)

    def reserve(self, n_instances: int):
        check(self._L.lafse3_reserve(self._ctx, int(n_instances)), "lafse3_reserve")

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._L.lafse3_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_kernel_ms(self) -> float:
        return float(self._L.lafse3_last_kernel_ms(self._ctx))

    def last_counters(self) -> dict:
        c = (ctypes.c_int64 * 3)()
        check(self._L.lafse3_last_counters(self._ctx, c), "lafse3_last_counters")
        return {"iterations": int(c[0]), "sweeps": int(c[1]), "trials": int(c[2])}

    def last_resto_counters(self) -> dict:
        """Restoration-phase entries and successful returns of the last launch (lafse3_last_resto_counters)."""
        c = (ctypes.c_int64 * 2)()
        check(self._L.lafse3_last_resto_counters(self._ctx, c), "lafse3_last_resto_counters")
        return {"resto_entries": int(c[0]), "resto_returns": int(c[1])}

    def debug_trace(self, buf=None, iters: int = 0):
        """Debug: per-iteration IPM trace into a (instances, iters, 16) float64 device tensor."""
        self._trace_buf = buf
        check(self._L.lafse3_debug_trace(self._ctx, _ptr(buf), int(iters)), "lafse3_debug_trace")

    def debug_dump(self, buf=None, it: int = -1, after_refine: bool = False):
        """Debug: Newton step of iteration `it` (before or after iterative refinement) and the iterate it was
        computed at into a (instances, 3732) float64 device tensor: [dx 51x13 | du 50x4 | lam+ 50x13] then
        [x 51x13 | u 50x4 | lam 50x13 | zLu 50x4 | zUu 50x4 | zLw 51x3 | zUw 51x3], stage-major, padded to 50
        stages, multipliers of the scaled-objective problem (lafse3_debug_dump in lafse3.h).  None disables."""
        self._dump_buf = buf
        check(self._L.lafse3_debug_dump(self._ctx, _ptr(buf), int(it), int(after_refine)), "lafse3_debug_dump")

    def debug_dump_resto(self, buf=None, entry: int = 0, it: int = 0, after_refine: bool = False):
        """Debug: the restoration phase's Newton step of iteration `it` of the entry-th entry into the phase (both
        0-based) of each solve, with the iterate and reference point it was formed at, its scalars and the entry's
        least-squares multiplier record, into a (instances, 9153) float64 device tensor (lafse3_debug_dump_resto in
        lafse3.h; ocp_solve launches only).  None disables."""
        if buf is not None and (buf.dtype != torch.float64 or not buf.is_contiguous() or buf.device != self.device
                                or buf.shape[-1] != 9153):
            raise ValueError("debug_dump_resto: a contiguous (instances, 9153) float64 tensor on the engine's device "
                             "is required")
        self._rdump_buf = buf
        check(self._L.lafse3_debug_dump_resto(self._ctx, _ptr(buf), int(entry), int(it), int(after_refine)),
              "lafse3_debug_dump_resto")

    def debug_timers(self, buf=None):
        """Debug: per-instance phase timers + placement record into an (instances, 32) int64 device tensor (None disables)."""
        self._timer_buf = buf
        check(self._L.lafse3_debug_timers(self._ctx, _ptr(buf)), "lafse3_debug_timers")

    def record_iters(self, buf=None):
        """Per-instance IPM iteration counts of later launches into an int32 device tensor (one entry per NLP
        instance, sol_gradient: (B, 9) in rewards9 order); None disables.  A launch that would write more
        entries than buf holds raises."""
        if buf is not None and (buf.dtype != torch.int32 or not buf.is_contiguous() or buf.device != self.device):
            raise ValueError("record_iters: a contiguous int32 tensor on the engine's device is required")
        self._iters_buf = buf
        check(self._L.lafse3_record_iters(self._ctx, _ptr(buf), 0 if buf is None else buf.numel()),
              "lafse3_record_iters")

    def check_device(self):
        """Wait for the last launch and raise Lafse3Error if the kernel raised its device error word (a lost
        sol_gradient probe task: its rewards9 slot is NaN and its status9 entry 7)."""
        check(self._L.lafse3_check_device(self._ctx), "lafse3_check_device")

    def debug_drop_push(self, sample: int = -1):
        """Debug: withhold the probe-queue entry of `sample` in later sol_gradient launches (-1 disables)."""
        check(self._L.lafse3_debug_drop_push(self._ctx, int(sample)), "lafse3_debug_drop_push")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ hot path
    def _solve_call(self, entry, B, inputs, out, before=(), after=()):
        """The one call into the solve entry points, whose C signatures share the skeleton
          ctx, B, ini_state .. u_last, [before], x, u, lam, cost, status, iters, [after], stream.
        ``inputs``: the six tensors of _solve_inputs; ``out``: _solve_outputs' dict plus the entry's own outputs;
        ``before`` / ``after``: the entry's own arguments on either side of the common outputs, as ctypes takes them.
        Raises Lafse3Error under the entry's name; returns ``out`` without its None entries."""
        check(getattr(self._L, entry)(self._ctx, B, *map(_ptr, inputs), *before,
                                      _ptr(out["x"]), _ptr(out["u"]), _ptr(out["lam"]), _ptr(out["cost"]),
                                      _ptr(out["status"]), _ptr(out["iters"]), *after, self._stream()), entry)
        return {k: v for k, v in out.items() if v is not None}

    def _rec_rows(self, rec, B):
        """``rec`` as a contiguous (B, rec_width()) float64 tensor on the engine's device; ValueError otherwise."""
        if rec is None:
            raise ValueError("rec is required")
        rec = rec.detach().to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(rec.shape) != (B, self.rec_width()):
            raise ValueError(f"rec: expected ({B}, {self.rec_width()}), got {tuple(rec.shape)}")
        return rec

    def _launch_counters(self) -> dict:
        return dict(self.last_counters(), **self.last_resto_counters(), kernel_ms=self.last_kernel_ms())

    def ocp_solve(self, ini_state, goal, p_tra, a_tra, t, u_last=None, want=("x", "u", "lam", "cost"),
                  costate_option: int | None = None, dtype=torch.float64):
        """Batched OCSys.ocSolver. Returns dict of device tensors (x, u, lam, cost, status, iters).

        ``costate_option`` (quad_OC.py:104 argument): 0 = IPOPT lam_g, 1 = PMP costates (quad_OC.py:188-201);
        None keeps the context's parameter.  ``dtype=torch.float32`` uses the fp32 twin
        (lafse3_ocp_solve_f32: float32 buffers at the boundary, fp64 solve inside).
        """
        f32 = dtype == torch.float32
        d, dt = self.device, (torch.float32 if f32 else torch.float64)
        B, *inputs, _ = _solve_inputs(d, dt, ini_state, goal, p_tra, a_tra, t, u_last)
        out = _solve_outputs(B, self.horizon, want, dt, d)
        with _param_override(self, "costate_option", costate_option):
            return self._solve_call("lafse3_ocp_solve_f32" if f32 else "lafse3_ocp_solve", B, inputs, out)

    def ocp_sensitivity(self, ini_state, goal, p_tra, a_tra, t, u_last=None, want=("x", "u", "dx", "du")):
        """ocp_solve plus the analytic sensitivities of its solution (lafse3_ocp_sensitivity), one launch.

        Returns ocp_solve's dict (x, u, lam, cost as named in ``want``; status, iters) and
          dx (B, 7, N+1, 13) = dx_k / dtheta_q,  du (B, 7, N, 4) = du_k / dtheta_q,
          theta = (p_tra[0..2], a_tra[0..2], t),
          sens_status (B,) int32: 0 ok, 1 the solve ended with status > 1, 2 wrong inertia at the optimum
          (dx and du of such an instance are zero).
        The derivative is that of the barrier problem at the final mu (include/lafse3.h).  float64 only."""
        d, f64 = self.device, torch.float64
        B, *inputs, _ = _solve_inputs(d, f64, ini_state, goal, p_tra, a_tra, t, u_last)
        N = self.horizon
        out = _solve_outputs(B, N, want, f64, d, dx=(B, 7, N + 1, NX), du=(B, 7, N, NU))
        # without dx and du the call is lafse3_ocp_solve
        out["sens_status"] = torch.empty((B,), dtype=torch.int32, device=d) if "dx" in want or "du" in want else None
        return self._solve_call("lafse3_ocp_sensitivity", B, inputs, out,
                                after=(_ptr(out["dx"]), _ptr(out["du"]), _ptr(out["sens_status"])))

    def _sensitivity_groups(self, entry, table, args, weights, groups, want):
        """ocp_sensitivity_ex and ocp_sensitivity_w, which differ in the entry point, the group table and the
        ``weights`` argument (passed when the table has the weights group)."""
        sens = any(k in want for k in ("dx", "du", "gain"))
        mask, columns = _parse_groups(groups, table, required=sens)
        P = len(columns)
        d, f64 = self.device, torch.float64
        B, *inputs, _ = _solve_inputs(d, f64, *args)
        w = _weight_rows(weights, B, d)
        N = self.horizon
        out = _solve_outputs(B, N, want, f64, d, dx=(B, P, N + 1, NX), du=(B, P, N, NU), gain=(B, NU, P))
        # without dx, du and gain the call is a plain solve
        out["sens_status"] = torch.empty((B,), dtype=torch.int32, device=d) if sens else None
        res = self._solve_call(entry, B, inputs, out, before=(_ptr(w),) if "weights" in table else (),
                               after=(mask, _ptr(out["dx"]), _ptr(out["du"]), _ptr(out["gain"]),
                                      _ptr(out["sens_status"])))
        res["columns"] = columns
        return res

    def ocp_sensitivity_ex(self, ini_state, goal, p_tra, a_tra, t, u_last=None, groups=("theta", "ini", "goal"),
                           want=("x", "u", "dx", "du", "gain")):
        """ocp_sensitivity with selectable parameter groups and the MPC feedback gain (lafse3_ocp_sensitivity_ex),
        one launch.

        ``groups``: any of "theta" (p_tra, a_tra, t: 7 columns), "ini" (ini_state: 13), "goal" (3), or the
        LAFSE3_SENS_* bit mask; the P columns come in that fixed order whatever the order given.  Returns
        ocp_sensitivity's dict with dx (B, P, N+1, 13), du (B, P, N, 4) and
          gain (B, 4, P) = du_0[a] / dparam_q, over the "ini" columns the feedback gain du*_0 / dx_0,
          columns: the P column names in order ("p_tra[0]", .., "ini_state[0]", .., "goal[2]").
        dx and du cost one sweep per column, gain four sweeps in all; want=("gain",) computes nothing else.
        After sens_status != 0 an instance's dx, du and gain are zero.  float64 only."""
        return self._sensitivity_groups("lafse3_ocp_sensitivity_ex", _lib.SENS_GROUPS,
                                        (ini_state, goal, p_tra, a_tra, t, u_last), None, groups, want)

    def weights(self):
        """The context's ten cost weights (_lib.WEIGHT_NAMES order) as a (10,) float64 device tensor: the row a
        ``weights=None`` stands for (lafse3_params_weights)."""
        w = (ctypes.c_double * _lib.NW)()
        check(self._L.lafse3_params_weights(ctypes.byref(self.params), w), "lafse3_params_weights")
        return torch.tensor(list(w), dtype=torch.float64, device=self.device)

    def ocp_sensitivity_w(self, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None,
                          groups=("theta", "ini", "goal", "weights"), want=("x", "u", "dx", "du", "gain")):
        """ocp_sensitivity_ex with per-instance cost weights and the sensitivities to them
        (lafse3_ocp_sensitivity_w), one launch.

        ``weights``: (B, 10) or (10,) (broadcast over the batch), the ten cost weights in _lib.WEIGHT_NAMES order
        (wrt wqt wthrust wrf wvf wqf wwf tra_w_peak tra_w_decay du_weight); instance b solves the NLP with row b,
        every other parameter is the context's.  None: the context's weights.  They are used as given.
        ``groups``: as ocp_sensitivity_ex plus "weights" (10 columns, last).  Returns ocp_sensitivity_ex's dict;
        ``columns`` ends with the ten weight names.  Without dx, du and gain in ``want`` the call is a plain solve
        with those weights.  float64 only."""
        return self._sensitivity_groups("lafse3_ocp_sensitivity_w", _lib.SENS_GROUPS_W,
                                        (ini_state, goal, p_tra, a_tra, t, u_last), weights, groups, want)

    def rec_width(self) -> int:
        """Doubles per instance of the optimum record (lafse3_rec_width; independent of the horizon)."""
        return int(self._L.lafse3_rec_width())

    def ocp_solve_rec(self, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None,
                      want=("x", "u", "lam", "cost")):
        """ocp_sensitivity_w as a plain solve that also saves its optimum (lafse3_ocp_solve_rec), one launch.

        Returns ocp_solve's dict (x, u, lam, cost as named in ``want``; status, iters) plus
          rec (B, rec_width()) float64: the primal-dual point the sensitivity passes factorise at (layout in
          include/lafse3.h), which ``ocp_vjp`` turns into gradients later.  ``weights`` as ocp_sensitivity_w."""
        d, f64 = self.device, torch.float64
        B, *inputs, _ = _solve_inputs(d, f64, ini_state, goal, p_tra, a_tra, t, u_last)
        w = _weight_rows(weights, B, d)
        out = _solve_outputs(B, self.horizon, want, f64, d)
        # zeros: the entries of stages beyond the horizon are not written
        out["rec"] = torch.zeros((B, self.rec_width()), dtype=f64, device=d)
        return self._solve_call("lafse3_ocp_solve_rec", B, inputs, out, before=(_ptr(w),), after=(_ptr(out["rec"]),))

    def ocp_solve_warm(self, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None, rec=None, shift=0,
                       mu_init=None, retry=True, want=("x", "u", "lam", "cost"), opts=None, counters=None):
        """ocp_solve_rec started from saved optima (lafse3_ocp_solve_warm): instance b starts from the record
        ``rec[b]`` of an earlier solve, advanced by ``shift`` stages (the receding-horizon successor: shift=1 with
        ini_state = the old x_1), instead of the cold initial point.

        ``rec`` (B, rec_width()): records of ocp_solve_rec or of this call; it is not modified.  ``mu_init``: the
        barrier parameter of a warm start (None: the default of lafse3_default_warm_opts, 1e-3; <= 0: the context's
        params.mu_init).  ``opts``: a _lib.WarmOpts for the pushes as well; ``shift`` and ``mu_init`` override its
        fields.  Returns ocp_solve_rec's dict (x, u, lam, cost as named in ``want``; status, iters, rec) plus
          warm_status (B,) int32: 0 warm start, 1 the record was unusable (wrong horizon, status > 1, a non-finite
          entry, mu or s not positive) and the instance started cold, bit for bit ocp_solve_rec's,
          2 the warm start ended with status > 1 and the instance was solved again cold (``retry``).
        ``retry=True``: the instances whose warm start failed are counted on the device (one host read), and when
        there are any they are gathered, solved with ocp_solve_rec in a second launch and scattered back: every
        output of such a row, its record included, is ocp_solve_rec's bit for bit, and ``iters`` is the retry's.
        After a retry last_counters / last_kernel_ms describe the second launch; ``counters``, a list, receives
        last_counters() + last_resto_counters() + kernel_ms after each launch made (diagnostics: each read waits for
        its launch).  The returned ``rec`` is a valid input of ``ocp_vjp`` (with these arguments) and of the next
        ocp_solve_warm.  The problem is nonconvex: a warm start may end in another local optimum than the cold
        solve.  float64 only."""
        d, f64 = self.device, torch.float64
        B, *inputs, _ = _solve_inputs(d, f64, ini_state, goal, p_tra, a_tra, t, u_last)
        w = _weight_rows(weights, B, d)
        rec = self._rec_rows(rec, B)
        o = _lib.default_warm_opts() if opts is None else opts
        o = _lib.WarmOpts(o.shift, o.mu_init, o.bound_push, o.bound_frac, o.mult_bound_push)
        o.shift = int(shift)
        if mu_init is not None:
            o.mu_init = float(mu_init)
        out = _solve_outputs(B, self.horizon, want, f64, d)
        out["warm_status"] = torch.empty((B,), dtype=torch.int32, device=d)
        out["rec"] = torch.zeros((B, self.rec_width()), dtype=f64, device=d)
        res = self._solve_call("lafse3_ocp_solve_warm", B, inputs, out, before=(_ptr(w), _ptr(rec), ctypes.byref(o)),
                               after=(_ptr(out["warm_status"]), _ptr(out["rec"])))
        if counters is not None:
            counters.append(self._launch_counters())
        if retry:
            failed = (res["status"] > 1) & (res["warm_status"] == 0)
            if int(failed.sum()) > 0:   # the one device-side count; the second launch only when it is non-zero
                idx = failed.nonzero().squeeze(1)
                cold = self.ocp_solve_rec(*(None if v is None else v[idx] for v in (*inputs, w)), want=want)
                if counters is not None:
                    counters.append(self._launch_counters())
                for k, v in cold.items():
                    res[k][idx] = v
                res["warm_status"][idx] = 2
        return res

    def ocp_vjp(self, ini_state, goal, p_tra, a_tra, t, u_last, weights, rec, g_x=None, g_u=None,
                groups=("theta", "ini", "goal", "weights")):
        """Gradients of a loss through the optimum from a saved record (lafse3_ocp_vjp), one small launch:
          grad (B, P) = sum g_x dx*/dparam_q + sum g_u du*/dparam_q over the P columns of ``groups``
        (ocp_sensitivity_w's groups and column order), by one factorisation and one adjoint sweep per instance.

        The first seven arguments are those of the ``ocp_solve_rec`` call that returned ``rec`` (B, rec_width()),
        under the same params.  g_x (B, N+1, 13), g_u (B, N, 4): the loss gradients w.r.t. x and u (None = zero).
        Returns {grad, sens_status (B,) int32: 0 ok, 1 the recorded solve ended with status > 1, 2 wrong inertia at
        the optimum, 3 the record's horizon is not this engine's (rows != 0 are zero), columns}.  float64 only."""
        mask, columns = _parse_groups(groups, _lib.SENS_GROUPS_W)
        d, f64 = self.device, torch.float64
        B, *inputs, _ = _solve_inputs(d, f64, ini_state, goal, p_tra, a_tra, t, u_last)
        w = _weight_rows(weights, B, d)
        N = self.horizon
        rec = self._rec_rows(rec, B)
        gx = _dev_tensor(g_x, (N + 1, NX), f64, d, "g_x", allow_none=True)
        gu = _dev_tensor(g_u, (N, NU), f64, d, "g_u", allow_none=True)
        gx, gu = _same_batch(B, g_x=gx, g_u=gu)
        grad = torch.empty((B, len(columns)), dtype=f64, device=d)
        ss = torch.empty((B,), dtype=torch.int32, device=d)
        check(self._L.lafse3_ocp_vjp(self._ctx, B, *map(_ptr, inputs), _ptr(w), _ptr(rec), _ptr(gx), _ptr(gu), mask,
                                     _ptr(grad), _ptr(ss), self._stream()), "lafse3_ocp_vjp")
        return {"grad": grad, "sens_status": ss, "columns": columns}

    def objective(self, ini_state, goal, gate12, p_tra, a_tra, t, u_last=None):
        """Batched run_quad.objective -> (reward (B,), status (B,))."""
        d, f64 = self.device, torch.float64
        B, ini, goal, p, a, tt, ul, g12 = _solve_inputs(d, f64, ini_state, goal, p_tra, a_tra, t, u_last, gate12, True)
        R = torch.empty((B,), dtype=f64, device=d)
        st = torch.empty((B,), dtype=torch.int32, device=d)
        check(self._L.lafse3_objective(self._ctx, B, _ptr(ini), _ptr(goal), _ptr(g12), _ptr(p), _ptr(a), _ptr(tt),
                                       _ptr(ul), _ptr(R), _ptr(st), self._stream()), "lafse3_objective")
        return R, st

    def sol_gradient(self, ini_state, goal, gate12, dnn_out, u_last=None, want_rewards=False, grad_mode=None,
                     verify=True):
        """Batched run_quad.sol_gradient: dnn_out (B,7) float32 -> out8 (B,8) float64 [+ rewards9, status9].
        ``grad_mode``: None = the context's setting, 0 = FD (9 solves, the reference), 1 = IFT (3 solves +
        six sensitivity sweeps, lafse3.h).  ``verify``: wait for the launch and raise Lafse3Error when a probe
        task was lost (its out8 row would carry a NaN into the DNN1 update); False leaves the launch
        asynchronous -- the caller then checks (check_device / last_counters) before using out8."""
        d, f64 = self.device, torch.float64
        B, ini, goal, dnn, ul, g12 = _dnn_inputs(d, ini_state, goal, dnn_out, u_last, gate12, True)
        out8 = torch.empty((B, 8), dtype=f64, device=d)
        R9 = torch.empty((B, 9), dtype=f64, device=d) if want_rewards else None
        S9 = torch.empty((B, 9), dtype=torch.int32, device=d) if want_rewards else None
        with _param_override(self, "grad_mode", grad_mode):
            check(self._L.lafse3_sol_gradient(self._ctx, B, _ptr(ini), _ptr(goal), _ptr(g12), _ptr(dnn), _ptr(ul),
                                              _ptr(out8), _ptr(R9), _ptr(S9), self._stream()), "lafse3_sol_gradient")
        if verify:
            self.check_device()
        if want_rewards:
            return out8, R9, S9
        return out8

    def dnn2_weights(self, net):
        """DNN2 (18-128-128-7 nn.Module, e.g. nn3_1.pth's weights) packed as lafse3_traversal_time expects:
        l1.weight, l1.bias, l2.weight, l2.bias, l3.weight row 6, l3.bias[6] (float32, device).
        Cached per module until its parameters change."""
        key = (id(net), tuple(p._version for p in net.parameters()))
        cached = getattr(self, "_dnn2_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        sd = {k: v.detach().to(device=self.device, dtype=torch.float32) for k, v in net.state_dict().items()}
        if sd["l1.weight"].shape != (128, 18) or sd["l2.weight"].shape != (128, 128) or sd["l3.weight"].shape[1] != 128:
            raise _lib.Lafse3Error("dnn2_weights: expected the 18-128-128-7 DNN2 of nn3_1.pth")
        w = torch.cat([sd["l1.weight"].reshape(-1), sd["l1.bias"], sd["l2.weight"].reshape(-1),
                       sd["l2.bias"], sd["l3.weight"][6], sd["l3.bias"][6:7]]).contiguous()
        if w.numel() != self._L.lafse3_dnn2_weight_count():
            raise _lib.Lafse3Error("dnn2_weights: packed size mismatch")
        self._dnn2_cache = (key, w)
        return w

    def traversal_time(self, state, final_point, gate12, velo, w, net, want_iters=False):
        """quad_moving.solver (quad_moving.py:29-57) for B episodes in one kernel: (B,) traversal times
        [+ (B,) fixed-point updates].  gate12: (B, 12) or (B, 4, 3) corners; velo (B, 3); w the pitch rate;
        net the DNN2 module."""
        d, f64 = self.device, torch.float64
        st = _dev_tensor(state, (NX,), f64, d, "state")
        B = st.shape[0]
        fin = _dev_tensor(final_point, (3,), f64, d, "final_point")
        g = torch.as_tensor(gate12, dtype=f64, device=d).reshape(-1, 12).contiguous()
        ve = _dev_tensor(velo, (3,), f64, d, "velo")
        fin, g, ve = _same_batch(B, final_point=fin, gate12=g, velo=ve)
        W = self.dnn2_weights(net)
        t = torch.empty((B,), dtype=f64, device=d)
        it = torch.empty((B,), dtype=torch.int32, device=d) if want_iters else None
        check(self._L.lafse3_traversal_time(self._ctx, B, _ptr(st), _ptr(fin), _ptr(g), _ptr(ve), float(w), _ptr(W),
                                            _ptr(t), _ptr(it), self._stream()), "lafse3_traversal_time")
        return (t, it) if want_iters else t

    def reward(self, x, goal, gate12):
        """Score given trajectories (B, N+1, 13) as run_quad.objective does -> reward (B,).
        Needs horizon >= 2, as objective and sol_gradient do: the goal path term reads rows N-4..N-1 with numpy's
        wrap of negative rows, which the reference cannot index at horizon 1 (Lafse3Error there)."""
        d, f64 = self.device, torch.float64
        xs = _dev_tensor(x, (self.horizon + 1, NX), f64, d, "x")
        B = xs.shape[0]
        goal = _dev_tensor(goal, (3,), f64, d, "goal")
        g12 = _dev_tensor(gate12, (12,), f64, d, "gate12")
        goal, g12 = _same_batch(B, goal=goal, gate12=g12)
        R = torch.empty((B,), dtype=f64, device=d)
        check(self._L.lafse3_reward(self._ctx, B, _ptr(xs), _ptr(goal), _ptr(g12), _ptr(R), self._stream()),
              "lafse3_reward")
        return R

    def get_input(self, ini_state, goal, dnn_out, u_last=None, want_x=False):
        """Batched run_quad.get_input: first control (B,4) [+ state trajectory (B,N+1,13)]."""
        d, f64 = self.device, torch.float64
        B, ini, goal, dnn, ul, _ = _dnn_inputs(d, ini_state, goal, dnn_out, u_last)
        u0 = torch.empty((B, NU), dtype=f64, device=d)
        x = torch.empty((B, self.horizon + 1, NX), dtype=f64, device=d) if want_x else None
        st = torch.empty((B,), dtype=torch.int32, device=d)
        check(self._L.lafse3_get_input(self._ctx, B, _ptr(ini), _ptr(goal), _ptr(ul), _ptr(dnn), _ptr(u0), _ptr(x),
                                       _ptr(st), self._stream()), "lafse3_get_input")
        return (u0, x, st) if want_x else (u0, st)
