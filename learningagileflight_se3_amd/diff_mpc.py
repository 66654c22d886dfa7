"""Differentiable MPC layer: ``loss.backward()`` through the batched solve.

``mpc_layer`` solves the NLP of OCSys.ocSolver (quad_OC.py:104-212) for a batch of traversal parameters
theta = (p_tra, a_tra, t) and returns the optimal trajectory as tensors that carry a gradient to theta.  The forward
pass is one ``Engine.ocp_sensitivity`` launch, which also returns the Jacobians dx*/dtheta and du*/dtheta from the
factorisation at the optimum (implicit function theorem, include/lafse3.h); the backward pass contracts them with
the incoming gradients.  This is the derivative the reference sketched as the PDP auxiliary system
(quad_OC.py:214-306, commented out there).

The derivative is that of the barrier problem at the solver's final mu: across an active-set change it is a
one-sided smoothing, not a subgradient.  Instances whose sensitivity is not available (the solve did not converge,
or the factorisation at the optimum met a wrong inertia: ``sens_status != 0``) contribute a zero gradient.

When ``ini_state`` or ``goal`` requires a gradient, ``mpc_layer`` goes through ``Engine.ocp_sensitivity_ex`` instead,
which also has their columns, and ``mpc_policy`` returns the first control u*_0 with a gradient to all five inputs from
the feedback gain alone (include/lafse3.h lafse3_ocp_sensitivity_ex): the layer for closed-loop rollouts.  u_last is
a constant throughout.

With ``weights=`` (the ten cost weights per instance, ``Engine.ocp_sensitivity_w``) both layers solve each instance
under its own weights and send a gradient to them: the derivative with respect to the learnable parameters of the
cost.  Without it they are the functions above, with the same launches.

``mpc_layer(..., backward="adjoint")`` keeps the optimum instead of its Jacobians: the forward pass is one
``Engine.ocp_solve_rec`` launch that saves the primal-dual point (about 18 KB per instance), and ``backward()`` is one
``Engine.ocp_vjp`` launch that factorises there and sweeps once on the incoming gradient (K is symmetric, so
g^T K^{-1} c_q for every column q costs one solve with g).  The default route stores B x P x 863 doubles and runs P sweeps.
"""
from __future__ import annotations

import torch


def _contract(dx, du, sens_status, g_x, g_u):
    """The trajectory contraction: g (B, P) with
      g[b, q] = sum_ki dx[b, q, k, i] g_x[b, k, i] + sum_ka du[b, q, k, a] g_u[b, k, a]
    (g_x, g_u None = zero), accumulated in the Jacobians' dtype; rows with sens_status != 0 are zero."""
    g = torch.zeros(dx.shape[:2], dtype=dx.dtype, device=dx.device)
    if g_x is not None:
        g = g + torch.einsum("bqki,bki->bq", dx, g_x.to(dx.dtype))
    if g_u is not None:
        g = g + torch.einsum("bqka,bka->bq", du, g_u.to(du.dtype))
    return torch.where((sens_status != 0).unsqueeze(1), torch.zeros_like(g), g)


def _contract_gain(gain, sens_status, g_u0):
    """The gain contraction: g[b, q] = sum_a gain[b, a, q] g_u0[b, a]; rows with sens_status != 0 are zero."""
    g = torch.einsum("baq,ba->bq", gain, g_u0.to(gain.dtype))
    return torch.where((sens_status != 0).unsqueeze(1), torch.zeros_like(g), g)


def mpc_backward(dx, du, sens_status, g_x, g_u, dtypes=None):
    """Vector-Jacobian product of the MPC layer on plain tensors (any device).

    dx (B, 7, N+1, 13), du (B, 7, N, 4): Jacobians, parameter order p_tra[0..2], a_tra[0..2], t;
    sens_status (B,): rows != 0 give zero; g_x (B, N+1, 13), g_u (B, N, 4): gradients w.r.t. x and u (None = zero).
    Returns (grad_p (B, 3), grad_a (B, 3), grad_t (B,)) with
      grad_theta[b, q] = sum_ki dx[b, q, k, i] g_x[b, k, i] + sum_ka du[b, q, k, a] g_u[b, k, a],
    cast to ``dtypes`` = (p, a, t dtypes) when given."""
    g = _contract(dx, du, sens_status, g_x, g_u)
    gp, ga, gt = g[:, 0:3], g[:, 3:6], g[:, 6]
    if dtypes is not None:
        gp, ga, gt = gp.to(dtypes[0]), ga.to(dtypes[1]), gt.to(dtypes[2])
    return gp, ga, gt


# The parameter groups of Engine.ocp_sensitivity_w in column order (Engine.ocp_sensitivity_ex has the first three,
# Engine.ocp_sensitivity the first), each with its columns and the positions of its inputs among (ini_state, goal,
# p_tra, a_tra, t, weights) and their column ranges inside the group.
_GROUPS = (("theta", 7, ((2, 0, 3), (3, 3, 6), (4, 6, 7))), ("ini", 13, ((0, 0, 13),)), ("goal", 3, ((1, 0, 3),)),
           ("weights", 10, ((5, 0, 10),)))


def _needs(ctx):
    """needs_input_grad of (ini_state, goal, p_tra, a_tra, t[, weights]) among a Function's inputs
    (engine, ini_state, goal, p_tra, a_tra, t, u_last[, weights])."""
    return ctx.needs_input_grad[1:6] + ctx.needs_input_grad[7:8]


def _needed_groups(needs):
    """The groups with an input that needs a gradient."""
    return tuple(name for name, _, members in _GROUPS if any(needs[i] for i, _, _ in members))


def _meta(v):
    return (v.dtype, v.shape, v.device) if isinstance(v, torch.Tensor) else None


def _input_grads(ctx, g):
    """g (B, P): the gradient w.r.t. the P columns of ``ctx.groups`` -> backward()'s return: the gradients of
    (ini_state, goal, p_tra, a_tra, t[, weights]) in the dtype, shape and device recorded in ``ctx.metas``, None for
    an input that is no tensor or needs none, and None for the engine and u_last."""
    needs = _needs(ctx)
    out = [None] * len(ctx.metas)
    col = 0
    for name, n, members in _GROUPS:
        if name not in ctx.groups:
            continue
        for i, lo, hi in members:
            if ctx.metas[i] is None or not needs[i]:
                continue
            dtype, shape, device = ctx.metas[i]
            gi = g[:, col + lo:col + hi]
            # an input of one row (a scalar t) was broadcast over the batch: sum its gradient back
            gi = gi if gi.numel() == shape.numel() else gi.sum(0)
            out[i] = gi.reshape(shape).to(device=device, dtype=dtype)
        col += n
    return (None, *out[:5], None, *out[5:])


class MPCFunction(torch.autograd.Function):
    """(engine, ini_state, goal, p_tra, a_tra, t, u_last) -> (x (B, N+1, 13), u (B, N, 4), status (B,)).

    x and u are float64 (the solve's precision) and differentiable w.r.t. p_tra, a_tra and t; float32 parameters
    (DNN outputs) are widened as ``Engine.ocp_solve`` does and receive float32 gradients.  ini_state, goal, u_last
    and the engine get no gradient."""

    @staticmethod
    def forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last=None):
        out = engine.ocp_sensitivity(ini_state, goal, p_tra, a_tra, t, u_last, want=("x", "u", "dx", "du"))
        ctx.save_for_backward(out["dx"], out["du"], out["sens_status"])
        ctx.groups = ("theta",)
        ctx.metas = tuple(_meta(v) for v in (ini_state, goal, p_tra, a_tra, t))
        ctx.mark_non_differentiable(out["status"])
        return out["x"], out["u"], out["status"]

    @staticmethod
    def backward(ctx, g_x, g_u, _g_status):
        return _input_grads(ctx, _contract(*ctx.saved_tensors, g_x, g_u))


def _sensitivity_forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights, plain, sens):
    """The forward pass of MPCFunctionEx and MPCPolicyFunction: one ``Engine.ocp_sensitivity_ex`` launch, or with
    ``weights`` one ``Engine.ocp_sensitivity_w`` launch, that asks for only the parameter groups with an input that
    needs a gradient, and for the outputs ``plain`` plus, when there is such a group, ``sens``, which are saved for
    backward() with sens_status.  Returns the engine's dict."""
    ctx.groups = _needed_groups(_needs(ctx))
    ctx.metas = tuple(_meta(v) for v in (ini_state, goal, p_tra, a_tra, t, weights))
    want = plain + sens if ctx.groups else plain
    if weights is None:
        out = engine.ocp_sensitivity_ex(ini_state, goal, p_tra, a_tra, t, u_last, groups=ctx.groups or ("theta",),
                                        want=want)
    else:
        out = engine.ocp_sensitivity_w(ini_state, goal, p_tra, a_tra, t, u_last, weights=weights,
                                       groups=ctx.groups or ("weights",), want=want)
    if ctx.groups:
        ctx.save_for_backward(*(out[k] for k in sens), out["sens_status"])
    ctx.mark_non_differentiable(out["status"])
    return out


class MPCFunctionEx(torch.autograd.Function):
    """MPCFunction with gradients to ini_state and goal as well, and under per-instance cost weights:
    (engine, ini_state, goal, p_tra, a_tra, t, u_last, weights) -> (x, u, status).  One launch
    (_sensitivity_forward); each input that needs a gradient receives it in its own dtype and shape.  ``weights`` is
    None (the context's weights), (B, 10) or (10,) (broadcast; its gradient is then summed over the batch).  u_last
    and the engine get none.  The quaternion entries of ini_state are differentiated as the four raw numbers the
    solver reads."""

    @staticmethod
    def forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights):
        out = _sensitivity_forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights,
                                   plain=("x", "u"), sens=("dx", "du"))
        return out["x"], out["u"], out["status"]

    @staticmethod
    def backward(ctx, g_x, g_u, _g_status):
        return _input_grads(ctx, _contract(*ctx.saved_tensors, g_x, g_u))


class MPCPolicyFunction(torch.autograd.Function):
    """(engine, ini_state, goal, p_tra, a_tra, t, u_last, weights) -> (u0 (B, 4), status (B,)): the first control of
    the optimum, differentiable in ini_state, goal, p_tra, a_tra, t and ``weights`` (as in MPCFunctionEx) through
    ``gain`` alone (four adjoint sweeps on the factorisation at the optimum; no dx, no du).  Over ini_state the
    Jacobian is the MPC feedback gain."""

    @staticmethod
    def forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights):
        out = _sensitivity_forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights,
                                   plain=("u",), sens=("gain",))
        return out["u"][:, 0].contiguous(), out["status"]

    @staticmethod
    def backward(ctx, g_u0, _g_status):
        return _input_grads(ctx, _contract_gain(*ctx.saved_tensors, g_u0))


class MPCFunctionAdj(torch.autograd.Function):
    """The adjoint route of MPCFunctionEx: (engine, ini_state, goal, p_tra, a_tra, t, u_last, weights) -> (x, u, status)
    with the same gradients, computed at ``backward()`` time instead of stored at forward time.

    forward is one ``Engine.ocp_solve_rec`` launch; it saves the optimum record (``Engine.rec_width()`` doubles per
    instance) and its inputs, never dx or du.  backward is one ``Engine.ocp_vjp`` launch, one factorisation and one
    sweep per instance, for the parameter groups with an input that needs a gradient.  ``weights`` may be None (the
    context's weights, no gradient).  ``backward()`` may be called again with ``retain_graph``.  Double backward is
    not supported: the gradients are returned as constants."""

    @staticmethod
    def forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last, weights):
        inputs = (ini_state, goal, p_tra, a_tra, t, u_last, weights)
        ctx.groups = _needed_groups(_needs(ctx))
        ctx.metas = tuple(_meta(v) for v in (ini_state, goal, p_tra, a_tra, t, weights))
        out = engine.ocp_solve_rec(ini_state, goal, p_tra, a_tra, t, u_last, weights=weights, want=("x", "u"))
        if ctx.groups:
            ctx.engine = engine
            # the tensors among the inputs are saved as such, the others (numpy, floats, None) kept as they are
            ctx.is_tensor = tuple(isinstance(v, torch.Tensor) for v in inputs)
            ctx.plain = tuple(None if s else v for v, s in zip(inputs, ctx.is_tensor))
            ctx.save_for_backward(out["rec"], *(v for v, s in zip(inputs, ctx.is_tensor) if s))
        ctx.mark_non_differentiable(out["status"])
        return out["x"], out["u"], out["status"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_u, _g_status):
        rec, *saved = ctx.saved_tensors
        saved = iter(saved)
        inputs = [next(saved) if s else v for v, s in zip(ctx.plain, ctx.is_tensor)]
        return _input_grads(ctx, ctx.engine.ocp_vjp(*inputs, rec, g_x, g_u, groups=ctx.groups)["grad"])


def _wants_grad(v):
    return isinstance(v, torch.Tensor) and v.requires_grad


def mpc_layer(engine, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None, backward="jacobian"):
    """Differentiable batched MPC solve -> (x, u, status); see MPCFunction.  When ini_state or goal is a tensor that
    requires a gradient, the solve goes through MPCFunctionEx, which also returns gradients to them.  ``weights``
    ((B, 10) or (10,), the cost weights of each instance): the solve goes through MPCFunctionEx under those weights
    (Engine.ocp_sensitivity_w), and a ``weights`` that requires a gradient receives one.

    ``backward``: "jacobian" (the default) is those two functions, which store dx*/dparam and du*/dparam of every
    selected column at forward time (B x P x 863 doubles) and contract them in ``backward()``.  "adjoint" selects
    MPCFunctionAdj for any combination of inputs and weights: the forward launch saves the optimum itself (about 18 KB
    per instance for any P) and ``backward()`` runs one adjoint sweep per instance.  Same gradients up to rounding;
    double backward is not supported on the adjoint route."""
    if backward == "adjoint":
        return MPCFunctionAdj.apply(engine, ini_state, goal, p_tra, a_tra, t, u_last, weights)
    if backward != "jacobian":
        raise ValueError(f'backward: expected "jacobian" or "adjoint", got {backward!r}')
    if weights is not None or _wants_grad(ini_state) or _wants_grad(goal):
        return MPCFunctionEx.apply(engine, ini_state, goal, p_tra, a_tra, t, u_last, weights)
    return MPCFunction.apply(engine, ini_state, goal, p_tra, a_tra, t, u_last)


def mpc_policy(engine, ini_state, goal, p_tra, a_tra, t, u_last=None, weights=None):
    """The MPC policy u0 = u*_0(ini_state, goal, p_tra, a_tra, t) -> (u0 (B, 4), status), differentiable in all five
    (see MPCPolicyFunction): the layer for closed-loop rollouts x_{t+1} = plant(x_t, u0(x_t, ..)).  ``weights`` as in
    mpc_layer."""
    return MPCPolicyFunction.apply(engine, ini_state, goal, p_tra, a_tra, t, u_last, weights)
