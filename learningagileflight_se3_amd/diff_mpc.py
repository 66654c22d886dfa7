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
"""
from __future__ import annotations

import torch


def mpc_backward(dx, du, sens_status, g_x, g_u, dtypes=None):
    """Vector-Jacobian product of the MPC layer on plain tensors (any device).

    dx (B, 7, N+1, 13), du (B, 7, N, 4): Jacobians, parameter order p_tra[0..2], a_tra[0..2], t;
    sens_status (B,): rows != 0 give zero; g_x (B, N+1, 13), g_u (B, N, 4): gradients w.r.t. x and u (None = zero).
    Returns (grad_p (B, 3), grad_a (B, 3), grad_t (B,)) with
      grad_theta[b, q] = sum_ki dx[b, q, k, i] g_x[b, k, i] + sum_ka du[b, q, k, a] g_u[b, k, a],
    cast to ``dtypes`` = (p, a, t dtypes) when given."""
    g = torch.zeros(dx.shape[:2], dtype=dx.dtype, device=dx.device)
    if g_x is not None:
        g = g + torch.einsum("bqki,bki->bq", dx, g_x.to(dx.dtype))
    if g_u is not None:
        g = g + torch.einsum("bqka,bka->bq", du, g_u.to(du.dtype))
    g = torch.where((sens_status != 0).unsqueeze(1), torch.zeros_like(g), g)
    gp, ga, gt = g[:, 0:3], g[:, 3:6], g[:, 6]
    if dtypes is not None:
        gp, ga, gt = gp.to(dtypes[0]), ga.to(dtypes[1]), gt.to(dtypes[2])
    return gp, ga, gt


class MPCFunction(torch.autograd.Function):
    """(engine, ini_state, goal, p_tra, a_tra, t, u_last) -> (x (B, N+1, 13), u (B, N, 4), status (B,)).

    x and u are float64 (the solve's precision) and differentiable w.r.t. p_tra, a_tra and t; float32 parameters
    (DNN outputs) are widened as ``Engine.ocp_solve`` does and receive float32 gradients.  ini_state, goal, u_last
    and the engine get no gradient."""

    @staticmethod
    def forward(ctx, engine, ini_state, goal, p_tra, a_tra, t, u_last=None):
        out = engine.ocp_sensitivity(ini_state, goal, p_tra, a_tra, t, u_last, want=("x", "u", "dx", "du"))
        ctx.save_for_backward(out["dx"], out["du"], out["sens_status"])
        ctx.theta = tuple((v.dtype, v.shape, v.device) if isinstance(v, torch.Tensor) else None
                          for v in (p_tra, a_tra, t))
        ctx.mark_non_differentiable(out["status"])
        return out["x"], out["u"], out["status"]

    @staticmethod
    def backward(ctx, g_x, g_u, _g_status):
        dx, du, sens_status = ctx.saved_tensors
        grads = mpc_backward(dx, du, sens_status, g_x, g_u)
        out = []
        for g, meta, need in zip(grads, ctx.theta, ctx.needs_input_grad[3:6]):
            if meta is None or not need:
                out.append(None)
                continue
            dtype, shape, device = meta
            # a t of one element was broadcast over the batch (Engine.ocp_solve does the same): sum its gradient back
            g = g if g.numel() == shape.numel() else g.sum()
            out.append(g.reshape(shape).to(device=device, dtype=dtype))
        return (None, None, None, out[0], out[1], out[2], None)


def mpc_layer(engine, ini_state, goal, p_tra, a_tra, t, u_last=None):
    """Differentiable batched MPC solve -> (x, u, status); see MPCFunction."""
    return MPCFunction.apply(engine, ini_state, goal, p_tra, a_tra, t, u_last)
