"""What the sensitivity tests share (test_gpu_sens.py, test_gpu_sens_ex.py, test_gpu_sens_w.py, test_gpu_vjp.py,
test_gpu_sens_queue.py, test_gpu_generic_sens.py, test_gpu_generic_sens_w.py): the inputs, the finite-difference
yardstick of the CPU oracle with its admission rule, the acceptance rule against it, the two adjoint identities and
the constants of all of them.  Not collected; torch is imported only where a function needs it.

Yardstick.  Central differences of the oracle's solve at a step h and at 2 h per parameter column, over the
(N+1) 13 + N 4 trajectory entries.  A (sample, column) pair is admitted, from the oracle alone and before any GPU value
is looked at, when its four perturbed solves end with status <= 1 and e = max|J_h - J_2h| / max|J_h| <= ADMIT: the
finite difference is then usable there (no other local optimum, no active-set change inside +-2h).

Acceptance.  On admitted pairs of instances with sens_status 0:  err = max|J_gpu - J_h| / max|J_h| <= 10 e + F.
10 e covers the finite difference's own truncation / solver noise, F what is not its fault (the barrier smoothing at the
final mu, the 1e-8 KKT tolerance of both optima).  At most 15 % of the pairs may be left out, and at most one instance
may be without a sensitivity.
"""
from __future__ import annotations

import numpy as np
import pytest

H = 1e-4             # finite-difference step of the oracle yardstick (and 2 H); for a weight w_j, H max(|w_j|, 1)
ADMIT = 1e-3         # admission: h-versus-2h disagreement relative to max|J_h|
# The default F: the largest err - 10 e over the admitted pairs of test_gpu_sens.py's first GPU run (horizon 50 and
# 20), 3.914e-4, rounded up to the next power of ten.  Never above ADMIT: above it the test could not tell a right
# column from a wrong one.  test_gpu_sens_w.py and test_gpu_generic_sens_w.py state smaller ones per case.
F = 1e-3
# gain == du_0 (adjoint_difference): the largest difference of test_gpu_sens_ex.py's first GPU run, 1.600e-07
# (horizons 50, 20, 2, 1; always in the ini_state group), rounded up to the next power of ten, never above 1e-5 (the
# project's parity scale): a larger difference is a wrong sign, row block or stage-0 contraction, not a bar to raise.
# All 33 columns of test_gpu_sens_w.py's launches keep it (first run there 3.190e-07).
ADJ_BAR = 1e-6
# the weight columns alone: test_gpu_sens_w.py's first GPU run 1.225e-13, rounded up likewise
ADJ_BAR_WEIGHTS = 1e-12
# ocp_vjp against the contracted forward Jacobians (vjp_relative): test_gpu_vjp.py's first GPU run 1.753e-07 (horizon
# 20, g_u alone, ini_state group), rounded up likewise
VJP_BAR = 1e-6
# the columns of lafse3_ocp_sensitivity_w / lafse3_ocp_vjp per parameter group, in the fixed order
SL = {"theta": slice(0, 7), "ini": slice(7, 20), "goal": slice(20, 23), "weights": slice(23, 33)}
GROUPS = tuple(SL)
# words of the optimum record of lafse3_ocp_solve_rec (include/lafse3.h)
REC_X, REC_U, REC_STATUS, REC_N, REC_W = 0, 663, 2221, 2222, 2223


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")


def batch():
    """scenario.synthetic_batch(64, seed=2025), the batch of tests/test_gpu_parity.py, with p, a, t widened to float64."""
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(64, seed=2025)
    sb["p"] = sb["dnn_out"][:, :3].astype(np.float64)
    sb["a"] = sb["dnn_out"][:, 3:6].astype(np.float64)
    sb["t"] = sb["dnn_out"][:, 6].astype(np.float64)
    return sb


def traj(x, u):
    """(.., N+1, 13), (.., N, 4) -> (.., 13 (N+1) + 4 N): the trajectory entries of one solve."""
    return np.concatenate([x.reshape(*x.shape[:-2], -1), u.reshape(*u.shape[:-2], -1)], axis=-1)


def to_numpy(out):
    """An engine call's dict with its tensors as numpy arrays; the other values (the column names) as they are."""
    import torch
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


# ---- the oracle's finite differences --------------------------------------------------------------------------

def fd_tables(z, ok, steps):
    """z (Q, 2, 2, n, E): the perturbed trajectories [column][h, 2h][+, -][sample]; ok: their status <= 1, (Q, 2, 2, n);
    steps: h per column, (Q,).  Returns J = J_h (n, Q, E) and e, admitted, scale = max|J_h| (n, Q)."""
    h = np.asarray(steps, dtype=np.float64).reshape(-1, 1, 1)
    J_h = np.transpose((z[:, 0, 0] - z[:, 0, 1]) / (2 * h), (1, 0, 2))
    J_2h = np.transpose((z[:, 1, 0] - z[:, 1, 1]) / (4 * h), (1, 0, 2))
    scale = np.abs(J_h).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(J_h - J_2h).max(-1) / scale
    e = np.where(np.isfinite(e), e, np.inf)              # a column that moves nothing (scale 0) is not admitted
    return {"J": J_h, "e": e, "admitted": ok.all(axis=(1, 2)).T & (e <= ADMIT), "scale": scale}


def oracle_fd(prob, n, horizon, cols, params=None):
    """The yardstick for the first n samples of `prob` (ini, goal, p, a, t and, if it has one, ulast) in the columns
    `cols` of z = (p_tra 3, a_tra 3, t, ini_state 13, goal 3) at steps H and 2 H, one batched oracle call.  params:
    the oracle's parameter block, the defaults at the horizon if None."""
    from oracle import oracle as O
    cols = list(cols)
    z0 = np.concatenate([prob["p"][:n], prob["a"][:n], prob["t"][:n, None], prob["ini"][:n], prob["goal"][:n]], axis=1)
    steps = [(q, s * m * H) for q in cols for m in (1, 2) for s in (+1, -1)]
    Z = np.repeat(z0[None], len(steps), 0)                                      # (steps, n, 23)
    for j, (q, d) in enumerate(steps):
        Z[j, :, q] += d
    Z = Z.reshape(-1, 23)
    quat = np.stack([O.rd2quat(a) for a in Z[:, 3:6]])
    ul = None if prob.get("ulast") is None else np.tile(prob["ulast"][:n], (len(steps), 1))
    r = O.solve(np.ascontiguousarray(Z[:, 7:20]), np.ascontiguousarray(Z[:, 20:23]), np.ascontiguousarray(Z[:, 0:3]),
                quat, np.ascontiguousarray(Z[:, 6]), ulast=ul,
                params=O.default_params(horizon=horizon) if params is None else params)
    Q = len(cols)
    return fd_tables(traj(r["x"], r["u"]).reshape(Q, 2, 2, n, -1), (r["status"] <= 1).reshape(Q, 2, 2, n), [H] * Q)


def oracle_fd_weights(prob, n, row, cols, params_for):
    """The yardstick for the first n samples of `prob` (ini, goal, p, t, q or a and, if it has one, ulast) in the
    weights `cols` of `row`, at steps h_j = H max(|w_j|, 1) (the max because wqf is 0 by default) and 2 h_j.
    params_for(row) returns the oracle's parameter block, horizon included, with the ten weights of the row."""
    from oracle import oracle as O
    cols = list(cols)
    quat = prob["q"][:n] if "q" in prob else np.stack([O.rd2quat(a) for a in prob["a"][:n]])
    ul = None if prob.get("ulast") is None else prob["ulast"][:n]
    z, ok, steps = [], [], []
    for j in cols:
        h = H * max(abs(row[j]), 1.0)
        for m in (1, 2):
            for s in (+1, -1):
                w = row.copy()
                w[j] += s * m * h
                r = O.solve(prob["ini"][:n], prob["goal"][:n], prob["p"][:n], quat, prob["t"][:n], ulast=ul,
                            params=params_for(w))
                z.append(traj(r["x"], r["u"]))
                ok.append(r["status"] <= 1)
        steps.append(h)
    Q = len(cols)
    return fd_tables(np.stack(z).reshape(Q, 2, 2, n, -1), np.stack(ok).reshape(Q, 2, 2, n), steps)


def check_against_fd(J_gpu, sens_status, fd, label, F, max_left_out=0.15, names=None):
    """err <= 10 e + F on the admitted pairs of instances with sens_status 0; prints every figure first.  names: the
    columns' names, for the printed lines.  Returns err, err - 10 e (-inf where not compared) and the compared pairs."""
    adm = fd["admitted"]
    per = "" if names is None else f"; per column {dict(zip(names, adm.sum(0).tolist()))}"
    print(f"{label}: oracle admits {int(adm.sum())} of {adm.size} pairs{per}; sens_status histogram "
          f"{np.bincount(sens_status, minlength=3).tolist()}")
    use = adm & (sens_status == 0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(J_gpu - fd["J"]).max(-1) / fd["scale"]
    excess = np.where(use, err - 10 * fd["e"], -np.inf)
    i, q = np.unravel_index(np.argmax(excess), excess.shape)
    col = f"parameter {q}" if names is None else f"column {names[q]}"
    print(f"{label}: {int(use.sum())} pairs compared; max err {err[use].max():.3e}; max(err - 10 e) {excess.max():.3e} "
          f"at sample {i} {col} (err {err[i, q]:.3e}, e {fd['e'][i, q]:.3e}); median err {np.median(err[use]):.3e} "
          f"(F {F:.0e})")
    assert (~adm).mean() <= max_left_out, f"{label}: {int((~adm).sum())} of {adm.size} pairs not admitted"
    assert use.sum() >= adm.sum() - adm.shape[1]          # at most one instance without a sensitivity
    assert excess.max() <= F, (label, float(excess.max()), int(i), int(q))
    return err, excess, use


# ---- the adjoint identities -----------------------------------------------------------------------------------

def adjoint_difference(g, label, groups, bar):
    """gain[b, a, q] against du[b, q, 0, a] of one launch, the identity K^-T = K^-1: the largest, over live instances
    and the column groups (name -> slice), of max|gain - du_0| / max|du_0|, both over the group's columns of the
    instance.  A group that does not move u_0 at all (theta at horizon 1: no traversal stage) must give exact zeros."""
    live = g["sens_status"] == 0
    du0 = np.transpose(g["du"][:, :, 0, :], (0, 2, 1))                         # (B, 4, P)
    gain = g["gain"]
    assert gain.shape == du0.shape and np.all(np.isfinite(gain)) and np.all(np.isfinite(du0))
    worst, where = 0.0, None
    for name, sl in groups.items():
        diff = np.abs(gain[:, :, sl] - du0[:, :, sl]).max(axis=(1, 2))
        scale = np.abs(du0[:, :, sl]).max(axis=(1, 2))
        rel = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff == 0, 0.0, np.inf))
        rel = np.where(live, rel, 0.0)
        b = int(np.argmax(rel))
        per_col = np.abs(du0[live][:, :, sl]).max(axis=(0, 1))
        print(f"{label}: group {name}: max relative |gain - du_0| {rel.max():.3e} (sample {b}, scale {scale[b]:.3e}); "
              f"largest |du_0| per column {dict(zip(g['columns'][sl], (f'{v:.2e}' for v in per_col)))}")
        if rel.max() >= worst:
            worst, where = float(rel.max()), (name, b)
    print(f"{label}: {int(live.sum())} of {live.size} instances live; max relative difference {worst:.3e} at {where} "
          f"(bar {bar:.0e})")
    assert live.sum() >= live.size - 1
    return worst


def vjp_reference(fwd, g_x, g_u):
    """grad (B, 33) from the forward Jacobians, and the (B, 4) group scales max_q sum|dx||g_x| + sum|du||g_u|."""
    ref = np.einsum("bqki,bki->bq", fwd["dx"], g_x) + np.einsum("bqka,bka->bq", fwd["du"], g_u)
    mag = np.einsum("bqki,bki->bq", np.abs(fwd["dx"]), np.abs(g_x)) + \
        np.einsum("bqka,bka->bq", np.abs(fwd["du"]), np.abs(g_u))
    return ref, np.stack([mag[:, SL[g]].max(1) for g in GROUPS], 1)


def vjp_relative(grad, ref, scale, label):
    """Largest |grad - ref| / group scale per group; a group with scale 0 must agree exactly.  Prints every figure."""
    worst = {}
    for j, g in enumerate(GROUPS):
        diff = np.abs(grad[:, SL[g]] - ref[:, SL[g]]).max(1)
        s = scale[:, j]
        rel = np.where(s > 0, diff / np.where(s > 0, s, 1.0), np.where(diff == 0, 0.0, np.inf))
        worst[g] = float(rel.max())
    print(f"{label}: largest relative difference per group " + ", ".join(f"{g} {v:.3e}" for g, v in worst.items()))
    return max(worst.values())
