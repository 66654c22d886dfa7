"""Inputs and the oracle yardstick of tests/test_gpu_sens_w.py (the weight columns of lafse3_ocp_sensitivity_w).

Inputs: scenario.synthetic_batch(64, seed=2025) with p, a, t widened to float64, as tests/test_gpu_sens_ex.py.  Two
rows of cost weights, in the column order of lafse3_params (WEIGHT_NAMES):
    D  the defaults                                    5, 80, 0.1, 5, 5, 0, 3, 60, 10, 1
    G  generic_params.GENERIC's weights                4, 60, 0.15, 6, 4, 2, 2.5, 50, 8, 0.7
Only the weights are taken from GENERIC: the model, the bounds and dt stay the defaults.

Yardstick: central differences of oracle.solve with weight j changed through oracle.default_params(**{name: value}),
at steps h_j and 2 h_j with h_j = 1e-4 max(|w_j|, 1) (the max because wqf is 0 by default).  A (sample, weight) pair
is admitted from the oracle alone when its four solves end with status <= 1 and e = max|J_h - J_2h| / max|J_h| <= 1e-3.
"""
from __future__ import annotations

import numpy as np

WEIGHT_NAMES = ("wrt", "wqt", "wthrust", "wrf", "wvf", "wqf", "wwf", "tra_w_peak", "tra_w_decay", "du_weight")
ROW_D = np.array([5.0, 80.0, 0.1, 5.0, 5.0, 0.0, 3.0, 60.0, 10.0, 1.0])
ROW_G = np.array([4.0, 60.0, 0.15, 6.0, 4.0, 2.0, 2.5, 50.0, 8.0, 0.7])
NON_TRAVERSAL = (2, 3, 4, 5, 6, 9)        # wthrust wrf wvf wqf wwf du_weight
H_REL = 1e-4
ADMIT = 1e-3


def batch():
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(64, seed=2025)
    sb["p"] = sb["dnn_out"][:, :3].astype(np.float64)
    sb["a"] = sb["dnn_out"][:, 3:6].astype(np.float64)
    sb["t"] = sb["dnn_out"][:, 6].astype(np.float64)
    return sb


def case_t(sb, horizon):
    """The traversal times of the finite-difference cases: as given at N = 50; clip(0.5 t, 0.3, 1.5) at N = 20, so
    that the traversal lies inside the 2 s horizon; 0.1 at N = 2 and N = 1."""
    if horizon == 50:
        return sb["t"].copy()
    if horizon == 20:
        return np.clip(0.5 * sb["t"], 0.3, 1.5)
    return np.full_like(sb["t"], 0.1)


def traj(x, u):
    """(.., N+1, 13), (.., N, 4) -> (.., 13 (N+1) + 4 N): the trajectory entries of one solve."""
    return np.concatenate([x.reshape(*x.shape[:-2], -1), u.reshape(*u.shape[:-2], -1)], axis=-1)


def oracle_solve(sb, n, horizon, t, row, ulast=None):
    """oracle.solve of the first n samples under the weight row."""
    from oracle import oracle as O
    prm = O.default_params(horizon=horizon, **dict(zip(WEIGHT_NAMES, map(float, row))))
    quat = np.stack([O.rd2quat(a) for a in sb["a"][:n]])
    return O.solve(sb["ini"][:n], sb["goal"][:n], sb["p"][:n], quat, t[:n], ulast=ulast, params=prm)


def oracle_fd(sb, n, horizon, t, row, cols=range(10)):
    """Central differences at h_j and 2 h_j of the first n samples' trajectories in the weights `cols` of `row`.
    Returns J (n, len(cols), E), e, admitted, scale = max|J_h| (n, len(cols))."""
    cols = list(cols)
    J_h, J_2h, ok = [], [], []
    for j in cols:
        h = H_REL * max(abs(row[j]), 1.0)
        z, st = {}, []
        for m in (1, 2):
            for s in (+1, -1):
                w = row.copy()
                w[j] += s * m * h
                r = oracle_solve(sb, n, horizon, t, w)
                z[m, s] = traj(r["x"], r["u"])
                st.append(r["status"] <= 1)
        J_h.append((z[1, 1] - z[1, -1]) / (2 * h))
        J_2h.append((z[2, 1] - z[2, -1]) / (4 * h))
        ok.append(np.all(st, axis=0))
    J_h, J_2h, ok = np.stack(J_h, 1), np.stack(J_2h, 1), np.stack(ok, 1)
    scale = np.abs(J_h).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(J_h - J_2h).max(-1) / scale
    e = np.where(np.isfinite(e), e, np.inf)
    return {"J": J_h, "e": e, "admitted": ok & (e <= ADMIT), "scale": scale, "cols": cols}
