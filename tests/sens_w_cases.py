"""Inputs of tests/test_gpu_sens_w.py (the weight columns of lafse3_ocp_sensitivity_w) and of the tests that share them.

Inputs: scenario.synthetic_batch(64, seed=2025) with p, a, t widened to float64, as tests/test_gpu_sens_ex.py.  Two
rows of cost weights, in the column order of lafse3_params (WEIGHT_NAMES):
    D  the defaults                                    5, 80, 0.1, 5, 5, 0, 3, 60, 10, 1
    G  generic_params.GENERIC's weights                4, 60, 0.15, 6, 4, 2, 2.5, 50, 8, 0.7
Only the weights are taken from GENERIC: the model, the bounds and dt stay the defaults.

Yardstick: sens_yardstick.oracle_fd_weights with weight j changed through oracle.default_params(**{name: value})
(params_for below), on a problem whose t is case_t's.
"""
from __future__ import annotations

import numpy as np

from sens_yardstick import batch  # noqa: F401  (the inputs: C.batch())

WEIGHT_NAMES = ("wrt", "wqt", "wthrust", "wrf", "wvf", "wqf", "wwf", "tra_w_peak", "tra_w_decay", "du_weight")
ROW_D = np.array([5.0, 80.0, 0.1, 5.0, 5.0, 0.0, 3.0, 60.0, 10.0, 1.0])
ROW_G = np.array([4.0, 60.0, 0.15, 6.0, 4.0, 2.0, 2.5, 50.0, 8.0, 0.7])
NON_TRAVERSAL = (2, 3, 4, 5, 6, 9)        # wthrust wrf wvf wqf wwf du_weight


def case_t(sb, horizon):
    """The traversal times of the finite-difference cases: as given at N = 50; clip(0.5 t, 0.3, 1.5) at N = 20, so
    that the traversal lies inside the 2 s horizon; 0.1 at N = 2 and N = 1."""
    if horizon == 50:
        return sb["t"].copy()
    if horizon == 20:
        return np.clip(0.5 * sb["t"], 0.3, 1.5)
    return np.full_like(sb["t"], 0.1)


def params_for(horizon):
    """row -> the oracle's default parameters at the horizon with the row's ten weights: the callback of
    sens_yardstick.oracle_fd_weights for these cases."""
    from oracle import oracle as O
    return lambda row: O.default_params(horizon=horizon, **dict(zip(WEIGHT_NAMES, map(float, row))))
