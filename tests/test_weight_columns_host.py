"""CPU unit tests of the dF/dw closed forms of the ten cost weights (csrc/weight_columns.hpp compiled for the host
with hipcc, tests/native/weight_columns_host.cpp) against the oracle's cost gradient (oracle.cost_eval) and a numpy
statement of the control terms.  The columns are those of lafse3_ocp_sensitivity_w's weights group, before the
objective scaling:

    wrt wqt wrf wvf wqf wwf   the stage-cost gradient at the parameter set whose six state weights are zero but a
                              one in that place: evaluated directly, no subtraction, 1e-13 on |a - b| / (1 + |b|)
                              (tests/test_model_host.py's scale);
    tra_w_peak, tra_w_decay   exp(-decay (dt k - t)^2) and -(dt k - t)^2 wk times the oracle's traversal gradient (its
                              gradient with the four path weights zero at stage weight 1), zero at the terminal stage.
                              The header forms the traversal gradient as state_cost_grad at stage weight 1 minus at 0,
                              so its position rows carry the rounding of the path term they cancel, 2 wrf |x - goal|
                              <= 2 * 6 * 15 * 2^-52 = 4e-14 here, times a factor <= peak / (e decay) < 3: the bar is
                              1e-12 on the same scale;
    wthrust, du_weight        2 u_k and 2 (u_k - u_{k-1}) - 2 (u_{k+1} - u_k) with u_{-1} = u_last and no second term
                              at k = N - 1, at N = 1, 2, 5: the same operations in numpy, so equal to the bit.
Rows D (the defaults) and G (generic_params.GENERIC's weights) supply the instance's weights."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from generic_params import GENERIC
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "weight_columns_host.cpp")
LIB = os.path.join(HERE, "native", "libweight_columns_host.so")
CSRC = os.path.join(REPO, "learningagileflight_se3_amd", "csrc")
NAMES = ("wrt", "wqt", "wthrust", "wrf", "wvf", "wqf", "wwf", "tra_w_peak", "tra_w_decay", "du_weight")
STATE_W = ("wrt", "wqt", "wrf", "wvf", "wqf", "wwf")
ROWS = {"D": {}, "G": {k: getattr(GENERIC, k) for k in NAMES}}

pd = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(pd)


@pytest.fixture(scope="module")
def host():
    deps = [SRC, os.path.join(CSRC, "weight_columns.hpp"), os.path.join(CSRC, "model.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I" + os.path.join(REPO, "include"), "-I" + CSRC, "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    L.weight_columns_host_x.argtypes = [ctypes.c_void_p, ctypes.c_int] + [pd] * 6 + [ctypes.POINTER(ctypes.c_int)] + [pd]
    L.weight_columns_host_u.argtypes = [ctypes.c_int, pd, pd, pd]
    return L


def _points(n, seed, row):
    """Seeded states with unit quaternions, unit traversal quaternions, stage times around the traversal, the stage
    weight the solver would build from the row's peak and decay, and a terminal stage every fifth point."""
    from learningagileflight_se3_amd._lib import default_params
    prm = default_params(**ROWS[row])
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5, 5, (n, 13))
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    x[:, 10:13] = rng.uniform(-1.5, 1.5, (n, 3))
    goal, ptra = rng.uniform(-10, 10, (n, 3)), rng.uniform(-10, 10, (n, 3))
    qtra = rng.normal(size=(n, 4))
    qtra /= np.linalg.norm(qtra, axis=1, keepdims=True)
    dtk = rng.uniform(-1.0, 1.0, n)
    dtk[::11] = 0.0                                       # t = dt k: the decay column vanishes
    last = np.zeros(n, np.int32)
    last[::5] = 1
    wk = np.where(last == 1, 0.0, prm.tra_w_peak * np.exp(-prm.tra_w_decay * dtk * dtk))
    return prm, x, goal, ptra, qtra, wk, dtk, last


def _columns(host, prm, x, goal, ptra, qtra, wk, dtk, last):
    n = x.shape[0]
    out = np.zeros((n, 10, 13))
    host.weight_columns_host_x(ctypes.addressof(prm), n, _p(x), _p(goal), _p(ptra), _p(qtra), _p(wk), _p(dtk),
                               last.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _p(out))
    return out


rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))


@pytest.mark.parametrize("row", ["D", "G"])
def test_linear_state_weight_columns_are_the_oracle_gradient_at_unit_weight(host, row):
    n = 257
    prm, x, goal, ptra, qtra, wk, dtk, last = _points(n, 960 + ord(row), row)
    cols = _columns(host, prm, x, goal, ptra, qtra, wk, dtk, last)
    zero = {k: 0.0 for k in STATE_W}
    for name in STATE_W:
        q = NAMES.index(name)
        _, _, g, _ = O.cost_eval(x, goal, ptra, qtra, wk, params=O.default_params(**{**zero, name: 1.0}))
        assert np.max(np.abs(g)) > 1.0, name              # the column is there
        assert rel(cols[:, q], g) < 1e-13, (name, rel(cols[:, q], g))
    # the goal-attitude column is the unit-weight gradient also where the instance's own wqf is 0 (row D)
    assert np.max(np.abs(cols[:, NAMES.index("wqf"), 6:10])) > 0.1
    # the traversal pair carries the stage weight: nothing at a terminal stage
    assert np.all(cols[last == 1][:, [0, 1]] == 0.0)
    # the two control weights have no x rows
    assert np.all(cols[:, [2, 9]] == 0.0)


@pytest.mark.parametrize("row", ["D", "G"])
def test_peak_and_decay_columns_are_multiples_of_the_oracle_traversal_gradient(host, row):
    n = 257
    prm, x, goal, ptra, qtra, wk, dtk, last = _points(n, 970 + ord(row), row)
    cols = _columns(host, prm, x, goal, ptra, qtra, wk, dtk, last)
    only_tra = O.default_params(wrt=prm.wrt, wqt=prm.wqt, wrf=0.0, wvf=0.0, wqf=0.0, wwf=0.0)
    _, _, gtra, _ = O.cost_eval(x, goal, ptra, qtra, np.ones(n), params=only_tra)
    live = (last == 0)[:, None]
    peak = live * np.exp(-prm.tra_w_decay * dtk * dtk)[:, None] * gtra
    decay = live * (-(dtk * dtk) * wk)[:, None] * gtra
    assert np.max(np.abs(peak)) > 1.0 and np.max(np.abs(decay)) > 1.0
    assert rel(cols[:, 7], peak) < 1e-12, rel(cols[:, 7], peak)
    assert rel(cols[:, 8], decay) < 1e-12, rel(cols[:, 8], decay)
    assert np.all(cols[last == 1][:, [7, 8]] == 0.0)
    assert np.all(cols[dtk == 0.0][:, 8] == 0.0)          # t = dt k
    # peak = 0 is fine: the exponential is computed directly, not as wk / peak
    from learningagileflight_se3_amd._lib import default_params
    prm0 = default_params(**{**ROWS[row], "tra_w_peak": 0.0})
    cols0 = _columns(host, prm0, x, goal, ptra, qtra, np.zeros(n), dtk, last)
    assert np.all(np.isfinite(cols0)) and np.array_equal(cols0[:, 7], cols[:, 7]) and np.all(cols0[:, 8] == 0.0)


@pytest.mark.parametrize("N", [1, 2, 5])
def test_control_weight_columns_equal_the_numpy_statement(host, N):
    rng = np.random.default_rng(980 + N)
    u, ulast = rng.uniform(0.0, 2.4, (N, 4)), rng.uniform(0.0, 2.4, 4)
    out = np.full((10, N, 4), np.nan)
    host.weight_columns_host_u(N, _p(u), _p(ulast), _p(out))
    um = np.concatenate([ulast[None], u[:-1]])            # u_{k-1}, u_last at k = 0
    du = 2 * (u - um)
    du[:-1] += -2 * (u[1:] - u[:-1])                      # no second term at k = N - 1
    assert np.array_equal(out[2], 2 * u)
    assert np.array_equal(out[9], du)
    assert np.all(out[[0, 1, 3, 4, 5, 6, 7, 8]] == 0.0)
    assert np.all(out[9, 0] == 2 * (u[0] - ulast) - (2 * (u[1] - u[0]) if N > 1 else 0.0))
