"""CPU unit tests of the DEVICE model closed forms (csrc/model.hpp compiled for the host with hipcc)
against the oracle's dense derivatives (which are pinned to the reference's sympy expressions by
tests/test_oracle_golden.py).  Catches sign/index errors in A^T lam, B^T lam, Hessian-vector products.

The golden fixtures hold the reference's constants, at which Model::az = (Jy - Jx) / Jz and the goal-attitude weight wqf
are zero; the *_generic tests repeat both comparisons at generic_params.GENERIC on seeded random points against the
oracle given the same parameters (same bounds), where every az term and every wqf branch of model.hpp contributes.
The oracle at those parameters is held to the autograd restatement by test_oracle_matches_the_restatement_generic."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from generic_params import GENERIC
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "model_host.cpp")
LIB = os.path.join(HERE, "native", "libmodel_host.so")


@pytest.fixture(scope="module")
def host():
    deps = [SRC, os.path.join(REPO, "learningagileflight_se3_amd", "csrc", "model.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I" + os.path.join(REPO, "include"),
                               "-I" + os.path.join(REPO, "learningagileflight_se3_amd", "csrc"),
                               "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    pd = ctypes.POINTER(ctypes.c_double)
    L.model_host_eval.argtypes = [ctypes.c_int] + [pd] * 10
    L.model_host_cost.argtypes = [ctypes.c_int] + [pd] * 9
    L.model_host_eval_p.argtypes = [ctypes.c_void_p, ctypes.c_int] + [pd] * 10
    L.model_host_cost_p.argtypes = [ctypes.c_void_p, ctypes.c_int] + [pd] * 9
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_device_jacobians_and_transposes(host, golden):
    g = golden("model")
    n = g["x"].shape[0]
    x, u, lam = [np.ascontiguousarray(g[k]) for k in ("x", "u", "lam")]
    f = np.zeros((n, 13)); A = np.zeros((n, 13, 13)); B = np.zeros((n, 13, 4))
    At = np.zeros((n, 13, 13)); Bt = np.zeros((n, 4, 13)); Hl = np.zeros((n, 13, 13)); qu = np.zeros((n, 4))
    host.model_host_eval(n, _p(x), _p(u), _p(lam), _p(f), _p(A), _p(B), _p(At), _p(Bt), _p(Hl), _p(qu))
    rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))
    assert rel(f, g["f"]) < 1e-13
    assert rel(A, g["A"]) < 1e-13                       # A v
    assert rel(At, np.swapaxes(g["A"], 1, 2)) < 1e-13   # A^T l
    assert rel(B, g["B"]) < 1e-13
    assert rel(Bt, np.swapaxes(g["B"], 1, 2)) < 1e-13
    # lambda-Hessian of f_d: x-x block and q-u coupling (same for every rotor)
    assert rel(Hl, g["Hxx"]) < 1e-13
    assert rel(np.repeat(qu[:, :, None], 4, axis=2), g["Hxu"][:, 6:10, :]) < 1e-13
    assert np.max(np.abs(g["Hxu"][:, [0, 1, 2, 3, 4, 5, 10, 11, 12], :])) == 0.0


def test_device_cost_derivatives(host, golden):
    g = golden("costs")
    n = g["x"].shape[0]
    x = np.ascontiguousarray(g["x"]); goal = np.ascontiguousarray(g["goal"]); ptra = np.ascontiguousarray(g["ptra"])
    qtra = np.ascontiguousarray(g["qtra"]); wk = np.ascontiguousarray(g["wk"])
    path = np.zeros(n); tra = np.zeros(n); grad = np.zeros((n, 13)); hess = np.zeros((n, 13, 13))
    host.model_host_cost(n, _p(x), _p(goal), _p(ptra), _p(qtra), _p(wk), _p(path), _p(tra), _p(grad), _p(hess))
    rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))
    assert rel(path, g["path"]) < 1e-13
    assert rel(tra, g["tra"]) < 1e-11
    assert rel(grad, g["grad"]) < 1e-11
    assert rel(hess, g["hess"]) < 1e-11


def _generic():
    """(lafse3_params block, oracle parameter block) of the generic set."""
    from learningagileflight_se3_amd._lib import Params
    p = Params()
    for k, v in GENERIC.fields().items():
        setattr(p, k, v)
    return p, O.default_params(**GENERIC.fields())


def _random_points(n, seed):
    """States with unit quaternions, rates and controls across (and beyond) the generic boxes, multipliers of the
    size the solver meets (up to 1e3), unit traversal quaternions, stage weights up to tra_w_peak."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5, 5, (n, 13))
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    x[:, 10:13] = rng.uniform(-1.5, 1.5, (n, 3))
    u = rng.uniform(0.0, 2.4, (n, 4))
    lam = rng.uniform(-1e3, 1e3, (n, 13))
    goal, ptra = rng.uniform(-10, 10, (n, 3)), rng.uniform(-10, 10, (n, 3))
    qtra = rng.normal(size=(n, 4))
    qtra /= np.linalg.norm(qtra, axis=1, keepdims=True)
    wk = rng.uniform(0, 50, n)
    wk[::7] = 0.0            # the wk == 0 branch of state_cost (stage N, far from the traversal)
    return x, u, lam, goal, ptra, qtra, wk


def test_device_jacobians_and_transposes_generic(host):
    n = 257
    x, u, lam, *_ = _random_points(n, 950)
    p, op = _generic()
    f = np.zeros((n, 13)); A = np.zeros((n, 13, 13)); B = np.zeros((n, 13, 4))
    At = np.zeros((n, 13, 13)); Bt = np.zeros((n, 4, 13)); Hl = np.zeros((n, 13, 13)); qu = np.zeros((n, 4))
    host.model_host_eval_p(ctypes.addressof(p), n, _p(x), _p(u), _p(lam), _p(f), _p(A), _p(B), _p(At), _p(Bt), _p(Hl),
                           _p(qu))
    rf, rA, rB, rHxx, rHxu = O.model_eval(x, u, lam, params=op)
    assert np.max(np.abs(rA[:, 12, 10])) > 1e-3 and np.max(np.abs(rHxx[:, 10, 11])) > 1.0   # the az terms are there
    rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))
    assert rel(f, rf) < 1e-13
    assert rel(A, rA) < 1e-13
    assert rel(At, np.swapaxes(rA, 1, 2)) < 1e-13
    assert rel(B, rB) < 1e-13
    assert rel(Bt, np.swapaxes(rB, 1, 2)) < 1e-13
    assert rel(Hl, rHxx) < 1e-13
    assert rel(np.repeat(qu[:, :, None], 4, axis=2), rHxu[:, 6:10, :]) < 1e-13
    assert np.max(np.abs(rHxu[:, [0, 1, 2, 3, 4, 5, 10, 11, 12], :])) == 0.0


def test_device_cost_derivatives_generic(host):
    n = 257
    x, _, _, goal, ptra, qtra, wk = _random_points(n, 951)
    p, op = _generic()
    path = np.zeros(n); tra = np.zeros(n); grad = np.zeros((n, 13)); hess = np.zeros((n, 13, 13))
    host.model_host_cost_p(ctypes.addressof(p), n, _p(x), _p(goal), _p(ptra), _p(qtra), _p(wk), _p(path), _p(tra),
                           _p(grad), _p(hess))
    rpath, rtra, rgrad, rhess = O.cost_eval(x, goal, ptra, qtra, wk, params=op)
    # the goal-attitude term is in all of it: the same call at wqf = 0 differs
    p0 = O.default_params(**{**GENERIC.fields(), "wqf": 0.0})
    zpath, _, zgrad, zhess = O.cost_eval(x, goal, ptra, qtra, wk, params=p0)
    assert np.max(np.abs(rpath - zpath)) > 1.0 and np.max(np.abs(rgrad - zgrad)) > 1.0
    assert np.max(np.abs(rhess - zhess)) > 1.0
    rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))
    assert rel(path, rpath) < 1e-13
    assert rel(tra, rtra) < 1e-11
    assert rel(grad, rgrad) < 1e-11
    assert rel(hess, rhess) < 1e-11


def test_oracle_matches_the_restatement_generic():
    """The yardstick of the two tests above at the generic set: the oracle's f, A, B and cost gradient against
    tests/kkt.py (torch autograd of the restated NLP, no code shared), 1e-11 relative."""
    torch = pytest.importorskip("torch")
    import kkt
    G = GENERIC
    n = 16
    x, u, lam, goal, ptra, qtra, wk = _random_points(n, 952)
    _, op = _generic()
    rf, rA, rB, _, _ = O.model_eval(x, u, lam, params=op)
    rpath, rtra, rgrad, _ = O.cost_eval(x, goal, ptra, qtra, wk, params=op)
    X, U = torch.tensor(x), torch.tensor(u)
    rel = lambda a, b: np.max(np.abs(a - b) / (1 + np.abs(b)))
    # the oracle's model_eval returns the continuous f and the Jacobians of the discrete map x + dt f
    fd = lambda xx, uu: xx + G.dt * kkt._f(xx, uu, G)
    for i in range(n):
        Ai, Bi = torch.autograd.functional.jacobian(fd, (X[i], U[i]))
        assert rel(rf[i], kkt._f(X[i], U[i], G).numpy()) < 1e-11, i
        assert rel(rA[i], Ai.numpy()) < 1e-11 and rel(rB[i], Bi.numpy()) < 1e-11, i

        def stage_cost(xx):
            # one stage of objective_and_defects' state cost with weight wk: two equal rows, N = 1, no controls' part
            Rx = kkt._dcm(xx[6:10])
            tau = 3 - (kkt._dcm(torch.tensor(qtra[i])) * Rx).sum()
            tr = G.wrt * ((xx[0:3] - torch.tensor(ptra[i])) ** 2).sum() + G.wqt * tau ** 2
            pa = (G.wrf * ((xx[0:3] - torch.tensor(goal[i])) ** 2).sum() + G.wvf * (xx[3:6] ** 2).sum()
                  + G.wwf * (xx[10:13] ** 2).sum() + G.wqf * (3 - Rx[0, 0] - Rx[1, 1] - Rx[2, 2]))
            return wk[i] * tr + pa
        gi = torch.autograd.functional.jacobian(stage_cost, X[i])
        assert rel(rgrad[i], gi.numpy()) < 1e-11, i
