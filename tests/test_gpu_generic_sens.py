"""lafse3_ocp_sensitivity_ex (csrc/sens.inc) at the generic parameter set (generic_params.py): dt,
mass, arm_l, c_tau, grav, wthrust, du_weight, tra_w_peak and tra_w_decay enter the products dtm, bwx..bwz and dwk of the
sensitivity right-hand sides, and an error that cancels at the reference's constants is invisible to
test_gpu_sens.py / test_gpu_sens_ex.py.  Rules, constants and checking functions are theirs (sens_yardstick.py).

Run on an MI355X:  python -m pytest tests/test_gpu_generic_sens.py -m gpu -q -s

(a) All 23 columns against central differences of the CPU oracle's solve with params = GENERIC at h = 1e-4 and 2h,
horizons 20 and 7 (t = 0.5 N dt, u_last = 1 on the odd samples): the 7 theta columns on 8 samples, the 13 ini_state
and 3 goal columns on the first 4.  Admission (oracle alone): four solves with status <= 1 and e <= 1e-3; bound
err <= 10 e + F, F = 1e-3; at most 15 % of the pairs left out.  Horizon 50 is not compared: the tight boxes of this set
put a third of the entries at a bound and the solution map is kinked there (the oracle admits 72 of 128 ini + goal
pairs), which the 15 % cap does not allow.  Oracle alone, on the CPU:
    horizon 20: theta 51 of 56 pairs admitted, ini + goal 59 of 64;   horizon 7: theta 56 of 56, ini + goal 64 of 64.
First GPU run (sens_status 0 on every instance), largest err - 10 e against the bound F = 1e-3:
    horizon 20: theta 6.253e-05 (sample 7, a_tra[1]: err 8.685e-05, e 2.432e-06; median err 3.857e-06),
                ini + goal 3.000e-06 (sample 2, ini_state[7]; median err 9.144e-07);
    horizon  7: theta 1.896e-05 (sample 1, p_tra[0]; median err 7.164e-07),
                ini + goal 5.158e-06 (sample 2, ini_state[5]; median err 4.359e-07).

(b) The adjoint identity gain == du_0 at horizons 20, 7, 2 and 1 under test_gpu_sens_ex.py's ADJ_BAR (1e-6, never
above 1e-5), 8 samples each.  First GPU run, largest relative difference (always in the ini_state group):
    horizon 20: 2.337e-08;  horizon 7: 5.007e-09;  horizon 2: 6.184e-16;  horizon 1: 1.210e-15.

(c) The theta columns of lafse3_ocp_sensitivity equal those of _ex bit for bit (same launches as (b)).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import generic_params as GP  # noqa: E402
import newton_cases as NC  # noqa: E402
import sens_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = GP.GENERIC
SL3 = {g: Y.SL[g] for g in ("theta", "ini", "goal")}
N_THETA, N_INI = 8, 4
_runs = {}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def gpu_run(batch, horizon):
    """One ocp_sensitivity_ex launch with all three groups on 8 samples of the horizon (shared, never modified)."""
    Y.require_gpu()
    if horizon not in _runs:
        from learningagileflight_se3_amd.engine import Engine
        e = Engine(horizon=horizon, **GENERIC.fields())
        prob = GP.problem(batch, horizon, range(N_THETA))
        args = (prob["ini"], prob["goal"], prob["p"], prob["a"], prob["t"])
        g = Y.to_numpy(e.ocp_sensitivity_ex(*args, u_last=prob["ulast"], want=("x", "u", "dx", "du", "gain")))
        old = Y.to_numpy(e.ocp_sensitivity(*args, u_last=prob["ulast"]))
        torch.cuda.synchronize()
        e.check_device()
        _runs[horizon] = (prob, g, old)
    return _runs[horizon]


def oracle_fd(prob, n, horizon, cols):
    """sens_yardstick.oracle_fd with the oracle at the generic set; u_last is the problem's."""
    return Y.oracle_fd(prob, n, horizon, cols, NC.oracle_params(GENERIC, horizon=horizon))


@pytest.mark.parametrize("horizon", [20, 7])
def test_theta_columns_against_oracle_finite_differences(batch, horizon):
    prob, g, _ = gpu_run(batch, horizon)
    fd = oracle_fd(prob, N_THETA, horizon, range(0, 7))
    assert np.all(g["status"] <= 1) and np.all(g["sens_status"] != 1)
    assert g["dx"].shape == (N_THETA, 23, horizon + 1, 13) and g["du"].shape == (N_THETA, 23, horizon, 4)
    Y.check_against_fd(Y.traj(g["dx"][:, :7], g["du"][:, :7]), g["sens_status"], fd,
                       f"generic set, horizon {horizon}, theta", Y.F)


@pytest.mark.parametrize("horizon", [20, 7])
def test_ini_and_goal_columns_against_oracle_finite_differences(batch, horizon):
    prob, g, _ = gpu_run(batch, horizon)
    n = N_INI
    fd = oracle_fd(prob, n, horizon, range(7, 23))
    label = f"generic set, horizon {horizon}, ini + goal"
    ini, goal = fd["admitted"][:, :13], fd["admitted"][:, 13:]
    print(f"{label}: oracle admits ini {int(ini.sum())} of {ini.size}, goal {int(goal.sum())} of {goal.size}")
    Y.check_against_fd(Y.traj(g["dx"][:n, 7:], g["du"][:n, 7:]), g["sens_status"][:n], fd, label, Y.F)


@pytest.mark.parametrize("horizon", [20, 7, 2, 1])
def test_adjoint_gain_equals_forward_du0(batch, horizon):
    _, g, _ = gpu_run(batch, horizon)
    assert g["gain"].shape == (N_THETA, 4, 23)
    assert np.all(np.isfinite(g["du"])) and np.all(np.isfinite(g["gain"]))
    assert Y.ADJ_BAR <= 1e-5
    assert Y.adjoint_difference(g, f"generic set, horizon {horizon}", SL3, Y.ADJ_BAR) <= Y.ADJ_BAR


@pytest.mark.parametrize("horizon", [20, 7, 2, 1])
def test_theta_columns_of_both_entry_points_are_equal(batch, horizon):
    _, g, old = gpu_run(batch, horizon)
    assert old["dx"].shape == (N_THETA, 7, horizon + 1, 13) and old["du"].shape == (N_THETA, 7, horizon, 4)
    assert np.array_equal(old["sens_status"], g["sens_status"])
    assert np.array_equal(old["x"], g["x"]) and np.array_equal(old["u"], g["u"])
    assert np.array_equal(g["dx"][:, :7], old["dx"]) and np.array_equal(g["du"][:, :7], old["du"])
    live = g["sens_status"] == 0
    assert np.any(g["du"][live][:, :7] != 0.0) or horizon == 1     # horizon 1 has no traversal stage to respond
