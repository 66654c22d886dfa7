"""One named problem away from the reference's: the "generic" parameter set.

At the reference's constants several pieces of kernel code are dead or multiplied by zero: Jx == Jy makes Model::az
(the omega_x omega_y coupling of the z rate) and with it two G-table slots, StageHess::wxy and a term of A_times /
At_times vanish; wqf == 0 skips every goal-attitude branch; u_lb == 0 and w_lb == -w_ub make the midpoints u_ub / 2
and 0 and the lower relaxation trivial; and dt, mass, arm_l, c_tau, grav, the weights and the traversal-weight shape
enter products that an error could cancel in.  GENERIC moves every one of them (wing_len, d_min and the solver options
stay at their defaults):

    mass 0.6  Jx 0.0021  Jy 0.0029  Jz 0.0043  arm_l 0.30  c_tau 0.03  grav 9.81  dt 0.08
    wrt 4  wqt 60  wthrust 0.15  wrf 6  wvf 4  wqf 2  wwf 2.5
    tra_w_peak 50  tra_w_decay 8  du_weight 0.7
    u_lb 0.1  u_ub 2.2  w_lb -1.2  w_ub 1.4

Problems: scenario.synthetic_batch(64, seed=2025); at N = 50 the traversal time is 0.8 times the sample's own (the
horizon spans 4 s instead of 5), at shorter horizons 0.5 N dt; u_last = 1 on the odd samples and 0 on the even.
"""
from __future__ import annotations

import numpy as np

import kkt
import newton_cases as NC

GENERIC = kkt.Problem(mass=0.6, Jx=0.0021, Jy=0.0029, Jz=0.0043, arm_l=0.30, c_tau=0.03, grav=9.81, dt=0.08,
                      wrt=4.0, wqt=60.0, wthrust=0.15, wrf=6.0, wvf=4.0, wqf=2.0, wwf=2.5,
                      tra_w_peak=50.0, tra_w_decay=8.0, du_weight=0.7,
                      u_lb=0.1, u_ub=2.2, w_lb=-1.2, w_ub=1.4)
T_SCALE = 0.8

# set name -> (kkt.Problem or None for the reference's, scale of the samples' own t at N = 50)
SETS = {"default": (None, 1.0), "generic": (GENERIC, T_SCALE)}


def problem(batch, N, samples, name="generic"):
    """newton_cases.problem for the named set on the given samples."""
    prm, ts = SETS[name]
    return NC.problem(batch, N, prm, ts, samples)


def solve_args(prob, idx=slice(None)):
    """(ini, goal, p, q, t) of a problem, the positional arguments of the oracle's solve and of yardstick's rules."""
    return tuple(np.ascontiguousarray(prob[k][idx]) for k in ("ini", "goal", "p", "q", "t"))
