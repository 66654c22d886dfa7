"""TEST INFRASTRUCTURE: the rounding yardstick of the iteration-path agreement tests.

The device factorises the same Newton systems as the oracle with another operation order (the MFMA Riccati stage,
riccati_mfma.inc), so device and oracle agree to rounding, and on long, ill-conditioned solves rounding alone
moves IPOPT's near-tie decisions (an inertia correction one factor of kappa apart, a filter entry, one backtracking
halving; tools/resto_diverge.py).  How often it does is measured here on the same jobs with the oracle against
itself: its -O3 / FMA-contraction build (liblafse3_oracle_fast.so, other rounding, same source) against its strict
parity build (liblafse3_oracle.so).  A device test then asks for at least that many exact paths minus 2 % of the
jobs, instead of a fixed fraction that a change of the device's rounding alone could flip.  Reference: IPOPT's
default options at /root/reference/quad_OC.py:170-174.
"""
import numpy as np


def grad_paths(args, status_strict, iters_strict, **kw):
    """sol_gradient jobs (B x 9 solves): how many the FMA build solves with the strict build's status and iteration
    count."""
    from oracle import oracle as O
    ito = np.zeros_like(iters_strict)
    _, _, so = O.sol_gradient(*args, fast=True, iters=ito, **kw)
    return int(((so == status_strict) & (ito == iters_strict)).sum())


def solve_paths(args, kw, ref_strict):
    """ocp solves: how many the FMA build solves with the strict build's status and iteration count."""
    from oracle import oracle as O
    r = O.solve(*args, fast=True, **kw)
    return int(((r["status"] == ref_strict["status"]) & (r["iters"] == ref_strict["iters"])).sum())


def solve_decisions(args, kw, ref_strict):
    """ocp solves: which of them the FMA build solves with the strict build's decisions, iteration by iteration (debug
    trace words mu, delta_w, accepted, filter size and the number of step halvings alpha_max / alpha).  Status and
    iteration count (solve_paths) are a proxy of this: a solve can leave the strict build's decisions and still end
    after as many iterations.  Returns a bool array, True where every decision agrees."""
    from oracle import oracle as O
    B = len(ref_strict["iters"])
    TI = int(np.max(ref_strict["iters"])) + 1
    tr = {}
    for fast in (False, True):
        buf = np.zeros((B, TI, 16))
        O.debug_trace(buf, TI, fast=fast)
        try:
            O.solve(*args, fast=fast, **kw)
        finally:
            O.debug_trace(None, 0, fast=fast)
        tr[fast] = buf
    a, b = tr[False], tr[True]
    with np.errstate(divide="ignore", invalid="ignore"):
        ha = np.where(a[:, :, 7] > 0, np.round(np.log2(a[:, :, 5] / a[:, :, 7])), -1.0)
        hb = np.where(b[:, :, 7] > 0, np.round(np.log2(b[:, :, 5] / b[:, :, 7])), -1.0)
    return np.all(a[:, :, [0, 8, 9, 10]] == b[:, :, [0, 8, 9, 10]], axis=(1, 2)) & np.all(ha == hb, axis=1)
