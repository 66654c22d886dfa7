"""The stage-parallel passes around the Newton step on the device (ipm_kernel.hip: compute_errors, eval_merit,
direction_stats, frac_to_bound, accept_step and the merit carried from an accepted trial into the next iteration)
against the independent reference of tests/globalisation.py, at the kernel's own dumped iterates.

Run on an MI355X:  python -m pytest tests/test_gpu_globalisation.py -m gpu -q -s

Cases, coverage and what is left out of the accepted-point comparison are those of test_globalisation_host.py, decided
on the oracle alone and asserted before the device is looked at (globalisation.coverage).  Per case two launches of at
most four instances, max_iter k + 1 and k + 2, dump iterations k and k + 1 after refinement.  Asserted:

  - rows 0..k of the two launches' traces are bit-equal (the iterate of k + 1 is compared with the step that made it),
    the stages beyond the horizon keep newton_cases.SENTINEL in both records, no launch enters a restoration phase;
  - the device takes the oracle's mu, delta_w, verdict and number of halvings (newton_gpu.decisions less the filter
    size) at iterations 0..k + 1 of every case: what is left out was decided from the oracle's traces, so it holds
    for the device only on the oracle's path.  The filter size is not among them: it does not bear on where the next
    iterate lies, and at N = 1 the defect is linear in x_1, so theta after a full step is rounding noise (5.8e-17 on
    the oracle's strict build, 4.9e-19 on its FMA build at default N = 1 sample 1 iteration 3) and the switching
    condition that decides the filter entry compares against it;
  - trace words 1..6, 14, 15 of iteration k at the dumped point of k and words 2, 3, 14, 15 of iteration k + 1 at the
    dumped point of k + 1 with the mu of k + 1 (the carried merit), each within newton_gpu.MARGIN (10) times the
    larger of the two oracle builds' largest error on the same group (computed here on the CPU); where both builds
    are exact or their figure is below it, within the counted floor (globalisation.FLOOR_ROUNDINGS,
    Reference.theta_floor): no bound is below the roundings of the shortest way to compute the word;
  - alpha_z and the accepted duals z + alpha_z dz on the same rule, their errors relative to the cancellation scale
    |mu / s| + |z| + |z d / s| of dz;
  - x + alpha dx, u + alpha du, lam + alpha (lam+ - lam) within two spacings of doubles at the largest magnitude among
    the operands and the result (globalisation.ulps; test_globalisation_host.py says why not at the result alone);
  - a clamped dual within three roundings of its bound (idle: no case clamps, see test_globalisation_host.py).

First run (MI355X), largest error per word and group, device / larger of the oracle's two builds (theta+ .. logsum+ are
the words of iteration k + 1, z the accepted duals; x, u, lam in spacings: the device fuses x + alpha dx); the device
takes the oracle's step decisions in every case:

    default  N=1                 N=2                 N=3                 N=50                
    E0       2.3e-17 / 1.7e-18   2.3e-14 / 2.0e-14   3.1e-14 / 5.1e-14   3.8e-13 / 1.3e-13
    theta    1.0e-15 / 1.3e-16   1.9e-15 / 3.6e-16   8.3e-16 / 2.7e-15   2.2e-14 / 1.9e-14
    phi      2.7e-16 / 2.7e-16   2.2e-16 / 2.2e-16   4.4e-16 / 4.4e-16   3.5e-16 / 8.9e-16
    gBD      5.7e-17 / 1.4e-16   7.2e-17 / 1.3e-16   1.0e-15 / 4.1e-16   3.4e-16 / 1.4e-15
    amax     0 / 0               0 / 0               4.1e-17 / 4.4e-17   6.0e-17 / 6.6e-17
    az       0 / 5.7e-17         0 / 5.4e-17         4.0e-17 / 5.0e-17   1.1e-16 / 5.6e-17
    J        2.7e-16 / 2.7e-16   2.0e-16 / 2.7e-16   3.7e-16 / 2.6e-16   3.3e-16 / 8.0e-16
    logsum   2.4e-16 / 1.2e-16   1.9e-16 / 1.9e-16   3.2e-16 / 5.0e-16   5.3e-16 / 5.8e-15
    theta+   1.0e-15 / 0         1.2e-15 / 8.5e-16   1.9e-15 / 2.6e-15   2.2e-14 / 2.0e-14
    phi+     2.6e-16 / 2.6e-16   4.3e-16 / 3.5e-16   4.4e-16 / 4.1e-16   2.4e-16 / 6.1e-16
    J+       2.6e-16 / 2.6e-16   4.0e-16 / 3.3e-16   3.8e-16 / 4.7e-16   2.2e-16 / 6.2e-16
    logsum+  1.1e-16 / 1.1e-16   1.9e-16 / 2.0e-16   3.2e-16 / 5.2e-16   6.4e-16 / 5.8e-15
    z        1.5e-16 / 1.3e-16   1.6e-16 / 1.7e-16   2.1e-16 / 1.6e-16   1.6e-16 / 2.3e-16
    x        0.46 / 0.50         0.50 / 0.50         0.50 / 0.88         0.50 / 0.99
    u        0.50 / 0.50         0.50 / 0.50         0.50 / 0.68         0.50 / 0.54
    lam      1.00 / 0.50         1.00 / 1.00         1.00 / 1.00         1.47 / 1.97

    generic  N=1                 N=2                 N=3                 N=50                
    E0       0 / 3.9e-17         2.2e-14 / 9.8e-15   2.1e-14 / 4.5e-14   6.4e-15 / 5.3e-15
    theta    7.6e-16 / 6.3e-16   7.4e-16 / 1.2e-15   6.6e-16 / 1.2e-15   5.0e-15 / 1.0e-14
    phi      2.0e-16 / 2.0e-16   4.1e-16 / 4.0e-16   4.3e-16 / 4.3e-16   2.3e-16 / 4.5e-16
    gBD      2.0e-16 / 2.0e-16   1.5e-16 / 1.5e-16   3.7e-15 / 2.9e-15   1.8e-16 / 1.6e-15
    amax     0 / 0               0 / 0               7.4e-17 / 7.4e-17   6.0e-17 / 5.6e-17
    az       0 / 0               5.2e-17 / 5.2e-17   3.7e-17 / 7.5e-17   5.5e-17 / 4.0e-17
    J        2.0e-16 / 2.0e-16   3.8e-16 / 2.8e-16   4.0e-16 / 4.0e-16   2.3e-16 / 4.9e-16
    logsum   2.3e-16 / 1.7e-16   3.7e-16 / 2.7e-16   2.6e-16 / 3.9e-16   3.8e-16 / 3.3e-15
    theta+   7.6e-16 / 8.8e-16   6.4e-16 / 1.2e-15   5.9e-16 / 1.4e-15   8.4e-15 / 2.2e-14
    phi+     2.2e-16 / 2.2e-16   4.1e-16 / 2.8e-16   2.9e-16 / 4.3e-16   3.4e-16 / 6.4e-16
    J+       2.2e-16 / 2.2e-16   3.8e-16 / 2.8e-16   2.7e-16 / 4.0e-16   3.5e-16 / 5.9e-16
    logsum+  2.3e-16 / 3.0e-16   1.8e-16 / 2.7e-16   3.4e-16 / 6.7e-16   4.3e-16 / 1.1e-15
    z        1.6e-16 / 1.6e-16   1.5e-16 / 1.6e-16   1.5e-16 / 1.5e-16   1.7e-16 / 2.2e-16
    x        0.50 / 0.50         0.50 / 0.50         0.50 / 0.68         0.50 / 1.00
    u        0.45 / 0.50         0.50 / 0.50         0.50 / 0.72         0.50 / 0.70
    lam      1.00 / 1.00         1.00 / 1.00         1.00 / 1.00         1.00 / 1.00

Mutation check (builds not kept, each run once on this file, test_gpu_parity.py and test_gpu_options.py; "existing"
counts the failures of those two files without test_native_library_is_the_hip_build, which only notices that another
library file was loaded):

  ph0 of a carried merit formed with the mu of the iteration that accepted the trial: all 8 tests here fail (phi of the
      mu-decrease cases and phi+ before one, up to 2.3e-3 against bounds of 4e-15 .. 9e-15; at N = 1, 2 the step
      decisions leave the oracle's first); existing 8 of 26 fail (test_shorter_horizon and seven option cases).
  the k1 < N guard of compute_errors dropped: all 8 fail, already on the bit-equality of the two launches' traces at
      iteration 0 (E0 then holds whatever lies behind the last multiplier and u); existing 22 of 26 fail.
  the kappa_sigma clamp of accept_step taken on the old slacks: all 8 pass, and so do the existing 26.  No iteration of
      any of the 64 samples clamps a dual (test_globalisation_host.py), so the mutation changes no number anywhere in
      the suite: the clamp's active branch is not covered.
  dzu of direction_stats with the sign of its last term flipped: all 8 fail (alpha_z of iteration 0 off by 0.06 .. 0.09
      where the decisions still hold, the step decisions elsewhere); existing 16 of 26 fail.
  J and the log sum of an accepted second-order correction not carried (the first trial's kept): the two N = 50 tests
      fail (phi+, J+, logsum+ of default sample 14 k = 40 off by 3e-4 .. 2e-3, of generic sample 26 k = 0 by 0.2 ..
      0.6), the six short-horizon ones pass (no correction there); existing 4 of 26 fail.
  the last stage's multipliers dropped from the sum behind s_d in compute_errors: 6 of 8 fail (E0 off by 1e-5 .. 2e-2;
      at N = 1 the dropped stage is the only one, both sums stay below s_max and the two tests pass); existing 0 of 26
      fail: before this file nothing in those two noticed.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/globalisation.py needs it

import globalisation as G  # noqa: E402
import newton_cases as NC  # noqa: E402
from newton_gpu import MARGIN, decisions, gpu_run  # noqa: E402

pytestmark = pytest.mark.gpu
STEP_DECISIONS = [0, 1, 2, 4]      # of newton_gpu.decisions: mu, delta_w, accepted, number of halvings


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def device_run(prob, N, k, after_refine, idx):
    rec, tr, resto = gpu_run(prob, N, k, after_refine, idx)
    assert resto == 0, (N, k, idx, "restoration phase entered")
    return rec, tr, resto


@pytest.mark.parametrize("pset,N", G.groups())
def test_device_passes_match_the_reference(batch, pset, N):
    G.coverage(batch)
    g = G.group(batch, pset, N)
    figs = G.oracle_figures(batch, pset, N)
    odata = figs[0][1]
    bound = G.bounds(MARGIN, [f[3] for f in figs])
    data = NC.collect_pairs(device_run, g["prob"], N, g["cases"])
    assert set(data) == set(g["cases"])
    for (s, k), d in data.items():
        assert np.array_equal(d["first"], d["trace"][:k + 1]), (pset, N, s, k, "the two launches part before k + 1")
        assert np.all(d["pad"] == NC.SENTINEL), (pset, N, s, k, "padding beyond the horizon written")
        for side in ("step", "point", "next_step", "next_point"):
            for f, a in d[side].items():
                assert np.all(np.isfinite(a)) and not np.any(a == NC.SENTINEL), (pset, N, s, k, side, f)
        dg, do = (decisions(t[None])[:, :, STEP_DECISIONS] for t in (d["trace"], odata[(s, k)]["trace"]))
        assert np.array_equal(dg, do), (pset, N, s, k, "the device leaves the oracle's decisions",
                                        np.argwhere(dg != do)[0].tolist())
    errs = G.measure(g["prob"], N, data, g["left"])
    big = G.largest(errs)
    obig = {w: max(f[3][w] for f in figs if w in f[3]) for w in big if any(w in f[3] for f in figs)}
    print(G.table_row(f"{pset} N={N} device:", big))
    print(G.table_row(f"{pset} N={N} oracle:", obig))
    print(G.table_row(f"{pset} N={N} bound: ", bound))
    bad = [(c, w, e[w], bound[w]) for c, e in errs.items() for w in e
           if not w.startswith("floor:") and not e[w] <= bound[w]]
    assert not bad, (pset, N, bad)
