"""The HIP kernel's Newton step (linear_solve: build_table, the f64-MFMA factorisation, the chains, the refinement)
in the dense, independent system of tests/newton.py, built at the kernel's own dumped point.

Cases (newton_cases.py, chosen on the CPU with the oracle, test_newton_host.py): samples 0..3 of
synthetic_batch(64, seed=2025) at N = 50 (iterations 0, 1, 3, 8 and iters - 2) and at N = 1, 2, 3, 7 with
t = 0.5 N dt (iterations 0, 1, 3, clipped below iters - 1); u_last = 1 on the odd samples.  None of the listed cases
lies in a restoration phase and both inertia verdicts occur among them (oracle: delta_w == 0 on 54, > 0 on 14 of 68),
so no sample was replaced.  One launch per (horizon, iteration, side) with max_iter = iteration + 1.

The kernel under test is `ipm_kernel_dump`, the instantiation of run_instance that lafse3_ocp_solve launches while a
dump is armed, not the production `ipm_kernel`: the noinline phases (`linear_solve` with the table build, the MFMA
factorisation, the chains, the residual and the refinement; `direction_stats`, `accept_step`) are one piece of code
common to both kernels; the iteration loop inlined around them is compiled separately for each.

Recorded on the first run (MI355X); "oracle" is the CPU oracle on the same cases, measured in the same test:

    largest residual ratio     unrefined step (item 2)      refined step (item 1)
    N     cases                GPU         oracle           GPU         oracle
    50    20                   7.445e-11   1.628e-10        3.747e-12   1.815e-11
    1     12                   4.455e-16   2.887e-16        5.170e-17   5.170e-17
    2     12                   3.067e-16   2.017e-16        3.067e-16   2.017e-16
    3     12                   3.026e-16   4.136e-16        3.190e-16   3.441e-16
    7     12                   4.779e-16   7.226e-16        2.287e-16   3.163e-16
    inertia (item 3): 68 cases, delta_w == 0 on 54, > 0 on 14, none left out
    least-squares multipliers (item 5), deviation from the dense value, GPU / oracle:
        N = 50: 0 / 0 (cut at 1e3 on every side: N = 50 checks the cut alone, no value; the uncut value is nowhere
        recorded, the dumped lam of iteration 0 is the cut one), N = 3: 3.650e-16 / 3.650e-16, N = 7: 2.903e-15 / 2.903e-15
    point parity (item 6): 65 of 68 cases on the oracle's path, all 40 cases with k <= 1 among them.  The norm is
        per array, relative to its largest entry (at least 1): an entry far below its array's scale, such as a bound dual
        near 1e-9 beside others of order 1, is not resolved by it

The margin of 10 did not have to be raised.  Mutation check (builds not kept): with one mf_gsrc table return swapped
the unrefined-step assertion fails at N = 50, 3 and 7; with delta_w dropped from the u diagonal of the MFMA stage the
refined ratio is 3.7e-2 at N = 50 and 1.0e-2 at N = 7 (the 1e-5 cap fails), while the inertia assertions do not see
it (68 cases, delta_w == 0 on 53, > 0 on 15, all verdicts right): K with delta_w on every diagonal entry has the right
inertia whenever K with delta_w on the x entries alone has, and Quu is positive definite without it (its control
weights are), so no retry is rejected wrongly either.  The same holds with delta_w dropped from the x diagonal (ratio
3.5e+1 at N = 50, the cap fails; inertia assertions pass, 50 / 18).  A mutation that changes a verdict does trip them:
with linear_solve accepting a factorisation whose Quu is not positive definite, test_inertia_verdicts reports
"delta_w == 0 on 68, > 0 on 0, left out 13" and fails both on the missing second verdict and on the 10 % cap (the 13
cases whose K(0) has the wrong eigenvalue count are all numerically singular, ratio below 1e-10: the zero quaternion of
the early iterates; without the cap the leave-out rule would have swallowed them).

The generic parameter set (test_set_*, generic_params.py: Engine(horizon=N, **GENERIC), the dense system built from
the same parameters).  At the reference's constants Jx == Jy makes Model::az zero, and with it the two Jw row-2 slots
of the G table, StageHess::wxy and the az terms of A_times / At_times; wqf == 0 removes the goal-attitude block of the
stage Hessian: every test above factorises systems in which those entries are identically zero, so a slot swapped,
dropped or read from a neighbour passes them.  Same cases, same six checks, same margins.  First run (MI355X):

    largest residual ratio     unrefined step               refined step
    N     cases                GPU         oracle           GPU         oracle
    50    20                   4.700e-11   5.414e-11        8.305e-13   1.452e-11
    1     12                   1.262e-16   5.545e-17        4.308e-17   4.308e-17
    2     12                   2.890e-16   2.890e-16        1.640e-16   1.454e-16
    3     12                   5.445e-15   3.197e-15        3.916e-16   3.737e-16
    7     12                   4.771e-16   1.887e-16        1.441e-16   1.712e-16
    inertia: 68 cases, delta_w == 0 on 54, > 0 on 14, none left out
    least-squares multipliers, GPU / oracle: N = 50: 0 / 0 (cut at 1e3), N = 3: 4.767e-16 / 4.767e-16,
        N = 7: 2.755e-15 / 2.755e-15
    point parity: 63 of 68 cases on the oracle's path, all 40 with k <= 1 among them

Mutation check at this set (builds not kept; each run once on test_gpu_newton.py, test_gpu_parity.py,
test_gpu_generic.py and test_gpu_generic_sens.py).  No test at the default set failed under any of the three: not one
of this file's 16 default cases, none of test_gpu_parity.py's.
  (a) M.az replaced by 0 in riccati.inc's Jw (the G table).  test_set_step_solves_the_dense_system fails at N = 50, 2,
      3 and 7: the unrefined ratio rises to 1.9e-05 at N = 50 (1e-5 cap) and the refined one to 3.7e-11 .. 9.2e-11 at
      N = 2, 3, 7 against the oracle's 1.5e-16 .. 3.7e-16 (MARGIN); N = 1 passes (one stage: no rate has moved yet).
      test_set_lsq_multipliers fails at N = 3 and 7 (deviation 4.3e-06 and 2.5e-06 against 4.8e-16 and 2.8e-15: that
      solve is not refined), test_set_point_parity at iteration 0.  Beyond this file: the solve of sample 0 at N = 50
      ends with status 6, both sol_gradient modes, the PMP costates and all four finite-difference comparisons fail
      (err - 10 e up to 1.4e-01).
  (b) the wqf term removed from the Hxx table (riccati.inc, `M.wqf != 0.0`).  test_set_step_solves_the_dense_system
      fails at all five horizons (unrefined ratio 5.5e-05 at N = 50, 2.1e-03 at N = 1), test_set_point_parity at
      iteration 1; the four finite-difference comparisons of test_gpu_generic_sens.py fail (err - 10 e 5.6e-03 ..
      1.5e-02).  The solve-parity test does not see it: the residual and the refinement read the exact Hessian, so the
      iterates still converge to the same optimum along the same path.
  (c) umid = 0.5 * prm.u_ub in ipm_kernel.hip.  test_set_dump_structure fails at every horizon (iteration 0 is not
      at newton.initial_point's u), test_set_lsq_multipliers at N = 3 and 7 (6.7e-04, 4.6e-04), test_set_point_parity
      at iteration 0; test_gpu_generic.py's iteration-0 NLP inputs (J off by 3.4e-04 relative), solve parity (cost off
      by 1.1e-03 at N = 50) and both sol_gradient modes fail.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import generic_params as GP  # noqa: E402
import newton  # noqa: E402
import newton_cases as NC  # noqa: E402
from newton_gpu import MARGIN, gpu_run, gpu_solve, step_solves_the_dense_system  # noqa: E402

pytestmark = pytest.mark.gpu

OTHER_SETS = tuple(n for n in GP.SETS if n != "default")   # the tests below keep their names at the default set
_cache = {}


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def horizon(batch, N, pset="default"):
    """(problem, oracle cases, GPU cases) of horizon N at the named parameter set; the dumped iterations come from the
    oracle's full solve."""
    if (pset, N) not in _cache:
        prob = GP.problem(batch, N, NC.SAMPLES, pset)
        iters = NC.oracle_full(prob, N)["iters"]
        _cache[(pset, N)] = (prob, NC.collect(NC.oracle_run, prob, N, iters), NC.collect(gpu_run, prob, N, iters))
    return _cache[(pset, N)]


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_step_solves_the_dense_system(batch, N, pset="default"):
    """Items 1 and 2: the refined step has a residual ratio <= 1e-5 in every case, and the largest ratio of the
    refined and of the unrefined steps is at most MARGIN times the oracle's on the same cases."""
    prob, ocases, gcases = horizon(batch, N, pset)
    assert set(ocases) == set(gcases)
    step_solves_the_dense_system(f"{pset} N={N}", "/" + pset, prob, N, ocases, gcases)


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_dump_structure(batch, N, pset="default"):
    """Item 4: dx of stage 0 exactly 0, padding beyond N untouched, iteration 0 at the stated initial point."""
    prob, _, gcases = horizon(batch, N, pset)
    NC.structure(prob, N, gcases)


def test_inertia_verdicts(batch, pset="default"):
    """Item 3: trace delta_w == 0 exactly where the dense K(0) has 13 N negative eigenvalues, and K(delta_w) has them
    where delta_w > 0, and not yet at the retry before the accepted one; both verdicts occur; at most 10 % of the
    cases left out as numerically singular."""
    total = left = zero = pos = 0
    for N in NC.HORIZONS:
        prob, _, gcases = horizon(batch, N, pset)
        n, l = NC.inertia("gpu/" + pset, prob, N, gcases)
        total, left = total + n, left + l
        dws = np.array([c["trace"][k, 8] for (s, k), c in gcases.items()])
        zero, pos = zero + int(np.sum(dws == 0)), pos + int(np.sum(dws > 0))
    print(f"{pset} inertia: {total} cases, delta_w == 0 on {zero}, > 0 on {pos}, left out {left}")
    assert zero > 0 and pos > 0
    assert left <= 0.1 * total


@pytest.mark.parametrize("N", (50, 3, 7))
def test_lsq_multipliers(batch, N, pset="default"):
    """Item 5: a max_iter = 0 solve returns the least-squares initial multipliers (status 2, iters 0); they agree with
    the dense value within MARGIN times the oracle's own deviation.  At N = 50 the value exceeds 1e3 on every sample,
    so all three sides return exactly 0 (constr_mult_init_max); N = 3 and N = 7 compare the values."""
    from oracle import oracle as O
    prob = GP.problem(batch, N, NC.SAMPLES, pset)
    prm = NC._prm(prob["prm"])
    idx = np.arange(len(NC.SAMPLES))
    g = gpu_solve(prob, N, idx, 0)
    r = O.solve(prob["ini"], prob["goal"], prob["p"], prob["q"], prob["t"], ulast=prob["ulast"],
                params=NC.oracle_params(prob["prm"], horizon=N, max_iter=0))
    assert np.all(g["status"] == 2) and np.all(g["iters"] == 0)
    assert g["lam"].shape == (len(idx), N, 13)
    gd, od = [], []
    for s in idx:
        ul = prob["ulast"][s] if np.any(prob["ulast"][s]) else None
        ns = newton.NewtonSystem(newton.initial_point(prob["ini"][s], N, prm), 0.1, prob["ini"][s], prob["goal"][s],
                                 prob["p"][s], prob["q"][s], prob["t"][s], ul, N, prm)
        dense = ns.lsq_multipliers() / ns.s_obj
        assert np.any(dense != 0.0) == (N != 50)
        gd.append(NC.lam_deviation(g["lam"][s], dense))
        od.append(NC.lam_deviation(r["lam"][s], dense))
    print(f"{pset} N={N}: least-squares multipliers, deviation from the dense value GPU {max(gd):.3e} oracle {max(od):.3e}")
    assert max(gd) <= MARGIN * max(od), (gd, od)


def test_point_parity(batch, pset="default"):
    """Item 6: where the GPU and oracle traces agree up to iteration k on alpha, alpha_z (1e-12 relative), delta_w and
    accepted (exactly), the two dumped points agree to 1e-9 relative to each array's largest entry (at least 1)."""
    covered = total = 0
    for N in NC.HORIZONS:
        prob, ocases, gcases = horizon(batch, N, pset)
        for (s, k), gc in gcases.items():
            oc = ocases[(s, k)]
            total += 1
            gt, ot = gc["trace"][:k + 1], oc["trace"][:k + 1]
            same = (np.array_equal(gt[:, [8, 9]], ot[:, [8, 9]]) and
                    np.all(np.abs(gt[:, [6, 7]] - ot[:, [6, 7]]) <= 1e-12 * np.abs(ot[:, [6, 7]])))
            assert same or k > 1, (N, s, k, "traces differ at an iteration <= 1", gt[:, 6:10], ot[:, 6:10])
            if not same:
                continue
            covered += 1
            for f in oc["point"]:
                d = np.max(np.abs(gc["point"][f] - oc["point"][f])) / max(1.0, np.max(np.abs(oc["point"][f])))
                assert d <= 1e-9, (N, s, k, f, d)
    print(f"{pset} point parity: {covered} of {total} cases on the oracle's path")


# The same six checks, same assertions and margins, with Engine(horizon=N, **GENERIC) (generic_params.py): Jx != Jy
# puts non-zero values into the az slots of the G table and into StageHess::wxy, wqf != 0 adds the goal-attitude block
# to the stage Hessian that the MFMA factorisation reads, and the asymmetric boxes move Sigma and the barrier gradient.
@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", NC.HORIZONS)
def test_set_step_solves_the_dense_system(batch, N, pset):
    test_step_solves_the_dense_system(batch, N, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", NC.HORIZONS)
def test_set_dump_structure(batch, N, pset):
    test_dump_structure(batch, N, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
def test_set_inertia_verdicts(batch, pset):
    test_inertia_verdicts(batch, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", (50, 3, 7))
def test_set_lsq_multipliers(batch, N, pset):
    test_lsq_multipliers(batch, N, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
def test_set_point_parity(batch, pset):
    test_point_parity(batch, pset)

