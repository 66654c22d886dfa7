"""The oracle's Newton step in the dense, independent system of tests/newton.py (no GPU).

The step `orc_debug_dump` records (before and after iterative refinement) is put into the dense KKT system built by
torch autograd at the dumped point: this validates tests/newton.py and oracle/lafse3_oracle.c against each other
before the HIP kernel is held to the same system (test_gpu_newton.py), on the same cases (newton_cases.py).

Measured (oracle, parity build; largest residual ratio over the cases of a horizon):

    N     cases   unrefined   refined
    50    20      1.628e-10   1.815e-11
    1     12      2.887e-16   5.170e-17
    2     12      2.017e-16   2.017e-16
    3     12      4.136e-16   3.441e-16
    7     12      7.226e-16   3.163e-16

Inertia: 68 cases, delta_w == 0 on 54, > 0 on 14, none left out as numerically singular.  No dumped iteration lies in
a restoration phase.

Least-squares multiplier initialisation, deviation from the dense value (newton_cases.lam_deviation):
    N = 50: 0 (both sides return exactly 0: the least-squares value exceeds 1e3), N = 3: 3.650e-16, N = 7: 2.903e-15

Every test runs a second time at the generic parameter set (generic_params.py: Jx != Jy, wqf != 0, asymmetric boxes,
other dt, mass, weights), same samples, same assertions, the dense system built from the same parameters.  Measured:

    N     cases   unrefined   refined
    50    20      5.414e-11   1.452e-11
    1     12      5.545e-17   4.308e-17
    2     12      2.890e-16   1.454e-16
    3     12      3.197e-15   3.737e-16
    7     12      1.887e-16   1.712e-16

Inertia: 68 cases, delta_w == 0 on 54, > 0 on 14, none left out; no dumped iteration in a restoration phase.
Least-squares multipliers: N = 50: 0 (cut at 1e3 again), N = 3: 4.767e-16, N = 7: 2.755e-15.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import generic_params as GP  # noqa: E402
import newton  # noqa: E402
import newton_cases as NC  # noqa: E402

OTHER_SETS = tuple(n for n in GP.SETS if n != "default")   # the tests below keep their names at the default set

_cache = {}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def horizon(batch, N, pset="default"):
    if (pset, N) not in _cache:
        prob = GP.problem(batch, N, NC.SAMPLES, pset)
        full = NC.oracle_full(prob, N)
        cases = NC.collect(NC.oracle_run, prob, N, full["iters"])
        _cache[(pset, N)] = (prob, full, cases)
    return _cache[(pset, N)]


def test_dense_system_is_self_consistent(batch, pset="default"):
    """The dense solve of K(delta) [d; lam+] = -b has a residual ratio at rounding level and, perturbed in one entry
    by 1e-6 relative, one far above it: residual_ratio measures what it says.  The entry is du[1, 2] at the default
    set; at another set it is the largest du entry, under the same 1e-6 relative rule (at the generic set du[1, 2] is
    -1.7e-3 beside a step of 5e3, and 1e-6 of it moves the ratio to 1.4e-12 only: that entry cannot show the property
    there)."""
    prob, _, cases = horizon(batch, 3, pset)
    (s, k), c = next(iter(cases.items()))
    ns = NC.system("oracle/" + pset, prob, 3, s, k, c)
    sol = np.linalg.solve(ns.K(0.5), -ns.b)
    step = {"dx": np.concatenate([np.zeros((1, 13)), sol[:39].reshape(3, 13)]), "du": sol[39:51].reshape(3, 4),
            "lamp": sol[51:].reshape(3, 13)}
    assert ns.residual_ratio(step, 0.5) < 1e-14
    entry = (1, 2) if pset == "default" else np.unravel_index(np.argmax(np.abs(step["du"])), step["du"].shape)
    step["du"][entry] *= 1.0 + 1e-6
    assert ns.residual_ratio(step, 0.5) > 1e-10
    assert ns.neg_eigs(0.5)[0] == ns.m


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_oracle_step_solves_the_dense_system(batch, N, pset="default"):
    prob, full, cases = horizon(batch, N, pset)
    assert np.all(full["status"] <= 1), full["status"]
    for (s, k), c in cases.items():
        assert np.all(c["trace"][:k + 1, 0] > 0.0), (N, s, k, "a dumped iteration lies in a restoration phase")
    r = NC.ratios("oracle/" + pset, prob, N, cases)
    pre = max(v[0] for v in r.values())
    post = max(v[1] for v in r.values())
    print(f"{pset} N={N}: {len(r)} cases, largest residual ratio unrefined {pre:.3e}, refined {post:.3e}")
    # IPOPT's residual_ratio_singular: above it the step would not count as a solution of the system at all
    assert post <= 1e-5 and pre <= 1e-5, r
    # refinement stops at 1e-10 (residual_ratio_max) or when it no longer improves: the oracle's own figure (trace
    # words 12, 13) and the dense one measure the same residual
    for (s, k), (a, b) in r.items():
        assert b <= max(1e-10, 10 * a), (N, s, k, a, b)
        own = cases[(s, k)]["trace"][k, 12]
        assert a <= 10 * own + 1e-15 and own <= 10 * a + 1e-15, (N, s, k, a, own)


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_oracle_dump_structure(batch, N, pset="default"):
    prob, _, cases = horizon(batch, N, pset)
    NC.structure(prob, N, cases)


def test_oracle_inertia_verdicts(batch, pset="default"):
    """delta_w == 0 exactly where K(0) has 13 N negative eigenvalues, K(delta_w) has them where delta_w > 0 and the
    retry before the accepted one does not; both verdicts occur among the cases; at most 10 % of the cases are left
    out as numerically singular."""
    total = left = zero = pos = 0
    for N in NC.HORIZONS:
        prob, _, cases = horizon(batch, N, pset)
        n, l = NC.inertia("oracle/" + pset, prob, N, cases)
        total, left = total + n, left + l
        dws = np.array([c["trace"][k, 8] for (s, k), c in cases.items()])
        zero, pos = zero + int(np.sum(dws == 0)), pos + int(np.sum(dws > 0))
    print(f"{pset} inertia: {total} cases, delta_w == 0 on {zero}, > 0 on {pos}, left out {left}")
    assert zero > 0 and pos > 0
    assert left <= 0.1 * total


@pytest.mark.parametrize("N", (50, 3, 7))
def test_oracle_lsq_multipliers(batch, N, pset="default"):
    """A max_iter = 0 solve returns the least-squares initial multipliers (status 2, no iteration), unscaled.  At
    N = 50 the least-squares value exceeds 1e3 on all four samples (3e3 .. 7e3), so both sides must return exactly 0
    (IPOPT's constr_mult_init_max); N = 3 and N = 7 compare the values themselves."""
    from oracle import oracle as O
    prob = GP.problem(batch, N, NC.SAMPLES, pset)
    prm = NC._prm(prob["prm"])
    r = O.solve(prob["ini"], prob["goal"], prob["p"], prob["q"], prob["t"], ulast=prob["ulast"],
                params=NC.oracle_params(prob["prm"], horizon=N, max_iter=0))
    assert np.all(r["status"] == 2) and np.all(r["iters"] == 0)
    devs = []
    for s in range(len(NC.SAMPLES)):
        ul = prob["ulast"][s] if np.any(prob["ulast"][s]) else None
        ns = newton.NewtonSystem(newton.initial_point(prob["ini"][s], N, prm), 0.1, prob["ini"][s], prob["goal"][s],
                                 prob["p"][s], prob["q"][s], prob["t"][s], ul, N, prm)
        dense = ns.lsq_multipliers() / ns.s_obj
        assert np.any(dense != 0.0) == (N != 50)
        devs.append(NC.lam_deviation(r["lam"][s], dense))
    print(f"{pset} N={N}: least-squares multipliers, oracle deviation from the dense value {max(devs):.3e}")
    # both are backward-stable solves of one well-conditioned system (identity (1,1) block, full-rank Jc)
    assert max(devs) <= 1e-10, devs


# The same five tests, same assertions, at every other named parameter set (generic_params.SETS).
@pytest.mark.parametrize("pset", OTHER_SETS)
def test_set_dense_system_is_self_consistent(batch, pset):
    test_dense_system_is_self_consistent(batch, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", NC.HORIZONS)
def test_set_oracle_step_solves_the_dense_system(batch, N, pset):
    test_oracle_step_solves_the_dense_system(batch, N, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", NC.HORIZONS)
def test_set_oracle_dump_structure(batch, N, pset):
    test_oracle_dump_structure(batch, N, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
def test_set_oracle_inertia_verdicts(batch, pset):
    test_oracle_inertia_verdicts(batch, pset)


@pytest.mark.parametrize("pset", OTHER_SETS)
@pytest.mark.parametrize("N", (50, 3, 7))
def test_set_oracle_lsq_multipliers(batch, N, pset):
    test_oracle_lsq_multipliers(batch, N, pset)
