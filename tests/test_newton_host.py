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
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import newton  # noqa: E402
import newton_cases as NC  # noqa: E402

_cache = {}


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def horizon(batch, N):
    if N not in _cache:
        prob = NC.problem(batch, N)
        full = NC.oracle_full(prob, N)
        cases = NC.collect(NC.oracle_run, prob, N, full["iters"])
        _cache[N] = (prob, full, cases)
    return _cache[N]


def test_dense_system_is_self_consistent(batch):
    """The dense solve of K(delta) [d; lam+] = -b has a residual ratio at rounding level and, perturbed in one entry
    by 1e-6 relative, one far above it: residual_ratio measures what it says."""
    prob, _, cases = horizon(batch, 3)
    (s, k), c = next(iter(cases.items()))
    ns = NC.system("oracle", prob, 3, s, k, c)
    sol = np.linalg.solve(ns.K(0.5), -ns.b)
    step = {"dx": np.concatenate([np.zeros((1, 13)), sol[:39].reshape(3, 13)]), "du": sol[39:51].reshape(3, 4),
            "lamp": sol[51:].reshape(3, 13)}
    assert ns.residual_ratio(step, 0.5) < 1e-14
    step["du"][1, 2] *= 1.0 + 1e-6
    assert ns.residual_ratio(step, 0.5) > 1e-10
    assert ns.neg_eigs(0.5)[0] == ns.m


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_oracle_step_solves_the_dense_system(batch, N):
    prob, full, cases = horizon(batch, N)
    assert np.all(full["status"] <= 1), full["status"]
    for (s, k), c in cases.items():
        assert np.all(c["trace"][:k + 1, 0] > 0.0), (N, s, k, "a dumped iteration lies in a restoration phase")
    r = NC.ratios("oracle", prob, N, cases)
    pre = max(v[0] for v in r.values())
    post = max(v[1] for v in r.values())
    print(f"N={N}: {len(r)} cases, largest residual ratio unrefined {pre:.3e}, refined {post:.3e}")
    # IPOPT's residual_ratio_singular: above it the step would not count as a solution of the system at all
    assert post <= 1e-5 and pre <= 1e-5, r
    # refinement stops at 1e-10 (residual_ratio_max) or when it no longer improves: the oracle's own figure (trace
    # words 12, 13) and the dense one measure the same residual
    for (s, k), (a, b) in r.items():
        assert b <= max(1e-10, 10 * a), (N, s, k, a, b)
        own = cases[(s, k)]["trace"][k, 12]
        assert a <= 10 * own + 1e-15 and own <= 10 * a + 1e-15, (N, s, k, a, own)


@pytest.mark.parametrize("N", NC.HORIZONS)
def test_oracle_dump_structure(batch, N):
    prob, _, cases = horizon(batch, N)
    NC.structure(prob, N, cases)


def test_oracle_inertia_verdicts(batch):
    """delta_w == 0 exactly where K(0) has 13 N negative eigenvalues, K(delta_w) has them where delta_w > 0 and the
    retry before the accepted one does not; both verdicts occur among the cases; at most 10 % of the cases are left
    out as numerically singular."""
    total = left = zero = pos = 0
    for N in NC.HORIZONS:
        prob, _, cases = horizon(batch, N)
        n, l = NC.inertia("oracle", prob, N, cases)
        total, left = total + n, left + l
        dws = np.array([c["trace"][k, 8] for (s, k), c in cases.items()])
        zero, pos = zero + int(np.sum(dws == 0)), pos + int(np.sum(dws > 0))
    print(f"inertia: {total} cases, delta_w == 0 on {zero}, > 0 on {pos}, left out {left}")
    assert zero > 0 and pos > 0
    assert left <= 0.1 * total


@pytest.mark.parametrize("N", (50, 3, 7))
def test_oracle_lsq_multipliers(batch, N):
    """A max_iter = 0 solve returns the least-squares initial multipliers (status 2, no iteration), unscaled.  At
    N = 50 the least-squares value exceeds 1e3 on all four samples (3e3 .. 7e3), so both sides must return exactly 0
    (IPOPT's constr_mult_init_max); N = 3 and N = 7 compare the values themselves."""
    from oracle import oracle as O
    prob = NC.problem(batch, N)
    r = O.solve(prob["ini"], prob["goal"], prob["p"], prob["q"], prob["t"], ulast=prob["ulast"],
                params=O.default_params(horizon=N, max_iter=0))
    assert np.all(r["status"] == 2) and np.all(r["iters"] == 0)
    devs = []
    for s in range(len(NC.SAMPLES)):
        ul = prob["ulast"][s] if np.any(prob["ulast"][s]) else None
        ns = newton.NewtonSystem(newton.initial_point(prob["ini"][s], N), 0.1, prob["ini"][s], prob["goal"][s],
                                 prob["p"][s], prob["q"][s], prob["t"][s], ul, N)
        dense = ns.lsq_multipliers() / ns.s_obj
        assert np.any(dense != 0.0) == (N != 50)
        devs.append(NC.lam_deviation(r["lam"][s], dense))
    print(f"N={N}: least-squares multipliers, oracle deviation from the dense value {max(devs):.3e}")
    # both are backward-stable solves of one well-conditioned system (identity (1,1) block, full-rank Jc)
    assert max(devs) <= 1e-10, devs
