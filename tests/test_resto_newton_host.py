"""The oracle's restoration-phase Newton step in the dense, independent system of tests/resto_newton.py (no GPU), and
the restoration phase's exits on the oracle.

The step `orc_debug_dump_resto` records (before and after iterative refinement) is put into the dense primal-dual
system built by torch autograd at the dumped point: this validates tests/resto_newton.py and the oracle's
riccati_resto / kkt_residual_resto against each other before the HIP kernel is held to the same system
(test_gpu_resto_newton.py), on the same cases (resto_newton_cases.py).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/resto_newton.py needs it

import resto_newton as RN  # noqa: E402
import resto_newton_cases as RC  # noqa: E402

_cache = {}
FAMILIES = RC.FAMILIES


def family(N, pset="default"):
    """(problem, uncut solve, cases) of the yaw family on the oracle."""
    if (pset, N) not in _cache:
        prob, dumps = RC.family(pset, N)
        out = RC.oracle_run(prob, N, 0, 0, 0, np.arange(len(dumps)))[2]
        _cache[(pset, N)] = (prob, out, RC.collect(RC.oracle_run, prob, N, RC.ENTRIES[(pset, N)], dumps))
    return _cache[(pset, N)]


def test_dense_system_is_self_consistent():
    """The dense solve of K(delta) step = -b has a residual ratio at rounding level and, perturbed in one entry by
    1e-6 relative, one far above it; K(delta) has 13 N negative eigenvalues."""
    prob, _, cases = family(3)
    c = cases[(0, 2, 1)]
    rs = RC.system("oracle/default", prob, 3, 0, (2, 1), c)
    step = rs.unpack_step(np.linalg.solve(rs.K(0.5), -rs.b))
    assert rs.residual_ratio(step, 0.5) < 1e-14
    e = np.unravel_index(np.argmax(np.abs(step["lamp"])), step["lamp"].shape)   # the right-hand side holds rho = 1000:
    step["lamp"][e] *= 1.0 + 1e-6                                               # only an entry of that size shows
    assert rs.residual_ratio(step, 0.5) > 1e-10
    assert rs.neg_eigs(0.5)[0] == rs.m
    assert RN.d_r2([0.0, 0.5, -4.0]).tolist() == [1.0, 1.0, 0.0625]


@pytest.mark.parametrize("pset,N", FAMILIES)
def test_recorded_entries(pset, N):
    """resto_newton_cases.ENTRIES is what the oracle does: every entry of every yaw solve, the iterations before it
    and inside it; the last entry ends the solve with status 9 and the counts add up to its iteration count."""
    prob, out, _ = family(N, pset)
    assert RC.probe_entries(RC.oracle_run, prob, N) == RC.ENTRIES[(pset, N)]
    assert np.all(out["status"] == 9), out["status"]
    for s, en in enumerate(RC.ENTRIES[(pset, N)]):
        assert out["iters"][s] == en[-1][0] + en[-1][1] and len(en) >= 2, (N, s, out["iters"][s], en)


@pytest.mark.parametrize("pset,N", FAMILIES)
def test_oracle_step_solves_the_dense_system(pset, N):
    prob, out, cases = family(N, pset)
    r = RC.ratios(f"oracle/{pset}", prob, N, cases)
    pre, post = max(v[0] for v in r.values()), max(v[1] for v in r.values())
    print(f"{pset} N={N}: {len(r)} cases, largest residual ratio unrefined {pre:.3e}, refined {post:.3e}")
    assert post <= 1e-5 and pre <= 1e-5, r           # IPOPT's residual_ratio_singular
    for key, (a, b) in r.items():
        assert b <= max(1e-10, 10 * a), (N, key, a, b)
        sc = cases[key]["scal"]      # the oracle's own figures measure the same residuals
        for dense, own in ((a, sc["ratio_pre"]), (b, sc["ratio_post"])):
            assert dense <= 10 * own + 1e-15 and own <= 10 * dense + 1e-15, (N, key, dense, own)


@pytest.mark.parametrize("pset,N", FAMILIES)
def test_oracle_dump_structure(pset, N):
    prob, _, cases = family(N, pset)
    RC.structure(f"oracle/{pset}", prob, N, cases)


def test_oracle_inertia_verdicts():
    total = left = zero = pos = 0
    for pset, N in FAMILIES:
        prob, _, cases = family(N, pset)
        n, l = RC.inertia(f"oracle/{pset}", prob, N, cases)
        total, left = total + n, left + l
        dws = np.array([c["scal"]["delta_w"] for c in cases.values()])
        zero, pos = zero + int(np.sum(dws == 0)), pos + int(np.sum(dws > 0))
    print(f"restoration inertia: {total} cases, delta_w == 0 on {zero}, > 0 on {pos}, left out {left}")
    assert zero > 0 and pos > 0
    assert left <= 0.1 * total


@pytest.mark.parametrize("pset,N", FAMILIES)
def test_oracle_lsq_multipliers(pset, N):
    prob, _, cases = family(N, pset)
    d = RC.lsq_deviation(f"oracle/{pset}", prob, N, cases)
    print(f"{pset} N={N}: least-squares multipliers, oracle deviation from the dense value {d:.3e}")
    assert d <= 1e-10, d


@pytest.mark.parametrize("N", RC.HORIZONS)
def test_oracle_infeasible_exit_holds_the_start_point(N):
    """Status 9: the outputs are the point where the last entry into the phase started (its iteration-0 dump, put
    onto the original bounds as every output is), bit for bit."""
    prob, out, cases = family(N)
    for s, en in enumerate(RC.ENTRIES[("default", N)]):
        x, u = RC.honoured(cases[(s, len(en) - 1, 0)]["point"])
        assert np.array_equal(out["x"][s], x) and np.array_equal(out["u"][s], u), (N, s)


@pytest.mark.parametrize("N", (50, 2))
def test_oracle_iteration_limit_inside_the_phase(N):
    prob = RC.yaw(N, wz=(RC.MAXITER_WZ,))
    en = RC.ENTRIES[("default", N)][RC.YAW.index(RC.MAXITER_WZ)]
    assert en[-1][0] < RC.MAXITER < en[-1][0] + en[-1][1]        # the limit falls inside the last entry
    rec, _, out = RC.oracle_run(prob, N, len(en) - 1, 0, 0, [0], RC.MAXITER)
    x, u = RC.honoured(RN.split_record(rec[0], N)[1])
    assert out["status"][0] == 2 and out["iters"][0] == RC.MAXITER
    assert np.array_equal(out["x"][0], x) and np.array_equal(out["u"][0], u)


def test_roll_pitch_instances_do_not_enter_the_phase():
    """The N = 50 roll / pitch instances are solved (status 0) without an entry into the restoration phase."""
    prob = RC.problem(50, RC.ROLL_PITCH)
    rec, _, out = RC.oracle_run(prob, 50, 0, 0, 0, np.arange(len(RC.ROLL_PITCH)))
    assert np.all(out["status"] == 0) and out["iters"].tolist() == [81, 98, 90], (out["status"], out["iters"])
    assert np.all(rec == RC.SENTINEL)
