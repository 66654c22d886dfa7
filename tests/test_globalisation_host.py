"""The oracle's line-search passes against the independent reference of tests/globalisation.py (no GPU).

The error measure, the merit pair, the directional derivative, the fraction-to-the-boundary steps and the accepted
iterate that the oracle records (debug trace, debug dump) are compared with what the reference computes from the dumped
iterate and step: this validates tests/globalisation.py and oracle/lafse3_oracle.c against each other, and it yields
the yardstick figures the HIP kernel is held to on the same cases (test_gpu_globalisation.py: its margin times the
larger of the two builds' figures).  Both builds of the oracle run: the strict one and the -O3 / FMA one.

Cases (globalisation.KS, EXTRA): scenario.synthetic_batch(64, seed=2025), both sets of generic_params.SETS, horizons 1,
2, 3 and 50, samples 0..3 at iterations 0, 1, 3 (and 7 at N = 3), launches of four samples; at N = 50 four more
(sample, iteration) pairs per set, found on the oracle's traces of all 64 samples.  Per case the iterations k and k + 1
are dumped after refinement.  Compared: trace words 1..6, 14, 15 of iteration k at the dumped point of k; words 2, 3,
14, 15 of iteration k + 1 at the dumped point of k + 1 with the mu of k + 1; the dumped point of k + 1 against
x + alpha d, lam + alpha (lam+ - lam), z + alpha_z dz with the kappa_sigma clamp, for the traced alpha and alpha_z.

Coverage, asserted from the oracle's traces before anything is compared (the test prints every case of a label):
    iteration 0, iteration 1           every group
    first iteration after a decrease of mu   default N=1 sample 0 k=1 and 28 more (every horizon of both sets)
    step halving (alpha < alpha_max)   default N=50 sample 35 k=27, generic N=50 sample 11 k=45
    delta_w > 0                        N=50, iterations 1 and 3 of samples 0..3 and the later ones (18 cases)
    alpha_z < 1                        56 cases
    accepted second-order correction   default N=50 sample 14 k=40, generic N=50 sample 26 k=0
    last three iterations, N=50        default sample 2 k=36, generic sample 2 k=46 and sample 11 k=45
    kappa_sigma clamp moving a dual    none: clamp_search went through every iteration of all 64 samples under both
                                       sets at the four horizons and found no dual on a bound of
                                       [mu / (1e10 s'), 1e10 mu / s'] (z s / mu stays within [5e-7, 6e3]), so the
                                       clamp's active branch stays uncovered; the comparison of a clamped dual is
                                       written (globalisation.measure) and idle, and test_no_iteration_clamps_a_dual
                                       repeats the search where it is cheap
The short horizons take no halving, no correction and no delta_w > 0 on any of the 64 samples under either set.

Left out of the accepted-point comparison, decided from the traces alone (globalisation.classify): the iterations whose
next iterate is not x + alpha d along the dumped direction.  Those are accepted second-order corrections (the first row
at which the trace differs from the max_soc = 0 solve's, when alpha or the verdict differs there; a case must lie at or
before that row, later rows cannot be told), soft-restoration steps (alpha_z equal to alpha below 1 and alpha_max),
iterations the line search rejects (a restoration phase follows; it writes no row), and the watchdog's returns to its
stored point, whose trace words are the stored point's: a case at or next to one is refused outright.  Among the
chosen cases only the two corrections are left out (1 of 16 in each N = 50 group; at most a quarter is allowed).  On a
correction iteration word 6 (alpha_z) belongs to the corrected direction and is not compared; every other word of every
case is.

Errors are relative to 1 + |reference|; grad phi . d relative to sum |g_i d_i|; alpha_z divided by scale / |dz| of its
binding dual; the accepted duals relative to |mu / s| + |z| + |z d / s|; x, u, lam in spacings of doubles at the
largest magnitude among the operands and the result.  (Spacings at the result alone are no bound on two separate
roundings: the strict build is 451 spacings off in lam and 50 in x at N = 50, where lam + alpha (lam+ - lam) and
x + alpha dx cancel.)

Largest error per word and group, strict build / FMA build (first run; theta+ .. logsum+ are the words of iteration
k + 1, z the accepted duals; x, u, lam in spacings):

    default  N=1                 N=2                 N=3                 N=50                
    E0       1.7e-18 / 1.7e-18   2.0e-14 / 1.1e-14   5.1e-14 / 3.4e-14   9.6e-15 / 1.3e-13
    theta    1.3e-16 / 1.3e-16   2.8e-16 / 3.6e-16   2.7e-15 / 1.2e-15   1.9e-14 / 9.0e-15
    phi      2.0e-16 / 2.6e-16   2.1e-16 / 2.2e-16   2.9e-16 / 4.4e-16   6.4e-16 / 8.9e-16
    gBD      1.4e-16 / 7.2e-17   1.4e-16 / 1.4e-16   4.1e-16 / 4.1e-16   1.4e-15 / 1.2e-15
    amax     0 / 0               0 / 0               4.4e-17 / 4.1e-17   6.6e-17 / 6.6e-17
    az       5.6e-17 / 5.6e-17   0 / 5.4e-17         4.0e-17 / 5.0e-17   5.6e-17 / 5.6e-17
    J        2.0e-16 / 2.6e-16   2.0e-16 / 2.7e-16   2.3e-16 / 2.6e-16   6.0e-16 / 8.0e-16
    logsum   1.2e-16 / 9.7e-17   1.0e-16 / 1.9e-16   3.3e-16 / 5.0e-16   5.8e-15 / 5.8e-15
    theta+   0 / 0               2.8e-16 / 8.4e-16   2.6e-15 / 2.6e-15   7.9e-15 / 2.0e-14
    phi+     1.9e-16 / 2.6e-16   2.3e-16 / 3.5e-16   3.3e-16 / 4.1e-16   6.1e-16 / 6.1e-16
    J+       1.9e-16 / 2.6e-16   2.7e-16 / 3.3e-16   2.9e-16 / 4.7e-16   5.9e-16 / 6.1e-16
    logsum+  1.1e-16 / 9.7e-17   2.0e-16 / 1.9e-16   3.5e-16 / 5.3e-16   5.8e-15 / 5.8e-15
    z        9.8e-17 / 1.3e-16   1.7e-16 / 1.4e-16   1.6e-16 / 1.6e-16   2.3e-16 / 1.6e-16
    x        0.45 / 0.50         0.50 / 0.50         0.87 / 0.50         0.99 / 0.50
    u        0.50 / 0.38         0.50 / 0.47         0.68 / 0.49         0.54 / 0.50
    lam      0.50 / 0.50         1.00 / 1.00         1.00 / 1.00         1.97 / 1.46

    generic  N=1                 N=2                 N=3                 N=50                
    E0       3.9e-17 / 3.4e-18   8.4e-15 / 9.8e-15   4.5e-14 / 4.4e-14   5.3e-15 / 4.1e-15
    theta    2.1e-16 / 6.3e-16   1.1e-15 / 1.2e-15   1.2e-15 / 9.6e-16   1.0e-14 / 5.7e-15
    phi      2.0e-16 / 2.0e-16   2.1e-16 / 4.0e-16   2.1e-16 / 4.3e-16   4.5e-16 / 3.7e-16
    gBD      1.1e-16 / 2.0e-16   1.5e-16 / 1.5e-16   2.9e-15 / 2.9e-15   1.6e-15 / 1.6e-15
    amax     0 / 0               0 / 0               7.4e-17 / 7.4e-17   5.6e-17 / 3.9e-17
    az       0 / 0               5.2e-17 / 0         7.5e-17 / 3.9e-17   3.9e-17 / 4.1e-17
    J        2.0e-16 / 2.0e-16   2.1e-16 / 2.8e-16   2.1e-16 / 4.0e-16   4.9e-16 / 3.7e-16
    logsum   1.7e-16 / 9.9e-17   1.2e-16 / 2.8e-16   3.9e-16 / 3.9e-16   3.3e-15 / 3.3e-15
    theta+   4.9e-16 / 8.8e-16   1.2e-15 / 1.2e-15   1.2e-15 / 1.4e-15   9.2e-15 / 2.2e-14
    phi+     2.0e-16 / 2.2e-16   2.1e-16 / 2.8e-16   3.0e-16 / 4.3e-16   6.4e-16 / 4.6e-16
    J+       2.0e-16 / 2.2e-16   1.9e-16 / 2.8e-16   3.0e-16 / 4.0e-16   5.9e-16 / 5.3e-16
    logsum+  2.1e-16 / 3.0e-16   2.8e-16 / 1.8e-16   6.7e-16 / 6.7e-16   1.1e-15 / 1.1e-15
    z        1.6e-16 / 1.6e-16   1.6e-16 / 1.4e-16   1.5e-16 / 1.4e-16   2.2e-16 / 1.9e-16
    x        0.50 / 0.38         0.50 / 0.50         0.68 / 0.50         1.00 / 0.50
    u        0.50 / 0.50         0.50 / 0.50         0.72 / 0.50         0.70 / 0.50
    lam      1.00 / 1.00         1.00 / 1.00         1.00 / 0.75         1.00 / 1.00

What the oracle itself must meet (it is the yardstick, so its own bound comes from the formats): every model-based word
within ORACLE_WORD = 1e-11 (the oracle's and the reference's model code are separate evaluations in double of sums
whose terms reach 1e3 to 1e4 beside a result of order 1, so a dozen digits is what agreement of two correct codes
guarantees, and a wrong term, lane, mu or sign is of the order of the word itself); alpha_max, alpha_z and the accepted
duals, which need no model, within their counted floors times 10; x, u, lam within two spacings.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/globalisation.py needs it

import globalisation as G  # noqa: E402
import newton_cases as NC  # noqa: E402

ORACLE_WORD = 1e-11


@pytest.fixture(scope="module")
def batch():
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


def test_cases_cover_the_line_search(batch):
    found = G.coverage(batch)
    for lab, where in found.items():
        print(f"{lab}: {len(where)} cases: " + ", ".join(f"{p} N={N} sample {s} k={k}" for p, N, s, k in where))
    for pset, N in G.groups():
        g = G.group(batch, pset, N)
        print(f"{pset} N={N}: {len(g['cases'])} cases, left out of the accepted-point comparison {len(g['left'])}: "
              f"{g['left']}")
        assert len(g["left"]) <= G.MAX_LEFT_OUT * len(g["cases"])
        assert all(why == "second-order correction" for why in g["left"].values()), g["left"]


@pytest.mark.parametrize("pset,N", G.groups())
def test_oracle_matches_the_reference(batch, pset, N):
    G.coverage(batch)
    g = G.group(batch, pset, N)
    for name, data, errs, big in G.oracle_figures(batch, pset, N):
        print(G.table_row(f"{pset} N={N} {name}:", big))
        assert set(errs) == set(g["cases"])
        for c, e in errs.items():
            assert set(G.WORDS_K) - {"az"} <= set(e) and set(G.WORDS_K1) <= set(e), (c, sorted(e))
            assert ("az" in e) == (g["left"].get(c) != "second-order correction"), c
            assert ("x" in e) == (c not in g["left"]), c
            for w in G.WORDS_K + G.WORDS_K1:
                if w in ("amax", "az") or w not in e:
                    continue
                assert e[w] <= ORACLE_WORD, (pset, N, name, c, w, e[w])
            assert e["amax"] <= 10 * G.FLOOR_ROUNDINGS["amax"] * G.EPS, (pset, N, name, c, e["amax"])
            if "az" in e:
                assert e["az"] <= 10 * G.FLOOR_ROUNDINGS["az"] * G.EPS, (pset, N, name, c, e["az"])
            if c not in g["left"]:
                assert e["z"] <= 10 * G.FLOOR_ROUNDINGS["z"] * G.EPS, (pset, N, name, c, e["z"])
                for w in ("x", "u", "lam"):
                    assert e[w] <= G.ULP_BOUND, (pset, N, name, c, w, e[w])
                if "clamped" in e:
                    assert e["clamped"] <= G.CLAMP_ROUNDINGS * G.EPS, (pset, N, name, c, e["clamped"])
        for c, d in data.items():
            assert np.all(d["pad"] == NC.SENTINEL), (pset, N, name, c, "padding beyond the horizon written")
            assert np.array_equal(d["first"], d["trace"][:c[1] + 1]), (pset, N, name, c, "the two launches part")


def test_reference_tells_a_wrong_pass(batch):
    """The reference separates what the device test is to catch: each of a carried phi with the previous mu, swapped
    lo and hi in dz, a clamp on the old slack (with a dual outside its bounds) and a dropped defect entry moves its
    figure by orders of magnitude more than the oracle's error."""
    g = G.group(batch, "generic", 3)
    name, data, errs, big = G.oracle_figures(batch, "generic", 3)[0]
    c = data[(0, 7)]
    t, prob = c["trace"], g["prob"]
    assert t[7, G.MU] < t[6, G.MU]
    R = G.reference(prob, 0, 3, c["point"], c["step"], t[7, G.MU])
    old = G.reference(prob, 0, 3, c["point"], c["step"], t[6, G.MU])
    assert G.rel(old.merit()["phi"], R.merit()["phi"]) > 1e6 * big["phi"]
    dz = R.dual_steps()["u"]
    mu, (sl, su), (zl, zu), d = G.LD(R.mu), R.slacks()["u"], R.duals()["u"], R.bounded_step()["u"]
    swapped = mu / su - zu - zu / su * d          # the sign of the last term as in the lower dual's step
    assert np.max(np.abs(swapped - dz[1]) / dz[3]) > 1e6 * max(big["z"], G.EPS)
    # a dual far above its upper clamp: the clamp must use the slack of the new point
    pt = {k: v.copy() for k, v in c["point"].items()}
    pt["zLu"][0, 0] = 1e12 * t[7, G.MU] / float(sl[0, 0])
    Rc = G.reference(prob, 0, 3, pt, c["step"], t[7, G.MU])
    new, moved, _ = Rc.accepted_point(t[7, G.ALPHA], 0.0)      # alpha_z = 0: the dual stays where it was put
    assert moved["zLu"][0, 0] and moved["zLu"].sum() == 1
    s_new = new["u"][0, 0] - G.LD(Rc.u_lo)
    assert abs(float(new["zLu"][0, 0] * s_new / (G.LD(1e10) * G.LD(Rc.mu))) - 1.0) < 4 * G.EPS
    s_old = Rc.slacks()["u"][0][0, 0]
    assert abs(float(s_old / s_new) - 1.0) > 1e-3, "the step does not move this slack: the case cannot tell the slacks"


def clamp_search(batch, pset, N, samples):
    """Iterations of the oracle's solves (strict build) whose kappa_sigma clamp moved a dual, and the range of
    z s / mu met.  A dual the clamp moved sits on its bound, z' s' = 1e10 mu or mu / 1e10 with s' the slack of the
    iterate it was stored with and mu the barrier parameter of the iteration that stored it, whatever direction that
    iteration took (a corrected one included): the search looks for such a product within 1e-6 relative in the dump
    of every iteration k >= 1."""
    hits, lo, hi = [], np.inf, 0.0
    prob = G.group(batch, pset, N)["prob"]
    res, tr = G.oracle_traces(prob, N)
    for k in range(1, int(res["iters"][list(samples)].max())):
        idx = [s for s in samples if k < res["iters"][s] and tr[s, k, G.MU] > 0 and tr[s, k - 1, G.MU] > 0]
        if not idx:
            continue
        rec, _, _ = NC.oracle_run(prob, N, k, 1, idx)
        for j, s in enumerate(idx):
            _, point, _ = G.newton.split_record(rec[j], N)
            R = G.Reference(point, None, tr[s, k - 1, G.MU], None, None, None, None, 0.0, None, N,
                            NC._prm(prob.get("prm")), s_obj=1.0)
            sl, z = R.slacks(), R.duals()
            r = np.concatenate([np.ravel(sl[b][i] * z[b][i]) for b in ("u", "w") for i in (0, 1)]) / R.mu
            lo, hi = min(lo, float(r.min())), max(hi, float(r.max()))
            if np.any(np.abs(r / G.KAPPA_SIGMA - 1) < 1e-6) or np.any(np.abs(r * G.KAPPA_SIGMA - 1) < 1e-6):
                hits.append((pset, N, s, k - 1))
    return hits, lo, hi


@pytest.mark.parametrize("pset", list(G.GP.SETS))
def test_no_iteration_clamps_a_dual(batch, pset):
    """No iteration's clamp moves a dual: all 64 samples at N = 1, 2, 3, and at N = 50 the samples the cases use (the
    search is quadratic in the iteration count).  All 64 samples at N = 50, clamp_search(batch, pset, 50, range(64)),
    were searched when the cases were chosen: z s / mu after every accepted step lies in [1.5e-06, 3.6e+03] at the
    default set and in [5.2e-07, 6.2e+03] at the generic one, nowhere near 1e-10 or 1e10.  Should a clamped iteration
    appear (this test then fails), it belongs in globalisation.EXTRA."""
    hits, lo, hi = [], np.inf, 0.0
    for N in G.HORIZONS:
        samples = range(G.BATCH) if N < 50 else sorted({s for s, _ in G.cases_of(pset, N)})
        h, a, b = clamp_search(batch, pset, N, samples)
        hits, lo, hi = hits + h, min(lo, a), max(hi, b)
    print(f"{pset}: z s / mu after every accepted step lies in [{lo:.3e}, {hi:.3e}]; iterations whose clamp moved a "
          f"dual: {hits}")
    assert not hits, hits
