"""The first step of the iterative refinement in the HIP kernel, kept and reverted, at the horizons at which the
stage-parallel passes that carry it change shape.

linear_solve copies the solution to a backup in the workspace ahead of a refinement sweep; costates_identity, the
sweep's last pass, adds that backup to the sweep's correction (lane l: lam+ and du of stage l, dx of stage l + 1; dx
of stage 0 stays 0), and a step that does not lower the residual ratio is copied back from the backup (lane = stage;
dx stages 0..N, lam+ and du stages 0..N-1).  At
N = 1, 2, 3 the x-row block of the residual is empty or one lane wide and the terminal lane sits next to lane 0; at
N = 50 the terminal lane is the last stage of the SoA stride.

Every case is one (sample, iteration) of a solve: the Newton step of that iteration is dumped before and after the
refinement in two launches of the same inputs with max_iter = k + 1, as test_gpu_chain_horizons.py does, and the
trace gives ratios[0] (word 12, the unrefined step's residual ratio) and ratios[1] (word 13, after the first
refinement step).  IPOPT's rule decides from them alone what happened:

    ratios[1] >= ratios[0]            the first step was reverted: the refined dump must equal the unrefined one bit
                                      for bit, and nothing beyond the horizon is written
    ratios[1] <  ratios[0]            the step was kept: the dumps differ, and the refined one solves the dense system
                                      of tests/newton.py within test_gpu_newton.py's bound (<= 1e-5, and at most MARGIN
                                      times the oracle's largest ratio on the same cases)
    ... and ratios[1] > 1e-10         a second step followed (the loop stops at ratio <= 1e-10)

The cases are chosen on the CPU from the oracle's trace of scenario.synthetic_batch(64, seed=2025), the oracle
following the same rule: per horizon and kind the first PER cases in (iteration, sample) order (see PER).  Where the 64 samples
show no reverted step, the 256-sample batch of the same seed is searched instead.  What the oracle shows (EXPECT):
reverted and kept steps at every horizon (at N = 1 reverted ones only among the 256; at N = 50 reverted ones only at
iteration 0); a second refinement step at no horizon (the first one always brings the ratio below 1e-10).  The
GPU's residuals differ from the oracle's in their rounding, and at the short horizons the ratios are rounding noise
(1e-19 .. 1e-16), so a case the oracle reverts may be kept on the GPU and the reverse: each case is judged by the
GPU's own ratios, and the test asserts that both outcomes ran at N = 1, 2 and 3.  At N = 50 the GPU keeps every
step the oracle reverts (all at iteration 0) and reverts other samples' there: test_reverted_step_at_n50 takes its
cases from the GPU's own trace of the same 64 samples.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import newton  # noqa: E402
import newton_cases as NC  # noqa: E402
from newton_gpu import MARGIN, gpu_run  # noqa: E402

HORIZONS = (1, 2, 3, 50)
KINDS = ("reverted", "kept", "several")
# cases per horizon and kind.  Reverted steps are the rare ones on the GPU (a ratio that rounding noise alone moves
# decides them), so more of the oracle's are tried; of the kept ones the first and the first of iteration 3 or later
PER = {"reverted": 6, "kept": 2, "several": 2}
# cases the oracle's trace yields per horizon: (samples searched, {kind: cases})
EXPECT = {1: (256, {"reverted": 6, "kept": 2, "several": 0}),
          2: (64, {"reverted": 6, "kept": 1, "several": 0}),
          3: (64, {"reverted": 6, "kept": 2, "several": 0}),
          50: (64, {"reverted": 6, "kept": 2, "several": 0})}
_chosen = {}
_cache = {}
_ran = {}


def kind(r0, r1):
    """What IPOPT's rule did with the first refinement step, from the two residual ratios."""
    if r1 >= r0:
        return "reverted"
    return "several" if r1 > 1e-10 else "kept"


def problem(batch, N, idx):
    """NC.problem's recipe on the samples `idx` of `batch`."""
    from oracle import oracle as O
    i = np.asarray(idx)
    d = batch["dnn_out"][i].astype(np.float64)
    ul = np.zeros((len(i), 4))
    ul[i % 2 == 1] = 1.0
    t = d[:, 6].copy() if N == 50 else np.full(len(i), 0.5 * N * NC.DT)
    return {"ini": batch["ini"][i], "goal": batch["goal"][i], "p": d[:, :3], "a": d[:, 3:6],
            "q": np.stack([O.rd2quat(a) for a in d[:, 3:6]]), "t": t, "ulast": ul}


def choose(N):
    """(samples searched, problem of the chosen samples, {kind: [(position in the problem, iteration)]}) from the
    oracle's trace of the full solves."""
    if N in _chosen:
        return _chosen[N]
    from learningagileflight_se3_amd import scenario as S
    from oracle import oracle as O
    for B in (64, 256):
        batch = S.synthetic_batch(B, seed=2025)
        prob = problem(batch, N, range(B))
        iters = NC.oracle_full(prob, N)["iters"]
        tr = np.zeros((B, int(iters.max()), 16))
        O.debug_trace(tr, tr.shape[1])
        try:
            NC.oracle_full(prob, N)
        finally:
            O.debug_trace(None, 0)
        found = {kd: [] for kd in KINDS}
        for k in range(int(iters.max()) - 1):
            for s in range(B):
                if k <= int(iters[s]) - 2 and tr[s, k, 0] > 0.0:
                    found[kind(tr[s, k, 12], tr[s, k, 13])].append((s, k))
        if found["reverted"] or B == 256:
            break
    picked = {kd: found[kd][:PER[kd]] for kd in KINDS}
    late = [c for c in found["kept"] if c[1] >= 3]
    picked["kept"] = found["kept"][:1] + (late[:1] if late else found["kept"][1:2])
    samples = sorted({s for v in picked.values() for s, _ in v})
    pos = {s: j for j, s in enumerate(samples)}
    _chosen[N] = (B, problem(batch, N, samples), {kd: [(pos[s], k) for s, k in v] for kd, v in picked.items()})
    return _chosen[N]


def collect(run, prob, N, wanted):
    """NC.collect on the chosen (position, iteration) cases: one launch per (iteration, side)."""
    cases = {}
    for k in sorted({k for _, k in wanted}):
        idx = sorted({s for s, kk in wanted if kk == k})
        side = [run(prob, N, k, ar, idx) for ar in (0, 1)]
        for j, s in enumerate(idx):
            pre, pt0, pad0 = newton.split_record(side[0][0][j], N)
            post, pt1, pad1 = newton.split_record(side[1][0][j], N)
            for f in pt0:   # the iterate does not change between the two dump points
                assert np.array_equal(pt0[f], pt1[f]), (N, s, k, f)
            assert np.array_equal(side[0][1][j], side[1][1][j]), (N, s, k, "trace of the two launches")
            cases[(s, k)] = {"pre": pre, "post": post, "point": pt0, "pad": np.concatenate([pad0, pad1]),
                             "trace": side[1][1][j], "resto": [side[0][2], side[1][2]]}
    return cases


def horizon(N):
    if N not in _cache:
        _, prob, picked = choose(N)
        wanted = sorted({c for v in picked.values() for c in v})
        _cache[N] = (prob, collect(NC.oracle_run, prob, N, wanted), collect(gpu_run, prob, N, wanted))
    return _cache[N]


@pytest.mark.parametrize("N", HORIZONS)
def test_oracle_shows_the_kinds(N):
    """The selection is not empty: the oracle's trace yields the cases of EXPECT, and its own dumps follow the rule."""
    B, prob, picked = choose(N)
    assert (B, {kd: len(v) for kd, v in picked.items()}) == EXPECT[N]
    ocases = collect(NC.oracle_run, prob, N, sorted({c for v in picked.values() for c in v}))
    for kd, v in picked.items():
        for s, k in v:
            c = ocases[(s, k)]
            assert kind(c["trace"][k, 12], c["trace"][k, 13]) == kd, (N, s, k)
            same = all(np.array_equal(c["pre"][f].view(np.int64), c["post"][f].view(np.int64)) for f in c["pre"])
            assert same == (kd == "reverted"), (N, s, k, kd)
            assert np.all(c["pad"] == NC.SENTINEL), (N, s, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", HORIZONS)
def test_first_refinement_step(N):
    """A reverted first step leaves the unrefined step bit for bit and nothing beyond the horizon; a kept one changes
    it and solves the dense system within test_gpu_newton.py's bound."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    prob, ocases, gcases = horizon(N)
    assert set(ocases) == set(gcases) and len(gcases) == sum(EXPECT[N][1].values())
    ran = {kd: [] for kd in KINDS}
    for (s, k), c in sorted(gcases.items()):
        assert c["resto"] == [0, 0], (N, s, k, "restoration phase entered")
        assert np.all(c["trace"][:k + 1, 0] > 0.0), (N, s, k)
        r0, r1 = c["trace"][k, 12], c["trace"][k, 13]
        assert r0 >= 0.0 and r1 >= 0.0, (N, s, k, r0, r1, "no refinement step taken")
        o = ocases[(s, k)]["trace"][k]
        kd = kind(r0, r1)
        ran[kd].append((s, k))
        print(f"N={N} case {(s, k)}: ratios GPU {r0:.3e} -> {r1:.3e} ({kd}), oracle {o[12]:.3e} -> {o[13]:.3e} "
              f"({kind(o[12], o[13])})")
        assert np.all(c["pad"] == NC.SENTINEL), (N, s, k, "padding beyond the horizon written")
        for side in ("pre", "post"):
            assert np.all(c[side]["dx"][0] == 0.0), (N, s, k, side, "dx at stage 0")
            for f in c[side]:
                assert np.all(np.isfinite(c[side][f])) and not np.any(c[side][f] == NC.SENTINEL), (N, s, k, side, f)
        same = all(np.array_equal(c["pre"][f], c["post"][f]) for f in c["pre"])
        if kd == "reverted":
            for f in c["pre"]:
                assert np.array_equal(c["pre"][f].view(np.int64), c["post"][f].view(np.int64)), (N, s, k, f)
        else:
            assert not same, (N, s, k, "a kept refinement step left the step unchanged")
    _ran[N] = {kd: len(v) for kd, v in ran.items()}
    print(f"N={N}: cases run by kind {_ran[N]}")
    assert sum(_ran[N].values()) == len(gcases)
    # both outcomes at every horizon, by the GPU's own ratios: a kept step is what puts the add through the dense
    # system's bound (a wrong add that made the residual worse would be reverted and pass as such), a reverted one is
    # what runs the copy back.  The kernel is deterministic, so these counts do not move from run to run.  At N = 50
    # the GPU keeps every case the oracle's trace yields; its own reverted steps are test_reverted_step_at_n50's.
    assert _ran[N]["kept"] + _ran[N]["several"] >= 1, (N, _ran[N])
    if N != 50:
        assert _ran[N]["reverted"] >= 1, (N, _ran[N])
    kept = {c: gcases[c] for kd in ("kept", "several") for c in ran[kd]}
    if kept:
        g = NC.ratios("gpu-refine", prob, N, kept)
        o = NC.ratios("oracle-refine", prob, N, {c: ocases[c] for c in kept})
        gpost, opost = max(v[1] for v in g.values()), max(v[1] for v in o.values())
        print(f"N={N}: {len(kept)} kept steps, largest refined residual ratio GPU {gpost:.3e} oracle {opost:.3e}")
        assert all(v[1] <= 1e-5 for v in g.values()), g           # IPOPT's residual_ratio_singular
        assert gpost <= MARGIN * opost, (gpost, opost)


@pytest.mark.gpu
def test_reverted_step_at_n50():
    """The copy back at the full horizon, where the terminal lane is lane 50 and the SoA stride has no padding.  None
    of the oracle-chosen cases is reverted by the GPU at N = 50, so the cases here are the GPU's own: iteration 0 of
    the 64 seed-2025 samples in one launch (refined dump, trace), the first samples whose ratios[1] >= ratios[0]
    again with the unrefined dump.  The two dumps must agree bit for bit."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    N = 50
    prob = problem(S.synthetic_batch(64, seed=2025), N, range(64))
    post, tr, resto = gpu_run(prob, N, 0, 1, range(64))
    assert resto == 0
    rev = [s for s in range(64) if tr[s, 0, 0] > 0.0 and kind(tr[s, 0, 12], tr[s, 0, 13]) == "reverted"]
    print(f"N=50, iteration 0: the GPU reverts the first refinement step on {len(rev)} of 64 samples: {rev}")
    assert len(rev) >= 1, "no reverted step at N = 50 among the 64 samples"
    rev = rev[:4]
    pre, tr0, _ = gpu_run(prob, N, 0, 0, rev)
    for j, s in enumerate(rev):
        assert np.array_equal(tr0[j], tr[s]), (s, "trace of the two launches")
        a, pa, pad_a = newton.split_record(pre[j], N)
        b, pb, pad_b = newton.split_record(post[s], N)
        for f in pa:
            assert np.array_equal(pa[f], pb[f]), (s, f)
        for f in a:
            assert np.all(np.isfinite(a[f])) and not np.any(a[f] == NC.SENTINEL), (s, f)
            assert np.array_equal(a[f].view(np.int64), b[f].view(np.int64)), (s, f, "reverted step differs")
        assert np.all(a["dx"][0] == 0.0) and np.any(a["dx"][N] != 0.0), s
        assert np.all(pad_a == NC.SENTINEL) and np.all(pad_b == NC.SENTINEL), s


@pytest.mark.gpu
def test_both_outcomes_ran():
    """The counts of all horizons together (every horizon is run here if the parametrised test has not run it in
    this process): the per-horizon assertions are test_first_refinement_step's."""
    for N in HORIZONS:
        if N not in _ran:
            test_first_refinement_step(N)
    total = {kd: sum(_ran[N][kd] for N in HORIZONS) for kd in KINDS}
    print("cases run by kind, all horizons:", total, _ran)
    assert total["reverted"] >= 1 and total["kept"] + total["several"] >= 1, _ran
    assert _ran[50]["kept"] + _ran[50]["several"] >= 1, _ran
