"""The device reward (`reward_fused`, csrc/ipm_kernel.hip: rotor tips, collis_det against the gate, goal path term)
against the CPU oracle on every branch of collis_det, at horizons 50, 7, 4, 3 and 2.

The trajectories are not solver outputs: a seeded generator (reward_cases.sweep) flies bent lines through, past and short
of randomly sized, pitched and shifted gates with unnormalised random attitudes, so that every one of the nine branch
codes of the oracle (0 = no crossing; per sector plane 1..4 "inside the window" 1, 5, 9, 13 and "at the frame" 2, 6,
10, 14), both outcomes of line.distance, early and late crossing stages, "starts behind" and "never crosses" occur.
That they occur is asserted from what the oracle's scorer reports it decided (`O.reward_detail`), not from geometry
restated here; tests/test_reward_host.py asserts the same coverage without a GPU.

Tolerance: |R_gpu - R_oracle| <= 1e-9 max(1, |R_oracle|), the project's bound for rewards of given trajectories
(test_reward_matches_reference_fixture), relative because frame collisions reach -1.9e4.  No sample is left out.

Coverage of the sweep (rotor results per branch code, B = 256 samples x 4 rotors per horizon; reward_cases.SEED):

    N    code 0    1    5    9   13     2    6   10   14   perp / end   starts behind  never crosses   bit-equal
    50      352   24   34   24   22   107  160  160  141    301 / 267            148            204    215 / 256
     7      356   18   20   21   23   124  140  164  158    294 / 292            151            205    235 / 256
     4      362   19   21   24   24   121  161  148  144    277 / 297            147            215    223 / 256
     3      371   31   26   26   18   157  130  130  135    264 / 288            151            220    231 / 256
     2      389   26   19   24   26   122  144  127  147    258 / 282            155            234    233 / 256

Rewards range from -1.86e4 to 98.7, all finite.  The last column is information, not an assertion: the samples whose
device reward equals the oracle's bit for bit, measured on an MI355X (both sides keep numpy's operation order with
contraction off; the others differ by at most 1.6e-15 of max(1, |R|)).  test_branch_sweep prints it on every run.
Crossing stages 1 and N-1 are guaranteed by the hand-placed samples 0 and 1 of the sweep.

The fused path (test_fused_reward_equals_scoring_launch) uses samples 0..7 of scenario.synthetic_batch(8, seed=11);
all converge with status 0 at both horizons, none had to be replaced, and the fused and the scored rewards were
bit-equal on 8 of 8 at N = 3 and at N = 7.
"""
import numpy as np
import pytest

from reward_cases import HORIZONS, INSIDE, assert_coverage, sweep_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9


# ------------------------------------------------------------------------------------------------ device side
_engines = {}


def engine(N, **prm):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    key = (N, tuple(sorted(prm.items())))
    if key not in _engines:
        from learningagileflight_se3_amd.engine import Engine
        _engines[key] = Engine(horizon=N, **prm)
    return _engines[key]


def gpu_reward(N, x, goal, gate12, **prm):
    # copies: the shared references are read-only, which torch.as_tensor warns about
    import torch
    R = engine(N, **prm).reward(np.array(x), np.array(goal), np.array(gate12))
    torch.cuda.synchronize()
    return R.cpu().numpy()


def assert_close(Rg, Ro, what):
    """|R_gpu - R_oracle| <= 1e-9 max(1, |R_oracle|) on every sample; where the oracle's reward is NaN the device's is."""
    assert Rg.shape == Ro.shape
    assert np.array_equal(np.isnan(Rg), np.isnan(Ro), equal_nan=True), (what, "NaN pattern", Rg, Ro)
    ok = ~np.isnan(Ro)
    err = np.abs(Rg[ok] - Ro[ok]) / np.maximum(1.0, np.abs(Ro[ok]))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: {Rg.size} samples, {int(np.sum(Rg[ok] == Ro[ok]))} bit-equal of {int(ok.sum())} finite, "
          f"largest scaled difference {worst:.3e}")
    assert worst <= RTOL, (what, worst, int(np.argmax(err)))


# ------------------------------------------------------------------------------------------------ a. branch sweep
@pytest.mark.parametrize("N", HORIZONS)
def test_branch_sweep(N):
    s = sweep_ref(N)
    h = assert_coverage(N, s)
    print(f"N={N} coverage {h}; rewards {s['R'].min():.4g} .. {s['R'].max():.4g}")
    assert_close(gpu_reward(N, s["x"], s["goal"], s["gate12"]), s["R"], f"sweep N={N}")


# ------------------------------------------------------------------------------------------------ b. exact edge cases
WING_A = 1.5 * 0.5 / np.sqrt(2.0)      # the tip offset, as the kernel computes it from wing_len = 1.5
GATE_Y0 = np.array([[-0.5, 0, 0.5], [0.5, 0, 0.5], [0.5, 0, -0.5], [-0.5, 0, -0.5]])   # plane y = 0, normal (0, -1, 0)
# identity quaternion: tip r = position + (bx, by, 0), exactly
TIP_OFF = np.array([[WING_A, WING_A, 0], [-WING_A, WING_A, 0], [-WING_A, -WING_A, 0], [WING_A, -WING_A, 0]])


def flat_traj(pos):
    """(N+1, 13) states at positions pos with the identity quaternion and everything else zero."""
    x = np.zeros((pos.shape[0], 13))
    x[:, 0:3] = pos
    x[:, 6] = 1.0
    return x


def score_both(N, x, gate, goal=(0.25, 4.0, -0.5)):
    from oracle import oracle as O
    x, goal, g12 = x[None], np.array([goal], dtype=np.float64), np.asarray(gate, dtype=np.float64).reshape(1, 12)
    Ro, br, cross, ld = O.reward_detail(x, goal, g12, params=O.default_params(horizon=N))
    return gpu_reward(N, x, goal, g12), Ro, br[0], cross[0], ld[0]


@pytest.mark.parametrize("k", (0, 3))
def test_tip_exactly_on_the_plane_is_not_behind(k):
    """Rotors 0 and 1 sit exactly on plane 1 at stage k (y = -a + a = 0) and behind it at k + 1: the crossing stage is
    k + 1.  At k = 0 a `<=` in the side test would read "starts behind" and score no collision at all."""
    N = 7
    s = np.arange(N + 1, dtype=np.float64)
    pos = np.stack([1.0 + 0.125 * s, -WING_A + (s - k) * 0.25, np.full(N + 1, 0.25)], -1)
    assert pos[k, 1] + WING_A == 0.0
    Rg, Ro, br, cross, _ = score_both(N, flat_traj(pos), GATE_Y0)
    assert cross[0] == k + 1 and cross[1] == k + 1, cross
    assert br[0] != 0 and br[1] != 0, br
    assert_close(Rg, Ro, f"tip on the plane at stage {k}")


@pytest.mark.parametrize("N", (50, 7, 2))
def test_behind_only_at_stage_N_is_no_collision(N):
    """The reference loops range(horizon): a track that is behind plane 1 at stage N only never collides, although it
    passes far outside the window (a guard `lane <= N` would score a frame collision for every rotor)."""
    from oracle import oracle as O
    s = np.arange(N + 1, dtype=np.float64)
    pos = np.stack([np.full(N + 1, 4.0), -2.0 - (N - s) * 0.0625, np.zeros(N + 1)], -1)
    pos[N, 1] = 2.0
    Rg, Ro, br, cross, _ = score_both(N, flat_traj(pos), GATE_Y0)
    assert np.all(br == 0) and np.all(cross == O.CROSS_NEVER), (br, cross)
    assert_close(Rg, Ro, f"behind only at stage N={N}")


def test_one_rotor_starts_behind_the_others_cross():
    """Gate in the plane x + y = 0 (corners at powers of two), flown along (1, 1, 0): rotor 0 leads by 2a and is behind
    at stage 0, rotors 1 and 3 cross at stage 2, rotor 2 at stage 4.  Rotor 0 contributes nothing: the reward is that
    of the other three tracks, each scored alone by the oracle's collis_det."""
    from oracle import oracle as O
    N = 7
    gate = np.array([[-0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, -0.5]])
    u = -0.375 + 0.25 * np.arange(N + 1)
    pos = np.stack([u, u, np.full(N + 1, 0.125)], -1)
    goal = (0.25, 4.0, -0.5)
    Rg, Ro, br, cross, _ = score_both(N, flat_traj(pos), gate, goal)
    assert cross[0] == O.CROSS_BEHIND and br[0] == 0, (cross, br)
    assert list(cross[1:]) == [2, 4, 2] and np.all(br[1:] != 0), (cross, br)
    tracks = pos[None, :, :] + TIP_OFF[:, None, :]
    col, _, _ = O.collis_det(np.tile(gate.reshape(1, 12), (4, 1)), tracks)
    assert col[0] == 0.0 and col[1] < 0.0 and col[3] < 0.0, col     # rotor 2 passes through the middle: -0.0
    path = sum(float(np.sum((pos[N - 1 - p] - np.array(goal)) ** 2)) for p in range(4))
    expect = 1000.0 * (col[1] + col[2] + col[3]) - 0.5 * path + 100.0
    assert abs(Ro[0] - expect) <= RTOL * max(1.0, abs(expect)), (Ro, expect)
    assert_close(Rg, Ro, "one rotor starts behind")


def test_four_rotors_four_branches():
    """One trajectory, four branch codes: rotors 0 and 1 pass a 4 x 4 gate inside its window in the right and the top
    sector (stage 2), then the track moves below the gate and rotors 3 and 2 pass at the frame in the bottom and the
    left sector (stage 4).  Each rotor's result reaches the sum through its own LDS slot."""
    N = 7
    gate = 4.0 * GATE_Y0
    pos = np.array([[1.0 + WING_A, -2.0, 0.25], [1.0 + WING_A - 1.0, -1.0, 0.25], [1.0 + WING_A - 1.0, -0.25, 0.25],
                    [-4.0 + WING_A, -0.25, -3.25], [-4.0 + WING_A, 1.0, -3.25], [-4.0, 2.0, -3.0],
                    [-4.0, 3.0, -3.0], [-4.0, 4.0, -3.0]])
    Rg, Ro, br, cross, _ = score_both(N, flat_traj(pos), gate)
    assert sorted(br) == [1, 5, 10, 14], br
    assert list(cross) == [2, 2, 4, 4], cross
    assert_close(Rg, Ro, "four rotors, four branches")


@pytest.mark.parametrize("N", (50, 7))
@pytest.mark.parametrize("where", ("mid", "tail"))
def test_nan_position_row(N, where):
    """A NaN position row in mid-trajectory (a side test that is neither behind nor in front, a NaN previous point)
    and one among the path term's rows N-4..N-1: the device's NaN pattern is the oracle's and the finite rewards agree."""
    from oracle import oracle as O
    s = sweep_ref(N)
    x = s["x"][:64].copy()
    row = max(1, (N - 4) // 2) if where == "mid" else N - 2     # mid: below the path term's rows
    x[:, row, 0:3] = np.nan
    Ro, _ = O.reward(x, s["goal"][:64], s["gate12"][:64], params=O.default_params(horizon=N))
    if where == "tail":
        assert np.all(np.isnan(Ro))
    else:
        assert np.any(np.isfinite(Ro))
    assert_close(gpu_reward(N, x, s["goal"][:64], s["gate12"][:64]), Ro, f"NaN row {row} of N={N}")


# ------------------------------------------------------------------------------------------------ c. parameters
@pytest.mark.parametrize("N", (50, 7))
def test_non_default_d_min_and_wing_len(N):
    from oracle import oracle as O
    s = sweep_ref(N)
    x, goal, g12 = s["x"][:64], s["goal"][:64], s["gate12"][:64]
    prm = {"d_min": 0.35, "wing_len": 1.0}
    Ro, br, _, _ = O.reward_detail(x, goal, g12, params=O.default_params(horizon=N, **prm))
    Rg = gpu_reward(N, x, goal, g12, **prm)
    assert_close(Rg, Ro, f"d_min 0.35, wing_len 1.0, N={N}")
    inside = np.any(np.isin(br, INSIDE), axis=1)
    assert inside.any(), "no inside-window sample in the slice"
    Rdef = gpu_reward(N, x, goal, g12)
    assert np.any(Rg[inside] != Rdef[inside]), "the parameters changed no inside-window collision term"


# ------------------------------------------------------------------------------------------------ d. fused path
@pytest.mark.parametrize("N,t", ((3, 0.2), (7, 0.4)))
def test_fused_reward_equals_scoring_launch(N, t):
    """lafse3_objective's reward, scored in the solver launch, against lafse3_reward on the trajectory the same
    engine's ocp_solve returns: both score the device's own final iterate, so no solver tolerance enters."""
    import torch
    from learningagileflight_se3_amd import scenario as S
    sb = S.synthetic_batch(8, seed=11)
    d = sb["dnn_out"].astype(np.float64)
    p, a, tt = d[:, 0:3], d[:, 3:6], np.full(8, t)
    eng = engine(N)
    Rf, st = eng.objective(sb["ini"], sb["goal"], sb["gate12"], p, a, tt)
    out = eng.ocp_solve(sb["ini"], sb["goal"], p, a, tt, want=("x",))
    Rs = eng.reward(out["x"], sb["goal"], sb["gate12"])
    torch.cuda.synchronize()
    Rf, Rs, st, st2 = Rf.cpu().numpy(), Rs.cpu().numpy(), st.cpu().numpy(), out["status"].cpu().numpy()
    assert np.all(st <= 1) and np.all(st2 <= 1), (st, st2)
    print(f"N={N}: fused and scored rewards bit-equal on {int(np.sum(Rf == Rs))} of 8")
    assert_close(Rf, Rs, f"fused against scoring launch, N={N}")


# ------------------------------------------------------------------------------------------------ e. horizon 1
def test_horizon_1_reward_entry_points_refuse():
    """The reference's path term indexes row -3 of a two-row trajectory at horizon 1 (IndexError): the three entry
    points that score a reward refuse that horizon, and the solve on the same engine still works."""
    import torch
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd._lib import Lafse3Error
    sb = S.synthetic_batch(2, seed=11)
    d = sb["dnn_out"].astype(np.float64)
    eng = engine(1)
    with pytest.raises(Lafse3Error, match="horizon 1"):
        eng.reward(np.zeros((2, 2, 13)), sb["goal"], sb["gate12"])
    with pytest.raises(Lafse3Error, match="horizon 1"):
        eng.objective(sb["ini"], sb["goal"], sb["gate12"], d[:, 0:3], d[:, 3:6], 0.1)
    with pytest.raises(Lafse3Error, match="horizon 1"):
        eng.sol_gradient(sb["ini"], sb["goal"], sb["gate12"], sb["dnn_out"])
    out = eng.ocp_solve(sb["ini"], sb["goal"], d[:, 0:3], d[:, 3:6], 0.05)
    torch.cuda.synchronize()
    assert np.all(out["status"].cpu().numpy() <= 1) and np.all(np.isfinite(out["x"].cpu().numpy()))
