"""The CPU oracle's reward scorer (oracle/lafse3_oracle.c reward_from_traj / collis_det) where tests/test_gpu_reward.py
relies on it: the goal path term at short horizons against the reference's numpy statement, the refusal of horizon 1,
the coverage of the GPU test's input generator, and d_min as a parameter.  No GPU.
"""
import numpy as np
import pytest

import reward_cases as GR
from oracle import oracle as O


def _random_traj(N, B, seed):
    rng = np.random.default_rng([seed, N])
    x = rng.normal(0.0, 2.0, (B, N + 1, 13))
    gate = np.array([[-0.5, 0, 0.5], [0.5, 0, 0.5], [0.5, 0, -0.5], [-0.5, 0, -0.5]]) + rng.normal(0, 1, (B, 1, 3))
    return x, rng.normal(0.0, 3.0, (B, 3)), rng.normal(0.0, 3.0, (B, 3)), gate.reshape(B, 12)


@pytest.mark.parametrize("N", (2, 3, 4, 50))
def test_path_term_is_the_numpy_statement(N):
    """quad_policy.py:88-89 sums |x[N-1-p, 0:3] - goal|^2 over p = 0..3 on an array of N+1 rows, so negative rows wrap.
    The path term is isolated as the difference of two rewards with different goals (the collision term cancels)."""
    B = 64
    x, g1, g2, gate = _random_traj(N, B, 7)
    prm = O.default_params(horizon=N)
    R1, _ = O.reward(x, g1, gate, params=prm)
    R2, _ = O.reward(x, g2, gate, params=prm)

    def path(goal):
        return sum(np.sum((x[:, (N - 1 - p) % (N + 1), 0:3] - goal) ** 2, axis=1) for p in range(4))

    want = -0.5 * (path(g1) - path(g2))
    got = R1 - R2
    # the rewards themselves stay below 1e5 here, so their rounding (1e-11) is far inside the bound on the difference
    scale = np.maximum(1.0, np.abs(want))
    assert max(np.max(np.abs(R1)), np.max(np.abs(R2))) < 1e5
    assert np.all(np.abs(got - want) <= 1e-9 * scale), float(np.max(np.abs(got - want) / scale))


def test_horizon_1_raises():
    x, g1, _, gate = _random_traj(1, 2, 7)
    prm = O.default_params(horizon=1)
    with pytest.raises(ValueError, match="horizon 1"):
        O.reward(x, g1, gate, params=prm)
    with pytest.raises(ValueError, match="horizon 1"):
        O.reward_detail(x, g1, gate, params=prm)
    with pytest.raises(ValueError, match="horizon 1"):
        O.sol_gradient(x[:, 0], g1, gate, np.zeros((2, 7), np.float32), params=prm)
    # the library itself refuses too, and writes nothing
    import ctypes
    r = np.full(2, -7.0)
    assert O.lib().orc_reward(ctypes.byref(prm), 2, O._ptr(x), O._ptr(g1), O._ptr(gate), O._ptr(r), None) != 0
    assert O.lib().orc_reward_detail(ctypes.byref(prm), 2, O._ptr(x), O._ptr(g1), O._ptr(gate), O._ptr(r), None, None) != 0
    out8 = np.full((2, 8), -7.0)
    dnn = np.zeros((2, 7), np.float32)
    assert O.lib().orc_sol_gradient(ctypes.byref(prm), 2, O._ptr(np.ascontiguousarray(x[:, 0])), O._ptr(g1), O._ptr(gate),
                                    O._ptr(dnn, ctypes.c_float), None, O._ptr(out8), None, None) != 0
    assert np.all(r == -7.0) and np.all(out8 == -7.0)
    # the solve keeps horizon 1
    sol = O.solve(x[:, 0] * 0 + np.eye(13)[6], g1, np.zeros((2, 3)), np.tile(np.eye(4)[0], (2, 1)), 0.05, params=prm)
    assert sol["x"].shape == (2, 2, 13)


@pytest.mark.parametrize("N", GR.HORIZONS)
def test_generator_reaches_every_branch(N):
    s = GR.sweep_ref(N)
    h = GR.assert_coverage(N, s)
    print(f"N={N} coverage {h}; rewards {s['R'].min():.4g} .. {s['R'].max():.4g}")
    # reward_detail's reward and branch codes are orc_reward's
    R, br = O.reward(s["x"], s["goal"], s["gate12"], params=O.default_params(horizon=N))
    assert np.array_equal(R, s["R"]) and np.array_equal(br, s["branch"])


def test_generator_is_seeded():
    a, b = GR.sweep(7, B=16), GR.sweep(7, B=16)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def _lead_rotor_tracks(B, seed):
    """Straight tracks along +y that stop 0.3 short of plane 1 with the body yawed by 45 degrees: one tip leads by
    a sqrt(2) = 0.75 and crosses inside the window, the other three never reach the plane."""
    rng = np.random.default_rng(seed)
    N = 7
    w, h = rng.uniform(0.5, 1.25, (2, B))
    cen = rng.normal(0.0, 1.0, (B, 3))
    rel = np.stack([np.stack([-w / 2, 0 * w, h / 2], -1), np.stack([w / 2, 0 * w, h / 2], -1),
                    np.stack([w / 2, 0 * w, -h / 2], -1), np.stack([-w / 2, 0 * w, -h / 2], -1)], 1)
    gate = rel + cen[:, None]
    off = rng.uniform(-0.3, 0.3, (B, 2)) * np.stack([w / 2, h / 2], -1)
    k = np.arange(N + 1)[None, :, None] / N
    start = cen + np.stack([off[:, 0], -3.0 + 0 * w, off[:, 1]], -1)
    end = cen + np.stack([off[:, 0], -0.3 + 0 * w, off[:, 1]], -1)
    x = np.zeros((B, N + 1, 13))
    x[:, :, 0:3] = start[:, None] + k * (end - start)[:, None]
    x[:, :, 6], x[:, :, 9] = np.cos(np.pi / 8), np.sin(np.pi / 8)
    return N, x, rng.normal(0.0, 3.0, (B, 3)), gate.reshape(B, 12)


def test_d_min_is_a_parameter():
    """With one rotor inside the window and the other three short of the plane the collision term is
    -(max(0, d_min - m))^2 of that rotor's margin m.  d_min = 0 scores no collision on any branch, so R(0) is the rest
    of the reward; m comes from a run at d_min = 2 (above every margin of these gates), and the run at d_min = 0.35 has
    to be the closed form in that m, both where 0.35 - m is clipped at 0 and where it is not."""
    N, x, goal, gate = _lead_rotor_tracks(48, 3)
    R = {d: O.reward_detail(x, goal, gate, params=O.default_params(horizon=N, d_min=d)) for d in (0.0, 2.0, 0.35, 0.2)}
    br = R[0.35][1]
    assert np.all(np.sort(br, axis=1)[:, :3] == 0) and np.all(np.isin(br.max(axis=1), GR.INSIDE)), br
    for d in R:   # d_min moves no branch decision
        assert np.array_equal(R[d][1], br)
    m = 2.0 - np.sqrt(-(R[2.0][0] - R[0.0][0]) / 1000.0)
    assert np.all(m > 0.0) and np.all(m < 0.625 + 1e-12)
    assert np.any(m < 0.35) and np.any(m > 0.35), m
    for d in (0.35, 0.2):
        want = R[0.0][0] - 1000.0 * np.maximum(0.0, d - m) ** 2
        assert np.all(np.abs(R[d][0] - want) <= 1e-9 * np.maximum(1.0, np.abs(want))), d
    assert np.any(R[0.35][0] != R[0.2][0])
    # the default is the reference's 0.2
    Rdef, _ = O.reward(x, goal, gate, params=O.default_params(horizon=N))
    assert np.array_equal(Rdef, R[0.2][0])
