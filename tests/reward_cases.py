"""The inputs of the reward tests (test_gpu_reward.py on the device, test_reward_host.py without one): the seeded sweep
of trajectories through, past and short of random gates, the oracle's verdict on it and the coverage it has to reach.
Needs numpy and the oracle alone."""
import math

import numpy as np

SEED = 20261
HORIZONS = (50, 7, 4, 3, 2)
B_SWEEP = 256
CODES = (0, 1, 2, 5, 6, 9, 10, 13, 14)
INSIDE, FRAME = (1, 5, 9, 13), (2, 6, 10, 14)
MODES = ("centre", "frame", "far", "behind", "short")
SIGMA = (0.15, 0.8, 3.0, 0.3, 0.3)     # crossing offset from the gate's centroid per mode


# ------------------------------------------------------------------------------------------------ generator
def sweep(N, B=B_SWEEP, seed=SEED):
    """B trajectories of horizon N with their gates and goals: dict(x (B, N+1, 13), goal (B, 3), gate12 (B, 12),
    mode (B,)).  Gate: width and height U(0.5, 1.25), pitched by U(-pi/2, pi/2) about y, shifted by N(0, 1).  Plane 1
    of such a gate faces -y: "in front" is y below the centroid's.  Centre track: a bent line from 2..9 in front
    of the plane to 1..6 behind it with per-step noise 0.02, through the point of the plane at an offset from the
    centroid drawn per mode (sample index mod 5): N(0, 0.15) centre, N(0, 0.8) frame, N(0, 3) far outside,
    N(0, 0.3) with the start up to 0.7 behind the plane, and a track that ends 0.8..1.5 in front of the plane.
    Attitude: a random unit quaternion plus N(0, 0.03) per step, not renormalised; velocities and rates N(0, 1).
    Samples 0 and 1 are hand-placed: no noise and the body's x-y plane turned into the world's x-z plane, so that all
    four tips pass the plane between the same two stages, 0|1 (sample 0) and N-2|N-1 (sample 1)."""
    rng = np.random.default_rng([seed, N])
    x = np.zeros((B, N + 1, 13))
    goal = np.zeros((B, 3))
    gate = np.zeros((B, 4, 3))
    mode = np.arange(B) % len(MODES)
    k = np.arange(N + 1, dtype=np.float64)[:, None]
    for i in range(B):
        w, h = rng.uniform(0.5, 1.25, 2)
        ang = rng.uniform(-math.pi / 2, math.pi / 2)
        cen = rng.normal(0.0, 1.0, 3)
        rel = np.array([[-w / 2, 0, h / 2], [w / 2, 0, h / 2], [w / 2, 0, -h / 2], [-w / 2, 0, -h / 2]])
        c, s = math.cos(ang), math.sin(ang)
        gate[i] = np.stack([c * rel[:, 0] - s * rel[:, 2], rel[:, 1], s * rel[:, 0] + c * rel[:, 2]], -1) + cen
        m = mode[i]
        off = rng.normal(0.0, SIGMA[m], 2)
        cross = cen + np.array([off[0], 0.0, off[1]])
        lat0, lat1 = rng.normal(0.0, 1.0, 2), rng.normal(0.0, 1.0, 2)
        start = cross + np.array([lat0[0], -rng.uniform(2.0, 9.0), lat0[1]])
        end = cross + np.array([lat1[0], rng.uniform(1.0, 6.0), lat1[1]])
        tau = rng.uniform(0.2, N - 1.2)
        q0 = rng.normal(0.0, 1.0, 4)
        q0 /= np.linalg.norm(q0)
        noise_p, noise_q = rng.normal(0.0, 0.02, (N + 1, 3)), rng.normal(0.0, 0.03, (N + 1, 4))
        hand = i < 2
        if hand:
            tau = 0.5 if i == 0 else max(0.5, N - 1.5)
            q0 = np.array([math.sqrt(0.5), math.sqrt(0.5), 0.0, 0.0])
            noise_p[:] = 0.0
            noise_q[:] = 0.0
        if MODES[m] == "behind" and not hand:
            first = cross + np.array([0.0, rng.uniform(0.0, 0.7), 0.0])
            pos = first + k / N * (end + np.array([0.0, 1.0, 0.0]) - first)
        elif MODES[m] == "short" and not hand:
            last = cross + np.array([0.0, -rng.uniform(0.8, 1.5), 0.0])
            half = 0.5 * (start + last) + np.array([lat1[0], 0.0, lat1[1]])
            pos = np.where(k <= N / 2, start + k / (N / 2) * (half - start), half + (k - N / 2) / (N / 2) * (last - half))
        else:
            pos = np.where(k <= tau, start + k / tau * (cross - start), cross + (k - tau) / (N - tau) * (end - cross))
        x[i, :, 0:3] = pos + noise_p
        x[i, :, 3:6] = rng.normal(0.0, 1.0, (N + 1, 3))
        x[i, :, 6:10] = q0 + noise_q
        x[i, :, 10:13] = rng.normal(0.0, 1.0, (N + 1, 3))
        goal[i] = cen + np.array([rng.normal(0.0, 2.0), rng.uniform(3.0, 9.0), rng.normal(0.0, 2.0)])
    return {"x": x, "goal": goal, "gate12": gate.reshape(B, 12), "mode": mode}


_sweeps = {}


def sweep_ref(N):
    """The sweep of horizon N with the oracle's verdict on it (default parameters), computed once:
    adds R (B,), branch, cross, ld (B, 4)."""
    if N not in _sweeps:
        from oracle import oracle as O
        s = sweep(N)
        s["R"], s["branch"], s["cross"], s["ld"] = O.reward_detail(s["x"], s["goal"], s["gate12"],
                                                                   params=O.default_params(horizon=N))
        for v in s.values():
            v.setflags(write=False)
        _sweeps[N] = s
    return _sweeps[N]


def histogram(s):
    from oracle import oracle as O
    h = {c: int(np.sum(s["branch"] == c)) for c in CODES}
    h["perp"], h["end"] = int(np.sum(s["ld"] == O.LD_PERP)), int(np.sum(s["ld"] == O.LD_END))
    h["behind"], h["never"] = int(np.sum(s["cross"] == O.CROSS_BEHIND)), int(np.sum(s["cross"] == O.CROSS_NEVER))
    return h


def assert_coverage(N, s):
    """What the sweep of horizon N has to reach, from the oracle's own report of its decisions.  A failure here means
    the seed or the generator has to change, never this function."""
    from oracle import oracle as O
    h = histogram(s)
    assert set(np.unique(s["branch"])) <= set(CODES)
    for c in CODES:
        assert h[c] > 0, (N, "branch code", c, "not reached", h)
    assert h["behind"] > 0 and h["never"] > 0, (N, h)
    # a frame branch always reports one of the two line-distance outcomes, every other branch none
    frame = np.isin(s["branch"], FRAME)
    assert np.all((s["ld"][frame] == O.LD_PERP) | (s["ld"][frame] == O.LD_END)) and np.all(s["ld"][~frame] == O.LD_NONE)
    # a branch other than 0 has a crossing stage in 1..N-1 (stage 0 behind is "starts behind")
    hit = s["branch"] != 0
    assert np.all((s["cross"][hit] >= 1) & (s["cross"][hit] <= N - 1)), N
    assert np.all(np.isfinite(s["R"])), N
    if N == 50:
        assert h["perp"] > 0 and h["end"] > 0, h
    if N in (50, 7):
        assert np.any(s["cross"] == 1) and np.any(s["cross"] == N - 1), (N, np.unique(s["cross"]))
    return h
