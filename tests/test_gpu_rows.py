"""GPU tests of the §8(f) rows built on the engine: imitation trajectories (nn_train_2.py:29-40) and the
RL loop (deep_learning.py:34-94) against the CPU oracle on the same samples."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd.engine import Engine
    return Engine()


def _q_f32(a32):
    """Rd2Rp + toQuaternion on a float32 angle vector: its norm in float32."""
    from oracle import oracle as O
    n = np.float64(np.sqrt(np.float32(sum(np.float64(np.float32(c * c)) for c in a32))))
    return O.rd2quat(a32.astype(np.float64), n)


def test_imitation_trajectories_match_oracle(eng):
    from learningagileflight_se3_amd import scenario
    from learningagileflight_se3_amd.imitation import imitation_pairs, trajectories
    from oracle import oracle as O
    sb = scenario.synthetic_batch(6, seed=31)
    x, st = trajectories(eng, sb["samples"], sb["dnn_out"])
    x = x.cpu().numpy()
    dn = sb["dnn_out"]
    q = np.stack([_q_f32(v) for v in dn[:, 3:6]])
    ref = O.solve(sb["ini"], sb["goal"], dn[:, :3].astype(np.float64), q, dn[:, 6].astype(np.float64), np.zeros(4))
    assert np.max(np.abs(x - ref["x"])) < 1e-5
    inp, tgt = imitation_pairs(sb["samples"], dn, x)
    assert inp.shape == (6 * 50, 18) and np.array_equal(inp[:50, :13], x[0, :50])


def test_rl_loop_rewards_match_oracle(eng):
    from learningagileflight_se3_amd import scenario
    from learningagileflight_se3_amd.policy_net import Network
    from learningagileflight_se3_amd.rl_loop import engine_gradient, run_rl
    from oracle import oracle as O
    torch.manual_seed(0)
    net = Network(9, 64, 64, 7).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    seen = []
    gpu_grad = engine_gradient(eng)

    def grad_fn(samples, out):
        g = gpu_grad(samples, out)
        seen.append((samples, out, g))
        return g

    res = run_rl(net, opt, grad_fn, epochs=1, batch_size=8, num_cores=4, update="reference",
                 rng=np.random.default_rng(3))
    assert res["every_reward"].shape == (1, 8)
    for samples, out, g in seen:
        ini = scenario.initial_state(samples[:, 0:3], samples[:, 6])
        gate12 = scenario.gate_corners(samples[:, 7], samples[:, 8])
        r8, _, rs = O.sol_gradient(ini, samples[:, 3:6], gate12, out)
        assert np.all(rs <= 1)
        # north_star: 1e-5 relative (gradients on the (1 + |g|) scale of parity_ref.grad_parity)
        assert np.max(np.abs(g[:, 7] - r8[:, 7]) / np.maximum(1.0, np.abs(r8[:, 7]))) < 1e-5
        assert np.max(np.abs(g[:, :7] - r8[:, :7]) / (1.0 + np.abs(r8[:, :7]))) < 1e-5


def test_moving_gate_receding_horizon_matches_reference_loop(eng, golden):
    """main.py:44-116 (120 plant steps, 12 MPC solves per episode; episode 0 = last_inputs.npy's scenario)
    against tests/golden/moving.npz, the reference's own loop with the trained DNN2 (nn3_1.pth) and the
    oracle in place of ocSolver; DNN2 evaluated per sample on the CPU as the reference does, so the only
    differences are the NLP solves (GPU get_input vs oracle) and their propagation through the plant."""
    from learningagileflight_se3_amd import moving_gate as MG
    from moving_cases import dnn2_from_fixture, fixture_episodes, per_sample
    g = golden("moving")
    n_ep, steps = g["t"].shape
    samples, noise = fixture_episodes(g)
    res = MG.run_episodes(eng, per_sample(dnn2_from_fixture(g)), samples, noise, steps=steps)
    assert res["solves"] == n_ep * (steps // MG.CTRL_EVERY) and np.all(res["status"] <= 1)
    # u to the IPOPT tolerance scale; a 1e-7 thrust difference moves w by ~1e-6 over a 10-step hold
    # (dt l / (2 J) ~ 0.76 per unit thrust-step)
    assert np.max(np.abs(res["controls"] - g["controls"])) < 1e-6
    assert np.max(np.abs(res["states"] - g["states"])) < 2e-5
    assert np.max(np.abs(res["t"] - g["t"])) < 1e-6


def test_moving_gate_full_length_episode(eng, golden):
    """configs[4] at main.py's full length (main.py:65: 500 plant steps of 10 ms, 50 receding-horizon MPC
    solves): episode 0 (last_inputs.npy's scenario) against tests/golden/moving500.npz, the reference's own loop
    with the trained DNN2 and the oracle in place of ocSolver.  DNN2 per sample on the CPU as the reference
    evaluates it, so the differences are the NLP solves (GPU get_input vs oracle, agreeing to IPOPT's tolerance)
    and their propagation through the closed loop."""
    from learningagileflight_se3_amd import moving_gate as MG
    from moving_cases import dnn2_from_fixture, fixture_episodes, per_sample
    g = golden("moving500")
    n_ep, steps = g["t"].shape
    assert (n_ep, steps) == (1, 500) and g["source"][0] == 0
    samples, noise = fixture_episodes(g)
    res = MG.run_episodes(eng, per_sample(dnn2_from_fixture(g)), samples, noise, steps=steps)
    assert res["solves"] == 50 and np.all(res["status"] <= 1)
    du = np.abs(res["controls"] - g["controls"]).max()
    dx = np.abs(res["states"] - g["states"]).max()
    dt = np.abs(res["t"] - g["t"]).max()
    print(f"500-step episode: max |du| {du:.3e}, max |dx| {dx:.3e}, max |dt| {dt:.3e}")
    assert du < 1e-5 and dx < 1e-4 and dt < 1e-5


def test_traversal_time_kernel_matches_reference_loop_t(eng, golden):
    """lafse3_traversal_time against the t values the REFERENCE's own loop computed (tests/golden/moving.npz: main.py
    with quad_moving.solver evaluating the trained DNN2 per sample in torch on the CPU, quad_moving.py:29-57), at every
    one of its 2 x 120 plant steps, from the fixture's plant state, gate corners and gate velocity.  The stopping
    test |t2 - t1| <= 0.001 is discontinuous: an fp32 rounding difference between the kernel's DNN2 and torch's can
    end the halving updates one step earlier or later, moving t by at most half the last update (<= 5e-4).
    Required: >= 98 % of the steps within 1e-5 of the reference, every step within 5e-4 + 1e-5."""
    from moving_cases import dnn2_from_fixture
    g = golden("moving")
    net = dnn2_from_fixture(golden("dnn2_nn3_1")).cuda()
    n_ep, steps = g["t"].shape
    st = torch.as_tensor(g["states"][:, :steps].reshape(-1, 13), device="cuda")
    fin = torch.as_tensor(np.repeat(g["inputs"][:, 3:6], steps, axis=0), device="cuda")
    gm = torch.as_tensor(g["gate_move"][:, :steps].reshape(-1, 4, 3), device="cuda")
    V = torch.as_tensor(g["V"][:, :steps].reshape(-1, 3), device="cuda")
    t, it = eng.traversal_time(st, fin, gm, V, np.pi / 2, net, want_iters=True)
    d = np.abs(t.cpu().numpy() - g["t"].reshape(-1))
    print(f"traversal time vs the reference loop: {np.mean(d <= 1e-5) * 100:.1f} % within 1e-5, max {d.max():.3e}, "
          f"steps off by an update: {int(np.sum(d > 1e-5))} of {d.size}")
    assert np.all(it.cpu().numpy() >= 0) and np.all(it.cpu().numpy() <= 200)
    assert np.mean(d <= 1e-5) >= 0.98 and d.max() <= 5e-4 + 1e-5


def test_moving_gate_device_path_matches_host_path(eng):
    """run_episodes_device (kinematics, DNN2, plant on the GPU) against run_episodes (host kinematics,
    scipy transforms) with the same DNN2 on the same device: 16 episodes x 30 plant steps."""
    from learningagileflight_se3_amd import moving_gate as MG
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.policy_net import Network
    rs = np.random.RandomState(77)
    samples = np.stack([S.nn_sample(rs) for _ in range(16)])
    noise = np.stack([MG.move_noise(rs, 30) for _ in range(16)])
    torch.manual_seed(0)
    net = Network(18, 128, 128, 7).cuda()
    host = MG.run_episodes(eng, MG.torch_dnn(net), samples, noise, steps=30)
    dev = MG.run_episodes_device(eng, net, samples, noise, steps=30)
    assert dev["solves"] == host["solves"]
    assert np.max(np.abs(dev["t"].cpu().numpy() - host["t"])) < 1e-6
    assert np.max(np.abs(dev["states"].cpu().numpy() - host["states"])) < 1e-5


def test_traversal_time_kernel_matches_torch_fixed_point(eng, golden):
    """lafse3_traversal_time (quad_moving.py:29-57 in one HIP kernel: DNN2 in fp32 with each lane's weight rows in
    registers, only the first layer's 128 activations exchanged through LDS) against solve_t_t
    (the same fixed point as batched torch ops) with the trained DNN2 (nn3_1.pth) along 64 episodes x 40
    plant steps.  The two evaluate DNN2 in fp32 with different summation orders, so t agrees to the fp32
    rounding of the network's output (carried through the halving updates), not bit for bit."""
    from learningagileflight_se3_amd import moving_gate as MG
    from learningagileflight_se3_amd import scenario as S
    from moving_cases import dnn2_from_fixture
    net = dnn2_from_fixture(golden("dnn2_nn3_1")).cuda()
    rs = np.random.RandomState(91)
    samples = np.stack([S.nn_sample(rs) for _ in range(64)])
    noise = np.stack([MG.move_noise(rs, 40) for _ in range(64)])
    run = MG.run_episodes_device(eng, net, samples, noise, steps=40, fixed_point="torch", graphs=False)
    gp0, _ = MG.initial_episodes(samples)
    gm, V = MG.move(gp0, (1.0, 0.3, 0.4), np.pi / 2, noise)
    gm, V = torch.as_tensor(gm, device="cuda"), torch.as_tensor(V, device="cuda")
    fin = torch.as_tensor(samples[:, 3:6].astype(np.float64), device="cuda")
    dt, n_it_diff = 0.0, 0
    for i in range(0, 40, 3):
        st = run["states"][:, i].contiguous()
        t_ref = MG.solve_t_t(net, st, fin, gm[:, i], V[:, i], np.pi / 2, check=1)
        t, it = eng.traversal_time(st, fin, gm[:, i], V[:, i], np.pi / 2, net, want_iters=True)
        assert torch.all(it >= 0) and torch.all(it <= 200)
        dt = max(dt, float((t - t_ref).abs().max()))
        n_it_diff += int((t - t_ref).abs().gt(1e-4).sum())
    print(f"max |t_kernel - t_torch| = {dt:.3e}, episodes off by an update: {n_it_diff}")
    assert n_it_diff == 0 and dt < 1e-5
    # the whole device loop on the kernel.  The stopping test |t2 - t1| <= 0.001 is discontinuous: an fp32
    # rounding difference can add or drop one halving update at some plant step (t moves by ~1e-4..1e-3) and the
    # episode then follows a slightly different, equally valid trajectory.  Episodes without such a flip agree
    # to the fp32 level; the flips are rare.
    ker = MG.run_episodes_device(eng, net, samples, noise, steps=40, fixed_point="kernel")
    dtk = np.abs(ker["t"].cpu().numpy() - run["t"].cpu().numpy())
    dsk = np.abs(ker["states"].cpu().numpy() - run["states"].cpu().numpy()).max(axis=(1, 2))
    same = dtk.max(axis=1) < 1e-5
    print(f"closed loop: {same.sum()} / 64 episodes agree; max |dt| there {dtk[same].max():.3e}, "
          f"max |dstate| {dsk[same].max():.3e}")
    # states: a 1e-6 change of t moves the MPC solution (its terminal time) and, through 10-step holds of the
    # thrusts, the angular rates by the IPM-tolerance scale amplified along the plant
    assert same.sum() >= 54 and np.all(dsk[same] < 1e-3)
    for e in np.flatnonzero(~same):
        first = np.flatnonzero(dtk[e] >= 1e-5)[0]
        print(f"  episode {e}: first |dt| >= 1e-5 at step {first}: {dtk[e, first]:.3e}")


def test_rl_loop_with_ift_gradients(eng):
    """run_rl on the IFT gradient (grad_mode 1): the first group's rewards (nominal solves, the same
    computation in both modes) equal the FD run's; the loop completes with finite rewards."""
    from learningagileflight_se3_amd.policy_net import Network
    from learningagileflight_se3_amd.rl_loop import engine_gradient, run_rl
    res = {}
    for m in (0, 1):
        torch.manual_seed(0)
        net = Network(9, 64, 64, 7).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        res[m] = run_rl(net, opt, engine_gradient(eng, grad_mode=m), epochs=1, batch_size=8, num_cores=4,
                        update="reference", rng=np.random.default_rng(5))
    assert eng.params.grad_mode == 0
    r0, r1 = res[0]["every_reward"], res[1]["every_reward"]
    assert r1.shape == (1, 8) and np.all(np.isfinite(r1))
    assert np.array_equal(r0[:, :4], r1[:, :4])


def test_queue_streams_overlap_two_contexts(eng):
    """Two contexts launched on two QueueStreams (lafse3_stream_create: a hardware queue each) run at the same time
    and give the single-stream results bit for bit.  Ordinary torch streams may share one of HIP's pooled hardware
    queues and then serialise (profiles/r05_moving_trace.log, the configs[4] episode groups at 2/3 rate)."""
    import time

    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.engine import Engine, QueueStream
    sb = S.synthetic_batch(64, seed=77)
    args = [torch.as_tensor(sb[k], device="cuda") for k in ("ini", "goal")]
    args += [torch.as_tensor(sb["dnn_out"][:, :3], device="cuda"), torch.as_tensor(sb["dnn_out"][:, 3:6], device="cuda"),
             torch.as_tensor(sb["dnn_out"][:, 6], device="cuda")]
    ref = eng.ocp_solve(*args)
    torch.cuda.synchronize()
    single_s = eng.last_kernel_ms() / 1e3
    e2 = Engine()
    qs = []
    try:                                           # e2 is closed whatever fails below
        qs = [QueueStream(), QueueStream()]
        try:
            for e, q in ((eng, qs[0]), (e2, qs[1])):   # warm both contexts on their streams
                with torch.cuda.stream(q.stream):
                    e.ocp_solve(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = []
            for e, q in ((eng, qs[0]), (e2, qs[1])):
                with torch.cuda.stream(q.stream):
                    outs.append(e.ocp_solve(*args))
            torch.cuda.synchronize()
            both_s = time.perf_counter() - t0
        finally:
            for q in qs:
                q.close()
        # the contexts outlive the streams they launched on: counters and the device check read on a stream of the
        # context's own (api.hip read_counters), not on the destroyed launch stream
        for e in (eng, e2):
            assert e.last_counters()["iterations"] > 0
            e.check_device()
    finally:
        e2.close()
    for o in outs:
        assert torch.equal(o["cost"], ref["cost"]) and torch.equal(o["x"], ref["x"])
    # 64 instances fill 64 of the 1024 wave slots: two launches on separate queues overlap almost entirely
    assert both_s < 1.6 * single_s, (both_s, single_s)


def test_graphed_train_step_equals_eager_step(eng):
    """bench.py's DNN1 step replayed from HIP graphs (rl_step.GraphedTrainStep) == the same step issued eagerly
    (Adam capturable in both), bit for bit over several steps with different MPC gradients, starting from the
    untouched network (the capture's warm-up steps are undone)."""
    from learningagileflight_se3_amd.policy_net import Network
    from learningagileflight_se3_amd.rl_step import GraphedTrainStep, train_step
    dev = eng.device
    g = torch.Generator(device="cpu").manual_seed(7)
    inputs = torch.randn(256, 9, generator=g).to(dev)
    grads = [torch.randn(256, 8, generator=g, dtype=torch.float64).to(dev) for _ in range(4)]
    torch.manual_seed(3)
    net_e = Network(9, 64, 64, 7).to(dev)
    torch.manual_seed(3)
    net_g = Network(9, 64, 64, 7).to(dev)
    init = [p.detach().clone() for p in net_g.parameters()]
    opt_e = torch.optim.Adam(net_e.parameters(), lr=1e-3, capturable=True)
    opt_g = torch.optim.Adam(net_g.parameters(), lr=1e-3, capturable=True)
    step_g = GraphedTrainStep(net_g, opt_g, inputs, (256, 8))
    for p, v in zip(net_g.parameters(), init):
        assert torch.equal(p.detach(), v)            # the warm-up steps were undone
    for o8 in grads:
        le = train_step(net_e, opt_e, inputs, o8)
        lg = step_g(o8)
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
    for pe, pg in zip(net_e.parameters(), net_g.parameters()):
        assert torch.equal(pe.detach(), pg.detach())
    assert not all(torch.equal(p.detach(), v) for p, v in zip(net_g.parameters(), init))
