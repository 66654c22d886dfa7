"""Cost of the two backward routes of the MPC layer at configs[1]'s shape: bench.py's configs[1] batch (seed 77) at
B = 1024 and B = 8192, five interleaved rounds in one process.  Per batch size:
  forward, Jacobian route   lafse3_last_kernel_ms of ocp_sensitivity_w with all four groups, dx and du stored
  forward, adjoint route    lafse3_last_kernel_ms of ocp_solve_rec
  backward, adjoint route   ocp_vjp (all four groups) between two torch events on the launch stream
and the bytes each route keeps for backward(), derived (B x P x 863 doubles against B x lafse3_rec_width() doubles)
and checked against the tensors.  Prints one JSON line (committed as profiles/vjp_cost.json)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from learningagileflight_se3_amd import scenario as S
from learningagileflight_se3_amd.engine import Engine

ROUNDS = int(os.environ.get("ROUNDS", "5"))
BATCHES = [int(b) for b in os.environ.get("B", "1024,8192").split(",")]
eng = Engine()
N, P = eng.horizon, 33
f64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "all": [round(x, 3) for x in v]}
result = {"tool": "tools/gpu_vjp.py", "command": "python tools/gpu_vjp.py", "rounds": ROUNDS, "horizon": N,
          "columns": P, "rec_width": eng.rec_width(), "device": torch.cuda.get_device_name(0), "batches": {}}
for B in BATCHES:
    sb = S.synthetic_batch(B, seed=int(os.environ.get("SEED", "77")))
    args = [f64(sb["ini"]), f64(sb["goal"]), f64(sb["dnn_out"][:, :3]), f64(sb["dnn_out"][:, 3:6]),
            f64(sb["dnn_out"][:, 6])]
    g = torch.Generator(device="cuda").manual_seed(7)
    g_x = torch.randn(B, N + 1, 13, dtype=torch.float64, device="cuda", generator=g)
    g_u = torch.randn(B, N, 4, dtype=torch.float64, device="cuda", generator=g)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def jac():
        out = eng.ocp_sensitivity_w(*args, want=("x", "u", "dx", "du"))
        torch.cuda.synchronize()
        return out, eng.last_kernel_ms()

    def rec():
        out = eng.ocp_solve_rec(*args, want=("x", "u"))
        torch.cuda.synchronize()
        return out, eng.last_kernel_ms()

    def vjp(r):
        ev0.record()
        out = eng.ocp_vjp(*args, None, None, r["rec"], g_x, g_u)
        ev1.record()
        torch.cuda.synchronize()
        return out, ev0.elapsed_time(ev1)

    j, _ = jac()          # warm every shape the timed rounds use
    r, _ = rec()
    v, _ = vjp(r)
    kept_jac = j["dx"].numel() * j["dx"].element_size() + j["du"].numel() * j["du"].element_size()
    kept_adj = r["rec"].numel() * r["rec"].element_size()
    assert kept_jac == B * P * ((N + 1) * 13 + N * 4) * 8 and kept_adj == B * eng.rec_width() * 8
    ref = torch.einsum("bqki,bki->bq", j["dx"], g_x) + torch.einsum("bqka,bka->bq", j["du"], g_u)
    live = (j["sens_status"] == 0) & (v["sens_status"] == 0)
    mag = torch.einsum("bqki,bki->bq", j["dx"].abs(), g_x.abs()) + torch.einsum("bqka,bka->bq", j["du"].abs(), g_u.abs())
    rel = ((v["grad"] - ref).abs() / mag.max(1, keepdim=True).values.clamp_min(1e-300))[live]
    hist_j = np.bincount(j["sens_status"].cpu().numpy(), minlength=4).tolist()
    hist_v = np.bincount(v["sens_status"].cpu().numpy(), minlength=4).tolist()
    del j, ref, mag
    ms = {"forward_jacobian_route": [], "forward_adjoint_route": [], "backward_adjoint_route": []}
    for _ in range(ROUNDS):   # interleaved rounds in one process on one device
        out, t = jac()
        del out
        ms["forward_jacobian_route"].append(t)
        r, t = rec()
        ms["forward_adjoint_route"].append(t)
        _, t = vjp(r)
        ms["backward_adjoint_route"].append(t)
    result["batches"][str(B)] = {
        "ms": {k: stat(v) for k, v in ms.items()},
        "bytes_kept_for_backward": {"jacobian_route": kept_jac, "adjoint_route": kept_adj,
                                    "per_instance": [kept_jac // B, kept_adj // B]},
        "sens_status_histogram": {"ocp_sensitivity_w": hist_j, "ocp_vjp": hist_v},
        "largest_relative_difference_of_the_two_routes": float(rel.max())}
print(json.dumps(result))
