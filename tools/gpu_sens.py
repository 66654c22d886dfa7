"""Cost of the sensitivity pass at configs[1]'s shape: B = 1024 forward solves of bench.py's configs[1] batch (seed 77),
lafse3_last_kernel_ms of ocp_solve and of ocp_sensitivity (the same solves plus one factorisation at the optimum and
7 refinement sweeps per instance, dx and du stored), interleaved in one process.  Prints one JSON line
(committed as profiles/sens_configs1.json)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from learningagileflight_se3_amd import scenario as S
from learningagileflight_se3_amd.engine import Engine

B = int(os.environ.get("B", "1024"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
eng = Engine()
sb = S.synthetic_batch(B, seed=int(os.environ.get("SEED", "77")))
f64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")
args = [f64(sb["ini"]), f64(sb["goal"]), f64(sb["dnn_out"][:, :3]), f64(sb["dnn_out"][:, 3:6]), f64(sb["dnn_out"][:, 6])]
eng.ocp_solve(*args)
eng.ocp_sensitivity(*args)
torch.cuda.synchronize()
solve_ms, sens_ms = [], []
for _ in range(ROUNDS):   # interleaved rounds in one process on one device
    eng.ocp_solve(*args)
    torch.cuda.synchronize()
    solve_ms.append(eng.last_kernel_ms())
    cnt = eng.last_counters()
    out = eng.ocp_sensitivity(*args)
    torch.cuda.synchronize()
    sens_ms.append(eng.last_kernel_ms())
ss = out["sens_status"].cpu().numpy()
st = out["status"].cpu().numpy()
print(json.dumps({
    "tool": "tools/gpu_sens.py", "B": B, "rounds": ROUNDS, "horizon": eng.horizon,
    "ocp_solve_kernel_ms": {"median": float(np.median(solve_ms)), "min": float(np.min(solve_ms)), "all": [round(v, 3) for v in solve_ms]},
    "ocp_sensitivity_kernel_ms": {"median": float(np.median(sens_ms)), "min": float(np.min(sens_ms)), "all": [round(v, 3) for v in sens_ms]},
    "ratio_median": float(np.median(sens_ms) / np.median(solve_ms)),
    "ratio_min": float(np.min(sens_ms) / np.min(solve_ms)),
    "sens_status_histogram": np.bincount(ss, minlength=3).tolist(),
    "solved_or_acceptable": int((st <= 1).sum()),
    "iterations_per_solve": cnt["iterations"] / B, "sweeps_per_iteration": cnt["sweeps"] / max(cnt["iterations"], 1),
    "device": torch.cuda.get_device_name(0)}))
