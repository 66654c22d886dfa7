"""Cost of lafse3_ocp_sensitivity_ex at configs[1]'s shape: B = 1024 forward solves of bench.py's configs[1] batch
(seed 77), lafse3_last_kernel_ms of the new call as the plain solve (no sensitivity output), gain-only (one
factorisation at the optimum + 4 adjoint sweeps per instance) and all 23 forward columns (one factorisation + 23
sweeps, dx and du stored), interleaved in one process.  Prints one JSON line (committed as
profiles/sens_ex_cost.json)."""
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
WANT = {"plain_solve": ("x", "u"), "gain_only": ("x", "u", "gain"), "forward_23_columns": ("x", "u", "dx", "du"),
        "forward_23_columns_and_gain": ("x", "u", "dx", "du", "gain")}
for want in WANT.values():
    eng.ocp_sensitivity_ex(*args, want=want)
torch.cuda.synchronize()
ms = {k: [] for k in WANT}
out = {}
for _ in range(ROUNDS):   # interleaved rounds in one process on one device
    for k, want in WANT.items():
        out[k] = eng.ocp_sensitivity_ex(*args, want=want)
        torch.cuda.synchronize()
        ms[k].append(eng.last_kernel_ms())
ss = out["gain_only"]["sens_status"].cpu().numpy()
st = out["gain_only"]["status"].cpu().numpy()
base = float(np.median(ms["plain_solve"]))
print(json.dumps({
    "tool": "tools/gpu_sens_ex.py", "command": "python tools/gpu_sens_ex.py", "B": B, "rounds": ROUNDS,
    "horizon": eng.horizon,
    "kernel_ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "all": [round(x, 3) for x in v]}
                  for k, v in ms.items()},
    "ratio_to_plain_solve_median": {k: float(np.median(v)) / base for k, v in ms.items()},
    "sens_status_histogram": np.bincount(ss, minlength=3).tolist(),
    "solved_or_acceptable": int((st <= 1).sum()),
    "device": torch.cuda.get_device_name(0)}))
