"""Two builds of liblafse3.so (the same ABI) against each other on the sensitivity / record / adjoint entry points, each
build in child processes of its own (LAFSE3_LIB):

    python tools/gpu_sens_identity.py identity PARENT.so CANDIDATE.so     (profiles/ext_kernel_identity.log)
    python tools/gpu_sens_identity.py ab PARENT.so CANDIDATE.so           (profiles/ext_kernel_ab.txt)

identity: the seeded inputs of tests/sens_w_cases.py (rows D and G through the weights array, half the instances
each; case_t's traversal times; at horizon 1 the non-zero u_last of tests/test_gpu_vjp.py) at horizon 50 / 24
instances, 20 / 8, 2 / 4 and 1 / 4.  Per shape: ocp_solve, ocp_sensitivity, ocp_sensitivity_ex (all groups, gain),
ocp_sensitivity_w (all groups, gain; weights=None and the array), ocp_solve_rec, ocp_vjp (all groups, standard-normal
g_x, g_u of a fixed seed, on that build's own record).  Every returned array is compared byte for byte; one that is not
equal is listed with its largest difference relative to the array's largest magnitude.  Exit status 1 when x, u, lam,
cost, status, iters, sens_status or rec differ anywhere.

ab: bench.py's configs[1] batch (scenario.synthetic_batch(B, seed=77), B = 1024 and 8192 as tools/gpu_vjp.py):
lafse3_last_kernel_ms of ocp_sensitivity (dx, du), ocp_sensitivity_ex (all groups, dx, du, gain) and ocp_solve_rec,
and ocp_vjp (all groups, on that process's own record) between two events on the launch stream; parent and candidate
alternating for five rounds, each round a process that warms every call up once before timing it.
Medians, per-round values, and the bar: the candidate's median may exceed the parent's by the parent's max - min."""
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 24), (20, 8), (2, 4), (1, 4))
MUST = ("x", "u", "lam", "cost", "status", "iters", "sens_status", "rec")
SOLVE = ("x", "u", "lam", "cost")
ROUNDS = 5


def child_identity(out):
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import sens_w_cases as C
    from learningagileflight_se3_amd.engine import Engine
    sb, res = C.batch(), {}

    def keep(tag, r):
        torch.cuda.synchronize()
        for k, v in r.items():
            if isinstance(v, torch.Tensor):
                res[tag + "/" + k] = v.cpu().numpy()

    for N, B in SHAPES:
        n = B // 2
        idx = np.concatenate([np.arange(n), np.arange(n)])
        ul = np.tile([0.4, 0.9, 0.2, 1.3], (B, 1)) if N == 1 else None
        W = np.concatenate([np.tile(C.ROW_D, (n, 1)), np.tile(C.ROW_G, (n, 1))])
        a = tuple(v[idx] for v in (sb["ini"], sb["goal"], sb["p"], sb["a"], C.case_t(sb, N))) + (ul,)
        eng, tag = Engine(horizon=N), "N%d " % N
        keep(tag + "ocp_solve", eng.ocp_solve(*a, want=SOLVE))
        keep(tag + "ocp_sensitivity", eng.ocp_sensitivity(*a, want=SOLVE + ("dx", "du")))
        keep(tag + "ocp_sensitivity_ex", eng.ocp_sensitivity_ex(*a, want=SOLVE + ("dx", "du", "gain")))
        keep(tag + "ocp_sensitivity_w(None)", eng.ocp_sensitivity_w(*a, weights=None, want=SOLVE + ("dx", "du", "gain")))
        keep(tag + "ocp_sensitivity_w(W)", eng.ocp_sensitivity_w(*a, weights=W, want=SOLVE + ("dx", "du", "gain")))
        rec = eng.ocp_solve_rec(*a, weights=W, want=SOLVE)
        keep(tag + "ocp_solve_rec", rec)
        rng = np.random.default_rng(7)
        g_x, g_u = rng.standard_normal((B, N + 1, 13)), rng.standard_normal((B, N, 4))
        keep(tag + "ocp_vjp", eng.ocp_vjp(*a, W, rec["rec"], g_x, g_u))
    np.savez(out, **res)


def child_ab(out):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from learningagileflight_se3_amd import scenario as S
    from learningagileflight_se3_amd.engine import Engine
    eng, res = Engine(), {}
    f64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")
    for B in (1024, 8192):
        sb = S.synthetic_batch(B, seed=77)
        a = [f64(sb["ini"]), f64(sb["goal"]), f64(sb["dnn_out"][:, :3]), f64(sb["dnn_out"][:, 3:6]),
             f64(sb["dnn_out"][:, 6])]
        calls = {"ocp_sensitivity": lambda: eng.ocp_sensitivity(*a, want=("x", "u", "dx", "du")),
                 "ocp_sensitivity_ex": lambda: eng.ocp_sensitivity_ex(*a, want=("x", "u", "dx", "du", "gain")),
                 "ocp_solve_rec": lambda: eng.ocp_solve_rec(*a, want=("x", "u"))}
        for name, f in calls.items():
            for _ in range(2):   # the first call warms the shape up
                r = f()
                torch.cuda.synchronize()
                ok = int((r["status"] <= 1).sum())
                del r
            res["B%d %s" % (B, name)] = [eng.last_kernel_ms(), ok]
        # vjp_kernel is no solver launch (it keeps the last solver launch's timing): two events on the launch stream,
        # as tools/gpu_vjp.py
        rec = eng.ocp_solve_rec(*a, want=("x", "u"))
        g = torch.Generator(device="cuda").manual_seed(7)
        g_x = torch.randn(B, eng.horizon + 1, 13, dtype=torch.float64, device="cuda", generator=g)
        g_u = torch.randn(B, eng.horizon, 4, dtype=torch.float64, device="cuda", generator=g)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            ev0.record()
            v = eng.ocp_vjp(*a, None, None, rec["rec"], g_x, g_u)
            ev1.record()
            torch.cuda.synchronize()
        res["B%d ocp_vjp" % B] = [ev0.elapsed_time(ev1), int((v["sens_status"] == 0).sum())]
    with open(out, "w") as fh:
        json.dump(res, fh)


def run_child(mode, lib, out):
    env = dict(os.environ, LAFSE3_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable, os.path.abspath(__file__), mode, out], env=env, check=True, timeout=600)


def identity(parent, cand):
    import numpy as np
    with tempfile.TemporaryDirectory() as d:
        pa, ca = os.path.join(d, "parent.npz"), os.path.join(d, "candidate.npz")
        run_child("child-identity", parent, pa)
        run_child("child-identity", cand, ca)
        P, Cd = dict(np.load(pa)), dict(np.load(ca))
    print("# Bit identity of this tree against its parent commit on the sensitivity, record and adjoint entry points (one")
    print("# MI355X, both builds in one call, each in a process of its own through LAFSE3_LIB): tools/gpu_sens_identity.py")
    print("# identity.  Every returned array compared byte for byte.")
    bad = 0
    assert sorted(P) == sorted(Cd), (sorted(P), sorted(Cd))
    for k in P:
        p, c = P[k], Cd[k]
        head = "[%s] %s %s" % (k, p.dtype, p.shape)
        if p.shape == c.shape and p.dtype == c.dtype and p.tobytes() == c.tobytes():
            print(head, "byte-equal")
            continue
        must = k.split("/")[1] in MUST
        bad += must
        rel = float(np.abs(p.astype(np.float64) - c).max() / max(np.abs(p).max(), 1e-300)) if p.shape == c.shape else None
        print(head, "DIFFERS%s: largest |parent - candidate| / max|parent| = %s, %d of %d entries"
              % (" (must be equal)" if must else "", rel, int((p != c).sum()) if p.shape == c.shape else -1, p.size))
    live = {k: int((v == 0).sum()) for k, v in Cd.items() if k.endswith("/sens_status")}
    print("sens_status == 0 (candidate):", json.dumps(live))
    return 1 if bad else 0


def ab(parent, cand):
    import numpy as np
    runs = {"parent": [], "candidate": []}
    with tempfile.TemporaryDirectory() as d:
        for r in range(ROUNDS):
            for who, lib in (("parent", parent), ("candidate", cand)):
                out = os.path.join(d, "%s%d.json" % (who, r))
                run_child("child-ab", lib, out)
                runs[who].append(json.load(open(out)))
    print("# lafse3_last_kernel_ms of the entry points that changed kernel, parent build and this tree alternating for %d" % ROUNDS)
    print("# rounds in one call (tools/gpu_sens_identity.py ab; each round a process that warms the call up once).  Bar:")
    print("# median(candidate) - median(parent) <= max(parent) - min(parent).")
    miss = 0
    for k in runs["parent"][0]:
        p = [r[k][0] for r in runs["parent"]]
        c = [r[k][0] for r in runs["candidate"]]
        okc = sorted({r[k][1] for r in runs["parent"] + runs["candidate"]})
        dm, spread = float(np.median(c) - np.median(p)), max(p) - min(p)
        verdict = "within" if dm <= spread else "EXCEEDS"
        miss += dm > spread
        print("[%s] parent median %.3f ms %s | candidate median %.3f ms %s | difference %+.3f ms, parent spread %.3f ms: %s"
              " | instances ok: %s" % (k, np.median(p), [round(v, 3) for v in p], np.median(c),
                                                     [round(v, 3) for v in c], dm, spread, verdict, okc))
    return 1 if miss else 0


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "child-identity":
        child_identity(sys.argv[2])
    elif mode == "child-ab":
        child_ab(sys.argv[2])
    else:
        sys.exit({"identity": identity, "ab": ab}[mode](sys.argv[2], sys.argv[3]))
