"""Bit identity of two builds of liblafse3 on the bench workloads:
    python tools/gpu_identity.py PARENT.so [CANDIDATE.so [LOG]]

Runs bench.py --steps 3 --dump-outputs in the default mode, with --grad-mode ift and with the moving-gate workload, once
per library (LAFSE3_LIB, a child process each, under its own time limit), compares every saved array byte for byte and
the JSON line's iteration, status, restoration and checksum fields, and writes the log to LOG (identity.log in the
current directory when not given) and to standard output.  Stops at the first child that fails; exit status 1 when
anything differs."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ([], ["--grad-mode", "ift"], ["--workload", "moving", "--batch", "256", "--plant-steps", "100"])
FIELDS = ("ipm_iterations_per_solve", "ipm_iterations", "status_hist", "restoration", "dnn1_param_checksum")


def run(lib, mode, out):
    env = dict(os.environ, LAFSE3_LIB=lib)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--no-extra", "--no-cpu-baseline",
           "--dump-outputs", out] + mode
    p = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=400)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit(f"bench.py {' '.join(mode)} with {lib}: exit status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    parent = os.path.abspath(sys.argv[1])
    cand = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(
        REPO, "learningagileflight_se3_amd", "liblafse3.so")
    log = sys.argv[3] if len(sys.argv) > 3 else "identity.log"
    lines = ["# Bit identity of this tree against its parent commit on the bench workloads (one MI355X, both builds in "
             "one call).", "# Each command run with the parent's liblafse3.so and with this tree's (LAFSE3_LIB), "
             "--dump-outputs DIR; every saved", "# array compared byte for byte, and the JSON line's iteration, status, "
             "restoration and checksum fields for equality."]
    bad = 0
    for mode in MODES:
        tag = "[bench.py --steps 3 " + " ".join(mode) + "]"
        with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
            ja, jb = run(parent, mode, da), run(cand, mode, db)
            names = sorted(set(os.listdir(da)) | set(os.listdir(db)))
            for n in names:
                if not n.endswith(".npy"):
                    continue
                try:
                    a, b = np.load(os.path.join(da, n)), np.load(os.path.join(db, n))
                    same = a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                    lines.append(f"{tag} {n} {a.dtype} {a.shape} " + ("byte-equal" if same else "DIFFERENT"))
                except OSError as e:
                    same = False
                    lines.append(f"{tag} {n} MISSING ({e})")
                bad += not same
        for f in FIELDS:
            if f not in ja and f not in jb:
                continue
            same = ja.get(f) == jb.get(f)
            bad += not same
            lines.append(f"{tag} {f} " + (f"equal: {json.dumps(ja.get(f))}" if same else
                                           f"DIFFERENT: parent {json.dumps(ja.get(f))} candidate {json.dumps(jb.get(f))}"))
        lines.append(f"{tag} kernel_ms parent {ja.get('kernel_ms')} candidate {jb.get('kernel_ms')}; value parent "
                     f"{ja.get('value')} candidate {jb.get('value')}")
    text = "\n".join(lines) + "\n"
    with open(log, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
