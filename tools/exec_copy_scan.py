"""Flag vector copies that a `hipcc --offload-arch=gfx950 --offload-device-only -S` listing places at the top of a block
before the instruction that switches lanes back on (s_or_b64 exec, exec, ..): they run under the mask of the region
that just ended, with no lane active behind a lane-retiring loop ("A compiler trap").

    python tools/exec_copy_scan.py api.s "vjp_kernel|ipm_kernel"      (listing, regex on the function names)

A hit is a block label and the copies in front of its exec restore.  A move of a constant is harmless; a copy of a
value that is read later (v_accvgpr_write, a scratch store) is the trap."""
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
name, block, pre, hits = None, None, [], {}
for line in open(path, errors="replace"):
    m = re.match(r"^([A-Za-z_][\w$.]*):", line)
    if m and not m.group(1).startswith(".L"):
        name = m.group(1)
        block, pre = None, []
        continue
    if name is None or not re.search(pat, name):
        continue
    if line.startswith(".Lfunc_end"):
        name = None
        continue
    m = re.match(r"^(\.LBB\d+_\d+):", line)
    if m:
        block, pre = m.group(1), []
        continue
    ins = line.split(";")[0].strip()
    if not ins or block is None:
        continue
    if re.match(r"s_or_b64 exec, exec", ins):
        bad = [i for i in pre if re.match(r"(v_accvgpr_write|scratch_store|v_mov_b32|v_accvgpr_read|buffer_store)", i)]
        if bad:
            hits.setdefault(name, []).append((block, bad))
        block = None
        continue
    if re.match(r"(s_cbranch|s_branch|s_swappc|s_setpc|s_endpgm)", ins) or "exec" in ins:
        block = None
        continue
    pre.append(ins)
for n, h in hits.items():
    print(n, len(h), "blocks")
    for b, bad in h[:12]:
        print("   ", b, bad[:6])
print("functions with hits:", len(hits))
