"""Compare the device functions of two `hipcc --offload-arch=gfx950 --offload-device-only -S` listings of csrc/api.hip,
function by function: python tools/listing_diff.py parent.s new.s

A function's body is the lines between its `name:` label and its `.Lfunc_end`, with comments, debug directives and
blank lines dropped and the function's ordinal taken out of its local labels (.LBB<ordinal>_<n>), which shifts when
a function is added in front, as does the module-wide counter of the long-branch labels (.Lpost_getpc<n>).  Prints the functions whose bodies differ, those only one side has, and the count of
identical ones; exit status 1 when a function both sides have differs."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and name is None and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or re.match(r"\s*\.(loc|file|cfi_|p2align|section|type|size|globl|protected|weak)\b", line):
            continue
        body.append(re.sub(r"\.L(BB|tmp|JTI|func_begin|func_end|post_getpc)\d+", r".L\1", line))
    return out


def main(a, b):
    fa, fb = functions(a), functions(b)
    same = [n for n in fa if n in fb and fa[n] == fb[n]]
    diff = [n for n in fa if n in fb and fa[n] != fb[n]]
    print("identical:", len(same))
    for n in diff:
        la, lb = fa[n], fb[n]
        nd = sum(1 for x, y in zip(la, lb) if x != y) + abs(len(la) - len(lb))
        print("DIFFERS:", n, len(la), "->", len(lb), "lines,", nd, "differing")
    print("only in", a + ":", sorted(set(fa) - set(fb)))
    print("only in", b + ":", sorted(set(fb) - set(fa)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
