#!/usr/bin/env python3
"""Compare the gfx950 ISA of two builds of a .hip file, function by function.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast --cuda-device-only -S x.hip -o x.s   (both trees)
    python profiles/strassen2_isa_compare.py parent/x.s change/x.s [--loop NEW_SUBSTR REF_SUBSTR]

Every function the first file has must be in the second one with the same instructions (comments, blank lines and the
function index inside basic-block labels aside).  --loop: the k-loop (the basic block with the most MFMAs) of the function
whose mangled name contains NEW_SUBSTR against that of REF_SUBSTR, both in the second file, opcode for opcode.
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L") and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";", 1)[0].strip()
            if not t or t.startswith((".p2align", ".loc", ".cfi", ".file")):
                continue
            body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
    return out


def k_loop(body):
    blocks, cur = [], []
    for t in body:
        if t.startswith(".LBB_") and t.endswith(":"):
            blocks.append(cur)
            cur = []
        else:
            cur.append(t)
    blocks.append(cur)
    return max(blocks, key=lambda b: sum(1 for t in b if t.startswith("v_mfma")))


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name in sorted(a):
        if name not in b:
            print("MISSING  ", name)
            bad += 1
        elif a[name] != b[name]:
            print("DIFFERENT", name, len(a[name]), len(b[name]))
            bad += 1
    print("%d functions in the first file, %d identical in the second, %d new: %s"
          % (len(a), len(a) - bad, len(set(b) - set(a)), " ".join(sorted(set(b) - set(a)))))
    if "--loop" in sys.argv:
        i = sys.argv.index("--loop")
        new = [n for n in b if sys.argv[i + 1] in n]
        ref = [n for n in b if sys.argv[i + 2] in n]
        assert len(new) == 1 and len(ref) == 1, (new, ref)
        ln, lr = k_loop(b[new[0]]), k_loop(b[ref[0]])
        on, orr = [t.split()[0] for t in ln], [t.split()[0] for t in lr]
        print("k-loop of %s: %d instructions, %d MFMAs; of %s: %d, %d; opcode for opcode: %s"
              % (new[0], len(on), sum(o.startswith("v_mfma") for o in on), ref[0], len(orr),
                 sum(o.startswith("v_mfma") for o in orr), "IDENTICAL" if on == orr else "DIFFERENT"))
        for j in range(min(len(on), len(orr))):
            if on[j] != orr[j]:
                print("  position %d: %s   |   %s" % (j, ln[j], lr[j]))
        bad += on != orr
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
