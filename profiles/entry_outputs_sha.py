#!/usr/bin/env python3
"""sha256 of the raw output bytes of every entry of tests/test_gpu_scratch_balance.py (its ENTRIES table, its shapes, its fixed
seeds) -- the comparison behind profiles/csrc_dedup_ab.txt and profiles/err_ladders_ab.txt.  Needs an MI355X.

    python profiles/entry_outputs_sha.py > A.txt                                   one line per entry, in a fresh process
    GPX_LIB_PATH=/path/to/another/libgpx_hip.so python profiles/entry_outputs_sha.py > B.txt
    GPX_CROSS_BYTES=1 python profiles/entry_outputs_sha.py --skip ivar_keep+ivar_update > A1.txt     chunks of 128 (the kept solve
                                                                                   exists for one chunk only)
    python profiles/entry_outputs_sha.py A.txt B.txt                               side by side, EQUAL / DIFFERENT per entry

What an entry returns is hashed as it comes: arrays and scalars as float64 / int64 bytes, a device matrix as its logical
contents, a FITC model as its log-determinant and dense covariance / precision; everything is freed afterwards.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)   # behind PYTHONPATH: another checkout of the package may be put in front


def feed(h, obj):
    from gpexp_amd import device as dev
    if obj is None:
        return
    if isinstance(obj, dev.DeviceMatrix):
        h.update(obj.to_host().tobytes())
    elif isinstance(obj, dev.FitcModel):
        h.update(np.asarray(obj.logdet()).tobytes())
        for a in obj.dense():
            h.update(a.tobytes())
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            feed(h, o)
    else:
        h.update(np.ascontiguousarray(obj).tobytes())


def main():
    if len(sys.argv) == 3 and "--skip" not in sys.argv:
        a, b = (dict(l.split() for l in open(p) if l.strip()) for p in sys.argv[1:])
        for name in a:
            print("%-28s %-10s parent %s  change %s" % (name, "EQUAL" if a[name] == b.get(name) else "DIFFERENT", a[name], b.get(name)))
        print("%d entry points, %d equal" % (len(a), sum(a[n] == b.get(n) for n in a)))
        return 0 if all(a[n] == b.get(n) for n in a) and len(a) == len(b) else 1
    sys.path.append(os.path.join(ROOT, "tests"))
    import test_gpu_scratch_balance as t
    skip = sys.argv[sys.argv.index("--skip") + 1].split(",") if "--skip" in sys.argv else []
    for name, make, n in t.ENTRIES:
        if name in skip:
            continue
        ctx, call = make(n)
        out = call()
        h = hashlib.sha256()
        feed(h, out)
        t.release(ctx, out)
        print("%s-N%d %s" % (name, n, h.hexdigest()[:16]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
