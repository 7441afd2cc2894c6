#!/usr/bin/env python3
"""The ISA comparison of profiles/csrc_dedup_isa_compare.txt: every .hip file of gpexp_amd/csrc, parent commit against a change.

In both trees, for every x.hip of gpexp_amd/csrc (the line profiles/strassen2_isa_compare.py documents, plus the resource remarks):
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast --cuda-device-only -S x.hip -o OUT/x.s \
          -Rpass-analysis=kernel-resource-usage 2> OUT/x.res
    python profiles/csrc_dedup_isa_report.py PARENT_OUT CHANGE_OUT > profiles/csrc_dedup_isa_compare.txt

Per file: the output of strassen2_isa_compare.py as it is.  Under every DIFFERENT line, derived here from the same listings: whether
the opcodes (operands dropped) and the floating-point opcodes among them come in the same order, and the register / scratch
figures of both builds from the .res files (parent | change).
"""
import os
import re
import subprocess
import sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from strassen2_isa_compare import functions
P, Cg = sys.argv[1].rstrip('/') + '/', sys.argv[2].rstrip('/') + '/'
def res(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r'Function Name: (\S+)', l)
        if m: cur = m.group(1); out[cur] = {}; continue
        m = re.search(r'remark:\s+([^:]+?): (\S+) \[', l)
        if m and cur: out[cur][m.group(1).strip()] = m.group(2)
    return out
FP = re.compile(r'^v_(add|mul|fma|fmac|div|rcp|rsq|sqrt|exp|log|ldexp|frexp|cmp|cmpx|max|min|trig|fract|floor|ceil|rndne|cvt|cndmask)\w*_f(16|32|64)|^v_\w+_f64|^v_\w+_f32')
def ops(body): return [t.split()[0] for t in body if not t.endswith(':')]
def fpops(body): return [o for o in ops(body) if FP.match(o)]
lines = []
w = lines.append
w("ISA of every translation unit of gpexp_amd/csrc, parent commit against this change (gfx950):")
w("    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast --cuda-device-only -S x.hip -o x.s -Rpass-analysis=kernel-resource-usage")
w("    python profiles/csrc_dedup_isa_report.py PARENT_OUT CHANGE_OUT   (runs profiles/strassen2_isa_compare.py per file and adds the indented lines)")
w("For every function that differs: instruction counts (parent, change), whether the opcode sequence and the sequence of floating-point")
w("opcodes are the same, and VGPRs / SGPRs / scratch / spills of both builds.")
w("")
for f in ['kfill','gemm_f64','chol','reduce','dist','fitc','loo','api','design','hyper','grad','acq','sample','paths','vfe_design']:
    w("== %s.hip" % f)
    out = subprocess.run([sys.executable, os.path.join(HERE, 'strassen2_isa_compare.py'), P+f+'.s', Cg+f+'.s'], capture_output=True, text=True).stdout
    a, b = functions(P+f+'.s'), functions(Cg+f+'.s')
    ra, rb = res(P+f+'.res'), res(Cg+f+'.res')
    for l in out.splitlines():
        w(l)
        if l.startswith('DIFFERENT'):
            n = l.split()[1]
            oa, ob = ops(a[n]), ops(b[n]); fa, fb = fpops(a[n]), fpops(b[n])
            def g(r, k): return r.get(n, {}).get(k, '?')
            w("          opcode sequence %s; floating-point opcodes %s (%d | %d); VGPRs %s | %s; SGPRs %s | %s; scratch %s | %s; VGPR spills %s | %s"
              % ("SAME (operands renamed only)" if oa == ob else "differs", "SAME in the same order" if fa == fb else "differ", len(fa), len(fb),
                 g(ra,'VGPRs'), g(rb,'VGPRs'), g(ra,'TotalSGPRs'), g(rb,'TotalSGPRs'), g(ra,'ScratchSize [bytes/lane]'), g(rb,'ScratchSize [bytes/lane]'),
                 g(ra,'VGPRs Spill'), g(rb,'VGPRs Spill')))
sys.stdout.write('\n'.join(lines) + '\n')
