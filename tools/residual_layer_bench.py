#!/usr/bin/env python3
"""time single conv layers with and without a residual input: what does the residual path of an epilogue cost?

For each layer and each res_mode in (0, 1, 2) one program of that one op (tiles autotuned as in a real run), HIP-event time of the op:
min and median of REPS runs.  The excess of a residual layer over its res_mode-0 twin is set against the floor, one extra read of the
output tensor.  Default layers: the four ISNet RSU closing shapes at batch 16 and the LeReS / ResNeXt 8 x 40^2 1024 -> 1024 1x1.

usage: tools/residual_layer_bench.py [n h w cin cout k]...      (six integers per layer; CSM_LIB=<path> times another build)
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cartoonsegmentation_amd.program import Program, CONV_FLAG_WINOGRAD4
from cartoonsegmentation_amd.runtime import CompiledProgram

LAYERS = [(16, 360, 360, 32, 64, 3), (16, 360, 360, 64, 64, 3), (16, 180, 180, 64, 128, 3), (16, 90, 90, 128, 256, 3),
          (8, 40, 40, 1024, 1024, 1)]
REPS = 12
HBM_GBS = 5000.0      # rate of a streaming read at these sizes (profiles/r06_elementwise.txt), for the "floor" column


def time_layer(n, h, w, cin, cout, k, res_mode):
    p = Program("l")
    x = p.buffer(n, h, w, cin); x.buf.first = 0
    r = None
    if res_mode:
        r = p.buffer(n, h, w, cout); r.buf.first = 0
    wt = (np.random.default_rng(0).standard_normal((cout, cin, k, k)) * 0.05).astype(np.float32)
    p.conv(x, wt, np.zeros(cout, np.float32), pad=k // 2, act='relu', res=r, res_mode=res_mode)
    p.plan()
    cp = CompiledProgram(p, 'cuda')
    cp.workspace.normal_()
    cp.run(); cp.run()
    t = sorted(cp.profile()[0] for _ in range(REPS))
    kind = "wino4" if p.ops[0]['flags'] & CONV_FLAG_WINOGRAD4 else "direct"
    return t[0] * 1e3, t[len(t) // 2] * 1e3, kind


def main():
    v = [int(a) for a in sys.argv[1:]]
    layers = [tuple(v[i:i + 6]) for i in range(0, len(v), 6)] if v else LAYERS
    print("library:", os.environ.get("CSM_LIB", "in-tree"))
    print("%-28s %-6s %4s %10s %10s %10s %9s" % ("layer", "kernel", "res", "min us", "median us", "excess us", "floor us"))
    for (n, h, w, cin, cout, k) in layers:
        floor = n * h * w * cout * 4 / (HBM_GBS * 1e3)
        base = None
        for rm in (0, 1, 2):
            lo, med, kind = time_layer(n, h, w, cin, cout, k, rm)
            base = lo if rm == 0 else base
            print("%-28s %-6s %4d %10.1f %10.1f %10s %9.1f" % ("%dx%dx%d %d->%d k%d" % (n, h, w, cin, cout, k), kind, rm, lo, med,
                                                                "" if rm == 0 else "%.1f" % (lo - base), floor))
            sys.stdout.flush()


if __name__ == '__main__':
    main()
