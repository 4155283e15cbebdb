#!/usr/bin/env python3
"""time one conv layer under every tile configuration: args n h w cin cout k [stride dil groups]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cartoonsegmentation_amd.program import Program
from cartoonsegmentation_amd.runtime import CompiledProgram, conv_cfg_table
from cartoonsegmentation_amd import _lib
v = [int(x) for x in sys.argv[1:]]
n, h, w, cin, cout, k = v[:6]
s, d, g = (v[6:] + [1, 1, 1])[:3] if len(v) > 6 else (1, 1, 1)
p = Program("l"); x = p.buffer(n, h, w, cin)
W = (np.random.default_rng(0).standard_normal((cout, cin // g, k, k)) * 0.05).astype(np.float32)
p.conv(x, W, np.zeros(cout, np.float32), stride=s, pad=d * (k // 2), dil=d, groups=g, act='relu'); p.plan()
os.environ["CSM_AUTOTUNE"] = "0"
cp = CompiledProgram(p, 'cuda'); cp.workspace.normal_()
if os.environ.get('ZERO') == '1':      # all-zero operands: same instruction stream, minimum switching power (DVFS check)
    cp.workspace.zero_(); cp.weights.zero_()
L = _lib.load()
names = [c['name'] for c in conv_cfg_table()]
print("ksplit", p.ops[0]['ksplit'], "GFLOP %.2f" % (p.flops / 1e9))
for cfg in range(len(names)):
    L.csm_debug_force_conv_cfg(cfg); cp.run()
    ms = min(cp.profile()[0] for _ in range(4))
    print("cfg %2d %-12s %9.1f us  %6.1f TF/s" % (cfg, names[cfg], ms * 1e3, p.flops / ms / 1e9))
