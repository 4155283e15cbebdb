#!/usr/bin/env python3
"""run N bench steps (8 frames each) and nothing else -- for `rocprofv3 --kernel-trace`: how much of a step is the GPU idle?
With --count (a run of its own, not the traced or timed one: the wrappers cost host time) it counts, per measured step, the host
reads that drain a stream (Tensor.tolist / .item / .cpu); the trace of kernels does not show them, tools/glue_window.py takes the
count of stats reads (float64 tensors of 6 columns) from that run's output."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

counts = {"tolist": 0, "item": 0, "cpu": 0, "stats_reads": 0}


def _counted(name):
    orig = getattr(torch.Tensor, name)

    def f(self, *a, **k):
        if self.is_cuda:
            counts[name] += 1
            if name == "tolist" and self.dtype == torch.float64 and self.shape[-1:] == (6,):
                counts["stats_reads"] += 1
        return orig(self, *a, **k)
    setattr(torch.Tensor, name, f)


COUNT = "--count" in sys.argv[1:]
if COUNT:
    for _n in ("tolist", "item", "cpu"):
        _counted(_n)
wl = bench.FrameWorkload(1024, 0, torch.device('cuda'), 8)
for _ in range(3):
    wl.step()
torch.cuda.synchronize()
for k in counts:
    counts[k] = 0
t0 = time.perf_counter()
marker = torch.zeros(3, device='cuda') + 1            # a recognisable tiny kernel right before the measured steps
for _ in range(6):
    wl.step()
torch.cuda.synchronize()
if not COUNT:
    print("6 steps: %.2f ms per step" % ((time.perf_counter() - t0) / 6 * 1e3), flush=True)
else:
    print("host reads per step: " + ", ".join("%s %.1f" % (k, v / 6) for k, v in counts.items()), flush=True)
