#!/usr/bin/env python3
"""The WebP writer on a clip of 75 different cartoon frames of 1024x1024 at quality 90 (tests/test_mjpeg.py's `cartoon`, seeds 0..74):
HIP events around every stage of csm_webp_measure (csm_webp_stage) and csm_webp_write for one chunk of frames, the wall time of
ops.webp_streams for the whole clip and for one still, and the same through Pillow's WebP encoder (method 4) on the host.  Every
figure is the median of REPEATS timed passes after one warm-up pass; the smallest and largest are printed beside it.
--method 1 times the second coding method (B_PRED and probability updates; its stage 3 is the counts, the tables
and the coder); --no-pillow leaves the host encoder out (for a second run in the same session).
Usage: time_webp.py [--method 0|1] [--no-pillow] [frames [side [repeats]]]"""
import io, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
from PIL import Image
from test_mjpeg import cartoon
from cartoonsegmentation_amd import _lib, ops, webpcode
from cartoonsegmentation_amd._lib import check, i32, i64, ptr, stream_ptr

argv = list(sys.argv[1:])
METHOD = 0
if '--method' in argv:
    at = argv.index('--method')
    METHOD = webpcode.check_method(int(argv[at + 1]), "time_webp")
    del argv[at:at + 2]
PILLOW = '--no-pillow' not in argv
argv = [a for a in argv if a != '--no-pillow']
n = int(argv[0]) if len(argv) > 0 else 75
side = int(argv[1]) if len(argv) > 1 else 1024
REPEATS = int(argv[2]) if len(argv) > 2 else 5
Q = 90
clip = np.stack([cartoon(side, side, seed=v) for v in range(n)])


def report(label, times, extra=""):
    t = sorted(times)
    print("%-58s median %9.2f ms  (min %.2f, max %.2f, %d passes)%s" % (label, t[len(t) // 2], t[0], t[-1], len(t), extra))


dev = torch.from_numpy(clip).cuda()
L = _lib.load()

# one chunk, stage by stage
per_frame = L.csm_webp_scratch_bytes_m(i32(1), i32(side), i32(side), i32(METHOD))
k = max(1, min(n, ops.WEBP_SCRATCH_BYTES // per_frame))
units = webpcode.partitions(side) + 1
info = torch.empty((k * units + 1, 2), dtype=torch.int64, device='cuda')
scratch = torch.empty(L.csm_webp_scratch_bytes_m(i32(k), i32(side), i32(side), i32(METHOD)), dtype=torch.uint8, device='cuda')
names = {1: 'colour', 2: 'macroblocks', 3: 'coder (counts, tables, code)' if METHOD else 'coder', 4: 'sizes'}
stage_ms = {name: [] for name in list(names.values()) + ['write']}
for rep in range(REPEATS + 1):                                                        # the first pass warms up
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    ev[0].record()
    for stage in (1, 2, 3, 4):
        check(L.csm_webp_stage_m(i32(stage), ptr(dev), i32(k), i32(side), i32(side), i32(Q), i32(METHOD), ptr(info), ptr(scratch), stream_ptr()),
              names[stage])
        ev[stage].record()
    total = int(info.cpu().numpy()[-1, 1])
    blob = torch.empty(total, dtype=torch.uint8, device='cuda')
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    check(L.csm_webp_write_m(i32(k), i32(side), i32(side), i32(METHOD), ptr(blob), i64(total), ptr(scratch), stream_ptr()), "write")
    ev[5].record()
    torch.cuda.synchronize()
    if rep:
        for stage in (1, 2, 3, 4):
            stage_ms[names[stage]].append(ev[stage - 1].elapsed_time(ev[stage]))
        stage_ms['write'].append(e0.elapsed_time(ev[5]))
print("method %d, one chunk of %d frames of %dx%d (scratch %.0f MB, %.1f MB per frame), %d bytes out:" % (METHOD, k, side, side, scratch.numel() / 2 ** 20, per_frame / 2 ** 20, total))
for name, times in stage_ms.items():
    report("  " + name, times)
del scratch, blob

for what, frames in (("clip of %d frames" % n, dev), ("one still", dev[:1])):
    times = []
    for rep in range(REPEATS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        streams = ops.webp_streams(frames, quality=Q, method=METHOD)[0]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    report("ops.webp_streams(method=%d), %s" % (METHOD, what), times[1:], ", %d bytes" % sum(len(s) for s in streams))

for what, frames in (("clip of %d frames" % n, clip), ("one still", clip[:1])) if PILLOW else ():
    ims = [Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])) for f in frames]
    times = []
    for rep in range(REPEATS + 1 if len(ims) == 1 else min(REPEATS, 3)):               # the clip: no warm-up, at most 3 passes
        t = time.perf_counter()
        buf = io.BytesIO()
        ims[0].save(buf, 'WEBP', save_all=True, append_images=ims[1:], quality=Q, method=4, duration=40)
        times.append((time.perf_counter() - t) * 1e3)
    report("Pillow WebP on the host (method 4), %s" % what, times[1:] if len(ims) == 1 else times, ", %d bytes" % len(buf.getvalue()))
