"""Times the device JPEG decode (ops.jpeg_decode, csrc/jpegdec.hip) against the host path it replaces, on the GPU machine.

  decode rate: JPEGDEC_FILES (64) PIL-written 1024x1024 files without restart markers, at 4:2:0 quality 90 and 4:4:4 quality 95
     host route:   PIL (libjpeg-turbo) in one thread from bytes in memory, then the upload of the pixels   (= utils.io_utils.imread)
     device route: ops.jpeg_decode from the same bytes, in chunks of det_batch (CSM_DET_BATCH, 16) files: the marker parse and the
                   table building on the host, the upload of the entropy bytes, the kernels
  end to end:  AnimeInsSeg('synthetic').infer(directory) frames/s with CSM_DEVICE_DECODE 0 and 1 over the 4:2:0 files

Wall times are host clocks around work that ends in a device synchronise, steady state (one warm-up pass per shape), best and
all of JPEGDEC_REPS repetitions, the two routes alternating.  The device route also reports the synchronisation passes between
workgroups and the host time of probe + tables.  For the per-kernel split run once under
`rocprofv3 --kernel-trace --stats -- python tools/jpegdec_profile.py decode`.

  progressive: `python tools/jpegdec_profile.py progressive` is the decode rate over the same pictures written as progressive files
     (PIL's scan script), the device route being ops.jpeg_decode(..., progressive=True) (csrc/jpegprog.hip); it
     also times one file alone, whose refinement scans run on one lane each, and all files in ONE call with the scratch budget
     (ops.JPEG_DECODE_SCRATCH_BYTES, by default 64 MiB: about ten 1024x1024 files) raised to 2 GiB: the refinement scans of all
     files then run side by side.  Per-kernel split: the same rocprofv3 line with `progressive`."""
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import jpegcode, ops, synth  # noqa: E402


def make_files(n, H, W, quality, subsampling, progressive=False):
    from PIL import Image
    out = []
    for k in range(n):
        img = synth.image_u8(H, W, 100 + k).astype(np.float64)              # smooth shapes plus sensor-like noise: files of a few 100 KB
        img = np.clip(np.rint(img + np.random.default_rng(k).normal(0, 2.0, img.shape)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, 'JPEG', quality=quality, subsampling=subsampling, progressive=progressive)
        out.append(buf.getvalue())
    return out


def host_route(files):
    from PIL import Image
    out = []
    for d in files:
        im = Image.open(io.BytesIO(d))
        out.append(torch.from_numpy(np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])).cuda())
    torch.cuda.synchronize()
    return out


def device_route(files, chunk, stats=None, progressive=False):
    out, passes = [], []
    for c0 in range(0, len(files), chunk):
        st = {}
        out += ops.jpeg_decode(files[c0:c0 + chunk], stats=st, progressive=progressive)
        passes += st['progressive_passes' if progressive else 'passes']
    torch.cuda.synchronize()
    if stats is not None:
        stats['passes'] = passes
    return out


def decode_rate(label, files, chunk, reps, progressive=False):
    host_route(files[:2]); device_route(files[:chunk], chunk, None, progressive)                      # library load, first launches
    host_ms, dev_ms, stats = [], [], {}
    for _ in range(reps):
        t = time.perf_counter(); a = host_route(files); host_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); b = device_route(files, chunk, stats, progressive); dev_ms.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    for d in files:
        if progressive:
            jpegcode.scan_tables(jpegcode.probe(d, progressive=True))
        else:
            jpegcode.file_tables(jpegcode.probe(d))
    parse_ms = (time.perf_counter() - t) * 1e3
    diff = max(int((x.int() - y.int()).abs().max()) for x, y in zip(a, b))
    n = len(files)
    fmt = lambda v: " ".join("%.1f" % x for x in v)   # noqa: E731
    print("%s: %d files, %.0f KB each" % (label, n, sum(len(d) for d in files) / n / 1e3))
    print("  host route (PIL one thread + upload): %s ms; best %.2f ms/file = %.1f files/s" % (fmt(host_ms), min(host_ms) / n, n / min(host_ms) * 1e3))
    print("  device route (jpeg_decode, chunks of %d): %s ms; best %.2f ms/file = %.1f files/s; of that about %.2f ms/file of host "
          "parsing and table building" % (chunk, fmt(dev_ms), min(dev_ms) / n, n / min(dev_ms) * 1e3, parse_ms / n))
    print("  synchronisation passes between workgroups per chunk: %s; max |device - PIL| = %d; speed-up %.2fx"
          % (stats['passes'], diff, min(host_ms) / min(dev_ms)))
    if progressive:
        one_h, one_d = [], []
        for _ in range(max(reps, 3)):
            t = time.perf_counter(); host_route(files[:1]); one_h.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); device_route(files[:1], 1, None, True); one_d.append((time.perf_counter() - t) * 1e3)
        print("  one file alone: host route %s ms, device route %s ms" % (fmt(one_h), fmt(one_d)))
        budget, ops.JPEG_DECODE_SCRATCH_BYTES = ops.JPEG_DECODE_SCRATCH_BYTES, 2 << 30
        try:
            all_ms, st = [], {}
            for _ in range(reps):
                t = time.perf_counter()
                ops.jpeg_decode(files, stats=st, progressive=True)
                torch.cuda.synchronize()
                all_ms.append((time.perf_counter() - t) * 1e3)
        finally:
            ops.JPEG_DECODE_SCRATCH_BYTES = budget
        print("  all %d files in one call, scratch budget 2 GiB (%d chunk): %s ms; best %.2f ms/file = %.1f files/s; speed-up %.2fx"
              % (n, len(st['levels']), fmt(all_ms), min(all_ms) / n, n / min(all_ms) * 1e3, min(host_ms) / min(all_ms)))


def end_to_end(files, reps):
    from animeinsseg import AnimeInsSeg
    with tempfile.TemporaryDirectory() as d:
        for k, data in enumerate(files):
            with open(os.path.join(d, 'f%03d.jpg' % k), 'wb') as f:
                f.write(data)
        nets = {}
        for flag in ('0', '1'):
            os.environ['CSM_DEVICE_DECODE'] = flag
            nets[flag] = AnimeInsSeg('synthetic', refine_kwargs={'refine_method': 'none'})
            nets[flag].infer(d)                                                    # programs, first launches
        torch.cuda.synchronize()
        fps = {'0': [], '1': []}
        for _ in range(reps):
            for flag in ('0', '1'):
                t = time.perf_counter()
                nets[flag].infer(d)
                torch.cuda.synchronize()
                fps[flag].append(len(files) / (time.perf_counter() - t))
        for flag in ('0', '1'):
            print("infer(directory of %d files) with CSM_DEVICE_DECODE=%s: %s frames/s (best %.1f)"
                  % (len(files), flag, " ".join("%.1f" % v for v in fps[flag]), max(fps[flag])))


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    n = int(os.environ.get("JPEGDEC_FILES", "64"))
    reps = int(os.environ.get("JPEGDEC_REPS", "3"))
    chunk = max(1, int(os.environ.get("CSM_DET_BATCH", "16")))
    size = int(os.environ.get("JPEGDEC_SIZE", "1024"))
    if what == 'progressive':
        decode_rate("progressive 4:2:0 quality 90", make_files(n, size, size, 90, 2, True), chunk, reps, True)
        decode_rate("progressive 4:4:4 quality 95", make_files(n, size, size, 95, 0, True), chunk, reps, True)
        return
    f420 = make_files(n, size, size, 90, 2)
    if what in ('all', 'decode'):
        decode_rate("4:2:0 quality 90", f420, chunk, reps)
        decode_rate("4:4:4 quality 95", make_files(n, size, size, 95, 0), chunk, reps)
    if what in ('all', 'infer'):
        end_to_end(f420, reps)


if __name__ == "__main__":
    main()
