"""Times the device PNG decode (ops.png_decode, csrc/pngdec.hip) against the host path it replaces, on the GPU machine.

  decode rate: PNGDEC_FILES (64) PIL-written 1024x1024 RGB files of two kinds: a smooth picture plus light noise, and a cartoon-like
               picture with flat regions and outlines
     host route:   PIL (zlib) in one thread from bytes in memory, then the upload of the pixels   (= utils.io_utils.imread)
     device route: ops.png_decode from the same bytes, in chunks of det_batch (CSM_DET_BATCH, 16) files: the chunk walk and the
                   CRCs on the host, the upload of the IDAT payloads, the kernels
  end to end:  AnimeInsSeg('synthetic').infer(directory) frames/s with CSM_DEVICE_DECODE 0 and 1 over the cartoon-like files

Wall times are host clocks around work that ends in a device synchronise, steady state (one warm-up pass per kind), best and all of
PNGDEC_REPS repetitions, the two routes alternating in this one process.  The device route also reports the pointer-doubling rounds
and the host time of the probe.  For the per-kernel split run once under
`rocprofv3 --kernel-trace --stats -- python tools/pngdec_profile.py decode`."""
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, pngread, synth  # noqa: E402


def smooth_picture(H, W, k):
    img = synth.image_u8(H, W, 100 + k).astype(np.float64)                  # smooth shapes plus sensor-like noise
    return np.clip(np.rint(img + np.random.default_rng(k).normal(0, 2.0, img.shape)), 0, 255).astype(np.uint8)


def cartoon_picture(H, W, k):
    """flat regions (discs and boxes over a softly shaded two-tone ground) with dark outlines, as cel shading leaves them; every
    third shape carries a faint texture"""
    rng = np.random.default_rng(1000 + k)
    img = np.empty((H, W, 3), np.int64)
    shade = (np.arange(H) * 24 // H)[:, None, None]
    img[:] = rng.integers(160, 232, 3) + shade
    horizon = (H * 0.6 + 20 * np.sin(np.arange(W) / 90.0)).astype(np.int64)
    ground = np.arange(H)[:, None] > horizon[None, :]
    img[ground] = rng.integers(60, 200, 3)
    for n in range(24):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(H // 40, H // 6))
        colour = rng.integers(0, 250, 3)
        y0, y1, x0, x1 = max(0, cy - r - 4), min(H, cy + r + 4), max(0, cx - 2 * r - 4), min(W, cx + 2 * r + 4)
        y, x = np.mgrid[y0:y1, x0:x1]
        box = img[y0:y1, x0:x1]
        if rng.integers(0, 2):
            d = np.hypot(y - cy, x - cx)
            inside, edge = d < r, (d >= r) & (d < r + 3)
        else:
            inside = (abs(y - cy) < r) & (abs(x - cx) < r * 1.5)
            edge = (abs(y - cy) < r + 3) & (abs(x - cx) < r * 1.5 + 3) & ~inside
        box[inside] = colour
        if n % 3 == 0:
            box[inside] += rng.integers(0, 3, (int(inside.sum()), 3))
        box[edge] = 20
    return np.clip(img, 0, 255).astype(np.uint8)


def make_files(n, H, W, picture):
    from PIL import Image
    out = []
    for k in range(n):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(picture(H, W, k)[:, :, ::-1])).save(buf, 'PNG')
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


def device_route(files, chunk, stats=None):
    out, rounds = [], []
    for c0 in range(0, len(files), chunk):
        st = {}
        out += ops.png_decode(files[c0:c0 + chunk], stats=st)
        rounds += st['rounds']
    torch.cuda.synchronize()
    if stats is not None:
        stats['rounds'] = rounds
    return out


def decode_rate(label, files, chunk, reps):
    host_route(files[:2]); device_route(files[:chunk], chunk)                      # library load, first launches
    host_ms, dev_ms, stats = [], [], {}
    for _ in range(reps):
        t = time.perf_counter(); a = host_route(files); host_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); b = device_route(files, chunk, stats); dev_ms.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    for d in files:
        pngread.zlib_stream(d, pngread.probe(d))
    parse_ms = (time.perf_counter() - t) * 1e3
    diff = max(int((x.int() - y.int()).abs().max()) for x, y in zip(a, b))
    n = len(files)
    fmt = lambda v: " ".join("%.1f" % x for x in v)   # noqa: E731
    print("%s: %d files, %.0f KB each" % (label, n, sum(len(d) for d in files) / n / 1e3))
    print("  host route (PIL one thread + upload): %s ms; best %.2f ms/file = %.1f files/s" % (fmt(host_ms), min(host_ms) / n, n / min(host_ms) * 1e3))
    print("  device route (png_decode, chunks of %d): %s ms; best %.2f ms/file = %.1f files/s; of that about %.2f ms/file of host "
          "chunk walking and CRCs" % (chunk, fmt(dev_ms), min(dev_ms) / n, n / min(dev_ms) * 1e3, parse_ms / n))
    print("  pointer-doubling rounds per chunk (launched, that did work): %s; max |device - imread| = %d; speed-up %.2fx"
          % (stats['rounds'], diff, min(host_ms) / min(dev_ms)))


def end_to_end(files, reps):
    from animeinsseg import AnimeInsSeg
    with tempfile.TemporaryDirectory() as d:
        for k, data in enumerate(files):
            with open(os.path.join(d, 'f%03d.png' % k), 'wb') as f:
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
    n = int(os.environ.get("PNGDEC_FILES", "64"))
    reps = int(os.environ.get("PNGDEC_REPS", "3"))
    chunk = max(1, int(os.environ.get("CSM_DET_BATCH", "16")))
    size = int(os.environ.get("PNGDEC_SIZE", "1024"))
    cartoon = make_files(n, size, size, cartoon_picture)
    if what in ('all', 'decode'):
        decode_rate("smooth picture plus noise", make_files(n, size, size, smooth_picture), chunk, reps)
        decode_rate("cartoon-like picture", cartoon, chunk, reps)
    if what in ('all', 'infer'):
        end_to_end(cartoon, reps)


if __name__ == "__main__":
    main()
