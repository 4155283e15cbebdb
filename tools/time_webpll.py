"""Times the lossless WebP writer against the host alternative, for the two loads it is for.

  case 1: 100 instance cut-outs with transparency from one 1024x1024 frame
      route A (device): ops.cutout_bgra + ops.webp_encode_lossless; only the box table, the histograms and the files cross to the host
      route B (host):   masks.cpu() and frame.cpu(), the numpy composition, then Pillow save(lossless=True, method=0) in one thread
  case 2: 21 opaque 1024x1024 frames: ops.webp_encode_lossless against ops.png_encode

Prints the median and the spread (min .. max) of WEBPLL_REPS passes (default 5) after a warm-up, the bytes that cross PCIe on
each route, the host time spent building the prefix codes, and the file sizes.  Run once under
`rocprofv3 --kernel-trace --stats -- python tools/time_webpll.py` for the per-kernel split."""
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, synth, webpcode  # noqa: E402
from png_profile import instance_masks, video_frames  # noqa: E402


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return out, ms


def show(ms):
    return "median %.1f ms (min %.1f .. max %.1f, %d passes)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def host_cutouts(frame, masks):
    """route B: everything on the host from the copied masks and frame"""
    from PIL import Image
    img, m = frame.cpu().numpy(), masks.cpu().numpy()
    files = []
    for k in range(m.shape[0]):
        ys, xs = np.nonzero(m[k])
        if ys.size == 0:
            continue
        y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        a = m[k, y0:y1, x0:x1]
        rgba = np.concatenate([np.where(a[..., None], img[y0:y1, x0:x1, ::-1], 0), (a * 255).astype(np.uint8)[..., None]], axis=2)
        buf = io.BytesIO()
        Image.fromarray(rgba.astype(np.uint8), 'RGBA').save(buf, 'WEBP', lossless=True, method=0)
        files.append(buf.getvalue())
    return files


def main():
    reps = int(os.environ.get("WEBPLL_REPS", "5"))
    n = int(os.environ.get("WEBPLL_CUTOUTS", "100"))
    frame = torch.from_numpy(synth.image_u8(1024, 1024, 3)).cuda()
    masks = instance_masks(n)

    def device_cutouts():
        cuts = [c for c in ops.cutout_bgra(frame, masks) if c is not None]
        return cuts, ops.webp_encode_lossless(cuts)

    device_cutouts()                                            # library load, first-launch costs
    host_cutouts(frame, masks[:2])
    (cuts, files), dev_ms = timed(device_cutouts, reps)
    _, compose_ms = timed(lambda: ops.cutout_bgra(frame, masks), reps)
    pil, host_ms = timed(lambda: host_cutouts(frame, masks), reps)
    _, copy_ms = timed(lambda: (masks.cpu(), frame.cpu()), reps)
    pixels = sum(int(c.shape[0] * c.shape[1]) for c in cuts)
    print("case 1: %d cut-outs (%d non-empty, %.1f Mpx in all) from one 1024x1024 frame" % (n, len(cuts), pixels / 1e6))
    print("  route A (cutout_bgra + webp_encode_lossless): %s; the composition alone: %s" % (show(dev_ms), show(compose_ms)))
    print("  route B (copy + numpy + Pillow lossless method=0, one thread): %s; the copy alone: %s" % (show(host_ms), show(copy_ms)))
    table = 2 * webpcode.LL_SYMS * 4 * len(cuts)
    print("  bytes over PCIe: route A %d to the host (files %d + histograms %d + boxes %d) and %d to the device (code tables, "
          "descriptors, jobs); route B %d to the host" % (sum(len(f) for f in files) + table + 16 * n, sum(len(f) for f in files), table, 16 * n,
                                                        2 * webpcode.LL_TABLE_WORDS * 4 * len(cuts) + 128 * len(cuts), masks.numel() + frame.numel()))
    print("  file bytes: ours %d, Pillow method=0 %d (ratio %.3f)" % (sum(len(f) for f in files), sum(len(f) for f in pil),
                                                                     sum(len(f) for f in files) / max(1, sum(len(f) for f in pil))))
    spent, real = [0.0], webpcode.ll_image_code

    def clocked(*args):
        t = time.perf_counter()
        out = real(*args)
        spent[0] += time.perf_counter() - t
        return out
    webpcode.ll_image_code = clocked                            # one more pass with the host's code building clocked
    try:
        device_cutouts()
    finally:
        webpcode.ll_image_code = real
    print("  of route A about %.1f ms is the host building the prefix codes and header bits" % (spent[0] * 1e3))
    print("  route B / route A = %.2fx" % (statistics.median(host_ms) / statistics.median(dev_ms)))

    frames = video_frames(int(os.environ.get("WEBPLL_FRAMES", "21")))
    ops.webp_encode_lossless(frames[:1]); ops.png_encode(frames[:1])
    webp, webp_ms = timed(lambda: ops.webp_encode_lossless(frames), reps)
    png, png_ms = timed(lambda: ops.png_encode(frames), reps)
    print("case 2: %d opaque frames %s" % (int(frames.shape[0]), tuple(frames.shape[1:])))
    print("  webp_encode_lossless: %s, %d bytes" % (show(webp_ms), sum(len(f) for f in webp)))
    print("  png_encode:           %s, %d bytes" % (show(png_ms), sum(len(f) for f in png)))


if __name__ == "__main__":
    main()
