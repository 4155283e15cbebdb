"""Times ops.png_encode against the host alternative, for the two loads the PNG writer is for: 75 colour frames of 1024x1024 and
100 instance masks of 1024x1024 on the device.

  device route: ops.png_encode(images) = filter, parse, histogram on the device, the codes on the host, the bits on the device,
                the copy of the compressed bytes
  host route:   images.cpu().numpy(), then PIL (zlib) writing every image with compress_level=1 in one thread

Prints both wall times (steady state, best of PNG_REPS), the bytes that cross to the host on either route, the host time spent
building the codes, and the file sizes.  Run once under `rocprofv3 --kernel-trace --stats -- python tools/png_profile.py` for the
per-kernel split."""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, pngcode, synth  # noqa: E402


def video_frames(n=75, H=1024, W=1024):
    """a zoom-and-pan over one synthetic picture, as the frame loop leaves it: uint8 [n,H,W,3] on the device"""
    src = torch.from_numpy(synth.image_u8(H + 128, W + 128, 3)).cuda().permute(2, 0, 1)[None].float()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device='cuda')
    for k in range(n):
        c = 128 * k // max(n - 1, 1)
        crop = src[:, :, c // 2:H + 128 - (c - c // 2), c // 2:W + 128 - (c - c // 2)]
        out[k] = torch.nn.functional.interpolate(crop, size=(H, W), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).round().to(torch.uint8)
    return out


def instance_masks(n=100, H=1024, W=1024):
    """blobs with ragged edges, one per mask: bool [n,H,W] on the device"""
    g = torch.Generator(device='cuda').manual_seed(5)
    y, x = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32), indexing='ij')
    out = torch.empty((n, H, W), dtype=torch.bool, device='cuda')
    for k in range(n):
        cy, cx, r = (torch.rand(3, generator=g, device='cuda') * torch.tensor([H, W, 0.3 * min(H, W)], device='cuda')).tolist()
        wob = 12 * torch.sin(x * 0.05 + k) * torch.cos(y * 0.07)
        out[k] = torch.hypot(y - cy, x - cx) + wob < r + 40
    return out


def profile(label, images, to_pil, reps):
    from PIL import Image
    ops.png_encode(images[:2])                                             # library load, first-launch costs
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(reps):
        t = time.perf_counter()
        files = ops.png_encode(images)
        dev_ms.append((time.perf_counter() - t) * 1e3)
    hist = np.bincount(images[0].cpu().numpy().view(np.uint8).reshape(-1), minlength=286)   # as many used symbols as a real one
    hist[256] = 1
    t = time.perf_counter()
    for _ in files:
        pngcode.build_code(hist)
    code_ms = (time.perf_counter() - t) * 1e3
    host_ms, copy_ms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        host = images.cpu().numpy()
        copy_ms.append((time.perf_counter() - t) * 1e3)
        pil = []
        for f in host:
            buf = io.BytesIO()
            Image.fromarray(to_pil(f)).save(buf, 'PNG', compress_level=1)
            pil.append(buf.getvalue())
        host_ms.append((time.perf_counter() - t) * 1e3)
    fmt = lambda v: " ".join("%.1f" % x for x in v)   # noqa: E731
    n = int(images.shape[0])
    print("%s: %d images %s" % (label, n, tuple(images.shape[1:])))
    print("  device route (png_encode, copy included): %s ms (min %.1f); of that about %.1f ms of host code building" % (fmt(dev_ms), min(dev_ms), code_ms))
    print("  host route (copy + PIL compress_level=1, one thread): %s ms (min %.1f); the copy alone: %s ms" % (fmt(host_ms), min(host_ms), fmt(copy_ms)))
    print("  bytes to the host: device route %d (+ %d of histograms), host route %d; PIL's files %d" %
          (sum(len(f) for f in files), 288 * 4 * n, images.numel() * images.element_size(), sum(len(p) for p in pil)))
    print("  speed-up %.2fx" % (min(host_ms) / min(dev_ms)))


def main():
    reps = int(os.environ.get("PNG_REPS", "3"))
    profile("frames", video_frames(int(os.environ.get("PNG_FRAMES", "75"))), lambda f: f[:, :, ::-1], reps)
    profile("masks", instance_masks(int(os.environ.get("PNG_MASKS", "100"))), lambda f: f.astype(np.uint8) * 255, reps)


if __name__ == "__main__":
    main()
