"""Times the Motion-JPEG route of npyframes2video against the host alternative, for one Ken Burns video: 75 frames of 1024x1024 on
the device, 4:2:0, quality 90.

  device route: npyframes2video(device frames, 'x.avi') = ops.jpeg_encode + the copy of the compressed bytes + the AVI file
  host route:   frames.cpu().numpy(), PIL (libjpeg) encoding every frame at the same settings in one thread, the same AVI writer

Prints both wall times (steady state, best of MJPEG_REPS), the bytes that cross to the host on either route and the encode-only
time.  Run once under `rocprofv3 --kernel-trace --stats -- python tools/mjpeg_profile.py` for the per-kernel split."""
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, synth, video  # noqa: E402
from cartoonsegmentation_amd.kenburns import npyframes2video  # noqa: E402


def video_frames(n=75, H=1024, W=1024):
    """a zoom-and-pan over one synthetic picture, as the frame loop leaves it: uint8 [n,H,W,3] on the device"""
    src = torch.from_numpy(synth.image_u8(H + 128, W + 128, 3)).cuda().permute(2, 0, 1)[None].float()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device='cuda')
    for k in range(n):
        c = 128 * k // max(n - 1, 1)
        crop = src[:, :, c // 2:H + 128 - (c - c // 2), c // 2:W + 128 - (c - c // 2)]
        out[k] = torch.nn.functional.interpolate(crop, size=(H, W), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).round().to(torch.uint8)
    return out


def main():
    from PIL import Image
    n, reps = int(os.environ.get("MJPEG_FRAMES", "75")), int(os.environ.get("MJPEG_REPS", "3"))
    frames = video_frames(n)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    tmp = tempfile.mkdtemp()
    dev_path, host_path = os.path.join(tmp, "device.avi"), os.path.join(tmp, "host.avi")
    ops.jpeg_encode(frames[:2])                                            # library load, first-launch costs
    torch.cuda.synchronize()

    dev_ms, enc_ms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        npyframes2video(frames, dev_path)
        dev_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        jpegs = ops.jpeg_encode(frames)
        enc_ms.append((time.perf_counter() - t) * 1e3)
    crossed = sum(len(j) for j in jpegs) + 16 * n

    host_ms, copy_ms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        host = frames.cpu().numpy()
        copy_ms.append((time.perf_counter() - t) * 1e3)
        pil = []
        for f in host:
            buf = io.BytesIO()
            Image.fromarray(f[:, :, ::-1]).save(buf, 'JPEG', quality=90, subsampling=2)
            pil.append(buf.getvalue())
        video.write_mjpeg_avi(host_path, pil, W, H)
        host_ms.append((time.perf_counter() - t) * 1e3)

    fmt = lambda v: " ".join("%.1f" % x for x in v)
    print("%d frames %dx%d, 4:2:0, quality 90" % (n, H, W))
    print("device route (encode + copy + file): %s ms (min %.1f); encode + copy alone: %s ms (min %.1f)" % (fmt(dev_ms), min(dev_ms), fmt(enc_ms), min(enc_ms)))
    print("host route (copy + PIL, one thread + file): %s ms (min %.1f); the copy alone: %s ms" % (fmt(host_ms), min(host_ms), fmt(copy_ms)))
    print("bytes to the host: device route %d (file %d), host route %d; PIL's streams %d" %
          (crossed, os.path.getsize(dev_path), frames.numel(), sum(len(p) for p in pil)))
    print("speed-up %.2fx" % (min(host_ms) / min(dev_ms)))


if __name__ == "__main__":
    main()
