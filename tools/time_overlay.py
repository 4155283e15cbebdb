"""Times the instance overlay of one 1024x1024 frame with 100, 10 and 1 instances (synthetic masks on the device).

  route A (host):   AnimeInstances.draw_instances(img) on device instances -- the masks are copied to the host and blended by numpy in
                    one thread -- then a Pillow PNG save
  route B (device): AnimeInstances.draw_instances(img, on_device=True) + utils.io_utils.imwrite('.png'); the draw alone is printed
                    too

Prints the median and the spread (min .. max) of OVERLAY_REPS passes (default 5) after a warm-up and the bytes that cross PCIe on each
route.  Run once under `rocprofv3 --kernel-trace --stats -- python tools/time_overlay.py` for the per-kernel split."""
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, synth  # noqa: E402
from cartoonsegmentation_amd.anime_instances import AnimeInstances  # noqa: E402
from png_profile import instance_masks  # noqa: E402
from utils.io_utils import imwrite  # noqa: E402


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
    return "median %.2f ms (min %.2f .. max %.2f, %d passes)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    from PIL import Image
    reps = max(5, int(os.environ.get("OVERLAY_REPS", "5")))
    img = synth.image_u8(1024, 1024, 3)
    frame = torch.from_numpy(img).cuda()
    every = instance_masks(100)
    tight = ops.mask_bboxes(every)
    boxes = torch.cat([tight[:, :2], tight[:, 2:] - tight[:, :2]], 1).int()
    out_dir = tempfile.mkdtemp()
    for n in (100, 10, 1):
        inst = AnimeInstances(masks=every[:n], bboxes=boxes[:n])

        def host_route():
            Image.fromarray(inst.draw_instances(img)[..., ::-1]).save(os.path.join(out_dir, "host.png"))

        def device_route():
            imwrite(inst.draw_instances(frame, on_device=True), os.path.join(out_dir, "device.png"))

        host_route(); device_route()                           # library load, first-launch costs
        _, host_ms = timed(host_route, reps)
        _, dev_ms = timed(device_route, reps)
        _, draw_ms = timed(lambda: inst.draw_instances(frame, on_device=True), reps)
        file_bytes = os.path.getsize(os.path.join(out_dir, "device.png"))
        print("%d instances over one 1024x1024 frame" % n)
        print("  route A (masks.cpu() + numpy + Pillow PNG): %s" % show(host_ms))
        print("  route B (draw on the device + imwrite .png): %s" % show(dev_ms))
        print("  the draw alone: %s" % show(draw_ms))
        print("  bytes over PCIe: route A %d to the host (masks and boxes); route B %d to the host (the file) and %d to the device (jobs, "
              "draw list, colours; the PNG writer's tables not counted)" % (every[:n].numel() + 16 * n, file_bytes, 128 + 7 * n))
        print("  route A / route B = %.2fx" % (statistics.median(host_ms) / statistics.median(dev_ms)))


if __name__ == "__main__":
    main()
