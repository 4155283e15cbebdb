"""Times ops.patchmatch_inpaint on one Ken-Burns-like 1024x1024 view (p = 3, about a quarter of the frame in disocclusion bands):
wall time per call over a few steady-state calls.  Run once under `rocprofv3 --kernel-trace --stats -- python tools/patchmatch_profile.py`
for the per-kernel times and the launch count."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import ops, synth  # noqa: E402


def view(H=1024, W=1024):
    img = synth.image_u8(H, W, 3)
    yy, xx = np.mgrid[:H, :W]
    hole = (np.abs(xx - 0.35 * W - 40 * np.sin(yy / 90.0)) < 0.09 * W) | (np.hypot(yy - 0.6 * H, xx - 0.75 * W) < 0.17 * min(H, W))
    hole |= (xx > W - 0.05 * W)                      # a border strip, as a shifted view leaves
    return img, hole.astype(np.uint8)


def main():
    img, m = view()
    dev = torch.device('cuda', 0)
    di, dm = torch.from_numpy(img).to(dev), torch.from_numpy(m).to(dev)
    out = ops.patchmatch_inpaint(di, dm, patch_size=3)
    torch.cuda.synchronize()
    ts = []
    for _ in range(int(os.environ.get("PM_REPS", "5"))):
        t = time.perf_counter()
        o2 = ops.patchmatch_inpaint(di, dm, patch_size=3)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    assert torch.equal(out, o2)
    print("patchmatch 1024x1024 p=3 hole %.3f: %s ms (min %.2f)" % (m.mean(), " ".join("%.2f" % t for t in ts), min(ts)))


if __name__ == "__main__":
    main()
