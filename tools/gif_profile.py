"""Times the GIF route against the host alternative for one Ken Burns video (75 colour frames of 1024x1024 on the device), and
compares file sizes with Pillow's own LZW on the same index frames.

  device route: ops.gif_encode(frames) = cell table, palette on the host, mapping, LZW and bit packing on the device, the copy of
                the compressed bytes, the container
  host route:   the same index frames and palette on the host, written by Pillow (save_all, optimize=False) in one thread

Prints the wall times of the parts (steady state, best of GIF_REPS) and the file sizes, then the sizes for the small synthetic
Ken Burns clip of the test suite (3 frames of 320x384).  Run once under `rocprofv3 --kernel-trace --stats -- python
tools/gif_profile.py` for the per-kernel split."""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cartoonsegmentation_amd import gifcode, ops  # noqa: E402
from png_profile import video_frames  # noqa: E402


def pillow_gif(idx, palette):
    from PIL import Image
    ims = []
    for f in idx:
        im = Image.fromarray(f, 'P')
        im.putpalette(palette.tobytes())
        ims.append(im)
    buf = io.BytesIO()
    ims[0].save(buf, 'GIF', save_all=True, append_images=ims[1:], optimize=False, duration=40, loop=0, disposal=0)
    return buf.getvalue()


def timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def profile(label, frames, reps, host=True):
    ops.gif_encode(frames[:2])                                             # library load, first-launch costs
    n = int(frames.shape[0])
    t_all, data = timed(lambda: ops.gif_encode(frames), reps)
    t_q, (idx, pal) = timed(lambda: ops.gif_quantize(frames), reps)
    t_qp, _ = timed(lambda: ops.gif_quantize(frames, palette=pal), reps)
    t_s, (streams, W, H) = timed(lambda: ops.gif_streams(idx), reps)
    t_c, _ = timed(lambda: gifcode.gif_file(streams, W, H, pal), reps)
    print("%s: %d frames %s" % (label, n, tuple(frames.shape[1:])))
    print("  device route (gif_encode, copies included): %.1f ms = quantize %.1f (of it mapping with a given palette %.1f; the rest is "
          "the cell table, its copy and the median cut) + streams %.1f + container %.1f" % (t_all, t_q, t_qp, t_s, t_c))
    print("  file %d bytes (LZW %d); bound per frame %d" % (len(data), sum(len(s) for s in streams), gifcode.stream_bound(H, W)))
    if host:
        idx_h = idx.cpu().numpy()
        t = time.perf_counter()
        pil = pillow_gif(idx_h, pal)
        t_h = (time.perf_counter() - t) * 1e3
        print("  host route (Pillow save_all, optimize=False, one thread, index frames already on the host): %.1f ms, file %d bytes" % (t_h, len(pil)))
        print("  size ratio ours / Pillow %.3f; time ratio Pillow / streams+container %.2f" % (len(data) / len(pil), t_h / (t_s + t_c)))
        singles = sum(len(pillow_gif(idx_h[k:k + 1], pal)) for k in range(min(n, 3)))
        ours = sum(len(gifcode.gif_file(streams[k:k + 1], W, H, pal)) for k in range(min(n, 3)))
        print("  first %d frames as single-frame files (no frame differencing on either side): ours %d, Pillow %d" % (min(n, 3), ours, singles))


def kenburns_clip():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    H, W = 320, 384
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False,
                         depth_field=False, focal=W / 2.0, num_frame=3,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    img = synth.image_u8(H, W, 11)
    inst = pipe.animeinsseg.infer(img, pred_score_thr=0.3, max_instances=2, det_size=96, refine_kwargs=cfg.mask_refine_kwargs)
    kc = pipe.generate_kenburns_config(img, instances=inst)
    W, H = kc['intWidth'], kc['intHeight']
    objFrom = {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(0.97 * W), 'intCropHeight': int(0.97 * H)}
    objTo = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': objFrom}, kc)
    frames, _ = pipe.process_kenburns({'fltSteps': [0.0, 0.5, 1.0], 'objFrom': objFrom, 'objTo': objTo, 'boolInpaint': False}, kc,
                                      inpaint=False, to_numpy=False)
    return frames


def main():
    reps = int(os.environ.get("GIF_REPS", "3"))
    profile("frames", video_frames(int(os.environ.get("GIF_FRAMES", "75"))), reps, host=os.environ.get("GIF_HOST", "1") == "1")
    if os.environ.get("GIF_KENBURNS", "1") == "1":
        profile("kenburns clip", kenburns_clip(), reps)


if __name__ == "__main__":
    main()
