"""Times the GIF decoder (ops.gif_decode, video.read_gif) against the host route of the same files: medians of 5
passes after one warm-up, each pass synchronised, in one process on one machine.

    python tools/time_gifdec.py [--files 64] [--side 1024] [--frames 75] [--out FILE]

Clips: `--frames` frames of side x side written by ops.gif_encode, and the same frames saved by Pillow (its own palette per clip,
delta rectangles with a transparent index), read by video.read_gif against a Pillow seek + convert('RGB') loop with an upload per
frame.  Stills: 1, 16 and `--files` single-frame files of side x side from ops.gif_encode, on the device in one ops.gif_decode call
against the same Pillow route per file.  The bytes that cross PCIe are the joined LZW sub-blocks and the colour tables against
H * W * 3 per frame.  The kernel-time split (the one-lane walker against everything behind it) comes from one profiled call per
input, at the default scratch budget."""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import gifread, ops, video  # noqa: E402
from tools.time_webpdec import frame  # noqa: E402


def median_ms(fn, passes=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(passes):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def kernel_split(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    parts = {}
    for ev in prof.key_averages():
        total = getattr(ev, 'device_time_total', None)
        total = ev.cuda_time_total if total is None else total
        for k in ('k_gd_walk', 'k_gd_identity', 'k_gd_double', 'k_gd_gather', 'k_gd_compose'):
            if k in ev.key:
                parts[k] = parts.get(k, 0.0) + total / 1e3
    return parts


def uploaded(datas):
    """bytes the device route uploads: every image's LZW bytes, and the 768-byte tables"""
    n = 0
    for d in datas:
        info = gifread.probe(d)
        n += 768 * ((info['global_palette'] is not None) + sum(fr['palette'] is not None for fr in info['frames']))
        n += sum(fr['stream_bytes'] for fr in info['frames'])
    return n


def seek_loop(paths):
    from PIL import Image
    out = []
    for p in paths:
        with Image.open(p) as im:
            k = 0
            while True:
                try:
                    im.seek(k)
                except EOFError:
                    break
                out.append(torch.from_numpy(np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])).cuda())
                k += 1
    return out


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--side', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(what, datas, paths, device_fn, frames):
        stats = {}
        ops.gif_decode(datas, stats=stats)
        say("%s: %.2f MB of LZW data and tables against %.1f MB of pixels over PCIe; native calls of %s images, doubling rounds %s"
            % (what, uploaded(datas) / 1e6, frames * a.side * a.side * 3 / 1e6, stats['groups'], stats['rounds']))
        got = device_fn()
        want = seek_loop(paths)
        assert len(want) == frames and all(torch.equal(g, w) for g, w in zip(got.reshape(-1, a.side, a.side, 3)[:3], want[:3]))
        del got, want
        dev = median_ms(device_fn)
        host = median_ms(lambda: seek_loop(paths))
        say("  device: %.1f ms (min %.1f, max %.1f)" % dev)
        say("  host, Pillow seek + convert('RGB') + upload per frame: %.1f ms (min %.1f, max %.1f)" % host)
        try:
            parts = kernel_split(device_fn)
            total = sum(parts.values())
            say("  kernel time %.1f ms: %s (the walker's share: %.0f %%)"
                % (total, ", ".join("%s %.1f" % (k[5:], v) for k, v in sorted(parts.items())), 100 * parts.get('k_gd_walk', 0.0) / max(total, 1e-9)))
        except Exception as e:                                      # the profiler is an aid: the medians above do not depend on it
            say("  kernel split not available: %r" % (e,))

    with tempfile.TemporaryDirectory() as tmp:
        frames_h = np.stack([frame(a.side, 100 + k % 8) for k in range(a.frames)])                    # R, G, B
        frames_h[:, :8, :8] = (np.arange(a.frames) % 251)[:, None, None, None]                        # no two frames alike
        frames = torch.from_numpy(np.ascontiguousarray(frames_h[..., ::-1])).cuda()
        ours = ops.gif_encode(frames, fps=25)
        del frames
        clip = os.path.join(tmp, 'ours.gif')
        with open(clip, 'wb') as fh:
            fh.write(ours)
        report("a clip of %d frames of %dx%d from ops.gif_encode (%.1f MB file)" % (a.frames, a.side, a.side, len(ours) / 1e6),
               [ours], [clip], lambda: video.read_gif(clip)[0], a.frames)
        ims = [Image.fromarray(f) for f in frames_h]
        b = io.BytesIO()
        ims[0].save(b, 'GIF', save_all=True, append_images=ims[1:], duration=40, loop=0)
        pil = b.getvalue()
        del ims
        clip = os.path.join(tmp, 'pillow.gif')
        with open(clip, 'wb') as fh:
            fh.write(pil)
        n = len(gifread.probe(pil)['frames'])
        report("the same frames saved by Pillow (%.1f MB file, %d frames)" % (len(pil) / 1e6, n), [pil], [clip],
               lambda: video.read_gif(clip)[0], n)
        stills, paths = [], []
        for k in range(a.files):
            f = torch.from_numpy(np.ascontiguousarray(frame(a.side, k)[..., ::-1])).cuda()
            stills.append(ops.gif_encode(f.unsqueeze(0)))
            paths.append(os.path.join(tmp, 's%d.gif' % k))
            with open(paths[-1], 'wb') as fh:
                fh.write(stills[-1])
        for n in sorted({1, min(16, a.files), a.files}):
            report("%d single-frame file(s) of %dx%d from ops.gif_encode" % (n, a.side, a.side), stills[:n], paths[:n],
                   lambda: torch.stack(ops.gif_decode(stills[:n])), n)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
