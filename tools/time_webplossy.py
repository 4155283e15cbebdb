"""Times the lossy WebP decoder (ops.webp_decode(lossy=True), video.read_webp) against the host route of the same
files: medians of 5 passes after one warm-up, each pass synchronised, in one process on one machine.

    python tools/time_webplossy.py [--files 64] [--side 1024] [--frames 75] [--out FILE]

Stills: 1, 16 and `--files` Pillow-written files of side x side at quality 80, on the device in one ops.webp_decode call against
imread + upload of each file.  Clip: `--frames` frames of side x side written by ops.webp_streams + video.write_webp, read by
video.read_webp against a Pillow seek loop with an upload per frame.  The bytes that cross PCIe are the VP8 chunks against H * W * 3.
Where the default scratch budget (ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES) splits a call into several native calls, the call is also
timed with the budget lifted.  The kernel-time split (the one-lane walker against everything behind it) comes from one profiled call
per input, at the default budget."""
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
from cartoonsegmentation_amd import ops, video, webpread  # noqa: E402
from utils.io_utils import imread  # noqa: E402
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
    walk = rest = 0.0
    for ev in prof.key_averages():
        total = getattr(ev, 'device_time_total', None)
        total = ev.cuda_time_total if total is None else total
        if 'k_vd_walk' in ev.key:
            walk += total
        elif 'k_vd_' in ev.key or 'k_wd_' in ev.key:
            rest += total
    return walk / 1e3, rest / 1e3


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

    default_budget = ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES
    files = []
    for k in range(a.files):
        b = io.BytesIO()
        Image.fromarray(frame(a.side, k)).save(b, 'WEBP', quality=80)
        files.append(b.getvalue())
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, d in enumerate(files):
            paths.append(os.path.join(tmp, 'f%d.webp' % k))
            with open(paths[-1], 'wb') as fh:
                fh.write(d)

        def host(ps):
            return [torch.from_numpy(imread(p)).cuda() for p in ps]

        assert all(torch.equal(w, g) for w, g in zip(host(paths[:2]), ops.webp_decode(files[:2], lossy=True)))
        for n in sorted({1, min(16, a.files), a.files}):
            infos = [webpread.probe(d, lossy=True) for d in files[:n]]
            payload = sum(i['payload'][1] - i['payload'][0] for i in infos)
            stats = {}
            ops.webp_decode(files[:n], stats=stats, lossy=True)
            say("%d Pillow quality-80 file(s) of %dx%d: %.2f MB of VP8 chunks against %.1f MB of pixels over PCIe; native calls of %s files"
                % (n, a.side, a.side, payload / 1e6, n * a.side * a.side * 3 / 1e6, stats['chunks_lossy']))
            say("  device, one ops.webp_decode call: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: ops.webp_decode(files[:n], lossy=True)))
            if len(stats['chunks_lossy']) > 1:
                ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES = 1 << 40
                say("  device, budget lifted (one native call): %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: ops.webp_decode(files[:n], lossy=True)))
                ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES = default_budget
            say("  host imread + upload: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: host(paths[:n])))
            try:
                walk, rest = kernel_split(lambda: ops.webp_decode(files[:n], lossy=True))
                say("  kernel time: walker %.1f ms, everything behind it %.1f ms (the walker's share: %.0f %%)" % (walk, rest, 100 * walk / max(walk + rest, 1e-9)))
            except Exception as e:                                  # the profiler is an aid: the medians above do not depend on it
                say("  kernel split not available: %r" % (e,))
        # the clip
        clip = os.path.join(tmp, 'clip.webp')
        frames = torch.from_numpy(np.stack([np.ascontiguousarray(frame(a.side, 100 + k % 8)[..., ::-1]) for k in range(a.frames)])).cuda()
        streams = ops.webp_streams(frames, quality=80)[0]
        del frames
        size = video.write_webp(clip, streams, a.side, a.side)

        def seek_loop():
            out = []
            with Image.open(clip) as im:
                for k in range(im.n_frames):
                    im.seek(k)
                    out.append(torch.from_numpy(np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])).cuda())
            return out

        got, _ = video.read_webp(clip)
        assert all(torch.equal(g, w) for g, w in zip(got[:2], seek_loop()[:2]))
        del got
        say("a clip of %d frames of %dx%d from our encoder: %.2f MB file against %.1f MB of pixels over PCIe"
            % (a.frames, a.side, a.side, size / 1e6, a.frames * a.side * a.side * 3 / 1e6))
        say("  device, video.read_webp: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: video.read_webp(clip)))
        ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES = 1 << 40
        say("  device, video.read_webp, budget lifted (one native call): %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: video.read_webp(clip)))
        ops.WEBP_LOSSY_DECODE_SCRATCH_BYTES = default_budget
        say("  host, Pillow seek loop + upload per frame: %.1f ms (min %.1f, max %.1f)" % median_ms(seek_loop))
        try:
            walk, rest = kernel_split(lambda: video.read_webp(clip))
            say("  kernel time: walker %.1f ms, everything behind it %.1f ms (the walker's share: %.0f %%)" % (walk, rest, 100 * walk / max(walk + rest, 1e-9)))
        except Exception as e:
            say("  kernel split not available: %r" % (e,))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
