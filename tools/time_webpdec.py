"""Times the lossless WebP decoder (ops.webp_decode) against imread + upload of the same files: medians of 5 passes
after one warm-up, each pass synchronised, in one process on one machine.

    python tools/time_webpdec.py [--files 64] [--side 1024] [--out FILE] [--cache DIR]

Two sets: cut-outs written by ops.webp_encode_lossless from frames of side x side, and Pillow-default (method 4) lossless files of
such frames.  Each set is decoded with all files in one call, in calls of 16, and as a single file, on the device and through
imread + upload on the host; the bytes that cross PCIe are the VP8L payloads against H * W * 3.  The scratch budget
(ops.WEBP_DECODE_SCRATCH_BYTES) is lifted for the device runs so that a call really is one native call; the default budget is
timed as well.  --cache keeps the Pillow-written files between runs (writing 64 of them takes a minute).  The kernel-time split (walker against everything behind it) comes from one profiled call."""
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
from cartoonsegmentation_amd import ops, webpread  # noqa: E402
from utils.io_utils import imread  # noqa: E402


def frame(side, seed):
    """a cartoon-like frame: flat regions, a gradient, some texture"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    img = np.stack([(x * 255) // (side - 1), (y * 255) // (side - 1), ((x + y) * 255) // (2 * side - 2)], axis=2).astype(np.uint8)
    for _ in range(24):
        cy, cx, rad = rng.integers(0, side), rng.integers(0, side), rng.integers(side // 32, side // 5)
        img[(y - cy) ** 2 + (x - cx) ** 2 < rad * rad] = rng.integers(0, 256, 3)
    q = side // 4
    img[:q, -q:] = rng.integers(0, 256, (q, q, 3))
    return img


def pillow_set(files, side, cache=''):
    """(frames, Pillow-default lossless files of them); with `cache`, the files are kept in that directory and read back from it"""
    from PIL import Image
    frames, pil = [], []
    for k in range(files):
        path = os.path.join(cache, 'pillow_%d_%d.webp' % (side, k)) if cache else ''
        if path and os.path.exists(path):
            with open(path, 'rb') as fh:
                pil.append(fh.read())
            with Image.open(io.BytesIO(pil[-1])) as im:
                frames.append(np.asarray(im.convert('RGB')))
            continue
        frames.append(frame(side, k))
        b = io.BytesIO()
        Image.fromarray(frames[-1]).save(b, 'WEBP', lossless=True)
        pil.append(b.getvalue())
        if path:
            os.makedirs(cache, exist_ok=True)
            with open(path, 'wb') as fh:
                fh.write(pil[-1])
    return frames, pil


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


def kernel_split(files):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ops.webp_decode(files)
        torch.cuda.synchronize()
    walk = rest = 0.0
    for ev in prof.key_averages():
        total = getattr(ev, 'device_time_total', None)
        total = ev.cuda_time_total if total is None else total
        if 'k_wd_walk' in ev.key:
            walk += total
        elif 'k_wd_' in ev.key:
            rest += total
    return walk / 1e3, rest / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--side', type=int, default=1024)
    ap.add_argument('--out', default='')
    ap.add_argument('--cache', default='')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    frames, pil = pillow_set(a.files, a.side, a.cache)
    y, x = np.mgrid[0:a.side, 0:a.side]
    cut = []
    for k, f in enumerate(frames):
        m = (y - a.side // 2) ** 2 + (x - a.side // 2) ** 2 < (a.side // 3 + k) ** 2
        cut.append(torch.from_numpy(np.concatenate([f * m[..., None], (m * 255).astype(np.uint8)[..., None]], axis=2)).cuda())
    ours = ops.webp_encode_lossless(cut)
    default_budget = ops.WEBP_DECODE_SCRATCH_BYTES
    with tempfile.TemporaryDirectory() as tmp:
        for label, files in (('cut-outs of our encoder', ours), ('Pillow method 4', pil)):
            paths = []
            for k, d in enumerate(files):
                paths.append(os.path.join(tmp, '%s%d.webp' % (label[0], k)))
                with open(paths[-1], 'wb') as fh:
                    fh.write(d)
            infos = [webpread.probe(d) for d in files]
            payload = sum(i['payload'][1] - i['payload'][0] for i in infos)
            raw = sum(i['width'] * i['height'] * 3 for i in infos)
            say("%s: %d files of %dx%d, %.2f MB of payloads against %.1f MB of pixels over PCIe" % (label, len(files), a.side, a.side, payload / 1e6, raw / 1e6))

            def host(ps):
                return [torch.from_numpy(imread(p)).cuda() for p in ps]

            def device(ds, per):
                out = []
                for c0 in range(0, len(ds), per):
                    out += ops.webp_decode(ds[c0:c0 + per])
                return out
            want = host(paths[:2])
            got = device(files[:2], 2)
            assert all(torch.equal(w, g) for w, g in zip(want, got))
            stats = {}
            ops.webp_decode(files, stats=stats)
            say("  default scratch budget (%d MiB): native calls of %s files" % (default_budget >> 20, sorted(set(stats['chunks']))))
            say("  device, all files, default budget: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: device(files, len(files))))
            ops.WEBP_DECODE_SCRATCH_BYTES = 1 << 40
            say("  device, all files in one native call: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: device(files, len(files))))
            say("  device, calls of 16: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: device(files, 16)))
            say("  device, one file: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: device(files[:1], 1)))
            say("  host imread + upload, all files: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: host(paths)))
            say("  host imread + upload, one file: %.1f ms (min %.1f, max %.1f)" % median_ms(lambda: host(paths[:1])))
            try:
                walk, rest = kernel_split(files)
                say("  kernel time of one call of all files: walker %.1f ms, transforms and store %.1f ms" % (walk, rest))
                walk, rest = kernel_split(files[:1])
                say("  kernel time of one file: walker %.1f ms, transforms and store %.1f ms" % (walk, rest))
            except Exception as e:                                  # the profiler is an aid: the medians above do not depend on it
                say("  kernel split not available: %r" % (e,))
            ops.WEBP_DECODE_SCRATCH_BYTES = default_budget
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
