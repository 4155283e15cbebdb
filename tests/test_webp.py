"""CPU: the WebP writer's contract.  libwebp (through Pillow) decodes the files of the numpy restatement
(tests/webp_restatement.py) to exactly the RGB the restatement predicts, byte for byte; the restatement's boolean coder round-trips
through the format's decoder; webpcode's containers equal the restatement's bytes; argument errors; the encoder is not degenerate."""
import functools
import io
import os
import random
import sys

import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as R  # noqa: E402
from test_mjpeg import cartoon, psnr  # noqa: E402
from cartoonsegmentation_amd import video, webpcode  # noqa: E402

ALL_Q = (1, 50, 90, 100)
# name -> (H, W, qualities); the shapes up to 100x101 at every quality, the larger ones at 90 alone
SHAPES = {
    '1x1': (1, 1, ALL_Q),                      # the smallest frame
    '16x16': (16, 16, ALL_Q),                  # one macroblock
    '17x33': (17, 33, ALL_Q),                  # edge replication, odd chroma
    '31x16': (31, 16, ALL_Q),                  # two macroblock rows of one macroblock
    '16x31': (16, 31, ALL_Q),                  # one macroblock row: one partition
    '48x64': (48, 64, ALL_Q),                  # a small ordinary frame
    '100x101': (100, 101, ALL_Q),              # odd sizes
    '243x317': (243, 317, (90,)),              # 16 macroblock rows, 8 partitions
    '16x1120': (16, 1120, (90,)),              # 70 diagonals of one macroblock
    '1120x16': (1120, 16, (90,)),
    'black': (33, 47, ALL_Q),                  # extreme flat frames
    'white': (33, 47, ALL_Q),
    'noise': (50, 70, ALL_Q),                  # 0 / 255 noise: long carry chains
    'gradient': (64, 80, ALL_Q),               # a smooth gradient: TM and H / V win
}
CASES = [(name, q) for name, (_, _, qs) in SHAPES.items() for q in qs]
IDS = ["%s-q%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def frame(name, v=0):
    """frame v of a case's clip, BGR uint8, read-only"""
    H, W, _ = SHAPES[name]
    if name == 'black':
        f = np.zeros((H, W, 3), np.uint8)
    elif name == 'white':
        f = np.full((H, W, 3), 255, np.uint8)
    elif name == 'noise':
        f = (np.random.default_rng(100 + v).integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    elif name == 'gradient':
        y, x = np.mgrid[0:H, 0:W]
        f = np.stack([20 + 2 * x + v, 30 + 3 * y, 10 + x + 2 * y + 3 * v], -1).astype(np.uint8)
    else:
        f = cartoon(H, W, seed=v)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(name, quality, v=0):
    """the restatement's result for frame v of a case, computed once and shared"""
    return R.encode_frame(frame(name, v), quality)


def pil_frames(data):
    """(list of RGB arrays, size, n_frames, list of durations, loop) of a WebP file"""
    im = Image.open(io.BytesIO(data))
    assert im.format == 'WEBP'
    n = getattr(im, 'n_frames', 1)
    frames, durations = [], []
    for k in range(n):
        im.seek(k)
        frames.append(np.asarray(im.convert('RGB')))
        durations.append(im.info.get('duration'))
    return frames, im.size, n, durations, im.info.get('loop')


# ---- pinned by libwebp ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quality", CASES, ids=IDS)
def test_libwebp_shows_exactly_what_the_restatement_reconstructs(name, quality):
    """equality, not a tolerance: an independent decoder reconstructs what the encoder predicted from"""
    H, W, _ = SHAPES[name]
    r = want(name, quality)
    frames, size, n, _, _ = pil_frames(R.still_file(r['vp8']))
    assert size == (W, H) and n == 1
    expect = R.decoded_rgb(r, H, W)
    diff = np.argwhere(frames[0] != expect)
    assert diff.size == 0, (name, quality, len(diff), diff[0].tolist())
    assert r['ymodes'].shape == r['uvmodes'].shape == ((H + 15) // 16, (W + 15) // 16)
    assert len(r['parts']) == webpcode.partitions(H) and all(len(p) > 0 for p in r['parts'])


def test_the_cases_take_every_mode_and_skip_and_code_macroblocks():
    """the case list reaches all four luma and chroma modes, skipped and coded macroblocks and a filtered frame"""
    y = np.concatenate([want(n, q)['ymodes'].ravel() for n, q in CASES if q == 90])
    uv = np.concatenate([want(n, q)['uvmodes'].ravel() for n, q in CASES if q == 90])
    assert set(y.tolist()) == {0, 1, 2, 3} and set(uv.tolist()) == {0, 1, 2, 3}
    g = want('gradient', 90)
    assert np.isin(g['ymodes'], (1, 2, 3)).mean() > 0.5, np.bincount(g['ymodes'].ravel(), minlength=4)
    black = want('black', 90)['skip'].ravel()
    assert not black[0] and black[1:].all() and not want('noise', 90)['skip'].any()      # the first macroblock predicts 128
    assert want('48x64', 50)['level'] > 0 and want('48x64', 100)['level'] == 0


@pytest.mark.parametrize("playback", [False, True])
def test_animation_of_five_frames(playback):
    H, W = 48, 64
    results = [want('48x64', 90, v) for v in range(5)]
    order = video.playback_order(5) if playback else None
    data = R.animation_file([r['vp8'] for r in results], W, H, fps=25, loop=0, order=order)
    frames, size, n, durations, loop = pil_frames(data)
    shown = order if playback else list(range(5))
    assert size == (W, H) and n == len(shown) == (8 if playback else 5) and durations == [40] * n and loop == 0
    for k, i in enumerate(shown):
        assert np.array_equal(frames[k], R.decoded_rgb(results[i], H, W)), (k, i)
    assert data == R.encode_animation([frame('48x64', v) for v in range(5)], 90, order=order)
    frames, _, _, durations, loop = pil_frames(R.animation_file([r['vp8'] for r in results], W, H, fps=10, loop=3))
    assert durations == [100] * 5 and loop == 3


# ---- the boolean coder alone ----------------------------------------------------------------------------------------------------
class BoolDecoder:
    """the format's boolean decoder (RFC 6386 section 7.3); bytes past the end read as zero"""

    def __init__(self, data):
        self.data, self.pos, self.range, self.bit_count = data, 2, 255, 0
        self.value = self._byte(0) << 8 | self._byte(1)

    def _byte(self, i):
        return self.data[i] if i < len(self.data) else 0

    def get(self, prob):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if self.value >= split << 8:
            bit = 1
            self.range -= split
            self.value -= split << 8
        else:
            bit = 0
            self.range = split
        while self.range < 128:
            self.value <<= 1
            self.range <<= 1
            self.bit_count += 1
            if self.bit_count == 8:
                self.bit_count = 0
                self.value |= self._byte(self.pos)
                self.pos += 1
        return bit


class _Watched(R.BoolEncoder):
    """records the longest run of 0xFF bytes that a carry went through"""
    carried = 0

    def _flush(self):
        bits = self.value >> (8 + self.nb_bits)
        if (bits & 0xFF) != 0xFF and bits >> 8:
            self.carried = max(self.carried, self.run)
        super()._flush()


def carry_pairs(steps, seed):
    """(probability, bit) pairs that keep the coder's interval astride the value one half -- low end 0.0111..., so finished bytes
    are 0xFF and held back -- and then step over it, so that the carry runs through all of them.  Exact integer arithmetic."""
    rnd = random.Random(seed)
    low, rng, shifts, pairs = 0, 254, 0, []

    def step(prob, bit):
        nonlocal low, rng, shifts
        split = (rng * prob) >> 8
        if bit:
            low, rng = low + split + 1, rng - split - 1
        else:
            rng = split
        if rng < 127:
            s = 8 - (rng + 1).bit_length()
            low, rng, shifts = low << s, ((rng + 1) << s) - 1, shifts + s
        pairs.append((prob, bit))

    for i in range(100000):
        prob = rnd.choice([1, 60, 100, 128, 200, 255])
        split, half = (rng * prob) >> 8, 1 << (7 + shifts)
        if half <= low + split:
            step(prob, int(i >= steps))            # one half lies in the lower part: stay, or at the end step over it
            if i >= steps:
                break
        else:
            exact = low + split + 1 == half        # the upper part begins exactly at one half
            step(prob, 1)
            if exact:
                break
    return pairs


def _round_trip(pairs):
    data = R.code_pairs(pairs)
    d = BoolDecoder(data)
    got = [d.get(p) for p, _ in pairs]
    assert got == [b for _, b in pairs], next(i for i, (g, (_, b)) in enumerate(zip(got, pairs)) if g != b)
    return data


def test_boolean_coder_round_trips_random_sequences():
    rnd = random.Random(7)
    for k in range(60):
        n = rnd.choice([0, 1, 2, 7, 8, 9, 100, 1000])
        skew = rnd.random()
        pairs = [(rnd.choice([1, 2, 3, 64, 127, 128, 129, 200, 253, 254, 255]) if k % 3 else rnd.randint(1, 255),
                  int(rnd.random() < skew)) for _ in range(n)]
        _round_trip(pairs)
    for prob in (1, 255):
        for bit in (0, 1):
            _round_trip([(prob, bit)] * 300)
            _round_trip([(prob, bit), (prob, 1 - bit)] * 150)


def test_boolean_coder_carries_through_runs_of_ff():
    longest = 0
    for seed in range(12):
        pairs = carry_pairs(1500, seed)
        e = _Watched()
        for p, b in pairs:
            e.put(p, b)
        data = e.finish()
        assert data == _round_trip(pairs)
        longest = max(longest, e.carried)
    assert longest >= 16, longest


# ---- the device's coder, built for the host: the end of a segment --------------------------------------------------------------
_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "csm_boolenc.h"
// stdin: cap, then "probability bit" per pair.  stdout: bytes needed, the over flag, whether the 64 guard bytes behind the
// segment are untouched, and the segment in hex.
int main() {
    long cap;
    if (scanf("%ld", &cap) != 1) return 2;
    std::vector<unsigned char> buf(cap + 64, 0xA5);
    csm::BoolEnc e;
    e.open(buf.data(), cap);
    int p, b;
    while (scanf("%d %d", &p, &b) == 2) e.put(p, b);
    const long need = (long)e.finish();
    int intact = 1;
    for (long i = cap; i < cap + 64; ++i) intact &= buf[i] == 0xA5;
    printf("%ld %d %d ", need, e.over, intact);
    for (long i = 0; i < cap; ++i) printf("%02x", buf[i]);
    printf("\n");
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _host_coder():
    """the path of csrc/csm_boolenc.h's coder compiled for the host with a small driver"""
    import shutil
    import subprocess
    import tempfile
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, "a host C++ compiler is needed"
    d = tempfile.mkdtemp(prefix='csm_boolenc_')
    src, exe = os.path.join(d, 'driver.cpp'), os.path.join(d, 'driver')
    with open(src, 'w') as f:
        f.write(_DRIVER)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cartoonsegmentation_amd', 'csrc')
    subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', '-I', inc, src, '-o', exe], check=True, capture_output=True, text=True)
    return exe


def _host_code(pairs, cap):
    import subprocess
    text = "%d\n" % cap + "".join("%d %d\n" % pb for pb in pairs)
    out = subprocess.run([_host_coder()], input=text, capture_output=True, text=True, check=True).stdout.split()
    return int(out[0]), int(out[1]), int(out[2]), bytes.fromhex(out[3]) if len(out) > 3 else b''


def test_device_coder_never_writes_past_its_segment():
    """csm_boolenc.h equals the restatement when the segment is long enough; when it is too short -- also where a carry has to go
    through a run of held-back 0xFF bytes that straddles the end -- the bytes before the end are the stream's, nothing behind the
    end is touched, the over flag is set and the size returned is the size the stream needs"""
    rnd = random.Random(3)
    streams = [[(rnd.randint(1, 255), int(rnd.random() < 0.5)) for _ in range(400)], [(255, 1)] * 60 + [(128, 1)] * 8, []]
    streams += [carry_pairs(1500, seed) for seed in (1, 3, 6, 10)]
    for pairs in streams:
        e = _Watched()
        for p, b in pairs:
            e.put(p, b)
        expect = e.finish()
        n = len(expect)
        caps = sorted({0, 1, 2, n // 2, n - 2, n - 1, n, n + 5} | set(range(max(0, n - 40), n)))
        for cap in (c for c in caps if c >= 0):
            need, over, intact, seg = _host_code(pairs, cap)
            assert need == n and intact == 1 and over == int(cap < n), (len(pairs), cap, need, n, over, intact)
            assert seg[:min(cap, n)] == expect[:min(cap, n)], (len(pairs), cap)


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_webpcode_containers_equal_the_restatement(tmp_path):
    results = [want('48x64', 90, v) for v in range(5)]
    streams = [webpcode.vp8_frame(r['first'], r['parts'], 64, 48) for r in results]
    assert streams == [r['vp8'] for r in results]
    assert [webpcode.still_file(s) for s in streams] == R.encode([frame('48x64', v) for v in range(5)], 90)
    odd, even = streams[0][:1001], streams[0][:1000]                           # an odd-sized chunk is padded, an even one is not
    for payload in (odd, even):
        still = webpcode.still_file(payload)
        assert still == R.still_file(payload) and len(still) == 20 + 1000 + (len(payload) & 1) * 2
        assert still[16:20] == len(payload).to_bytes(4, 'little') and still[4:8] == (len(still) - 8).to_bytes(4, 'little')
        anim = webpcode.animation_file([payload, even], 64, 48, order=[0, 1, 0])
        assert anim == R.animation_file([payload, even], 64, 48, order=[0, 1, 0])
        at = anim.index(b'ANMF')                                               # ANMF size: 16 header bytes + the padded 'VP8 ' chunk
        assert int.from_bytes(anim[at + 4:at + 8], 'little') == 16 + 8 + 1000 + (len(payload) & 1) * 2
        assert anim[at + 8 + 16:at + 8 + 20] == b'VP8 ' and int.from_bytes(anim[at + 28:at + 32], 'little') == len(payload)
        assert len(anim) % 2 == 0 and int.from_bytes(anim[4:8], 'little') == len(anim) - 8
    for order in (None, video.playback_order(5), [4, 4, 0]):
        for fps, loop in ((25, 0), (10, 3), (29.97, 65535)):
            assert webpcode.animation_file(streams, 64, 48, fps=fps, loop=loop, order=order) == \
                R.animation_file(streams, 64, 48, fps=fps, loop=loop, order=order)
    path = str(tmp_path / "a.webp")
    size = video.write_webp(path, streams, 64, 48, fps=25, order=video.playback_order(5))
    data = open(path, 'rb').read()
    assert size == len(data) and data == R.animation_file(streams, 64, 48, order=[0, 1, 2, 3, 4, 3, 2, 1])
    assert pil_frames(data)[2] == 8
    for q in range(1, 101):
        assert webpcode.quality_to_qi(q) == R.quality_to_qi(q)
        assert q == 1 or R.quality_to_qi(q) <= R.quality_to_qi(q - 1)
    assert R.quality_to_qi(1) == 127 and R.quality_to_qi(100) == 0
    assert [webpcode.partitions(h) for h in (1, 16, 17, 32, 33, 64, 112, 113, 16383)] == [1, 1, 2, 2, 2, 4, 4, 8, 8]


def test_container_argument_errors():
    s = [want('16x16', 90)['vp8']]
    for kw in ({'fps': 0}, {'fps': -1}, {'fps': float('nan')}, {'fps': 'x'}, {'fps': 1e-9}, {'order': [1]}, {'order': [-1]},
               {'order': []}, {'loop': -1}, {'loop': 65536}):
        with pytest.raises(ValueError):
            webpcode.animation_file(s, 16, 16, **kw)
    for w, h in ((0, 16), (16, 0), (16384, 16), (16, 16384)):
        with pytest.raises(ValueError):
            webpcode.animation_file(s, w, h)
    with pytest.raises(ValueError):
        webpcode.animation_file([], 16, 16)
    with pytest.raises(ValueError):
        webpcode.vp8_frame(b'\x00' * (1 << 19), [b'\x00'], 16, 16)
    with pytest.raises(ValueError):
        webpcode.vp8_frame(b'\x00', [b'\x00', b'\x00'], 16, 16)


def test_ops_argument_errors():
    torch = pytest.importorskip("torch")
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for fn in (ops.webp_encode, ops.webp_streams):
        for q in (0, 101, -1, True, 90.0, '90', None):
            with pytest.raises(ValueError):
                fn(x, quality=q)
        for bad in (torch.zeros((8, 8, 3)), torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((8, 8, 4), dtype=torch.uint8),
                    torch.zeros((1, 1, 8, 8, 3), dtype=torch.uint8), np.zeros((8, 8, 3), np.uint8)):
            with pytest.raises(CsmError):
                fn(bad)
        for shape in ((16384, 1, 3), (1, 16384, 3), (2, 1, 16384, 3), (0, 4, 3)):
            with pytest.raises(ValueError):
                fn(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(CsmError):
            fn(x)                                                            # a CPU tensor
        with pytest.raises(CsmError):
            fn(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), quality=50)


# ---- not a degenerate encoder -----------------------------------------------------------------------------------------------------
# PSNR (dB, RGB against the source) of the three 243x317 cartoon frames below Pillow's WebP (method 4) at the largest quality whose
# file is not larger than ours.  We write no B_PRED and no probability updates, so we lose; measured deficits are in DESIGN.md
# §4.12: quality 50: 2.04, 1.87, 2.27; quality 75: 1.65, 1.35, 1.83; quality 90: 0.65, 0.52, 0.74.  The bound is the largest of them
# (2.27) rounded up to the next 0.5 dB (2.5) plus 0.5 dB.
MAX_DEFICIT_DB = 3.0
OUR_LOWEST_PSNR_Q90_DB = 30.66         # of the three frames at quality 90 (31.25, 30.66, 32.53)


def pillow_webp(frame_bgr, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, 'WEBP', quality=quality, method=4)
    return buf.getvalue()


def deficit(v, quality):
    """(our bytes, our PSNR, Pillow's quality, bytes, PSNR) for cartoon frame v"""
    f = frame('243x317', v)
    r = want('243x317', quality, v)
    ours = R.still_file(r['vp8'])
    mine = psnr(R.decoded_rgb(r, 243, 317), f[:, :, ::-1])
    for q in range(100, 0, -1):
        theirs = pillow_webp(f, q)
        if len(theirs) <= len(ours):
            break
    else:
        raise AssertionError("Pillow's smallest file (%d bytes) is larger than ours (%d)" % (len(theirs), len(ours)))
    return len(ours), mine, q, len(theirs), psnr(pil_frames(theirs)[0][0], f[:, :, ::-1])


@pytest.mark.parametrize("quality", [50, 75, 90])
def test_not_a_degenerate_encoder(quality):
    for v in range(3):
        ours, mine, q, theirs, ref = deficit(v, quality)
        print("frame %d quality %d: ours %d B %.2f dB; Pillow quality %d %d B %.2f dB; deficit %.2f dB" % (v, quality, ours, mine, q, theirs, ref, ref - mine))
        assert ref - mine <= MAX_DEFICIT_DB, (v, quality, ours, mine, q, theirs, ref)
