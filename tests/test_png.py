"""CPU: the PNG contract as tests/png_restatement.py states it -- every stream inflates to the filtered scanlines
and every file decodes (PIL) to its input exactly; the product's host code builder (cartoonsegmentation_amd/pngcode.py) agrees with
the restatement's; sizes; the APNG container of video.write_apng."""
import functools
import heapq
import io
import os
import struct
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_restatement as R  # noqa: E402
from test_mjpeg import cartoon  # noqa: E402


def disc_mask(n=256):
    y, x = np.mgrid[0:n, 0:n]
    return (y - n // 2) ** 2 + (x - n // 2) ** 2 < (n * 3 // 8) ** 2


@functools.lru_cache(maxsize=None)
def image(name):
    """the test images by name (read-only): 'grey-HxW-k' / 'bgr-HxW-k' cartoon frames, 'const-W' constant grey rows, and specials"""
    from cartoonsegmentation_amd import synth
    rng = np.random.default_rng(11)
    kind, _, rest = name.partition('-')
    if kind in ('grey', 'bgr'):
        size, _, k = rest.partition('-')
        H, W = (int(v) for v in size.split('x'))
        a = cartoon(H, W, H * 1000 + W + 7919 * int(k))
        a = np.ascontiguousarray(a[:, :, 1]) if kind == 'grey' else a
    elif kind == 'const':                                       # 3 scanlines of one value: runs of W + 1, W, W
        a = np.full((3, int(rest)), 2, np.uint8)
    elif kind == 'constbgr':
        a = np.full((2, int(rest), 3), 200, np.uint8)
    else:
        a = {'white': lambda: np.full((33, 47, 3), 255, np.uint8), 'black': lambda: np.zeros((33, 47, 3), np.uint8),
             'whitegrey': lambda: np.full((33, 47), 255, np.uint8), 'blackgrey': lambda: np.zeros((33, 47), np.uint8),
             'saturated': lambda: (rng.integers(0, 2, (50, 70, 3)) * 255).astype(np.uint8),
             'saturatedgrey': lambda: (rng.integers(0, 2, (50, 70)) * 255).astype(np.uint8),
             'noise': lambda: rng.integers(0, 256, (50, 70, 3), dtype=np.uint8),
             'noisegrey': lambda: rng.integers(0, 256, (50, 70), dtype=np.uint8),
             'disc': lambda: disc_mask(256), 'flat64x1024': lambda: np.full((64, 1024), 131, np.uint8),
             'wide4100': lambda: rng.integers(0, 256, (9, 4100, 3), dtype=np.uint8),
             'wide65535': lambda: rng.integers(0, 256, (2, 65535, 3), dtype=np.uint8),
             'widegrey65535': lambda: (np.arange(65535)[None, :] // 700 * np.ones((2, 1), np.int64)).astype(np.uint8),
             'synth': lambda: synth.image_u8(320, 384, 11)}[name]()
    a.setflags(write=False)
    return a


SHAPES = [(1, 1), (64, 1), (1, 300), (8, 8), (17, 23), (100, 101), (243, 317), (720, 540)]
CONST_WIDTHS = list(range(258, 264)) + list(range(516, 521))
SPECIALS = ['white', 'black', 'whitegrey', 'blackgrey', 'saturated', 'saturatedgrey', 'noise', 'noisegrey', 'disc', 'flat64x1024',
            'wide4100', 'wide65535', 'widegrey65535']
CPU_CASES = (['%s-%dx%d-0' % (k, H, W) for k in ('grey', 'bgr') for H, W in SHAPES[:-1]] + ['bgr-720x540-0']
             + ['const-%d' % w for w in CONST_WIDTHS] + ['constbgr-%d' % w for w in (86, 87, 172, 173)] + SPECIALS)


@functools.lru_cache(maxsize=None)
def want(name):
    """(file, filtered scanlines) of the restatement"""
    a = image(name)
    return R.encode(a), R.filtered(a)


def expected_pixels(a):
    if a.dtype == np.bool_:
        return a.astype(np.uint8) * 255
    return a[:, :, ::-1] if a.ndim == 3 else a


def chunks(data):
    """[(type, payload)] of a PNG file; checks the signature, every CRC and that nothing trails IEND"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    out, p = [], 8
    while p < len(data):
        n, kind = struct.unpack('>I4s', data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        assert len(body) == n
        assert struct.unpack('>I', data[p + 8 + n:p + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        p += 12 + n
    assert p == len(data) and out[-1] == (b'IEND', b'') and out[0][0] == b'IHDR'
    return out


def pil_pixels(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode in ('L', 'RGB')
        return np.asarray(im).copy()


def check_file(data, a, filt=None):
    """a PNG file of image a: one IDAT that inflates to the restatement's filtered scanlines (filt, where the caller has them), and
    PIL decodes the input"""
    cs = chunks(data)
    assert [k for k, _ in cs] == [b'IHDR', b'IDAT', b'IEND']
    H, W = a.shape[:2]
    assert cs[0][1] == struct.pack('>IIBBBBB', W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    assert cs[1][1][:2] == b'\x78\x01'
    assert zlib.decompress(cs[1][1]) == (R.filtered(a) if filt is None else filt).tobytes()
    assert np.array_equal(pil_pixels(data), expected_pixels(a))


@pytest.mark.parametrize("name", CPU_CASES)
def test_restatement_files_decode_to_their_input(name):
    data, filt = want(name)
    a = image(name)
    check_file(data, a, filt)
    assert filt.shape == (a.shape[0], 1 + a.shape[1] * (3 if a.ndim == 3 else 1)) and filt[:, 0].max() <= 4
    # the fixed code's worst case, which the chooser can always fall back to
    assert len(data) <= filt.size * 9 / 8 + 128, (len(data), filt.size)


def test_filter_choice_on_known_rows():
    """a horizontal ramp takes Sub, a repeated row takes Up, ties go to the lowest type, row 0 sees zeros above"""
    ramp = np.tile((np.arange(64) * 3).astype(np.uint8), (4, 1))
    f = R.filtered(ramp)
    assert f[0, 0] == 1 and f[1:, 0].tolist() == [2, 2, 2]
    assert R.filtered(np.zeros((3, 5), np.uint8))[:, 0].tolist() == [0, 0, 0]
    rows = np.array([[10, 250, 10, 250]] * 2, np.uint8)         # None costs 32; Sub costs 10 + 16 * 3; Up of row 1 costs 0
    assert R.filtered(rows)[:, 0].tolist() == [0, 2]


def test_parse_splits_runs_as_the_contract_says():
    """a run of L equal bytes: one literal, (L - 1) // 258 matches of 258, then one match of the rest if >= 3, else literals"""
    for L in [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 518, 519, 520, 521, 775]:
        f = np.zeros((1, L), np.uint8)
        sym, eb, ev, match = R.tokens(f)
        rest = L - 1
        full, rem = divmod(rest, 258)
        lits = 1 + (rem if rem < 3 else 0)
        assert int((sym == 0).sum()) == lits and int((sym == 285).sum()) == full, L
        assert int(match.sum()) == full + (1 if rem >= 3 else 0), L
    f = np.array([[5, 5, 5, 5, 9], [9, 9, 9, 9, 9]], np.uint8)  # the 9s do not join across the scanlines
    sym, _, _, match = R.tokens(f)
    assert sym.tolist() == [5, 257, 9, 9, 258]


# ---- the code builder, the product's and the restatement's ------------------------------------------------------------------------
def _product_lengths(hist, limit):
    from cartoonsegmentation_amd import pngcode
    return pngcode.limited_lengths(hist, limit)


BUILDERS = {'product': _product_lengths, 'restatement': R.code_lengths}


def huffman(hist):
    """(cost, depth) of a plain Huffman tree"""
    heap = [(int(c), 0, k) for k, c in enumerate(hist) if c > 0]
    heapq.heapify(heap)
    cost, tick = 0, len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick))
        tick += 1
    return cost, heap[0][1]


def _special_histograms():
    rng = np.random.default_rng(3)
    two = [0] * 286; two[0] = 5; two[256] = 1
    dominating = [1] * 286; dominating[7] = 10 ** 7
    every = (rng.integers(1, 5000, 286)).tolist(); every[256] = 1
    fib = [0] * 286
    fib[256], a, b = 1, 1, 2                                    # 30 symbols with the counts 1, 1, 2, 3, 5, ...: the end-of-block
    for k in range(29):                                         # symbol takes the first 1
        fib[3 * k] = a
        a, b = b, a + b
    out = {'two': two, 'dominating': dominating, 'all286': every, 'fibonacci': fib, 'equal': [1] * 286}
    for k in range(12):
        h = np.zeros(286, np.int64)
        used = rng.choice(286, int(rng.integers(2, 286)), replace=False)
        h[used] = np.maximum(1, (rng.pareto(0.7, len(used)) * 20)).astype(np.int64)
        h[256] = 1
        out['random%d' % k] = h.tolist()
    return out


HISTOGRAMS = _special_histograms()


@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_code_lengths_are_complete_limited_optimal_and_agree(name):
    hist = HISTOGRAMS[name]
    cost, depth = huffman(hist)
    if name == 'fibonacci':
        assert depth == 29
    got = {}
    for who, fn in BUILDERS.items():
        ln = fn(hist, 15)
        got[who] = ln
        assert all((l > 0) == (c > 0) for l, c in zip(ln, hist)), who
        assert max(ln) <= 15, who
        assert sum(Fraction(1, 2 ** l) for l in ln if l) == 1, who
        mine = sum(l * c for l, c in zip(ln, hist))
        assert mine >= cost and (depth > 15 or mine == cost), (who, mine, cost, depth)
        # a higher count never gets a longer code; of two equal counts the lower symbol never gets the longer one
        used = sorted((s for s in range(286) if hist[s]), key=lambda s: (hist[s], -s))
        assert all(ln[a] >= ln[b] for a, b in zip(used, used[1:])), who
    assert got['product'] == got['restatement']


@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_block_header_and_sizes_agree(name):
    from cartoonsegmentation_amd import pngcode
    hist = HISTOGRAMS[name]
    p, r = pngcode.build_code(hist), R.build(hist)
    assert p['btype'] == r['btype'] and list(p['lengths']) == list(r['lengths']) and p['dist_bits'] == r['dist_bits']
    assert list(p['codes']) == [R.mirrored(c, n) for c, n in zip(r['codes'], r['lengths'])]
    assert p['header'] & 0xFFFF == 0x0178
    assert [(p['header'] >> (16 + k)) & 1 for k in range(p['header_bits'] - 16)] == list(r['header'])
    assert (p['fixed_bits'] - 16, p['dynamic_bits'] - 16, p['bits'] - 16, p['bytes']) == (r['fixed_bits'], r['dynamic_bits'], r['bits'], r['bytes'])
    assert p['btype'] == (2 if p['dynamic_bits'] < p['fixed_bits'] else 1)
    # the fixed size from RFC 1951 §3.2.6 alone
    fixed = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    extra = [0] * 257 + [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    assert r['fixed_bits'] == 3 + sum(c * (fixed[s] + extra[s] + (5 if s > 256 else 0)) for s, c in enumerate(hist))


def test_code_length_code_stays_within_seven_bits():
    """the dynamic headers of the histograms above, re-read: HCLEN lengths <= 7 and complete, and the lengths they spell are the code's"""
    for name, hist in sorted(HISTOGRAMS.items()):
        code = R.build(hist)
        if code['btype'] != 2:
            continue
        bits = code['header']
        take = lambda at, n: sum(bits[at + k] << k for k in range(n))   # noqa: E731
        assert take(0, 3) == 0b101                              # BFINAL 1, BTYPE 2
        hlit, hdist, hclen = take(3, 5) + 257, take(8, 5) + 1, take(13, 4) + 4
        cl = [0] * 19
        for k in range(hclen):
            cl[R.ORDER_OF_CODE_LENGTHS[k]] = take(17 + 3 * k, 3)
        assert max(cl) <= 7 and sum(Fraction(1, 2 ** l) for l in cl if l) == 1, name
        assert hdist == 1 and 257 <= hlit <= 286


TIES = [{151: 7, 175: 2, 228: 7}, {31: 8, 56: 6, 75: 5}, {101: 10, 178: 3, 200: 3}]


@pytest.mark.parametrize("k", range(len(TIES)))
def test_fixed_code_wins_a_tie(k):
    from cartoonsegmentation_amd import pngcode
    hist = [0] * 286
    for s, c in TIES[k].items():
        hist[s] = c
    hist[256] = 1
    for b in (pngcode.build_code(hist), R.build(hist)):
        assert b['fixed_bits'] == b['dynamic_bits'] and b['btype'] == 1 and b['dist_bits'] == 5
    more = list(hist); more[min(TIES[k])] += 40                  # more of one symbol: now the dynamic code is smaller
    for b in (pngcode.build_code(more), R.build(more)):
        assert b['dynamic_bits'] < b['fixed_bits'] and b['btype'] == 2 and b['dist_bits'] == 1


def test_tiny_images_take_the_fixed_code():
    data, _ = want('grey-1x1-0')
    assert len(data) == 8 + 25 + 12 + 12 + (2 + 4 + 4)           # signature, IHDR, IDAT, IEND; the block: 3 + 8 + 8 + 7 bits
    assert chunks(data)[1][1][2] & 7 == 0b011                   # BFINAL 1, BTYPE 1


def test_table_row_layout():
    from cartoonsegmentation_amd import pngcode
    hist = HISTOGRAMS['random0']
    code = pngcode.build_code(hist)
    row = pngcode.table_row(code, 0xDEADBEEF, (5 << 32) + 64)
    assert row.dtype == np.uint32 and row.shape == (384,)
    assert all(int(row[s]) == code['codes'][s] | code['lengths'][s] << 16 for s in range(286))
    assert (int(row[286]), int(row[287]), int(row[288]), int(row[289]), int(row[290]), int(row[291])) == \
        (code['header_bits'], 0xDEADBEEF, 64, 5, code['dist_bits'], code['bytes'])
    words = (code['header_bits'] + 31) // 32
    assert sum(int(row[292 + k]) << 32 * k for k in range(words)) == code['header'] and not row[292 + words:].any()


def test_product_container_equals_the_restatement():
    from cartoonsegmentation_amd import pngcode
    for name in ('bgr-17x23-0', 'grey-17x23-0', 'disc'):
        a = image(name)
        assert pngcode.png_file(R.stream(a), a.shape[1], a.shape[0], 2 if a.ndim == 3 else 0) == want(name)[0]


# ---- sizes ------------------------------------------------------------------------------------------------------------------
def test_flat_and_mask_images_compress_as_the_contract_demands():
    flat, _ = want('flat64x1024')
    assert len(flat) < 64 * 1024 / 50, len(flat)
    disc, _ = want('disc')
    assert len(disc) < 256 * 256 / 25, len(disc)


def pil_level1(a):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(expected_pixels(a))).save(bio, 'PNG', compress_level=1)
    return len(bio.getvalue())


@pytest.mark.parametrize("name", ['bgr-128x160', 'bgr-243x317', 'synth'])
def test_size_against_pil_level_1(name):
    """measured: 0.90, 0.93 and 0.88 of PIL's compress_level=1 file"""
    from cartoonsegmentation_amd import synth
    a = {'bgr-128x160': lambda: cartoon(128, 160, 3), 'bgr-243x317': lambda: cartoon(243, 317, 5),
         'synth': lambda: synth.image_u8(320, 384, 11)}[name]()
    mine, pil = len(R.encode(a)), pil_level1(a)
    print("%s: %d B, PIL compress_level=1 %d B, ratio %.4f" % (name, mine, pil, mine / pil))
    assert mine <= 1.05 * pil, (mine, pil)


# ---- APNG -------------------------------------------------------------------------------------------------------------------
def check_apng(data, frames, order, fps=25):
    """an APNG of `frames` (arrays as given to the encoder) in `order`: chunk CRCs, acTL, the sequence numbers, and PIL's frames"""
    from PIL import Image
    cs = chunks(data)
    kinds = [k for k, _ in cs]
    n = len(order)
    assert kinds == [b'IHDR', b'acTL', b'fcTL', b'IDAT'] + [b'fcTL', b'fdAT'] * (n - 1) + [b'IEND']
    H, W = frames[0].shape[:2]
    assert struct.unpack('>II', cs[1][1]) == (n, 0)
    seq = 0
    for kind, body in cs[2:-1]:
        if kind == b'fcTL':
            assert struct.unpack('>IIIIIHHBB', body) == (seq, W, H, 0, 0, 1, fps, 0, 0)
            seq += 1
        elif kind == b'fdAT':
            assert struct.unpack('>I', body[:4])[0] == seq
            seq += 1
    assert seq == 2 * n - 1
    payloads = [b for k, b in cs if k == b'IDAT'] + [b[4:] for k, b in cs if k == b'fdAT']
    for i, p in zip(order, payloads):
        assert zlib.decompress(p) == R.filtered(frames[i]).tobytes()
    with Image.open(io.BytesIO(data)) as im:
        assert getattr(im, 'n_frames', 1) == n
        for k, i in enumerate(order):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert('RGB' if frames[i].ndim == 3 else 'L')), expected_pixels(frames[i])), (k, i)


@pytest.mark.parametrize("kind", ['bgr', 'grey'])
def test_write_apng_from_restatement_streams(kind, tmp_path):
    from cartoonsegmentation_amd import video
    frames = [image('%s-17x23-0' % kind), image('%s-17x23-0' % kind)[::-1].copy(), np.zeros_like(image('%s-17x23-0' % kind)),
              image('%s-17x23-0' % kind)[:, ::-1].copy()]
    streams = [R.stream(f) for f in frames]
    ct = 2 if kind == 'bgr' else 0
    for order in (None, [0, 1, 2, 3, 2, 1]):
        path = str(tmp_path / "a.apng")
        size = video.write_apng(path, streams, 23, 17, ct, fps=25, order=order)
        data = open(path, 'rb').read()
        assert size == len(data)
        used = list(range(4)) if order is None else order
        assert data == R.apng(streams, 23, 17, ct, 25, used)
        check_apng(data, frames, used)
    assert video.playback_order(4) == [0, 1, 2, 3, 2, 1]
    with pytest.raises(ValueError):
        video.write_apng(str(tmp_path / "b.apng"), streams, 23, 17, ct, order=[4])


def test_imwrite_refuses_an_unknown_suffix(tmp_path):
    from utils.io_utils import imwrite
    with pytest.raises(ValueError):
        imwrite(np.zeros((4, 4, 3), np.uint8), str(tmp_path / "a.bmp"))
    with pytest.raises(ValueError):
        imwrite(np.zeros((4, 4, 3), np.uint8), str(tmp_path / "a"))
    assert not os.listdir(str(tmp_path))
