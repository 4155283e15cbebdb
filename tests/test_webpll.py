"""CPU tests of the lossless WebP writer (contract DESIGN.md §4.13): the restatement's files decode under Pillow (libwebp) to their
input, bit for bit, and the host half of the product (cartoonsegmentation_amd/webpcode.py: the prefix codes, every header bit, the
sizes, the container) agrees with the restatement without a GPU.  tests/test_gpu_webpll.py holds the device half to the same
bytes."""
import functools
import heapq
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webpll_restatement as R  # noqa: E402

Image = pytest.importorskip("PIL.Image")


# ---- the cases (shared with tests/test_gpu_webpll.py) -------------------------------------------------------------------------
def mixed(H, W, C, seed):
    """flat areas, gradients, an edge and a noisy patch: blocks that prefer different predictor modes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    chans = [(xx * 3 + yy * (k + 1) + 40 * k) % 256 for k in range(3)]
    a = np.stack(chans, axis=-1)
    a[(yy // 9 + xx // 11) % 3 == 0] = (200, 30, 90)
    a[yy > xx + H // 3] = (10, 220, 130)
    h2, w2 = max(1, H // 3), max(1, W // 3)
    a[:h2, W - w2:] = rng.integers(0, 256, (h2, w2, 3))
    a = a.astype(np.uint8)
    if C == 1:
        return np.ascontiguousarray(a[..., 1])
    if C == 4:
        alpha = ((yy * 7 + xx * 5) % 256).astype(np.uint8)
        return np.concatenate([a, alpha[..., None]], axis=2)
    return a


def fibonacci_row():
    """a 1 x 6764 colour row whose green residuals follow a Fibonacci histogram of 18 symbols (a plain Huffman code would be 17
    deep, so the limit of 15 binds); the red residual alternates, so that no two neighbours are equal and nothing becomes a run"""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(18), fib)
    np.random.default_rng(4).shuffle(vals)
    n = len(vals)
    g = np.cumsum(vals) % 256
    rg = np.cumsum(1 + np.arange(n) % 2) % 256                  # red - green
    a = np.zeros((1, n, 3), np.uint8)
    a[0, :, 1], a[0, :, 2], a[0, :, 0] = g, (rg + g) % 256, g   # blue - green stays 0
    return a


def disc(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 2.5) ** 2


@functools.lru_cache(maxsize=None)
def image(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == '1x1':
        return np.array([[77]], np.uint8)
    if name == '1x1-bgra':
        return np.array([[[1, 2, 3, 4]]], np.uint8)
    if name == '1xW':
        return rng.integers(0, 256, (1, 37, 3), dtype=np.uint8)
    if name == 'Hx1':
        return rng.integers(0, 256, (37, 1), dtype=np.uint8)
    if name == 'max-w':
        return ((np.arange(16384) // 5) % 256).astype(np.uint8)[None, :]
    if name == 'max-h':
        a = np.zeros((16384, 1, 4), np.uint8)
        a[:, 0, :] = (np.arange(16384)[:, None] // np.array([3, 5, 7, 11])) % 256
        return a
    if name.startswith('block-'):                               # one below, at and one above the predictor block size
        h, w = (int(v) for v in name[6:].split('x'))
        return mixed(h, w, 3, 5)
    if name.startswith('stretch-'):                             # around a multiple of the parse kernel's thread stretch
        w = int(name[8:])
        a = rng.integers(0, 4, (3, w), dtype=np.uint8) * 60
        a[1, w // 3:] = 9
        return a
    if name.startswith('const-'):                               # a constant row: maximal references and their remainders
        return np.full((1, int(name[6:])), 7, np.uint8)
    if name == 'black-column':                                  # every residual is zero and no row has a run
        return np.zeros((40, 1), np.uint8)
    if name == 'one-colour':
        return np.full((40, 50, 3), (30, 60, 90), np.uint8)
    if name == 'two-colour':
        yy, xx = np.mgrid[:33, :47]
        return np.where(((yy // 5 + xx // 7) % 2 == 0)[..., None], (250, 10, 40), (0, 128, 255)).astype(np.uint8)
    if name == 'noise':
        return rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    if name == 'noise-bgra':
        return rng.integers(0, 256, (21, 19, 4), dtype=np.uint8)
    if name == 'fibonacci':
        return fibonacci_row()
    if name == 'opaque-bgra':
        a = mixed(40, 45, 4, 6).copy()
        a[..., 3] = 255
        return a
    if name == 'bordered-bgra':                                 # a cut-out: a zero-alpha, zero-colour border
        a = mixed(47, 65, 4, 7).copy()
        a[..., 3] |= 1
        a[:6] = 0; a[-5:] = 0; a[:, :7] = 0; a[:, -4:] = 0
        return a
    if name == 'mask':
        return disc(50, 60)
    if name == 'list-1x1x4':
        return np.array([[[9, 8, 7, 0]]], np.uint8)
    if name == 'list-5x300x3':
        return mixed(5, 300, 3, 8)
    if name == 'list-33x17':
        return mixed(33, 17, 1, 9)
    if name == 'list-bool-9x9':
        return disc(9, 9)
    raise KeyError(name)


BLOCKS = ['block-15x17', 'block-16x16', 'block-17x15', 'block-16x33']
STRETCHES = ['stretch-1023', 'stretch-1024', 'stretch-1025', 'stretch-1031']
CONSTS = ['const-8200', 'const-4098', 'const-4099', 'const-4100', 'const-4101']
MIXED_LIST = ['list-1x1x4', 'list-5x300x3', 'list-33x17', 'list-bool-9x9']
CASES = (['1x1', '1x1-bgra', '1xW', 'Hx1', 'max-w', 'max-h'] + BLOCKS + STRETCHES + CONSTS
         + ['black-column', 'one-colour', 'two-colour', 'noise', 'noise-bgra', 'fibonacci', 'opaque-bgra', 'bordered-bgra', 'mask'] + MIXED_LIST)


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's file of a case: computed once and shared"""
    return R.encode(image(name))


def expected_rgba(a):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8) * 255
    if a.ndim == 2:
        return np.stack([a, a, a, np.full_like(a, 255)], axis=-1)
    if a.shape[2] == 3:
        return np.concatenate([a[..., ::-1], np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return a[..., [2, 1, 0, 3]]


def check_file(data, a):
    """a complete, even-sized simple-format file with one VP8L chunk that Pillow decodes to `a` exactly, as RGBA exactly when `a`
    has four channels"""
    a = np.asarray(a)
    assert data[:4] == b'RIFF' and data[8:16] == b'WEBPVP8L' and len(data) % 2 == 0
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    size = struct.unpack('<I', data[16:20])[0]
    assert 20 + size + (size & 1) == len(data)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.format == 'WEBP' and im.size == (a.shape[1], a.shape[0])
    assert (im.mode == 'RGBA') == (a.ndim == 3 and a.shape[2] == 4), im.mode
    assert np.array_equal(np.asarray(im.convert('RGBA')), expected_rgba(a))


# ---- the restatement under libwebp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_files_decode_to_their_input(name):
    check_file(want(name), image(name))
    a = image(name)
    assert len(want(name)) <= R.worst_case_bytes(a.shape[1], a.shape[0])


def test_prediction_and_parse_on_known_images():
    # a black column: every residual is zero, every row one literal, every alphabet a simple code, the pixels cost no bit
    mode, res, _ = R.planes(image('black-column'))
    assert not res.any() and np.array_equal(mode, np.full((3, 1), 0xff000000, np.uint32))
    assert R.plane_bits(res) == (5 * 4, 0) and R.plane_bits(mode)[1] == 0
    # one colour: only pixel (0, 0) has a residual, and every block's mode is 1 (L: the lowest of the modes that tie at zero)
    mode, res, _ = R.planes(image('one-colour'))
    assert np.count_nonzero(res) == 1 and res[0, 0] == (0 << 24 | (90 - 60) << 16 | 60 << 8 | ((30 - 60) & 255))
    assert np.array_equal(mode, np.full(mode.shape, 0xff000100, np.uint32))
    # a constant row: pixel (0, 0), a literal, two references of 4096, one of the remainder
    assert R.tokens(R.planes(image('const-8200'))[1]) == [('lit', 7 << 8), ('lit', 0), ('ref', 4096), ('ref', 4096), ('ref', 6)]
    for w, rest in ((4098, [4096]), (4099, [4096, 1]), (4100, [4096, 2]), (4101, [4096, 3])):
        plane = R.planes(image('const-%d' % w))[1]
        assert R.tokens(plane) == [('lit', int(plane[0, 0])), ('lit', 0)] + [('ref', v) for v in rest]
    # the length and distance prefixes of the format
    assert [R.prefix(v) for v in (1, 2, 4, 5, 6, 7, 9, 4096)] == [(0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0), (6, 2, 0),
                                                                 (23, 10, 1023)]


def test_modes_differ_between_blocks_and_ties_go_low():
    mode, _, _ = R.planes(mixed(64, 80, 3, 3))
    assert len(np.unique(mode)) >= 3                             # the candidates are really chosen among
    flat = np.zeros((16, 16, 3), np.uint8)
    assert (R.planes(flat)[0] >> 8 & 255).tolist() == [[0]]


# ---- the product's host half ---------------------------------------------------------------------------------------------------
def _huffman_depth(hist):
    heap = [(c, 0) for c in hist if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def _bits():
    from cartoonsegmentation_amd.pngcode import _Bits
    return _Bits()


def test_code_builder_is_complete_limited_and_agrees_with_the_restatement():
    from cartoonsegmentation_amd import webpcode
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    geometric = [2 ** k for k in range(24)]
    rng = np.random.default_rng(2)
    for hist in (fib + [0] * 250, [0] * 7 + geometric + [0] * 225, rng.integers(0, 50, 256).tolist(), [5, 0, 9] + [0] * 37,
                 rng.integers(1, 3, 280).tolist()):
        b = _bits()
        lengths, codes = webpcode.ll_write_code(b, hist)
        used = [l for l in lengths if l]
        assert sum(2.0 ** -l for l in used) == 1.0 and max(used) <= 15
        assert all((l > 0) == (c > 0) for l, c in zip(lengths, hist))
        w = R.BitWriter()
        want_len, want_codes = R.write_code(w, hist)
        assert lengths == want_len and b.n == len(w.bits)
        assert [(b.value >> k) & 1 for k in range(b.n)] == w.bits
        assert codes == [R.mirrored(c, l) for c, l in zip(want_codes, want_len)]
    for hist in (fib + [0] * 250, [0] * 7 + geometric + [0] * 225):
        assert _huffman_depth(hist) > 15 and max(webpcode.ll_write_code(_bits(), hist)[0]) == 15   # the limit binds


def test_simple_code_rule():
    from cartoonsegmentation_amd import webpcode
    for hist, bits in (([0] * 40, [1, 0, 0, 0]), ([0, 3] + [0] * 38, [1, 0, 0, 1]),
                       ([0] * 255 + [9], [1, 0, 1] + [1] * 8), ([0, 0, 4] + [0] * 253, [1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0])):
        b = _bits()
        lengths, codes = webpcode.ll_write_code(b, hist)
        assert not any(lengths) and not any(codes)              # zero bits per occurrence
        assert [(b.value >> k) & 1 for k in range(b.n)] == bits
    lengths, _ = webpcode.ll_write_code(_bits(), [0, 3, 0, 7] + [0] * 252)
    assert lengths[:4] == [0, 1, 0, 1]                          # two used symbols: a normal code of two 1-bit codes
    with pytest.raises(ValueError):
        webpcode.ll_write_code(_bits(), [0] * 256 + [5] + [0] * 23)


@pytest.mark.parametrize("name", ['1x1', 'black-column', 'one-colour', 'noise', 'noise-bgra', 'fibonacci', 'bordered-bgra', 'mask', 'const-8200',
                                  'block-16x33'])
def test_sizes_from_histograms_equal_the_bytes_written(name):
    """everything the host decides comes from the histograms alone: the payload's size, where each plane's pixels begin, and the
    header bits in front of them, which are the restatement's bits at those places"""
    from cartoonsegmentation_amd import webpcode
    a = image(name)
    mode, res, has_alpha = R.planes(a)
    payload = R.payload(a)
    code = webpcode.ll_image_code(np.concatenate(R.histograms(mode)), np.concatenate(R.histograms(res)), a.shape[1], a.shape[0], has_alpha)
    assert code['bytes'] == len(payload) and (code['bits'] + 7) // 8 == len(payload)
    bits = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder='little')
    for plane, img in zip(code['planes'], (mode, res)):
        head, pixels = R.plane_bits(img)
        assert plane['pixel_bits'] == pixels
        assert plane['start'] == plane['header_at'] + plane['header_bits']
        got = [(plane['header'] >> k) & 1 for k in range(plane['header_bits'])]
        assert got == bits[plane['header_at']:plane['start']].tolist()
        row = webpcode.ll_table_row(plane, 64, code['bytes'])
        assert row.shape == (webpcode.LL_TABLE_WORDS,) and row[1088] == 64 and row[1090] == len(payload)
        assert int(row[1091]) | int(row[1092]) << 32 == plane['start'] and row[1093] == plane['header_at'] // 32
        words = sum(int(v) << (32 * k) for k, v in enumerate(row[1095:1095 + int(row[1094])]))
        assert words == plane['header'] << (plane['header_at'] % 32)
    assert code['planes'][1]['header_at'] == code['planes'][0]['start'] + code['planes'][0]['pixel_bits']
    assert code['bits'] == code['planes'][1]['start'] + code['planes'][1]['pixel_bits']
    if name in ('1x1', 'black-column'):
        assert code['planes'][0]['pixel_bits'] == code['planes'][1]['pixel_bits'] == 0       # simple codes only


def test_prefix_extra_bits_agree():
    from cartoonsegmentation_amd import webpcode
    for v in range(1, 4097):
        p, eb, _ = R.prefix(v)
        assert webpcode.ll_prefix_extra_bits(p) == eb and p < 24


def test_container_lengths_and_padding():
    from cartoonsegmentation_amd import webpcode
    for payload in (b'\x2f' + bytes(8), b'\x2f' + bytes(9)):
        f = webpcode.lossless_file(payload)
        assert f == R.container(payload) and len(f) % 2 == 0
        assert struct.unpack('<I', f[4:8])[0] == len(f) - 8 and struct.unpack('<I', f[16:20])[0] == len(payload)
        assert f[20:20 + len(payload)] == payload and f[20 + len(payload):] == (b'\x00' if len(payload) & 1 else b'')
    with pytest.raises(ValueError):
        webpcode.ll_check_size(16385, 1)
    with pytest.raises(ValueError):
        webpcode.ll_check_size(1, 0)
    assert webpcode.ll_check_size(16384, 16384) == (16384, 16384)


def test_worst_case_cap():
    """§4.13's cap: every pixel of both planes as four literals of 15 bits, ten headers of the longest form.  It is derived, not
    measured: no case may exceed it, and noise, the worst content, stays within it."""
    from cartoonsegmentation_amd import webpcode
    for W, H in ((1, 1), (53, 37), (16384, 1), (300, 5), (1024, 1024)):
        assert webpcode.ll_worst_case_bytes(W, H) == R.worst_case_bytes(W, H)
    assert R.worst_case_bytes(1, 1) == 20 + 2006                # 53 + 2 * 7931 + 60 * 2 bits = 16035 bits = 2005 bytes, padded
    for name in ('noise', 'noise-bgra'):
        a = image(name)
        assert len(want(name)) <= R.worst_case_bytes(a.shape[1], a.shape[0])
        assert len(want(name)) > a.size // 2                    # (noise does not compress: the cap is not idle)


# ---- sizes --------------------------------------------------------------------------------------------------------------------
def soft_cutout():
    """a BGRA cut-out with a soft edge: a disc of cartoon(243, 317, 5) whose alpha falls off over 6 px, colour zero outside"""
    from test_mjpeg import cartoon
    img = cartoon(243, 317, 5)
    yy, xx = np.mgrid[:243, :317]
    alpha = (np.clip((100 - np.hypot(yy - 120, xx - 160)) / 6, 0, 1) * 255).astype(np.uint8)
    out = np.concatenate([np.where(alpha[..., None] > 0, img, 0), alpha[..., None]], axis=2).astype(np.uint8)
    return np.ascontiguousarray(out[14:227, 54:267])


def _size_fixture(name):
    from cartoonsegmentation_amd import synth
    from test_mjpeg import cartoon
    return {'cartoon-128x160': lambda: cartoon(128, 160, 3), 'cartoon-243x317': lambda: cartoon(243, 317, 5),
            'synth-320x384': lambda: synth.image_u8(320, 384, 11), 'soft-cutout': soft_cutout}[name]()


# the restatement's measured ratio to Pillow save(lossless=True, method=0) on §4.7's fixtures and one soft-edged cut-out
# (Pillow 12.2: 0.938, 0.943, 0.894, 0.915), plus 5 % for future contract tweaks
@pytest.mark.parametrize("name,bound", [('cartoon-128x160', 0.988), ('cartoon-243x317', 0.993), ('synth-320x384', 0.944), ('soft-cutout', 0.965)])
def test_size_against_pillow_method_0(name, bound):
    a = _size_fixture(name)
    ours = R.encode(a)
    check_file(ours, a)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a[..., ::-1] if a.shape[2] == 3 else a[..., [2, 1, 0, 3]])).save(buf, 'WEBP', lossless=True, method=0)
    ratio = len(ours) / len(buf.getvalue())
    print("%s: ours %d bytes, Pillow method=0 %d, ratio %.3f (bound %.3f)" % (name, len(ours), len(buf.getvalue()), ratio, bound))
    assert ratio <= bound
