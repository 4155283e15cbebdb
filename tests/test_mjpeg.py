"""CPU: the baseline-JPEG contract of csrc/mjpeg.hip as restated in tests/mjpeg_restatement.py against an
independent decoder and encoder (PIL / libjpeg), and the Motion-JPEG AVI writer (cartoonsegmentation_amd/video.py) against a RIFF
parser written here from the container's layout."""
import io
import os
import struct
import sys

import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mjpeg_restatement as R  # noqa: E402
from cartoonsegmentation_amd import video  # noqa: E402

SIZES = [(8, 8), (17, 23), (64, 80), (100, 101), (243, 317), (720, 720)]
SUBSAMPLINGS = ['420', '444']
QUALITIES = [50, 90, 100]
PSNR_SLACK_DB = 1.0                    # below PIL's own encoder at the same settings
SIZE_RATIO = 1.15                      # of PIL's bytes, for frames of 64x80 and larger (the excess is the restart markers)


def cartoon(H, W, seed=0):
    """uint8 BGR [H,W,3]: a drawn-looking frame -- a smooth gradient, flat discs with hard edges, thin dark lines, a textured
    patch and a little sensor-like noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = float(max(H, W))
    img = np.stack([60 + 150 * x / s, 200 - 120 * y / s, 90 + 60 * (x + y) / (2 * s)], -1)
    for k in range(6):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.05, 0.25) * s
        img[np.hypot(y - cy, x - cx) < rad] = rng.uniform(0, 255, 3)
    img[(np.abs((x - y * 0.7) % 37.0) < 1.5)] *= 0.25
    ty, tx = H // 2, W // 2
    img[ty:, tx:] += 40 * np.sin(x[ty:, tx:, None] * 1.3) * np.cos(y[ty:, tx:, None] * 0.9)
    img += rng.normal(0, 2.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float((d * d).mean()), 1e-12))


def pil_encode(frame_bgr, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, 'JPEG', quality=quality,
                                                                      subsampling={'444': 0, '420': 2}[subsampling])
    return buf.getvalue()


def pil_decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.format == 'JPEG' and im.mode == 'RGB'
    return np.asarray(im)[:, :, ::-1]


def check_against_pil(stream, frame, quality, subsampling, label):
    """the decode rule of DESIGN §4.6: PIL decodes `stream` to the frame's size, at most PSNR_SLACK_DB below PIL's own encoder,
    and (from 64x80 on) in at most SIZE_RATIO of its bytes"""
    H, W = frame.shape[:2]
    dec = pil_decode(stream)
    assert dec.shape == (H, W, 3), label
    ref = pil_encode(frame, quality, subsampling)
    ours, pils = psnr(dec, frame), psnr(pil_decode(ref), frame)
    print("%s: psnr %.2f dB (PIL %.2f dB), %d bytes (PIL %d, x%.3f)" % (label, ours, pils, len(stream), len(ref), len(stream) / len(ref)))
    assert ours >= pils - PSNR_SLACK_DB, (label, ours, pils)
    if H * W >= 64 * 80:
        assert len(stream) <= SIZE_RATIO * len(ref), (label, len(stream), len(ref))


def segments(data):
    """[(marker, payload)] of the marker segments up to and including SOS, and the offset of the entropy data"""
    assert data[:2] == b'\xff\xd8'
    out, p = [(0xD8, b'')], 2
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        n = struct.unpack('>H', data[p + 2:p + 4])[0]
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out, p


# ---- decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("sub", SUBSAMPLINGS)
@pytest.mark.parametrize("H,W", SIZES)
def test_pil_decodes_the_restatement(H, W, sub, q):
    frame = cartoon(H, W, H * 1000 + W)
    check_against_pil(R.encode(frame, q, sub), frame, q, sub, "%dx%d %s q%d" % (H, W, sub, q))


# ---- tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 10, 50, 75, 90, 100])
def test_dqt_equals_pil(q):
    frame = cartoon(16, 16)
    ours = [p for m, p in segments(R.encode(frame, q, '420'))[0] if m == 0xDB]
    pil = b''.join(p for m, p in segments(pil_encode(frame, q, '420'))[0] if m == 0xDB)     # libjpeg may pack both in one segment
    assert len(ours) == 2 and [len(p) for p in ours] == [65, 65]
    assert b''.join(ours) == pil


def test_dht_equals_pil():
    frame = cartoon(16, 16)
    ours = [p for m, p in segments(R.encode(frame, 90, '420'))[0] if m == 0xC4]
    pil = b''.join(p for m, p in segments(pil_encode(frame, 90, '420'))[0] if m == 0xC4)
    assert len(ours) == 4 and [p[0] for p in ours] == [0x00, 0x10, 0x01, 0x11]
    assert b''.join(ours) == pil


def test_huffman_luts_are_complete_prefix_codes():
    for _, bits, vals in R.HUFF_SPECS:
        code, ln = R.huff_lut(bits, vals)
        words = sorted(format(int(code[v]), '0%db' % int(ln[v])) for v in vals)
        assert len(set(words)) == len(vals)
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))
        assert not any(w == '1' * len(w) for w in words)                   # no code of all ones (T.81 C.2)


# ---- stream structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBSAMPLINGS)
@pytest.mark.parametrize("H,W", [(8, 8), (17, 23), (100, 101), (243, 317)])
def test_stream_structure(H, W, sub):
    frame = cartoon(H, W, 7)
    data = R.encode(frame, 100, sub)
    segs, p = segments(data)
    assert [m for m, _ in segs] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert p == len(R.header(H, W, 100, sub)) == 629
    m = 16 if sub == '420' else 8
    mx, my = -(-W // m), -(-H // m)
    d = dict((k, v) for k, v in segs)
    assert d[0xE0] == b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
    assert struct.unpack('>H', d[0xDD])[0] == mx
    sof = d[0xC0]
    assert sof[0] == 8 and struct.unpack('>HH', sof[1:5]) == (H, W) and sof[5] == 3
    assert sof[6:] == bytes([1, 0x22 if sub == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert data[-2:] == b'\xff\xd9'
    body = data[p:-2]
    rst, i = [], 0
    while i < len(body):
        if body[i] == 0xFF:
            assert i + 1 < len(body), "a bare FF ends the entropy data"
            nxt = body[i + 1]
            assert nxt == 0 or 0xD0 <= nxt <= 0xD7, "bare FF %02x inside the entropy data" % nxt
            if nxt:
                rst.append(nxt - 0xD0)
            i += 2
        else:
            i += 1
    assert rst == [r % 8 for r in range(my - 1)]
    rows = R.entropy_segments(frame, 100, sub)
    assert len(rows) == my and all(len(r) > 0 for r in rows)


def test_restart_rows_are_independent():
    """a row's segment depends on its own pixels only: DC predictors restart at 0"""
    a = cartoon(64, 48, 1)
    b = a.copy()
    b[16:32] = cartoon(16, 48, 2)
    ra, rb = R.entropy_segments(a, 90, '420'), R.entropy_segments(b, 90, '420')
    assert ra[0] == rb[0] and ra[2] == rb[2] and ra[3] == rb[3] and ra[1] != rb[1]


def test_stuffing_and_zero_runs_are_exercised():
    """the frames the GPU parity tests use contain FF bytes to stuff and runs of 16 zeros (ZRL)"""
    frame = cartoon(100, 101, 100101)
    assert any(b'\xff\x00' in s for s in R.entropy_segments(frame, 100, '444'))
    q, _ = R.quantised_blocks(frame, 50, '420')
    nzpos = [np.nonzero(b[1:])[0] for b in q.reshape(-1, 64)]
    assert any(len(p) and (np.diff(np.concatenate([[-1], p])) > 16).any() for p in nzpos)


# ---- AVI -------------------------------------------------------------------------------------------------------------------
def parse_avi(data):
    """A RIFF parser from the container's layout (no helper of the writer): returns the header fields, the payload of every
    '00dc' chunk in file order and the idx1 entries, checking every size on the way."""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    out = {'chunks': [], 'offsets': []}

    def walk(p, end, depth):
        while p < end:
            cc, n = data[p:p + 4], struct.unpack('<I', data[p + 4:p + 8])[0]
            body = p + 8
            assert body + n <= end, (cc, n)
            if cc == b'LIST':
                kind = data[body:body + 4]
                out.setdefault('lists', []).append((kind, depth))
                if kind == b'movi':
                    out['movi'] = body                                       # position of the 'movi' fourcc
                walk(body + 4, body + n, depth + 1)
            elif cc == b'00dc':
                out['chunks'].append(data[body:body + n])
                out['offsets'].append(p)
            else:
                assert cc not in out, cc
                out[cc] = data[body:body + n]
            p = body + n
            if n & 1:
                assert data[p] == 0, "pad byte"
                p += 1
            assert p % 2 == 0
        assert p == end
    walk(12, len(data), 0)
    return out


def check_avi(data, jpegs, order, width, height, fps=25):
    a = parse_avi(data)
    assert a['lists'] == [(b'hdrl', 0), (b'strl', 1), (b'movi', 0)]
    n = len(order)
    avih = struct.unpack('<14I', a[b'avih'])
    assert avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == n and avih[6] == 1 and avih[8:10] == (width, height)
    strh = a[b'strh']
    assert len(strh) == 56 and strh[:8] == b'vidsMJPG'
    scale, rate, start, length = struct.unpack('<4I', strh[20:36])
    assert (scale, rate, start, length) == (1, fps, 0, n)
    assert struct.unpack('<4H', strh[48:56]) == (0, 0, width, height)
    strf = struct.unpack('<IiiHH4sIiiII', a[b'strf'])
    assert strf[:6] == (40, width, height, 1, 24, b'MJPG')
    assert len(a['chunks']) == n
    for k, i in enumerate(order):
        assert a['chunks'][k] == jpegs[i], k
    idx = a[b'idx1']
    assert len(idx) == 16 * n
    for k in range(n):
        cc, flags, off, size = struct.unpack('<4sIII', idx[16 * k:16 * k + 16])
        assert cc == b'00dc' and flags & 0x10 and size == len(a['chunks'][k])
        p = a['movi'] + off
        assert p == a['offsets'][k] and data[p:p + 4] == b'00dc' and struct.unpack('<I', data[p + 4:p + 8])[0] == size
    return a


def _fake_jpegs(n):
    rng = np.random.default_rng(n)
    return [b'\xff\xd8' + rng.integers(0, 255, 30 + 7 * k, dtype=np.uint8).tobytes() + b'\xff\xd9' for k in range(n)]


def test_avi_layout(tmp_path):
    jpegs = _fake_jpegs(7)
    assert {len(j) & 1 for j in jpegs} == {0, 1}                             # both paddings occur
    path = str(tmp_path / "a.avi")
    written = video.write_mjpeg_avi(path, jpegs, 320, 200)
    data = open(path, 'rb').read()
    assert written == len(data)
    check_avi(data, jpegs, list(range(7)), 320, 200)


def test_avi_order_and_playback(tmp_path):
    n = 6
    jpegs = _fake_jpegs(n)
    order = video.playback_order(n)
    assert order == list(range(n)) + list(range(n - 2, 0, -1)) and len(order) == 2 * n - 2
    path = str(tmp_path / "b.avi")
    video.write_mjpeg_avi(path, jpegs, 64, 48, fps=25, order=order)
    a = check_avi(open(path, 'rb').read(), jpegs, order, 64, 48)
    for k in range(n, 2 * n - 2):                                            # each reverse chunk equals its forward twin
        assert a['chunks'][k] == a['chunks'][2 * n - 2 - k]


def test_avi_of_real_streams_decodes(tmp_path):
    frames = [cartoon(40, 56, k) for k in range(3)]
    jpegs = [R.encode(f, 90, '420') for f in frames]
    path = str(tmp_path / "c.avi")
    video.write_mjpeg_avi(path, jpegs, 56, 40, order=video.playback_order(3))
    a = check_avi(open(path, 'rb').read(), jpegs, [0, 1, 2, 1], 56, 40)
    for k, i in enumerate([0, 1, 2, 1]):
        assert pil_decode(a['chunks'][k]).shape == (40, 56, 3)


def test_avi_refuses_bad_order_and_2gib(tmp_path, monkeypatch):
    jpegs = _fake_jpegs(2)
    with pytest.raises(ValueError):
        video.write_mjpeg_avi(str(tmp_path / "d.avi"), jpegs, 8, 8, order=[0, 2])
    assert video.MAX_FILE_BYTES == 2 ** 31
    size = video.write_mjpeg_avi(str(tmp_path / "d.avi"), jpegs, 8, 8)
    monkeypatch.setattr(video, 'MAX_FILE_BYTES', size)                       # the limit itself is refused ...
    with pytest.raises(ValueError):
        video.write_mjpeg_avi(str(tmp_path / "e.avi"), jpegs, 8, 8)
    assert not os.path.exists(str(tmp_path / "e.avi"))
    monkeypatch.setattr(video, 'MAX_FILE_BYTES', size + 1)                   # ... one byte below it is written
    assert video.write_mjpeg_avi(str(tmp_path / "e.avi"), jpegs, 8, 8) == size


# ---- error cases -----------------------------------------------------------------------------------------------------------
def test_bad_quality_raises_value_error():
    torch = pytest.importorskip("torch")
    from cartoonsegmentation_amd import ops
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for q in (0, 101):
        with pytest.raises(ValueError):
            ops.jpeg_encode(x, quality=q)
        with pytest.raises(ValueError):
            R.encode(np.zeros((8, 8, 3), np.uint8), q)
    with pytest.raises(ValueError):
        ops.jpeg_encode(x, subsampling='422')


def test_cpu_tensor_raises_csm_error():
    torch = pytest.importorskip("torch")
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    with pytest.raises(CsmError):
        ops.jpeg_encode(torch.zeros((8, 8, 3), dtype=torch.uint8))
    with pytest.raises(CsmError):
        ops.jpeg_encode(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), quality=50, subsampling='444')


def test_other_suffixes_keep_the_moviepy_route(monkeypatch):
    from cartoonsegmentation_amd.kenburns import npyframes2video
    monkeypatch.setitem(sys.modules, 'moviepy.editor', None)                 # the import fails, as where moviepy is absent
    with pytest.raises(RuntimeError, match="moviepy"):
        npyframes2video([np.zeros((8, 8, 3), np.uint8)] * 3, "out.mp4", playback=True)
