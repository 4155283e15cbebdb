"""GPU: the WebP writer's method 1 (csrc/webp.hip: B_PRED and probability updates; contract DESIGN.md §4.12b) is byte-identical to its
restatement (tests/webp_m1_restatement.py) through ops.webp_streams and ops.webp_encode, whole, in chunks and on another stream; the
device's own lossy decoder reads the files back to the restatement's reconstruction; npyframes2video's .webp route; a 1024x1024
frame against method 0."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as R  # noqa: E402
from test_mjpeg import cartoon, psnr  # noqa: E402
from test_webp import SHAPES, frame, pil_frames  # noqa: E402
from test_webp_method1 import large, want1  # noqa: E402

NAMES = ('1x1', '16x16', '17x33', '31x16', '16x31', '48x64', '100x101', 'black', 'white', 'noise', 'gradient', '243x317', '16x1120')
CASES = [(name, q) for name in NAMES for q in SHAPES[name][2]]
IDS = ["%s-q%d" % c for c in CASES]


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


def _clip(name, n):
    return torch.from_numpy(np.stack([frame(name, v) for v in range(n)])).cuda()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("name,quality", CASES, ids=IDS)
def test_method1_streams_are_byte_identical_to_the_restatement(name, quality, n):
    """n = 5 different frames: one coder workgroup holds several frames' probability tables"""
    from cartoonsegmentation_amd import ops
    H, W, _ = SHAPES[name]
    dev = _clip(name, n)
    got, w, h = ops.webp_streams(dev, quality=quality, method=1)
    assert (w, h) == (W, H) and len(got) == n and all(isinstance(g, bytes) for g in got)
    for v, g in enumerate(got):
        assert g == want1(name, quality, v)['vp8'], (name, quality, v) + _first_difference(g, want1(name, quality, v)['vp8'])
    assert ops.webp_encode(dev, quality=quality, method=1) == [R.still_file(g) for g in got]
    if n == 1:
        assert ops.webp_streams(dev[0], quality=quality, method=1)[0] == got       # [H,W,3] is a clip of one frame


def test_method1_chunks_second_call_and_another_stream_give_the_same_bytes(monkeypatch):
    from cartoonsegmentation_amd import ops
    dev = _clip('100x101', 5)
    expect = [want1('100x101', 90, v)['vp8'] for v in range(5)]
    assert ops.webp_streams(dev, method=1)[0] == expect
    assert ops.webp_streams(dev, method=1)[0] == expect                            # a second call
    monkeypatch.setattr(ops, 'WEBP_SCRATCH_BYTES', 1)                              # one frame per call
    assert ops.webp_streams(dev, method=1)[0] == expect
    per_frame = int(ops._lib.load().csm_webp_scratch_bytes_m(1, 101, 100, 1))
    monkeypatch.setattr(ops, 'WEBP_SCRATCH_BYTES', 2 * per_frame + 1)              # chunks of 2, 2 and 1 frames
    assert ops.webp_streams(dev, method=1)[0] == expect
    monkeypatch.undo()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.webp_streams(dev, method=1)[0]
    torch.cuda.current_stream().wait_stream(side)
    assert got == expect
    assert ops.webp_streams(dev[::2], method=1)[0] == expect[::2]                  # a non-contiguous view
    assert ops.webp_streams(dev[:0], method=1)[0] == [] and ops.webp_encode(dev[:0], method=1) == []
    assert ops.webp_streams(dev, method=0)[0] == ops.webp_streams(dev)[0] != expect


@pytest.mark.parametrize("name,quality", [('17x33', 90), ('100x101', 50), ('noise', 90), ('gradient', 90), ('243x317', 90), ('black', 90)])
def test_the_device_decoder_reads_method1_files_back(name, quality):
    """the GPU decoder's B_PRED and probability-update paths on files that Pillow did not write: every byte is what the restatement
    predicts a decoder shows"""
    from cartoonsegmentation_amd import ops
    H, W, _ = SHAPES[name]
    n = 3
    files = ops.webp_encode(_clip(name, n), quality=quality, method=1)
    back = ops.webp_decode(files, lossy=True)
    for v, t in enumerate(back):
        expect = R.decoded_rgb(want1(name, quality, v), H, W)[:, :, ::-1]
        assert np.array_equal(t.cpu().numpy(), expect), (name, quality, v)


def test_npyframes2video_webp_route_with_method1(tmp_path):
    from anime_3dkenburns import npyframes2video
    from cartoonsegmentation_amd import video, webpcode
    n = 5
    frames = [frame('48x64', v) for v in range(n)]
    results = [want1('48x64', 90, v) for v in range(n)]
    a, b = str(tmp_path / "a.webp"), str(tmp_path / "b.webp")
    npyframes2video(_clip('48x64', n), a, playback=True, method=1)
    npyframes2video(frames, b, playback=False, method=1)
    assert open(a, 'rb').read() == webpcode.animation_file([r['vp8'] for r in results], 64, 48, fps=25, order=[0, 1, 2, 3, 4, 3, 2, 1])
    assert open(b, 'rb').read() == webpcode.animation_file([r['vp8'] for r in results], 64, 48)
    got, durations = video.read_webp(b)
    assert tuple(got.shape) == (n, 48, 64, 3) and durations == [40] * n
    for v in range(n):
        assert np.array_equal(got[v].cpu().numpy(), R.decoded_rgb(results[v], 48, 64)[:, :, ::-1]), v
    with pytest.raises(ValueError):
        npyframes2video(frames, a, method=2)


def test_a_frame_of_1024x1024_is_smaller_and_no_worse_than_method_0():
    from cartoonsegmentation_amd import ops
    f = cartoon(1024, 1024, seed=0)
    dev = torch.from_numpy(f).cuda()
    one, zero = ops.webp_encode(dev, quality=90, method=1)[0], ops.webp_encode(dev, quality=90, method=0)[0]
    shown, size, frames, _, _ = pil_frames(one)
    assert size == (1024, 1024) and frames == 1
    r = large()
    assert one == R.still_file(r['vp8']), _first_difference(one, R.still_file(r['vp8']))
    assert np.array_equal(shown[0], R.decoded_rgb(r, 1024, 1024))
    p1, p0 = psnr(shown[0], f[:, :, ::-1]), psnr(pil_frames(zero)[0][0], f[:, :, ::-1])
    print("1024x1024 at quality 90: method 1 %d bytes %.2f dB, method 0 %d bytes %.2f dB" % (len(one), p1, len(zero), p0))
    assert p1 >= p0 and len(one) < len(zero), (p1, p0, len(one), len(zero))
