"""GPU: the HIP WebP writer (csrc/webp.hip + webpcode.py) is byte-identical to its numpy restatement (tests/webp_restatement.py,
contract DESIGN.md §4.12) through ops.webp_streams and ops.webp_encode; Pillow decodes the files; npyframes2video's .webp route."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as R  # noqa: E402
from test_mjpeg import cartoon, psnr  # noqa: E402
from test_webp import CASES, IDS, OUR_LOWEST_PSNR_Q90_DB, SHAPES, frame, pil_frames, want  # noqa: E402


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


def _clip(name, n):
    return torch.from_numpy(np.stack([frame(name, v) for v in range(n)])).cuda()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("name,quality", CASES, ids=IDS)
def test_streams_are_byte_identical_to_the_restatement(name, quality, n):
    from cartoonsegmentation_amd import ops
    H, W, _ = SHAPES[name]
    dev = _clip(name, n)
    got, w, h = ops.webp_streams(dev, quality=quality)
    assert (w, h) == (W, H) and len(got) == n and all(isinstance(g, bytes) for g in got)
    for v, g in enumerate(got):
        assert g == want(name, quality, v)['vp8'], (name, quality, v) + _first_difference(g, want(name, quality, v)['vp8'])
    files = ops.webp_encode(dev, quality=quality)
    assert files == [R.still_file(g) for g in got]
    if n == 1:
        assert ops.webp_streams(dev[0], quality=quality)[0] == got                 # [H,W,3] is a clip of one frame
        shown, size, frames, _, _ = pil_frames(files[0])
        assert size == (W, H) and frames == 1 and np.array_equal(shown[0], R.decoded_rgb(want(name, quality), H, W))


def test_chunks_second_call_and_another_stream_give_the_same_bytes(monkeypatch):
    from cartoonsegmentation_amd import ops
    dev = _clip('100x101', 5)
    expect = [want('100x101', 90, v)['vp8'] for v in range(5)]
    assert ops.webp_streams(dev)[0] == expect
    assert ops.webp_streams(dev)[0] == expect                                      # a second call
    monkeypatch.setattr(ops, 'WEBP_SCRATCH_BYTES', 1)                              # one frame per call
    assert ops.webp_streams(dev)[0] == expect
    monkeypatch.undo()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.webp_streams(dev)[0]
    torch.cuda.current_stream().wait_stream(side)
    assert got == expect
    assert ops.webp_streams(dev[::2])[0] == expect[::2]                            # a non-contiguous view
    assert ops.webp_streams(dev[:0])[0] == [] and ops.webp_encode(dev[:0]) == []


def test_npyframes2video_webp_route(tmp_path):
    """a device tensor and a list of numpy frames give the same file: webpcode over the restatement's streams, with the ping-pong
    order 2n - 2 frames of 40 ms"""
    from anime_3dkenburns import npyframes2video
    from cartoonsegmentation_amd import webpcode
    n = 5
    frames = [frame('48x64', v) for v in range(n)]
    streams = [want('48x64', 90, v)['vp8'] for v in range(n)]
    a, b, c = str(tmp_path / "a.webp"), str(tmp_path / "b.WEBP"), str(tmp_path / "c.webp")
    npyframes2video(_clip('48x64', n), a, playback=True)
    npyframes2video(frames, b, playback=True)                                      # the suffix in any letter case
    data = open(a, 'rb').read()
    assert data == open(b, 'rb').read() == webpcode.animation_file(streams, 64, 48, fps=25, order=[0, 1, 2, 3, 4, 3, 2, 1])
    shown, size, count, durations, loop = pil_frames(data)
    assert size == (64, 48) and count == 2 * n - 2 and durations == [40] * count and loop == 0
    npyframes2video(frames, c, playback=False, quality=50)
    assert open(c, 'rb').read() == webpcode.animation_file([want('48x64', 50, v)['vp8'] for v in range(n)], 64, 48)


def test_a_frame_of_1024x1024_decodes():
    """size and a PSNR floor only: the lowest PSNR of the 243x317 table at quality 90, minus 3 dB"""
    from cartoonsegmentation_amd import ops
    f = cartoon(1024, 1024, seed=0)
    data = ops.webp_encode(torch.from_numpy(f).cuda(), quality=90)[0]
    shown, size, frames, _, _ = pil_frames(data)
    got = psnr(shown[0], f[:, :, ::-1])
    print("1024x1024 at quality 90: %d bytes, %.2f dB" % (len(data), got))
    assert size == (1024, 1024) and frames == 1
    assert got >= OUR_LOWEST_PSNR_Q90_DB - 3.0, got
