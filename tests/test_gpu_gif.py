"""GPU: the HIP GIF writer (csrc/gif.hip + gifcode.py) is byte-identical to its numpy restatement (tests/gif_restatement.py, contract
DESIGN.md §4.10) through ops.gif_streams, ops.gif_quantize and ops.gif_encode; Pillow decodes the files; npyframes2video's .gif
route."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gif_restatement as R  # noqa: E402
from test_gif import CASES, PALETTE, check_gif, colour_frames, indices, pil_frames, want  # noqa: E402


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_streams_are_byte_identical_to_the_restatement(name, n):
    from cartoonsegmentation_amd import gifcode, ops
    clip = [indices(name, v) for v in range(n)]
    H, W = clip[0].shape
    got, w, h = ops.gif_streams(torch.from_numpy(np.stack(clip)).cuda())
    assert (w, h) == (W, H) and len(got) == n and all(isinstance(g, bytes) for g in got)
    for v, g in enumerate(got):
        assert g == want(name, v)[0], (name, v) + _first_difference(g, want(name, v)[0])
    check_gif(gifcode.gif_file(got, W, H, PALETTE), clip, PALETTE)
    if n == 1:
        assert ops.gif_streams(torch.from_numpy(np.array(clip[0])).cuda())[0] == got          # [H,W] is a clip of one frame


@pytest.mark.parametrize("name", ['noise', 'five'])
def test_cell_table_equals_the_restatement(name):
    """2 random BGR frames of 17x23, and 2 of 40x56 that hold only 5 colours (so most pixels share an LDS slot)"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, i64, ptr, stream_ptr
    frames = colour_frames(name)
    dev = torch.from_numpy(frames).cuda()
    for bgr in (True, False):
        table = torch.empty((32768, 4), dtype=torch.int32, device='cuda')
        check(_lib.load().csm_gif_histogram(ptr(dev), i64(frames.size // 3), i32(1 if bgr else 0), ptr(table), stream_ptr()), "hist")
        assert np.array_equal(table.cpu().numpy().view(np.uint32), R.cell_table(frames, bgr))


def test_cell_table_of_more_pixels_than_one_workgroup_takes():
    """3 frames of 61x67: 12 261 pixels, two workgroups, the second one partly filled; random colours collide in the LDS slots"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, i64, ptr, stream_ptr
    frames = np.random.default_rng(5).integers(0, 256, (3, 61, 67, 3), dtype=np.uint8)
    table = torch.empty((32768, 4), dtype=torch.int32, device='cuda')
    check(_lib.load().csm_gif_histogram(ptr(torch.from_numpy(frames).cuda()), i64(frames.size // 3), i32(1), ptr(table), stream_ptr()), "hist")
    assert np.array_equal(table.cpu().numpy().view(np.uint32), R.cell_table(frames))


@pytest.mark.parametrize("name", ['noise', 'five', 'smooth'])
def test_quantize_equals_the_restatement(name):
    from cartoonsegmentation_amd import gifcode, ops
    frames = colour_frames(name)
    dev = torch.from_numpy(frames).cuda()
    for bgr in (True, False):
        pal = gifcode.build_palette(R.cell_table(frames, bgr))
        for dither in ('none', 'ordered'):
            idx, p = ops.gif_quantize(dev, dither=dither, bgr=bgr)
            assert idx.dtype == torch.uint8 and idx.is_cuda and tuple(idx.shape) == frames.shape[:3]
            assert p.dtype == np.uint8 and np.array_equal(p, pal)
            assert np.array_equal(idx.cpu().numpy(), R.quantize(frames, pal, dither, bgr)), (name, bgr, dither)
    # a passed palette (with duplicate entries: the lower index wins) skips the histogram
    given = PALETTE.copy()
    given[200] = given[10]
    for dither in ('none', 'ordered'):
        idx, p = ops.gif_quantize(dev, palette=given, dither=dither)
        assert np.array_equal(p, given)
        assert np.array_equal(idx.cpu().numpy(), R.quantize(frames, given, dither))
    one, _ = ops.gif_quantize(dev[1], palette=given)                                          # [H,W,3] is a clip of one frame
    assert np.array_equal(one.cpu().numpy(), R.quantize(frames[1], given, 'ordered'))


def test_grey_and_mask_input_keep_their_bytes():
    from cartoonsegmentation_amd import ops
    g = np.stack([indices('noise-50x91', v) for v in range(2)])
    idx, p = ops.gif_quantize(torch.from_numpy(g).cuda())
    assert np.array_equal(idx.cpu().numpy(), g) and np.array_equal(p, np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))
    m = g > 127
    idx, p2 = ops.gif_quantize(torch.from_numpy(m).cuda())
    assert idx.dtype == torch.uint8 and np.array_equal(idx.cpu().numpy(), m * np.uint8(255)) and np.array_equal(p2, p)
    data = ops.gif_encode(torch.from_numpy(m).cuda())
    assert data == R.encode_indices(m * np.uint8(255), p)
    check_gif(data, list(m * np.uint8(255)), p)
    assert ops.gif_encode(torch.from_numpy(g).cuda()) == R.encode_indices(g, p)


@pytest.mark.parametrize("name", ['five', 'few'])
def test_a_clip_of_at_most_256_colours_round_trips_exactly(name):
    from cartoonsegmentation_amd import ops
    frames = colour_frames(name)
    for dither in ('ordered', 'none'):
        data = ops.gif_encode(torch.from_numpy(frames).cuda(), dither=dither)
        got, durations, loop = pil_frames(data)
        assert len(got) == frames.shape[0] and loop == 0 and durations == [40] * len(got)
        for g, f in zip(got, frames):
            assert np.array_equal(g, f[..., ::-1])


def test_chunked_encode_equals_one_call(monkeypatch):
    """frames beyond the scratch bound are coded in several library calls: the same bytes; non-contiguous views are taken"""
    from cartoonsegmentation_amd import ops
    frames = torch.from_numpy(np.stack([indices('rect-67x131', v) for v in range(5)])).cuda()
    whole = ops.gif_streams(frames)[0]
    assert whole == [want('rect-67x131', v)[0] for v in range(5)]
    monkeypatch.setattr(ops, 'GIF_SCRATCH_BYTES', 1)                         # one frame per call
    assert ops.gif_streams(frames)[0] == whole
    monkeypatch.undo()
    assert ops.gif_streams(frames[::2])[0] == whole[::2]                     # a non-contiguous view: every other frame
    assert ops.gif_streams(frames[:, ::2, 1::3])[0] == [R.lzw(f) for f in frames[:, ::2, 1::3].cpu().numpy()]
    colour = torch.from_numpy(colour_frames('smooth')).cuda()
    a = ops.gif_encode(colour)
    assert ops.gif_encode(colour) == a
    pal = ops.gif_quantize(colour)[1]
    assert ops.gif_quantize(colour[:, ::2, 1::3], palette=pal)[0].cpu().numpy().tobytes() == \
        R.quantize(colour_frames('smooth')[:, ::2, 1::3], pal).tobytes()
    assert ops.gif_streams(frames[:0])[0] == []


def test_npyframes2video_gif_route(tmp_path):
    """a device tensor and a list of numpy frames give the same file: ops.gif_encode with the ping-pong order; 2n - 2 frames of 40 ms"""
    from anime_3dkenburns import npyframes2video
    from cartoonsegmentation_amd import gifcode, ops, video
    frames = np.concatenate([colour_frames('smooth'), colour_frames('smooth')[:, ::-1]])      # 4 frames of 64x64
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    a, b = str(tmp_path / "a.GIF"), str(tmp_path / "b.gif")                  # the suffix in any letter case
    npyframes2video(dev, a, playback=True)
    npyframes2video(list(frames), b, playback=True)
    data = open(a, 'rb').read()
    assert data == open(b, 'rb').read() == ops.gif_encode(dev, order=video.playback_order(4))
    pal = gifcode.build_palette(R.cell_table(frames))
    idx = R.quantize(frames, pal, 'ordered')
    assert data == R.encode_indices(idx, pal, order=[0, 1, 2, 3, 2, 1])
    check_gif(data, list(idx), pal, [0, 1, 2, 3, 2, 1])
    npyframes2video(dev[:3], a, playback=False)
    assert open(a, 'rb').read() == ops.gif_encode(dev[:3])
