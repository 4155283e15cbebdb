"""GPU: ops.gif_decode (csrc/gifdec.hip) equals Pillow's seek(i) on every byte over the files of tests/gifdec_cases.py (DESIGN.md
§4.17), with and without alpha, alone and with all files in one call, under any scratch budget; video.read_gif / read_avi /
read_apng / read_video read back what the project's writers write; utils.io_utils.imread_device_many routes .gif files only with its
option on.  The two corrupt streams decoded here have passed the host walker under the sanitizers first (tests/test_gifdec.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gifdec_cases as C  # noqa: E402
from cartoonsegmentation_amd import _lib, gifread, ops, video  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def together():
    """every file in one call, per alpha: mixed sizes and frame counts"""
    out = {}
    for alpha in (False, True):
        stats = {}
        got = ops.gif_decode([C.case_file(name) for name in C.NAMES], alpha=alpha, stats=stats)
        assert isinstance(got, list) and len(got) == len(C.NAMES) and len(stats['rounds']) == 1
        out[alpha] = (dict(zip(C.NAMES, got)), stats)
    return out


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("name", C.NAMES)
def test_decode_equals_pillow(name, alpha, together):
    data = C.case_file(name)
    gifread.probe(data)                           # every case must be one the decoder takes: none drops out silently
    want = C.reference(name, alpha)
    t = ops.gif_decode(data, alpha=alpha)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    got = t.cpu().numpy()
    for k in range(len(want)):
        wrong = int((got[k] != want[k]).any(axis=-1).sum())
        assert wrong == 0, "%s frame %d: %d pixels differ from Pillow" % (name, k, wrong)
    assert torch.equal(together[alpha][0][name], t)


def test_a_small_scratch_limit_gives_several_native_calls(monkeypatch, together):
    monkeypatch.setattr(ops, 'GIF_DECODE_SCRATCH_BYTES', 64 << 10)
    for alpha in (False, True):
        stats = {}
        out = ops.gif_decode([C.case_file(name) for name in C.NAMES], alpha=alpha, stats=stats)
        images = sum(len(gifread.probe(C.case_file(name))['frames']) for name in C.NAMES)
        assert 3 <= len(stats['groups']) < images and sum(stats['groups']) == images and len(stats['rounds']) == len(stats['groups'])
        for name, t in zip(C.NAMES, out):
            assert torch.equal(t, together[alpha][0][name]), name
    # a clip larger than the budget: every image in a call of its own
    monkeypatch.setattr(ops, 'GIF_DECODE_SCRATCH_BYTES', 256)
    stats = {}
    out = ops.gif_decode(C.case_file('anim_disposal_t'), alpha=True, stats=stats)
    assert stats['groups'] == [1] * 7
    assert torch.equal(out, together[True][0]['anim_disposal_t'])


def test_doubling_rounds_follow_the_largest_image(together):
    """the launches are ceil(log2(pixels of the largest image of the native call)), whatever the data.  How many of them do work
    has no lower bound to assert beyond 1: the doubling is done in place, so a round may already read what it has just resolved."""
    stats = {}
    out = ops.gif_decode(C.case_file('flat'), stats=stats)
    launched, worked = stats['rounds'][0]
    print("flat: %d rounds launched, %d did work" % (launched, worked))
    assert launched == 11 and 1 <= worked <= launched               # ceil(log2(40 * 40))
    assert np.array_equal(out.cpu().numpy(), C.reference('flat'))
    assert together[False][1]['rounds'][0][0] == 13                # the largest image of the set: 64 * 80 pixels
    stats = {}
    ops.gif_decode(C.case_file('size_1x1'), stats=stats)
    assert stats['rounds'] == [(0, 0)]


def clip(H, W):
    """three frames of at most 256 colours, and their R, G, B palette"""
    rng = np.random.default_rng(H * 100 + W)
    palette = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    palette = np.unique(palette, axis=0)
    palette = np.concatenate([palette, np.repeat(palette[-1:], 256 - len(palette), axis=0)])
    ind = rng.integers(0, len(np.unique(palette, axis=0)), (3, H, W))
    ind[1, H // 4:H // 2] = ind[1, 0, 0]                            # a flat band: long copies
    frames = palette[ind][:, :, :, ::-1].copy()                     # B, G, R
    return frames, palette


@pytest.mark.parametrize("shape", [(37, 53), (64, 48)])
def test_round_trip_through_gif_encode(shape, tmp_path):
    frames, palette = clip(*shape)
    order = video.playback_order(3)
    data = ops.gif_encode(torch.from_numpy(frames).cuda(), fps=20, loop=3, order=order, palette=palette)
    path = tmp_path / "clip.gif"
    path.write_bytes(data)
    got, durations = video.read_gif(str(path))
    assert tuple(got.shape) == (len(order),) + shape + (3,) and durations == [50] * len(order)
    assert np.array_equal(got.cpu().numpy(), frames[order])
    assert gifread.probe(data)['loop'] == 3
    again, _ = video.read_gif(data, alpha=True)
    assert torch.equal(again[..., :3], got) and bool((again[..., 3] == 255).all())


def test_read_apng_returns_the_frames_written(tmp_path):
    frames, _ = clip(37, 53)
    grey = np.ascontiguousarray(frames[:, :, :, 0])
    for name, fr in (("colour", frames), ("grey", grey)):
        streams, W, H, ct = ops.png_streams(torch.from_numpy(fr).cuda())
        path = tmp_path / (name + ".apng")
        order = video.playback_order(3)
        video.write_apng(str(path), streams, W, H, ct, fps=20, order=order)
        got, durations = video.read_apng(str(path))
        want = fr[order] if fr.ndim == 4 else np.repeat(fr[order][..., None], 3, axis=3)
        assert np.array_equal(got.cpu().numpy(), want) and durations == [50.0] * len(order)


def test_read_avi_equals_jpeg_decode_of_the_chunks(tmp_path):
    frames, _ = clip(64, 48)
    jpegs = ops.jpeg_encode(torch.from_numpy(frames).cuda(), quality=90)
    order = video.playback_order(3)
    path = tmp_path / "clip.avi"
    video.write_mjpeg_avi(str(path), jpegs, 48, 64, fps=25, order=order)
    got, durations = video.read_avi(str(path))
    want = torch.stack(ops.jpeg_decode([jpegs[i] for i in order]))
    assert torch.equal(got, want) and durations == [40.0] * len(order)


def test_read_video_dispatches_on_the_suffix(tmp_path):
    frames, palette = clip(37, 53)
    dev = torch.from_numpy(frames).cuda()
    order = video.playback_order(3)
    (tmp_path / "c.gif").write_bytes(ops.gif_encode(dev, fps=25, order=order, palette=palette))
    streams, W, H, ct = ops.png_streams(dev)
    video.write_apng(str(tmp_path / "c.APNG"), streams, W, H, ct, fps=25, order=order)
    video.write_mjpeg_avi(str(tmp_path / "c.avi"), ops.jpeg_encode(dev), W, H, fps=25, order=order)
    streams, W, H = ops.webp_streams(dev)
    video.write_webp(str(tmp_path / "c.webp"), streams, W, H, fps=25, order=order)
    for name, reader in (("c.gif", video.read_gif), ("c.APNG", video.read_apng), ("c.avi", video.read_avi), ("c.webp", video.read_webp)):
        got, durations = video.read_video(str(tmp_path / name))
        want, want_durations = reader(str(tmp_path / name))
        assert tuple(got.shape) == (len(order), 37, 53, 3) and torch.equal(got, want) and list(durations) == list(want_durations)
    with pytest.raises(ValueError, match="mp4"):
        video.read_video(str(tmp_path / "c.mp4"))


def with_stream(name, stream):
    """the single-image case `name` with its LZW data replaced"""
    data = C.case_file(name)
    fr = gifread.probe(data)['frames'][0]
    head = fr['blocks'][0][0] - 1
    return data[:head] + C.sub_blocks(stream) + b';'


def test_corrupt_lzw_data_is_a_data_error():
    (_, _, early), (_, _, invalid) = C.corrupt_streams()
    for stream, word in ((early, "0x4"), (invalid, "0x1")):
        data = with_stream('mcs4', stream)
        assert len(gifread.probe(data)['frames']) == 1
        with pytest.raises(_lib.CsmError, match="corrupt LZW data") as e:
            ops.gif_decode(data)
        assert word in str(e.value)
    # a good file beside the corrupt one does not rescue the call, and decodes alone afterwards
    with pytest.raises(_lib.CsmError):
        ops.gif_decode([C.case_file('mcs4'), with_stream('mcs4', early)])
    assert np.array_equal(ops.gif_decode(C.case_file('mcs4')).cpu().numpy(), C.reference('mcs4'))


def test_imread_device_many_routes_gif_only_with_the_option(tmp_path, monkeypatch):
    from utils.io_utils import imread, imread_device, imread_device_many
    from PIL import Image
    monkeypatch.delenv('CSM_DEVICE_DECODE_GIF', raising=False)
    paths = []
    for name in ('anim_disposal_t', 'mcs5', 'lace_h9'):
        p = tmp_path / (name + ".gif")
        p.write_bytes(C.case_file(name))
        paths.append(str(p))
    refused = tmp_path / "grey.gif"
    refused.write_bytes(C.REFUSED['grey_ramp'][0]())
    png = tmp_path / "a.png"
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (9, 11, 3)).astype(np.uint8)).save(png)
    paths += [str(refused), str(png)]
    want = [imread(p) for p in paths]
    off = {}
    out = imread_device_many(paths, stats=off)
    assert sorted(off) == ['host', 'jpeg', 'png'] and off['host'] == [0, 1, 2, 3] and off['png'] == [4]
    for t, w in zip(out, want):
        assert np.array_equal(t.cpu().numpy(), w)
    on = {}
    out = imread_device_many(paths, stats=on, gif=True)
    assert on['gif'] == [0, 1, 2] and on['host'] == [3] and on['png'] == [4] and on['jpeg'] == []
    for t, w in zip(out, want):
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), w)
    assert np.array_equal(imread_device(paths[0], gif=True).cpu().numpy(), want[0])
    monkeypatch.setenv('CSM_DEVICE_DECODE_GIF', '1')
    env = {}
    imread_device_many(paths, stats=env)
    assert env['gif'] == [0, 1, 2]
