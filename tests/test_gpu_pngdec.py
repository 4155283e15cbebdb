"""GPU: ops.png_decode (csrc/pngdec.hip) equals utils.io_utils.imread on every byte over the files of tests/pngdec_cases.py
(DESIGN.md §4.9), alone and with all files in one call; utils.io_utils.imread_device(_many) and AnimeInsSeg's device_decode route PNG
files as documented.  Valid streams only: corrupt deflate data is exercised on the host (tests/test_pngdec.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_cases as J  # noqa: E402
import pngdec_cases as C  # noqa: E402
from cartoonsegmentation_amd import _lib, ops, pngread  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def together():
    """every accepted file in one call: mixed sizes and colour types"""
    stats = {}
    out = ops.png_decode([C.case_file(name) for name in C.NAMES], stats=stats)
    assert isinstance(out, list) and len(out) == len(C.NAMES) and len(stats['rounds']) == 1
    return dict(zip(C.NAMES, out)), stats


@pytest.mark.parametrize("name", C.NAMES)
def test_decode_equals_imread(name, together):
    data = C.case_file(name)
    pngread.probe(data)                           # every case must be one the decoder takes: none drops out silently
    want = C.reference(name)
    t = ops.png_decode(data)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    assert torch.equal(together[0][name], t)


def test_doubling_rounds_are_launched_by_the_raw_size(together):
    """the launches are ceil(log2(raw bytes)), whatever the data.  How many of them do work is reported but has no lower bound to
    assert beyond 1: the doubling is done in place, so a round may already read what it has just resolved and settle sooner than
    the synchronous rounds of the restatement (which needs 11 on this file, tests/test_pngdec.py)."""
    stats = {}
    out = ops.png_decode(C.case_file('deep'), stats=stats)
    launched, worked = stats['rounds'][0]
    print("deep: %d rounds launched, %d did work" % (launched, worked))
    assert launched == 13 and 1 <= worked <= launched          # ceil(log2(3 * 1501))
    assert np.array_equal(out.cpu().numpy(), C.reference('deep'))
    assert together[1]['rounds'][0][0] == 18                   # the largest file of the set: 300 * (1 + 200 * 4) bytes


def test_a_small_scratch_limit_gives_several_chunks(monkeypatch, together):
    monkeypatch.setattr(ops, 'PNG_DECODE_SCRATCH_BYTES', 64 << 10)
    stats = {}
    out = ops.png_decode([C.case_file(name) for name in C.NAMES], stats=stats)
    assert 3 <= len(stats['rounds']) < len(C.NAMES)            # 'natural' and 'far' are larger than the limit and are still taken
    for name, t in zip(C.NAMES, out):
        assert torch.equal(t, together[0][name]), name


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 48)])
def test_round_trip_through_png_encode(shape):
    H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    grey = torch.randint(0, 256, (H, W), dtype=torch.uint8, generator=g).cuda()
    bgr = torch.from_numpy(C.cartoon(H, W, 3, 5)).cuda()
    mask = (torch.from_numpy(C.cartoon(H, W, 1, 6)[:, :, 0]) > 100).cuda()
    files = ops.png_encode(grey.unsqueeze(0)) + ops.png_encode(bgr.unsqueeze(0)) + ops.png_encode(mask.unsqueeze(0))
    back = ops.png_decode(files)
    assert torch.equal(back[0], grey.unsqueeze(2).expand(H, W, 3))
    assert torch.equal(back[1], bgr)
    assert torch.equal(back[2], (mask.to(torch.uint8) * 255).unsqueeze(2).expand(H, W, 3))


def test_a_wrong_adler_trailer_is_a_data_error():
    data = C.wrong_adler()
    pngread.probe(data)
    with pytest.raises(_lib.CsmError, match="corrupt"):
        ops.png_decode(data)
    good = C.case_file('fixed')
    assert np.array_equal(ops.png_decode(good).cpu().numpy(), C.reference('fixed'))      # the library goes on working


def test_errors():
    for name in ('depth16', 'interlaced', 'apng', 'exif6'):
        with pytest.raises(pngread.Unsupported):
            ops.png_decode(C.REFUSED[name][0]())
    with pytest.raises(TypeError):
        ops.png_decode(["not bytes"])
    with pytest.raises(_lib.CsmError):
        ops.png_decode(C.case_file('1x1'), device='cpu')
    assert ops.png_decode([]) == []


def test_imread_device_routes_png_files(tmp_path, monkeypatch):
    from utils.io_utils import imread, imread_device, imread_device_many
    accepted = ['natural', 'palette_trns', 'cycle_ct4', 'ancillary', 'idat_1']
    refused = ['depth16', 'xmp', 'exif6', 'depth1', 'ztxt']
    names = []
    for k, name in enumerate(accepted + refused):
        fn = '%s.%s' % (name, 'PNG' if k % 2 else 'png')
        (tmp_path / fn).write_bytes(C.case_file(name) if name in C.ACCEPTED else C.REFUSED[name][0]())
        names.append(fn)
    img = J.frame('cartoon', 40, 56, 5)
    (tmp_path / 'base.jpg').write_bytes(J.pil_jpeg(img, '420'))
    (tmp_path / 'prog.jpg').write_bytes(J.pil_jpeg(img, '420', progressive=True))
    names += ['base.jpg', 'prog.jpg']
    paths = [str(tmp_path / n) for n in names]
    calls = []
    real = ops.png_decode
    monkeypatch.setattr(ops, 'png_decode', lambda files, *a, **kw: calls.append(len(files)) or real(files, *a, **kw))
    stats = {}
    many = imread_device_many(paths, stats=stats)
    assert calls == [len(accepted)]                            # one call for all accepted PNG files
    assert stats['png'] == list(range(len(accepted))) and stats['jpeg'] == [len(names) - 2]
    assert stats['host'] == list(range(len(accepted), len(accepted) + len(refused))) + [len(names) - 1]
    for n, p, t in zip(names, paths, many):
        assert t.is_cuda and t.dtype == torch.uint8
        if n != 'base.jpg':                                    # the device JPEG decode has its own contract
            assert np.array_equal(t.cpu().numpy(), imread(p)), n
    assert tuple(many[names.index('exif6.PNG')].shape) == (5, 8, 3)                      # rotated by imread
    one = imread_device(paths[0])
    assert calls == [len(accepted), 1] and torch.equal(one, many[0])


def test_infer_with_device_decode_lists_the_same_images(tmp_path, monkeypatch):
    from animeinsseg import AnimeInsSeg
    src = tmp_path / 'in'
    src.mkdir()
    for k, ct in enumerate((2, 6, 0)):
        (src / ('f%d.png' % k)).write_bytes(C.png(C.cartoon(64, 80, C.CHANNELS[ct], 10 + k), ct))
    (src / 'f3.png').write_bytes(C.png(C.cartoon(64, 80, 1, 13) % 7, 3, palette=C.noise(1, 7, 3, 1)[0]))
    images, calls = {}, []
    real = ops.png_decode
    monkeypatch.setattr(ops, 'png_decode', lambda files, *a, **kw: calls.append(len(files)) or real(files, *a, **kw))
    for flag in ('0', '1'):
        monkeypatch.setenv('CSM_DEVICE_DECODE', flag)
        net = AnimeInsSeg('synthetic', default_det_size=64)
        assert net.device_decode == (flag == '1')
        out = tmp_path / ('out%s.json' % flag)
        net.infer(str(src), save_annotation=str(out), save_dir=str(tmp_path / ('sd' + flag)), pred_score_thr=0.3, max_instances=2)
        images[flag] = json.loads(out.read_text())['images']
        assert sum(calls) == (4 if flag == '1' else 0)
    assert len(images['0']) == 4 and all(im['height'] == 64 and im['width'] == 80 for im in images['0'])
    assert images['0'] == images['1']
