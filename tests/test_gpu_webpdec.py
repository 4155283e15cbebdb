"""GPU: ops.webp_decode (csrc/webpdec.hip) equals utils.io_utils.imread (alpha=False) and PIL's RGBA (alpha=True) on every byte over
the files of tests/webpdec_cases.py, alone and with all files in one call; the lossless writer's files come back
as the images they were made from; utils.io_utils.imread_device(_many) and AnimeInsSeg's device_decode route .webp files as
documented.  Valid streams only: corrupt data is exercised on the host (tests/test_webpdec.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_cases as J  # noqa: E402
import pngdec_cases as P  # noqa: E402
import webpdec_cases as C  # noqa: E402
from cartoonsegmentation_amd import _lib, ops, webpread  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def together():
    """every accepted file in one native call, once per output form: mixed sizes and features.  The default scratch budget splits
    this set (a 200 x 300 file plans tables for 2600 groups, 23 MB), so it is lifted for the fixture"""
    files = [C.case_file(name) for name in C.NAMES]
    stats = {}
    ops.webp_decode(files, stats=stats)
    assert 1 < len(stats['chunks']) < len(C.NAMES) and sum(stats['chunks']) == len(C.NAMES)
    budget = ops.WEBP_DECODE_SCRATCH_BYTES
    ops.WEBP_DECODE_SCRATCH_BYTES = 1 << 30
    try:
        bgr = ops.webp_decode(files, stats=stats)
        bgra = ops.webp_decode(files, alpha=True)
    finally:
        ops.WEBP_DECODE_SCRATCH_BYTES = budget
    assert isinstance(bgr, list) and len(bgr) == len(C.NAMES) and stats['chunks'] == [len(C.NAMES)]
    return dict(zip(C.NAMES, bgr)), dict(zip(C.NAMES, bgra))


@pytest.mark.parametrize("name", C.NAMES)
def test_decode_equals_imread_and_pil_rgba(name, together, tmp_path):
    from utils.io_utils import imread
    data = C.case_file(name)
    webpread.probe(data)                          # every case must be one the decoder takes: none drops out silently
    path = tmp_path / 'f.webp'
    path.write_bytes(data)
    want = imread(str(path))
    t = ops.webp_decode(data)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    assert torch.equal(together[0][name], t)
    want = C.reference_bgra(name)
    t = ops.webp_decode(data, alpha=True)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    assert torch.equal(together[1][name], t)


def test_a_small_scratch_limit_gives_several_chunks(monkeypatch, together):
    monkeypatch.setattr(ops, 'WEBP_DECODE_SCRATCH_BYTES', 2 << 20)
    stats = {}
    out = ops.webp_decode([C.case_file(name) for name in C.NAMES], alpha=True, stats=stats)
    assert 3 <= len(stats['chunks']) < len(C.NAMES) and sum(stats['chunks']) == len(C.NAMES)
    for name, t in zip(C.NAMES, out):
        assert torch.equal(t, together[1][name]), name


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 48)])
def test_round_trip_through_webp_encode_lossless(shape):
    H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    grey = torch.randint(0, 256, (H, W), dtype=torch.uint8, generator=g).cuda()
    bgr = torch.from_numpy(np.ascontiguousarray(C.cartoon(H, W, 5))).cuda()
    bgra = torch.from_numpy(np.ascontiguousarray(C.cartoon(H, W, 6, 4))).cuda()
    mask = (torch.from_numpy(np.ascontiguousarray(C.cartoon(H, W, 7)[:, :, 0])) > 100).cuda()
    files = ops.webp_encode_lossless([mask, grey, bgr, bgra])
    back = ops.webp_decode(files, alpha=True)
    opaque = torch.full((H, W, 1), 255, dtype=torch.uint8, device='cuda')
    assert torch.equal(back[0], torch.cat([(mask.to(torch.uint8) * 255).unsqueeze(2).expand(H, W, 3), opaque], dim=2))
    assert torch.equal(back[1], torch.cat([grey.unsqueeze(2).expand(H, W, 3), opaque], dim=2))
    assert torch.equal(back[2], torch.cat([bgr, opaque], dim=2))
    assert torch.equal(back[3], bgra)
    back = ops.webp_decode(files)
    assert torch.equal(back[2], bgr) and torch.equal(back[3], bgra[:, :, :3])
    assert torch.equal(back[1], grey.unsqueeze(2).expand(H, W, 3))


def test_cutouts_come_back_with_their_alpha():
    H, W = 72, 90
    img = torch.from_numpy(np.ascontiguousarray(C.cartoon(H, W, 8))).cuda()
    y, x = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
    masks = torch.stack([(y - 30) ** 2 + (x - 40) ** 2 < 400, (y > 50) & (x < 33), (y == 3) & (x == 80)])
    alpha = ((x + y).float() / (H + W)).contiguous()
    cuts = ops.cutout_bgra(img, masks, alpha=alpha, pad=2)
    assert all(c is not None for c in cuts)
    back = ops.webp_decode(ops.webp_encode_lossless(cuts), alpha=True)
    for c, b in zip(cuts, back):
        assert torch.equal(c, b)
    assert any(0 < int(v) < 255 for v in back[0][..., 3].unique())


def test_errors():
    for name in ('lossy', 'lossy_alpha', 'animated', 'version', 'exif6'):
        with pytest.raises(webpread.Unsupported):
            ops.webp_decode(C.REFUSED[name][0]())
    with pytest.raises(TypeError):
        ops.webp_decode(["not bytes"])
    with pytest.raises(_lib.CsmError):
        ops.webp_decode(C.case_file('c1_m0_q75'), device='cpu')
    assert ops.webp_decode([]) == []
    assert ops.webp_decode([], alpha=True) == []


def test_refused_containers_raise_before_any_gpu_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a refused file")
    monkeypatch.setattr(_lib, 'load', no_library)
    for name in sorted(C.REFUSED):
        with pytest.raises(webpread.Unsupported):
            ops.webp_decode([C.case_file('c37_m0_q20'), C.REFUSED[name][0]()])


def test_imread_device_routes_webp_files(tmp_path, monkeypatch):
    from utils.io_utils import imread, imread_device, imread_device_many
    monkeypatch.delenv('CSM_DEVICE_DECODE_WEBP', raising=False)
    accepted = ['cut_m4_q75', 'vp8x_meta', 'hand_palette_predictor', 'i4_m2_q75']
    refused = ['lossy', 'lossy_alpha', 'exif6', 'animated']
    names = []
    for k, name in enumerate(accepted + refused):
        fn = '%s.%s' % (name, 'WEBP' if k % 2 else 'webp')
        (tmp_path / fn).write_bytes(C.case_file(name) if name in C.ACCEPTED else C.REFUSED[name][0]())
        names.append(fn)
    (tmp_path / 'base.jpg').write_bytes(J.pil_jpeg(J.frame('cartoon', 40, 56, 5), '420'))
    (tmp_path / 'p.png').write_bytes(P.case_file('natural'))
    names += ['base.jpg', 'p.png']
    paths = [str(tmp_path / n) for n in names]
    n_webp = len(accepted) + len(refused)
    calls = []
    real = ops.webp_decode
    monkeypatch.setattr(ops, 'webp_decode', lambda files, *a, **kw: calls.append(len(files)) or real(files, *a, **kw))
    # off (the default): every .webp goes through imread, and stats is the dict it was
    stats = {}
    off = imread_device_many(paths, stats=stats)
    assert calls == [] and stats == {'jpeg': [n_webp], 'png': [n_webp + 1], 'host': list(range(n_webp))}
    want = {'jpeg': [n_webp], 'png': [n_webp + 1], 'host': list(range(len(accepted), n_webp)), 'webp': list(range(len(accepted)))}
    # the keyword
    stats = {}
    many = imread_device_many(paths, stats=stats, webp=True)
    assert calls == [len(accepted)] and stats == want        # one call for all accepted files
    for n, p, t, o in zip(names, paths, many, off):
        assert t.is_cuda and t.dtype == torch.uint8 and torch.equal(t, o), n
        if n != 'base.jpg':                                    # the device JPEG decode has its own contract
            assert np.array_equal(t.cpu().numpy(), imread(p)), n
    assert tuple(many[names.index('exif6.webp')].shape) == (8, 5, 3)                     # rotated by imread
    # the variable
    monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP', '1')
    stats = {}
    again = imread_device_many(paths, stats=stats)
    assert calls == [len(accepted)] * 2 and stats == want and all(torch.equal(a, b) for a, b in zip(again, many))
    stats = {}
    imread_device_many(paths, stats=stats, webp=False)
    assert calls == [len(accepted)] * 2 and 'webp' not in stats
    one = imread_device(paths[0])
    assert calls == [len(accepted)] * 2 + [1] and torch.equal(one, many[0])


def test_a_file_over_the_group_cap_goes_through_imread(tmp_path):
    """five groups in an 8 x 8 image (four blocks of 4 x 4): valid for libwebp, over this file's cap"""
    from utils.io_utils import imread, imread_device_many
    argb = C.argb_of(C.cartoon(8, 8, 60))
    w = C.L.BitWriter()
    w.number(0x2f, 8); w.number(7, 14); w.number(7, 14); w.number(0, 1); w.number(0, 3); w.number(0, 1)
    C._write_image(w, [int(v) for v in argb.reshape(-1)], 8, 8, 0, [0, 1, 2, 4], 2, main=True)
    over = C.L.container(w.tobytes())
    good = C.case_file('hand_groups4')
    with pytest.raises(webpread.Unsupported, match="groups") as e:
        ops.webp_decode([good, over, good])
    assert e.value.files == (1,)
    (tmp_path / 'a.webp').write_bytes(good)
    (tmp_path / 'b.webp').write_bytes(over)
    stats = {}
    out = imread_device_many([str(tmp_path / 'b.webp'), str(tmp_path / 'a.webp')], stats=stats, webp=True)
    assert stats['webp'] == [1] and stats['host'] == [0]
    for t, n in zip(out, ('b.webp', 'a.webp')):
        assert np.array_equal(t.cpu().numpy(), imread(str(tmp_path / n)))


def test_infer_with_device_decode_lists_the_same_instances(tmp_path, monkeypatch):
    from animeinsseg import AnimeInsSeg
    src = tmp_path / 'in'
    src.mkdir()
    paths = []
    for k in range(3):
        p = src / ('f%d.webp' % k)
        p.write_bytes(C.pil_webp(C.cartoon(64, 80, 10 + k, 4 if k == 1 else 3), (0, 4, 6)[k], 75))
        paths.append(str(p))
    annotations, calls = {}, []
    real = ops.webp_decode
    monkeypatch.setattr(ops, 'webp_decode', lambda files, *a, **kw: calls.append(len(files)) or real(files, *a, **kw))
    monkeypatch.setenv('CSM_DEVICE_DECODE', '1')
    net = AnimeInsSeg('synthetic', default_det_size=64)
    assert net.device_decode
    for flag in ('0', '1'):                                     # without the variable the files go through imread, inside the same path
        monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP', flag)
        out = tmp_path / ('out%s.json' % flag)
        net.infer(list(paths), save_annotation=str(out), save_dir=str(tmp_path / ('sd' + flag)), pred_score_thr=0.3, max_instances=2)
        annotations[flag] = json.loads(out.read_text())
        assert sum(calls) == (3 if flag == '1' else 0)
    assert len(annotations['0']['images']) == 3 and all(im['height'] == 64 and im['width'] == 80 for im in annotations['0']['images'])
    assert annotations['0']['images'] == annotations['1']['images'] and annotations['0']['annotations'] == annotations['1']['annotations']
    assert len(annotations['0']['annotations']) >= 1
