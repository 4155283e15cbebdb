"""GPU: ops.webp_decode(lossy=True) (csrc/webplossy.hip) equals utils.io_utils.imread (alpha=False) and PIL's RGBA (alpha=True) on
every byte over the files of tests/webplossy_cases.py, alone and with all files in one call; the files of the
project's own VP8 writer come back as libwebp shows them; lossless and lossy files share a call; video.read_webp reads the clips
video.write_webp writes; utils.io_utils.imread_device(_many) and AnimeInsSeg's device_decode route lossy .webp files as documented.
Valid streams only: corrupt data is exercised on the host (tests/test_webplossy.py)."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webpdec_cases as LC  # noqa: E402
import webplossy_cases as C  # noqa: E402
from cartoonsegmentation_amd import _lib, ops, video, webpread  # noqa: E402

pytestmark = pytest.mark.gpu


def pil_bgr(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


@pytest.fixture(scope="module")
def together():
    """every file in one call, once per output form: mixed sizes and features"""
    files = [C.case_file(name) for name in C.NAMES]
    stats = {}
    bgr = ops.webp_decode(files, stats=stats, lossy=True)
    bgra = ops.webp_decode(files, alpha=True, lossy=True)
    assert isinstance(bgr, list) and len(bgr) == len(C.NAMES) and stats == {'chunks': [], 'chunks_lossy': [len(C.NAMES)]}
    return dict(zip(C.NAMES, bgr)), dict(zip(C.NAMES, bgra))


@pytest.mark.parametrize("name", C.NAMES)
def test_decode_equals_imread_and_pil_rgba(name, together, tmp_path):
    from utils.io_utils import imread
    data = C.case_file(name)
    assert webpread.probe(data, lossy=True)['kind'] == 'lossy'       # every case must be one the decoder takes: none drops out silently
    path = tmp_path / 'f.webp'
    path.write_bytes(data)
    want = imread(str(path))
    t = ops.webp_decode(data, lossy=True)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    assert torch.equal(together[0][name], t)
    want = C.reference_bgra(name)
    t = ops.webp_decode(data, alpha=True, lossy=True)
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    assert torch.equal(together[1][name], t)


def test_a_small_scratch_limit_gives_several_chunks(monkeypatch, together):
    monkeypatch.setattr(ops, 'WEBP_LOSSY_DECODE_SCRATCH_BYTES', 1 << 20)
    stats = {}
    out = ops.webp_decode([C.case_file(name) for name in C.NAMES], alpha=True, stats=stats, lossy=True)
    assert 3 <= len(stats['chunks_lossy']) < len(C.NAMES) and sum(stats['chunks_lossy']) == len(C.NAMES) and stats['chunks'] == []
    for name, t in zip(C.NAMES, out):
        assert torch.equal(t, together[1][name]), name


@pytest.mark.parametrize("shape", [(37, 53), (272, 544)])
@pytest.mark.parametrize("quality", [30, 90])
def test_files_of_webp_encode_come_back_as_pil_shows_them(shape, quality):
    H, W = shape
    frames = torch.from_numpy(np.stack([np.ascontiguousarray(LC.cartoon(H, W, 70 + k)[..., ::-1]) for k in range(2)])).cuda()
    files = ops.webp_encode(frames, quality=quality)
    back = ops.webp_decode(files, lossy=True)
    for data, t in zip(files, back):
        assert np.array_equal(t.cpu().numpy(), pil_bgr(data))


def test_a_mixed_call_comes_back_in_order():
    names = [('lossy', 'cartoon_m4_q75'), ('lossless', 'c37_m4_q75'), ('lossless', 'cut_m4_q75'), ('lossy', 'rgba_aq50'), ('lossless', 'i4_m2_q75'),
             ('lossy', 'alph_c0_f3')]
    files = [(C if kind == 'lossy' else LC).case_file(name) for kind, name in names]
    stats = {}
    out = ops.webp_decode(files, alpha=True, stats=stats, lossy=True)
    assert stats == {'chunks': [3], 'chunks_lossy': [3]}
    for (kind, name), t in zip(names, out):
        assert np.array_equal(t.cpu().numpy(), (C if kind == 'lossy' else LC).reference_bgra(name)), name


def test_read_webp_equals_pil_seek(tmp_path):
    H, W = 64, 80
    frames = torch.from_numpy(np.stack([np.ascontiguousarray(LC.cartoon(H, W, 80 + k)[..., ::-1]) for k in range(5)])).cuda()
    streams = ops.webp_streams(frames, quality=80)[0]
    path = tmp_path / 'clip.webp'
    video.write_webp(str(path), streams, W, H, fps=20)
    got, durations = video.read_webp(str(path))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (5, H, W, 3) and durations == [50] * 5
    with Image.open(str(path)) as im:
        assert im.n_frames == 5
        for k in range(5):
            im.seek(k)
            assert np.array_equal(got[k].cpu().numpy(), np.asarray(im.convert('RGB'))[:, :, ::-1]), k
    again, _ = video.read_webp(path.read_bytes())
    assert torch.equal(again, got)
    for other in (C.case_file('size_17x33'), LC.REFUSED['animated'][0]()):
        with pytest.raises(webpread.Unsupported):
            video.read_webp(other)


def test_errors():
    lossy = C.case_file('size_17x33')
    with pytest.raises(webpread.Unsupported, match="lossy"):
        ops.webp_decode(lossy)                                   # without the keyword a lossy file is refused as before
    with pytest.raises(webpread.Unsupported, match="lossy"):
        ops.webp_decode([LC.case_file('c37_m0_q20'), lossy])
    with pytest.raises(_lib.CsmError):
        ops.webp_decode(lossy, device='cpu', lossy=True)
    assert ops.webp_decode([], lossy=True) == []
    cut = bytearray(lossy)
    del cut[-40 - (len(cut) & 1):]                                 # an even length: no padding byte to account for
    cut[4:8] = (len(cut) - 8).to_bytes(4, 'little')
    cut[16:20] = (len(cut) - 20).to_bytes(4, 'little')             # a bare VP8 file whose last partition ends early
    with pytest.raises(_lib.CsmError, match="corrupt"):
        ops.webp_decode(bytes(cut), lossy=True)


def test_refused_containers_raise_before_any_gpu_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a refused file")
    monkeypatch.setattr(_lib, 'load', no_library)
    for name in sorted(C.REFUSED):
        with pytest.raises(webpread.Unsupported):
            ops.webp_decode([C.case_file('size_16x16'), C.REFUSED[name][0]()], lossy=True)


def test_imread_device_routes_lossy_webp_files(tmp_path, monkeypatch):
    from utils.io_utils import imread, imread_device, imread_device_many
    monkeypatch.delenv('CSM_DEVICE_DECODE_WEBP', raising=False)
    monkeypatch.delenv('CSM_DEVICE_DECODE_WEBP_LOSSY', raising=False)
    files = [('a.webp', C.case_file('cartoon_m4_q75')), ('b.WEBP', LC.case_file('cut_m4_q75')), ('c.webp', C.case_file('rgba_aq100')),
             ('d.webp', C.REFUSED['exif6'][0]()), ('e.webp', C.REFUSED['animated'][0]()), ('f.webp', C.case_file('t_parts8'))]
    for fn, data in files:
        (tmp_path / fn).write_bytes(data)
    paths = [str(tmp_path / fn) for fn, _ in files]
    calls = []
    real = ops.webp_decode
    monkeypatch.setattr(ops, 'webp_decode', lambda fl, *a, **kw: calls.append(len(fl)) or real(fl, *a, **kw))
    stats = {}
    off = imread_device_many(paths, stats=stats)
    assert calls == [] and stats == {'jpeg': [], 'png': [], 'host': [0, 1, 2, 3, 4, 5]}
    # the lossy option alone does nothing, and the webp option alone is what it was
    stats = {}
    imread_device_many(paths, stats=stats, webp_lossy=True)
    assert calls == [] and stats == {'jpeg': [], 'png': [], 'host': [0, 1, 2, 3, 4, 5]}
    stats = {}
    imread_device_many(paths, stats=stats, webp=True)
    assert calls == [1] and stats == {'jpeg': [], 'png': [], 'host': [0, 2, 3, 4, 5], 'webp': [1]}
    # the keyword
    want = {'jpeg': [], 'png': [], 'host': [3, 4], 'webp': [0, 1, 2, 5], 'webp_lossy': [0, 2, 5]}
    stats = {}
    many = imread_device_many(paths, stats=stats, webp=True, webp_lossy=True)
    assert calls == [1, 4] and stats == want                      # one call for lossless and lossy files together
    for p, t, o in zip(paths, many, off):
        assert t.is_cuda and t.dtype == torch.uint8 and torch.equal(t, o), p
        assert np.array_equal(t.cpu().numpy(), imread(p)), p
    # the variable
    monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP', '1')
    monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP_LOSSY', '1')
    stats = {}
    again = imread_device_many(paths, stats=stats)
    assert calls == [1, 4, 4] and stats == want and all(torch.equal(a, b) for a, b in zip(again, many))
    stats = {}
    imread_device_many(paths, stats=stats, webp_lossy=False)
    assert calls == [1, 4, 4, 1] and 'webp_lossy' not in stats and stats['webp'] == [1]
    one = imread_device(paths[0])
    assert calls == [1, 4, 4, 1, 1] and torch.equal(one, many[0])


def test_infer_with_device_decode_lists_the_same_instances(tmp_path, monkeypatch):
    from animeinsseg import AnimeInsSeg
    src = tmp_path / 'in'
    src.mkdir()
    paths = []
    for k in range(3):
        p = src / ('f%d.webp' % k)
        p.write_bytes(C.pil_webp(LC.cartoon(64, 80, 10 + k, 4 if k == 1 else 3), (0, 4, 6)[k], 75))
        paths.append(str(p))
    annotations, calls = {}, []
    real = ops.webp_decode
    monkeypatch.setattr(ops, 'webp_decode', lambda files, *a, **kw: calls.append(len(files)) or real(files, *a, **kw))
    monkeypatch.setenv('CSM_DEVICE_DECODE', '1')
    monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP', '1')
    net = AnimeInsSeg('synthetic', default_det_size=64)
    assert net.device_decode
    for flag in ('0', '1'):                                     # without the variable the files go through imread, inside the same path
        monkeypatch.setenv('CSM_DEVICE_DECODE_WEBP_LOSSY', flag)
        out = tmp_path / ('out%s.json' % flag)
        net.infer(list(paths), save_annotation=str(out), save_dir=str(tmp_path / ('sd' + flag)), pred_score_thr=0.3, max_instances=2)
        annotations[flag] = json.loads(out.read_text())
        assert sum(calls) == (3 if flag == '1' else 0)
    assert len(annotations['0']['images']) == 3 and all(im['height'] == 64 and im['width'] == 80 for im in annotations['0']['images'])
    assert annotations['0']['images'] == annotations['1']['images'] and annotations['0']['annotations'] == annotations['1']['annotations']
    assert len(annotations['0']['annotations']) >= 1
