"""GPU: ops.jpeg_decode(..., progressive=True) (csrc/jpegprog.hip) equals the restatement of its contract
(tests/jpegprog_restatement.py + jpegdec_restatement.pixels) byte for byte, and therefore PIL; files of both kinds
share a call; utils.io_utils.imread_device_many routes progressive files to the device only when asked to.  Nothing corrupt is fed
to the device."""
import io
import os
import sys

import numpy as np
import pytest
import torch

Image = pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegprog_cases as C  # noqa: E402
from cartoonsegmentation_amd import _lib, jpegcode, ops  # noqa: E402

pytestmark = pytest.mark.gpu

WORKGROUP_BYTES = 32 * 256          # entropy bytes of one workgroup: csm_jpeg_decode_subseq_bytes() x 256 lanes


def test_all_small_files_in_one_call():
    """every case and every writer file, sizes, modes, restart settings and scan scripts mixed, in one call"""
    files = C.all_small_files()
    stats = {}
    out = ops.jpeg_decode([d for _, d in files], progressive=True, stats=stats)
    assert stats['progressive'] == list(range(len(files))) and len(stats['levels']) == 1 and stats['passes'] == []
    assert stats['levels'][0] == 4                              # the three-step chain: a first level and three refinements
    for (name, data), t in zip(files, out):
        want = C.reference(data)[2]
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == want.shape, name
        assert np.array_equal(t.cpu().numpy(), want), name
        assert np.array_equal(want, C.pil_decode(data)), name


def test_a_first_scan_that_spans_two_workgroups():
    assert _lib.load().csm_jpeg_decode_subseq_bytes() * 256 == WORKGROUP_BYTES
    data = C.progressive_jpeg(C.frame('noise', 112, 112, 7), '444', 100)
    info = jpegcode.probe(data, progressive=True)
    assert max(s['entropy'][1] - s['entropy'][0] for s in info['scans'] if s['ah'] == 0) > WORKGROUP_BYTES
    stats = {}
    t = ops.jpeg_decode(data, progressive=True, stats=stats)
    assert stats['progressive_passes'][0] >= 1
    assert np.array_equal(t.cpu().numpy(), C.pil_decode(data))


def test_restart_markers_counted_across_a_workgroup_boundary():
    """a first scan of more than one workgroup with a restart marker every 2 blocks: the write pass places the second workgroup's
    slots by the marker counts of the first"""
    data = C.progressive_jpeg(C.frame('noise', 112, 112, 7), '444', 100, restart_marker_blocks=2)
    info = jpegcode.probe(data, progressive=True)
    assert max(s['entropy'][1] - s['entropy'][0] for s in info['scans'] if s['ah'] == 0) > WORKGROUP_BYTES
    stats = {}
    t = ops.jpeg_decode(data, progressive=True, stats=stats)
    assert stats['progressive_passes'][0] >= 1
    assert np.array_equal(t.cpu().numpy(), C.pil_decode(data))


@pytest.mark.parametrize('grey, dc_bytes', [(200, 4128), (90, 8256)])
def test_a_flat_grey_file_with_capped_eob_runs(grey, dc_bytes):
    """33024 blocks: the AC scans are one EOB run at the cap of 32767 blocks and a remainder, the DC refinement is 33024 bits: all
    zero at grey 200, all one at grey 90, where every byte of the scan is a stuffed FF 00 pair"""
    data = C.progressive_jpeg(np.full((1032, 2048, 3), grey, np.uint8), 'grey', 90)
    info = jpegcode.probe(data, progressive=True)
    assert jpegcode.scan_block_count(info, info['scans'][1]) == (33024, 1)
    lens = [(s['ss'], s['ah'], s['entropy'][1] - s['entropy'][0]) for s in info['scans']]
    assert all(n <= 8 for ss, _, n in lens if ss > 0), lens
    assert [n for ss, ah, n in lens if ss == 0 and ah] == [dc_bytes]
    t = ops.jpeg_decode(data, progressive=True)
    assert np.array_equal(t.cpu().numpy(), C.pil_decode(data))


def test_a_1024_frame_equals_pil():
    data = C.progressive_jpeg(C.frame('cartoon', 1024, 1024, 4), '420', 90)
    t = ops.jpeg_decode(data, progressive=True)
    assert np.array_equal(t.cpu().numpy(), C.pil_decode(data))


def _mixed():
    img = C.frame('cartoon', 40, 56, 5)
    noise = C.frame('noise', 33, 17, 6)
    return [C.pil_jpeg(img, '420'), C.progressive_jpeg(img, '420', 90), C.progressive_jpeg(noise, '444', 100, restart_marker_blocks=2),
            C.pil_jpeg(noise, '422', restart='mcu3'), C.writer_file('chain', 'cartoon')[0], C.pil_jpeg(img, 'grey'),
            C.progressive_jpeg(img, 'grey', 30)]


def test_baseline_and_progressive_files_interleaved():
    files = _mixed()
    kinds = [jpegcode.probe(d, progressive=True)['progressive'] for d in files]
    assert kinds == [False, True, True, False, True, False, True]
    stats = {}
    out = ops.jpeg_decode(files, progressive=True, stats=stats)
    assert stats['progressive'] == [1, 2, 4, 6] and len(stats['passes']) == 1
    for d, t, prog in zip(files, out, kinds):
        assert torch.equal(t, ops.jpeg_decode(d, progressive=True))
        if prog:
            assert np.array_equal(t.cpu().numpy(), C.pil_decode(d))
        else:
            assert torch.equal(t, ops.jpeg_decode(d))              # the baseline path, untouched by the keyword


def test_chunks_below_one_file_s_scratch(monkeypatch):
    files = _mixed()
    whole = ops.jpeg_decode(files, progressive=True)
    monkeypatch.setattr(ops, 'JPEG_DECODE_SCRATCH_BYTES', 1 << 10)
    stats = {}
    out = ops.jpeg_decode(files, progressive=True, stats=stats)
    assert len(stats['levels']) == 4 and len(stats['passes']) == 3  # every file alone
    for a, b in zip(whole, out):
        assert torch.equal(a, b)


def test_imread_device_many_routes_progressive_files_when_asked(tmp_path, monkeypatch):
    from utils.io_utils import imread, imread_device, imread_device_many
    monkeypatch.delenv('CSM_DEVICE_DECODE_PROGRESSIVE', raising=False)
    img = C.frame('cartoon', 40, 56, 5)
    exif = Image.Exif()
    exif[0x0112] = 6
    files = {'base.jpg': C.pil_jpeg(img, '420'), 'prog.jpg': C.progressive_jpeg(img, '420', 90),
             'rot.jpg': C.progressive_jpeg(img, '422', 90, exif=exif.tobytes())}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, 'PNG')
    (tmp_path / 'pic.png').write_bytes(buf.getvalue())
    names = ['base.jpg', 'prog.jpg', 'rot.jpg', 'pic.png']
    paths = [str(tmp_path / n) for n in names]
    # neither the keyword nor the variable: exactly today's routes
    stats = {}
    plain = imread_device_many(paths, stats=stats)
    assert stats == {'jpeg': [0], 'png': [3], 'host': [1, 2]}
    for p, t in zip(paths[1:], plain[1:]):
        assert np.array_equal(t.cpu().numpy(), imread(p))
    assert torch.equal(plain[0], ops.jpeg_decode(files['base.jpg']))
    monkeypatch.setenv('CSM_DEVICE_DECODE_PROGRESSIVE', '0')
    stats = {}
    imread_device_many(paths, stats=stats)
    assert stats == {'jpeg': [0], 'png': [3], 'host': [1, 2]}

    def asked(**kw):
        stats = {}
        many = imread_device_many(paths, stats=stats, **kw)
        assert stats == {'jpeg': [0, 1], 'png': [3], 'host': [2], 'jpeg_progressive': [1]}
        for a, b in zip(many, plain):
            assert torch.equal(a, b)                               # the progressive file from the device equals imread
        assert tuple(many[2].shape) == (56, 40, 3)                 # rotated by imread
    asked(progressive=True)
    assert torch.equal(imread_device(paths[1], progressive=True), plain[1])
    monkeypatch.setenv('CSM_DEVICE_DECODE_PROGRESSIVE', '1')
    asked()
    stats = {}
    imread_device_many(paths, stats=stats, progressive=False)      # the keyword wins
    assert stats == {'jpeg': [0], 'png': [3], 'host': [1, 2]}


def test_errors():
    prog = C.progressive_jpeg(C.frame('cartoon', 16, 16, 0), '420', 90)
    with pytest.raises(_lib.CsmError):
        ops.jpeg_decode(prog, device='cpu', progressive=True)
    with pytest.raises(jpegcode.Unsupported):
        ops.jpeg_decode(prog)
    with pytest.raises(jpegcode.Unsupported):
        ops.jpeg_decode(prog, _infos=[jpegcode.probe(prog, progressive=True)])
    assert ops.jpeg_decode([], progressive=True) == []
