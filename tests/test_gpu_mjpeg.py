"""GPU: the HIP JPEG encoder (csrc/mjpeg.hip) is byte-identical to its numpy restatement (tests/mjpeg_restatement.py, contract
DESIGN.md §4.6) through ops.jpeg_encode, and npyframes2video's .avi route writes a Motion-JPEG AVI whose every chunk PIL decodes."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mjpeg_restatement as R  # noqa: E402
from test_mjpeg import cartoon, check_against_pil, check_avi, pil_decode  # noqa: E402

SIZES = [(8, 8), (17, 23), (64, 80), (100, 101), (243, 317), (720, 720), (720, 540), (1024, 1024)]


@functools.lru_cache(maxsize=None)
def _frame(H, W, k):
    f = cartoon(H, W, H * 1000 + W + 7919 * k)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(H, W, k, q, sub):
    return R.encode(_frame(H, W, k), q, sub)


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("q", [50, 90, 100])
@pytest.mark.parametrize("sub", ['420', '444'])
@pytest.mark.parametrize("H,W", SIZES)
def test_op_is_byte_identical_to_the_restatement(H, W, sub, q, n):
    from cartoonsegmentation_amd import ops
    frames = np.stack([_frame(H, W, k) for k in range(n)])
    got = ops.jpeg_encode(torch.from_numpy(frames).cuda(), quality=q, subsampling=sub)
    assert len(got) == n and all(isinstance(g, bytes) for g in got)
    for k in range(n):
        want = _want(H, W, k, q, sub)
        assert got[k] == want, (k,) + _first_difference(got[k], want)


@pytest.mark.parametrize("sub", ['420', '444'])
@pytest.mark.parametrize("H,W", [(24, 1969), (9, 4100), (40, 1968)])
def test_rows_wider_than_lds_are_byte_identical(H, W, sub):
    """rows of more than 739 blocks (wider than 1968 pixels) assemble their bits in device scratch instead of LDS"""
    from cartoonsegmentation_amd import ops
    frames = np.stack([_frame(H, W, k) for k in range(2)])
    got = ops.jpeg_encode(torch.from_numpy(frames).cuda(), quality=100, subsampling=sub)
    for k in range(2):
        want = _want(H, W, k, 100, sub)
        assert got[k] == want, (k,) + _first_difference(got[k], want)


def test_extreme_frames_are_byte_identical():
    """black, white, saturated noise (the longest codes, many FF bytes) and a single pixel, at the ends of the quality range"""
    from cartoonsegmentation_amd import ops
    rng = np.random.default_rng(5)
    cases = [np.zeros((33, 47, 3), np.uint8), np.full((33, 47, 3), 255, np.uint8),
             (rng.integers(0, 2, (50, 70, 3)) * 255).astype(np.uint8), rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
             rng.integers(0, 256, (64, 1, 3), dtype=np.uint8), rng.integers(0, 256, (1, 300, 3), dtype=np.uint8)]
    for f in cases:
        for sub in ('420', '444'):
            for q in (1, 100):
                got = ops.jpeg_encode(torch.from_numpy(f).cuda(), quality=q, subsampling=sub)
                want = R.encode(f, q, sub)
                assert len(got) == 1 and got[0] == want, (f.shape, sub, q) + _first_difference(got[0], want)
                assert pil_decode(got[0]).shape == f.shape


def test_chunked_encode_equals_one_call(monkeypatch):
    """frames beyond the scratch bound are encoded in several library calls: the same bytes"""
    from cartoonsegmentation_amd import ops
    frames = torch.from_numpy(np.stack([_frame(100, 101, k) for k in range(5)])).cuda()
    whole = ops.jpeg_encode(frames)
    monkeypatch.setattr(ops, 'JPEG_SCRATCH_BYTES', 1)                        # one frame per call
    assert ops.jpeg_encode(frames) == whole
    assert ops.jpeg_encode(frames[::2]) == whole[::2]                        # a non-contiguous view


def test_two_calls_give_identical_bytes():
    from cartoonsegmentation_amd import ops
    frames = torch.from_numpy(np.stack([_frame(243, 317, k) for k in range(5)])).cuda()
    for sub in ('420', '444'):
        a = ops.jpeg_encode(frames, quality=90, subsampling=sub)
        b = ops.jpeg_encode(frames, quality=90, subsampling=sub)
        assert a == b
    one = ops.jpeg_encode(frames[2])
    assert one == ops.jpeg_encode(frames)[2:3]                               # [H,W,3] is a batch of one


def test_numpy_list_and_device_tensor_write_the_same_file(tmp_path):
    from cartoonsegmentation_amd.kenburns import npyframes2video
    frames = [_frame(100, 101, k) for k in range(4)]
    a, b = str(tmp_path / "list.avi"), str(tmp_path / "dev.AVI")
    npyframes2video(frames, a, playback=True, quality=75, subsampling='444')
    npyframes2video(torch.from_numpy(np.stack(frames)).cuda(), b, playback=True, quality=75, subsampling='444')
    data = open(a, 'rb').read()
    assert data == open(b, 'rb').read()
    jpegs = [R.encode(f, 75, '444') for f in frames]
    check_avi(data, jpegs, [0, 1, 2, 3, 2, 1], 101, 100)


@pytest.fixture(scope="module")
def pipe_and_cfg():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    H, W = 320, 384
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False,
                         depth_field=False, focal=W / 2.0, num_frame=4,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    img = synth.image_u8(H, W, 11)
    inst = pipe.animeinsseg.infer(img, pred_score_thr=0.3, max_instances=2, det_size=96, refine_kwargs=cfg.mask_refine_kwargs)
    return pipe, pipe.generate_kenburns_config(img, instances=inst)


def test_kenburns_frames_to_avi_end_to_end(pipe_and_cfg, tmp_path):
    """process_kenburns(to_numpy=False) -> npyframes2video(device frames, 'a.avi', playback=True): the frames never reach the host
    uncompressed; every chunk decodes to its frame under the PIL rule"""
    from anime_3dkenburns import npyframes2video
    pipe, kc = pipe_and_cfg
    W, H = kc['intWidth'], kc['intHeight']
    objFrom = {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(0.97 * W), 'intCropHeight': int(0.97 * H)}
    objTo = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': objFrom}, kc)
    steps = np.linspace(0.0, 1.0, 4).tolist()
    dev_frames, _ = pipe.process_kenburns({'fltSteps': steps, 'objFrom': objFrom, 'objTo': objTo, 'boolInpaint': False}, kc,
                                          inpaint=False, to_numpy=False)
    assert isinstance(dev_frames, torch.Tensor) and dev_frames.is_cuda and tuple(dev_frames.shape) == (4, H, W, 3)
    path = str(tmp_path / "a.avi")
    npyframes2video(dev_frames, path, playback=True)
    host = dev_frames.cpu().numpy()
    jpegs = [R.encode(f, 90, '420') for f in host]                           # the defaults: quality 90, 4:2:0
    order = [0, 1, 2, 3, 2, 1]
    a = check_avi(open(path, 'rb').read(), jpegs, order, W, H)
    assert len(a['chunks']) == 2 * 4 - 2
    for k, i in enumerate(order):
        check_against_pil(a['chunks'][k], host[i], 90, '420', "chunk %d (frame %d)" % (k, i))


def test_autozoom_keeps_frames_on_the_device(pipe_and_cfg):
    pipe, kc = pipe_and_cfg
    dev_frames = pipe.autozoom(kc, inpaint=False, to_numpy=False)
    assert isinstance(dev_frames, torch.Tensor) and dev_frames.is_cuda and dev_frames.dtype == torch.uint8
    frames = pipe.autozoom(kc, inpaint=False)
    assert isinstance(frames, list) and len(frames) == dev_frames.shape[0]
    assert all(isinstance(f, np.ndarray) and f.shape == tuple(dev_frames.shape[1:]) for f in frames)


def test_error_paths():
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    ok = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(CsmError):
        ops.jpeg_encode(ok.float())                                          # wrong dtype
    with pytest.raises(CsmError):
        ops.jpeg_encode(ok[..., 0])                                          # wrong rank
    with pytest.raises(CsmError):
        ops.jpeg_encode(torch.zeros((16, 16, 4), dtype=torch.uint8, device='cuda'))
    with pytest.raises(CsmError):
        ops.jpeg_encode(ok.cpu())                                            # a CPU tensor
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, subsampling='422')
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, quality=0)
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, quality=101)
    assert ops.jpeg_encode(ok[:0].reshape(0, 16, 16, 3)) == []
