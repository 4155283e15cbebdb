"""GPU: the HIP PNG encoder (csrc/png.hip + pngcode.py) is byte-identical to its numpy restatement (tests/png_restatement.py,
contract DESIGN.md §4.7) through ops.png_encode and decodes (PIL) to its input exactly; utils.io_utils.imwrite, the mask PNGs of
_infer_save_annotations(save_mask_only=True) and npyframes2video's .apng route."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_restatement as R  # noqa: E402
from test_png import CONST_WIDTHS, SHAPES, SPECIALS, check_apng, check_file, image, pil_pixels, want  # noqa: E402


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


def _check_names(names, **kw):
    """one png_encode call over the stacked images `names`: every file is the restatement's, and decodes to its image"""
    from cartoonsegmentation_amd import ops
    batch = torch.from_numpy(np.stack([image(nm) for nm in names])).cuda()
    got = ops.png_encode(batch, **kw)
    assert len(got) == len(names) and all(isinstance(g, bytes) for g in got)
    for nm, g in zip(names, got):
        w = want(nm)[0]
        assert g == w, (nm,) + _first_difference(g, w)
        check_file(g, image(nm), want(nm)[1])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ['grey', 'bgr'])
@pytest.mark.parametrize("H,W", SHAPES)
def test_op_is_byte_identical_to_the_restatement(H, W, kind, n):
    _check_names(['%s-%dx%d-%d' % (kind, H, W, k) for k in range(n)])


@pytest.mark.parametrize("W", CONST_WIDTHS)
def test_constant_rows_hit_every_remainder_of_the_258_split(W):
    """scanlines of W + 1, W and W equal bytes (the first holds its type byte 0 too): every remainder 0..5 behind one and two
    matches of 258, with and without the tail of one or two literals"""
    _check_names(['const-%d' % W])


@pytest.mark.parametrize("W", [86, 87, 172, 173])
def test_constant_colour_rows(W):
    _check_names(['constbgr-%d' % W])


@pytest.mark.parametrize("name", SPECIALS)
def test_extreme_and_wide_images_are_byte_identical(name):
    """white, black, saturated and uniform noise, a bool disc mask, a flat image, and scanlines of 12 300 and 196 605 bytes (no
    scanline is staged in LDS, so the wide ones take the same kernels: DESIGN.md §4.7)"""
    _check_names([name])


def test_rgb_memory_order_is_kept_with_bgr_false():
    from cartoonsegmentation_amd import ops
    a = image('bgr-17x23-0')
    got = ops.png_encode(torch.tensor(a).cuda(), bgr=False)
    assert got == [R.encode(a, bgr=False)]
    assert np.array_equal(pil_pixels(got[0]), a)


def test_uint8_mask_and_bool_mask():
    """a bool mask is written 0 / 255; the same bytes as uint8 0 / 1 are written as they are"""
    from cartoonsegmentation_amd import ops
    m = image('disc')
    dev = torch.tensor(m).cuda()
    assert ops.png_encode(dev) == [want('disc')[0]] == ops.png_encode(torch.stack([dev, ~dev]))[:1]
    as_u8 = ops.png_encode(dev.to(torch.uint8))
    assert as_u8 == [R.encode(m.astype(np.uint8))] and pil_pixels(as_u8[0]).max() == 1


def test_chunked_encode_equals_one_call(monkeypatch):
    """images beyond the scratch bound are encoded in several library calls: the same bytes"""
    from cartoonsegmentation_amd import ops
    for kind in ('grey', 'bgr'):
        frames = torch.from_numpy(np.stack([image('%s-100x101-%d' % (kind, k)) for k in range(5)])).cuda()
        whole = ops.png_encode(frames)
        assert whole == [want('%s-100x101-%d' % (kind, k))[0] for k in range(5)]
        monkeypatch.setattr(ops, 'PNG_SCRATCH_BYTES', 1)                     # one image per call
        assert ops.png_encode(frames) == whole
        monkeypatch.undo()
        assert ops.png_encode(frames[::2]) == whole[::2]                     # a non-contiguous view: every other image
        assert ops.png_encode(frames[:, ::2, 1::3]) == [R.encode(np.ascontiguousarray(f)) for f in frames[:, ::2, 1::3].cpu().numpy()]


def test_two_calls_give_identical_bytes():
    from cartoonsegmentation_amd import ops
    for kind in ('grey', 'bgr'):
        frames = torch.from_numpy(np.stack([image('%s-243x317-%d' % (kind, k)) for k in range(5)])).cuda()
        a, b = ops.png_encode(frames), ops.png_encode(frames)
        assert a == b
        assert ops.png_encode(frames[2]) == a[2:3]                           # [H,W] / [H,W,3] is a batch of one


def test_error_paths():
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    ok = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(CsmError):
        ops.png_encode(ok.float())                                           # wrong dtype
    with pytest.raises(CsmError):
        ops.png_encode(torch.zeros((2, 16, 16, 4), dtype=torch.uint8, device='cuda'))   # four channels
    with pytest.raises(CsmError):
        ops.png_encode(ok.cpu())                                             # a CPU tensor
    with pytest.raises(CsmError):
        ops.png_encode(ok[0, :, 0])                                          # rank 1
    with pytest.raises(CsmError):
        ops.png_encode(torch.zeros((1, 2, 16, 16, 3), dtype=torch.uint8, device='cuda'))
    with pytest.raises(CsmError):
        ops.png_encode(torch.zeros((2, 16, 16, 3), dtype=torch.bool, device='cuda'))    # masks have no channels
    with pytest.raises(ValueError):
        ops.png_encode(torch.zeros((1, 65536), dtype=torch.uint8, device='cuda'))
    assert ops.png_encode(ok[:0].reshape(0, 16, 16, 3)) == []
    assert ops.png_encode(ok[:0].reshape(0, 16, 16)) == []


def test_imwrite_png_and_jpg(tmp_path):
    from cartoonsegmentation_amd import ops
    from utils.io_utils import imread, imwrite
    a = image('bgr-100x101-0')
    dev = torch.tensor(a).cuda()
    p1, p2 = str(tmp_path / "sub" / "dev.png"), str(tmp_path / "host.PNG")
    assert imwrite(dev, p1) is True and imwrite(a, p2) is True               # auto_mkdir made sub/
    data = open(p1, 'rb').read()
    assert data == open(p2, 'rb').read() == want('bgr-100x101-0')[0]
    assert np.array_equal(imread(p1), a)
    g = image('grey-100x101-0')
    imwrite(g, str(tmp_path / "grey.png"))
    assert open(str(tmp_path / "grey.png"), 'rb').read() == want('grey-100x101-0')[0]
    assert np.array_equal(imread(str(tmp_path / "grey.png")), np.repeat(g[:, :, None], 3, axis=2))
    for suffix in ('.jpg', '.jpeg'):
        pj = str(tmp_path / ("a" + suffix))
        imwrite(dev, pj)
        assert [open(pj, 'rb').read()] == ops.jpeg_encode(dev, 95, '420')
    with pytest.raises(FileNotFoundError):
        imwrite(a, str(tmp_path / "nowhere" / "a.png"), auto_mkdir=False)
    with pytest.raises(ValueError):
        imwrite(dev, str(tmp_path / "a.tiff"))


def test_save_mask_only_writes_one_png_per_instance(tmp_path):
    """_infer_save_annotations(save_mask_only=True), reference animeinsseg/__init__.py:597-598 and :616: mask_XXX_<name>.png per
    instance, each 0 / 255 of the mask a plain infer gives; no JSON; a frame without instances writes nothing"""
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    net = AnimeInsSeg('synthetic', default_det_size=96, refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    imgs = [synth.image_u8(160, 192, 50 + k) for k in range(2)]
    plain = net.infer(imgs, pred_score_thr=0.0, max_instances=3, output_type='numpy')
    assert sum(len(p) for p in plain) >= 1
    sd, js = tmp_path / "sd", tmp_path / "pred.json"
    assert net._infer_save_annotations(imgs, 0.0, str(sd), str(js), -1, -1, None, save_mask_only=True) is None
    assert not js.exists()
    expected = {'mask_%03d_%012d.jpg.png' % (j, k): np.asarray(res.masks[j]).astype(bool)
                for k, res in enumerate(plain) for j in range(len(res))}
    assert sorted(os.listdir(str(sd))) == sorted(expected)
    for nm, m in expected.items():
        data = (sd / nm).read_bytes()
        assert m.shape == (160, 192)
        check_file(data, m)                                                  # decodes to masks[j] * 255
        assert data == R.encode(m)
    # no score passes 1.5: no instance, no file, no JSON
    none = tmp_path / "none"
    net._infer_save_annotations(imgs, 1.5, str(none), str(tmp_path / "none.json"), -1, -1, None, save_mask_only=True)
    assert none.is_dir() and os.listdir(str(none)) == [] and not (tmp_path / "none.json").exists()
    # infer() does not forward the flag: it still writes the JSON and no PNG
    via = tmp_path / "via_infer"
    net.infer(imgs, save_annotation=str(tmp_path / "a.json"), save_dir=str(via), save_mask_only=True, pred_score_thr=0.0, max_instances=3)
    assert (tmp_path / "a.json").exists() and os.listdir(str(via)) == []


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


def test_kenburns_frames_to_apng_end_to_end(pipe_and_cfg, tmp_path):
    """process_kenburns(to_numpy=False) -> npyframes2video(device frames, 'a.apng', playback=True): the frames never reach the host
    uncompressed; PIL reads 2n - 2 frames, each exactly its device frame"""
    from anime_3dkenburns import npyframes2video
    pipe, kc = pipe_and_cfg
    W, H = kc['intWidth'], kc['intHeight']
    objFrom = {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(0.97 * W), 'intCropHeight': int(0.97 * H)}
    objTo = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': objFrom}, kc)
    steps = np.linspace(0.0, 1.0, 4).tolist()
    dev_frames, _ = pipe.process_kenburns({'fltSteps': steps, 'objFrom': objFrom, 'objTo': objTo, 'boolInpaint': False}, kc,
                                          inpaint=False, to_numpy=False)
    assert isinstance(dev_frames, torch.Tensor) and dev_frames.is_cuda and tuple(dev_frames.shape) == (4, H, W, 3)
    path = str(tmp_path / "a.APNG")                                          # the suffix in any letter case
    npyframes2video(dev_frames, path, playback=True)
    host = list(dev_frames.cpu().numpy())
    data = open(path, 'rb').read()
    check_apng(data, host, [0, 1, 2, 3, 2, 1])
    assert data == R.apng([R.stream(f) for f in host], W, H, 2, 25, [0, 1, 2, 3, 2, 1])
    # a list of numpy frames is uploaded and gives the same file
    again = str(tmp_path / "b.apng")
    npyframes2video(host, again, playback=True)
    assert open(again, 'rb').read() == data
