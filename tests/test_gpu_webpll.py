"""GPU: the HIP lossless WebP encoder (csrc/webpll.hip + webpcode.py) is byte-identical to its numpy restatement
(tests/webpll_restatement.py, contract DESIGN.md §4.13) through ops.webp_encode_lossless, and Pillow decodes its files to the
input exactly; ops.mask_bboxes / ops.cutout_bgra (csrc/cutout.hip) against numpy; and the surfaces: AnimeInstances.cutouts /
save_cutouts, _infer_save_annotations(save_cutout_only=True), utils.io_utils.imwrite('.webp') and get_cutout."""
import io
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webpll_restatement as R  # noqa: E402
from test_webpll import BLOCKS, CONSTS, MIXED_LIST, STRETCHES, check_file, image, mixed, want  # noqa: E402


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else m)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_names(names, as_list=True):
    """one webp_encode_lossless call over the images `names`: every file is the restatement's, and decodes to its image"""
    from cartoonsegmentation_amd import ops
    arg = [_dev(image(nm)) for nm in names] if as_list else _dev(np.stack([image(nm) for nm in names]))
    got = ops.webp_encode_lossless(arg)
    assert len(got) == len(names) and all(isinstance(g, bytes) for g in got)
    for nm, g in zip(names, got):
        assert g == want(nm), (nm,) + _first_difference(g, want(nm))
        check_file(g, image(nm))


# ---- the encoder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['1x1', '1x1-bgra', '1xW', 'Hx1', 'max-w', 'max-h'])
def test_degenerate_and_maximal_sides(name):
    _check_names([name])


@pytest.mark.parametrize("name", BLOCKS)
def test_sizes_around_the_predictor_block(name):
    _check_names([name])


@pytest.mark.parametrize("name", STRETCHES)
def test_widths_around_the_thread_stretch(name):
    _check_names([name])


@pytest.mark.parametrize("name", CONSTS)
def test_constant_rows_and_the_remainders_behind_a_maximal_reference(name):
    _check_names([name])


@pytest.mark.parametrize("name", ['black-column', 'one-colour', 'two-colour', 'noise', 'noise-bgra', 'fibonacci', 'opaque-bgra',
                                  'bordered-bgra', 'mask'])
def test_special_contents(name):
    """all simple codes (zero bits per pixel), one and two colours, uniform noise, the histogram that forces the length limit,
    four channels with an opaque and with a zero-alpha border, a bool mask"""
    _check_names([name])


def test_mixed_list_in_one_call_and_batches():
    from cartoonsegmentation_amd import ops
    _check_names(MIXED_LIST)                                    # (1,1,4), (5,300,3), (33,17), a bool (9,9): one native call
    _check_names(['block-16x16', 'block-16x16'], as_list=False)  # a stacked [n,H,W,3] batch
    batch = _dev(np.stack([mixed(20, 24, 4, k) for k in range(3)]))
    got = ops.webp_encode_lossless(batch)
    assert got == [R.encode(mixed(20, 24, 4, k)) for k in range(3)]
    assert ops.webp_encode_lossless(batch[1]) == got[1:2]       # [H,W,4] is a batch of one
    grey = _dev(np.stack([mixed(20, 24, 1, k) for k in range(2)]))
    assert ops.webp_encode_lossless(grey) == [R.encode(mixed(20, 24, 1, k)) for k in range(2)]
    masks = _dev(np.stack([image('mask'), ~image('mask')]))
    assert ops.webp_encode_lossless(masks) == [R.encode(image('mask')), R.encode(~image('mask'))]
    assert ops.webp_encode_lossless(batch[:, ::2, 1::3]) == [R.encode(np.ascontiguousarray(f)) for f in batch[:, ::2, 1::3].cpu().numpy()]


def test_chunked_encode_equals_one_call_and_is_deterministic(monkeypatch):
    from cartoonsegmentation_amd import ops
    items = [_dev(image(nm)) for nm in MIXED_LIST + ['noise', 'mask']]
    whole = ops.webp_encode_lossless(items)
    assert ops.webp_encode_lossless(items) == whole
    monkeypatch.setattr(ops, 'WEBPLL_SCRATCH_BYTES', 1)         # one image per chunk
    assert ops.webp_encode_lossless(items) == whole
    monkeypatch.setattr(ops, 'WEBPLL_SCRATCH_BYTES', 40000)     # a few per chunk
    assert ops.webp_encode_lossless(items) == whole


def test_empty_inputs_and_error_paths():
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    ok = torch.zeros((2, 16, 16, 4), dtype=torch.uint8, device='cuda')
    assert ops.webp_encode_lossless([]) == [] and ops.webp_encode_lossless(ok[:0]) == []
    assert ops.webp_encode_lossless(torch.zeros((0, 16, 16), dtype=torch.uint8, device='cuda')) == []
    with pytest.raises(CsmError):
        ops.webp_encode_lossless(ok.cpu())                      # a CPU tensor
    with pytest.raises(CsmError):
        ops.webp_encode_lossless([ok[0], ok[1].cpu()])
    with pytest.raises(CsmError):
        ops.webp_encode_lossless(ok.float())                    # wrong dtype
    with pytest.raises(CsmError):
        ops.webp_encode_lossless(ok[0, :, 0, 0])                # rank 1
    with pytest.raises(CsmError):
        ops.webp_encode_lossless(torch.zeros((1, 2, 16, 16, 3), dtype=torch.uint8, device='cuda'))
    with pytest.raises(CsmError):
        ops.webp_encode_lossless([torch.zeros((16, 16, 2), dtype=torch.uint8, device='cuda')])
    with pytest.raises(CsmError):
        ops.webp_encode_lossless(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        ops.webp_encode_lossless(torch.zeros((1, 16385), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.webp_encode_lossless([torch.zeros((16385, 1, 3), dtype=torch.uint8, device='cuda')])
    with pytest.raises(ValueError):
        ops.webp_encode_lossless([torch.zeros((0, 5), dtype=torch.uint8, device='cuda')])


# ---- boxes and cut-outs against numpy -----------------------------------------------------------------------------------------
def np_bbox(m):
    ys, xs = np.nonzero(m)
    return [0, 0, 0, 0] if ys.size == 0 else [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def np_cutout(img, m, alpha=None, pad=0):
    """the numpy composition: None for an empty mask, else uint8 [h,w,4] B, G, R, A over the padded, clipped box"""
    H, W = img.shape[:2]
    full = np.zeros((H, W), bool)
    full[:m.shape[0], :m.shape[1]] = m != 0
    x0, y0, x1, y1 = np_bbox(m)
    if x1 == 0:
        return None
    x0, y0, x1, y1 = max(0, x0 - pad), max(0, y0 - pad), min(W, x1 + pad), min(H, y1 + pad)
    a = np.where(full, 255, 0).astype(np.uint8)
    if alpha is not None:
        soft = (np.clip(alpha, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)   # fp32 product, truncated
        a = np.where(full, soft, 0).astype(np.uint8)
    out = np.concatenate([np.where((a > 0)[..., None], img, 0).astype(np.uint8), a[..., None]], axis=2)
    return out[y0:y1, x0:x1]


def _masks(H, W):
    m = np.zeros((8, H, W), bool)
    m[1, 0, 0] = m[2, 0, W - 1] = m[3, H - 1, 0] = m[4, H - 1, W - 1] = True   # [0] stays empty; one pixel in each corner
    m[5] = True                                                 # the full frame
    yy, xx = np.mgrid[:H, :W]
    m[6] = (yy - 40) ** 2 + (xx - 30) ** 2 < 300                # a disc
    m[7, 33:71, 2:W - 1] = (yy[33:71, 2:W - 1] + xx[33:71, 2:W - 1]) % 3 > 0   # spans several bands of rows, with holes
    return m


def test_mask_bboxes_against_numpy():
    from cartoonsegmentation_amd import ops
    for H, W in ((75, 90), (1, 1), (32, 33), (33, 300)):
        m = _masks(max(H, 75), max(W, 90))[:, :H, :W] if (H, W) != (75, 90) else _masks(H, W)
        want_boxes = np.array([np_bbox(k) for k in m], np.int32)
        for dev in (_dev(m), _dev(m.astype(np.uint8) * 3)):
            got = ops.mask_bboxes(dev)
            assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want_boxes)
    assert tuple(ops.mask_bboxes(torch.zeros((0, 5, 5), dtype=torch.bool, device='cuda')).shape) == (0, 4)


def _alpha_plane(H, W):
    rng = np.random.default_rng(12)
    alpha = rng.random((H, W), dtype=np.float32) * np.float32(1.6) - np.float32(0.3)      # values below 0 and above 1
    k = rng.integers(0, 256, (H, W // 2)).astype(np.float32)
    alpha[:, :W // 2] = k / np.float32(255)                     # exact multiples of 1 / 255 (as fp32 quotients)
    alpha[0, :4] = (0.0, 1.0, -0.0, 0.999999)
    return alpha


@pytest.mark.parametrize("pad", [0, 3, 200])
def test_cutout_bgra_against_numpy(pad):
    from cartoonsegmentation_amd import ops
    H, W = 75, 90
    img, m, alpha = mixed(H, W, 3, 2), _masks(H, W), _alpha_plane(H, W)
    cuts = ops.cutout_bgra(_dev(img), _dev(m), pad=pad)
    assert len(cuts) == 8 and cuts[0] is None
    base = [c for c in cuts if c is not None][0]
    for k in range(8):
        w = np_cutout(img, m[k], pad=pad)
        assert (cuts[k] is None) == (w is None)
        if w is not None:
            assert cuts[k].dtype == torch.uint8 and cuts[k].is_cuda and np.array_equal(cuts[k].cpu().numpy(), w), k
            assert cuts[k].untyped_storage().data_ptr() == base.untyped_storage().data_ptr()   # views of ONE buffer
    if pad == 200:
        assert tuple(cuts[6].shape) == (H, W, 4)                # the pad clips on all four sides
    soft = ops.cutout_bgra(_dev(img), _dev(m.astype(np.uint8)), alpha=_dev(alpha), pad=pad, indices=[6, 0, 5])
    assert len(soft) == 3 and soft[1] is None
    for got, k in ((soft[0], 6), (soft[2], 5)):
        assert np.array_equal(got.cpu().numpy(), np_cutout(img, m[k], alpha=alpha, pad=pad)), k
    assert ops.cutout_bgra(_dev(img), _dev(m), indices=[]) == []
    assert ops.cutout_bgra(_dev(img), _dev(m), indices=[0]) == [None]


def test_cutout_masks_smaller_than_the_frame_and_refusals():
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd._lib import CsmError
    H, W = 75, 90
    img = mixed(H, W, 3, 2)
    for dh, dw in ((1, 1), (2, 0), (0, 2)):
        m = _masks(H, W)[:, :H - dh, :W - dw]
        cuts = ops.cutout_bgra(_dev(img), _dev(m), pad=2)
        for k in range(8):
            w = np_cutout(img, m[k], pad=2)
            assert (cuts[k] is None) == (w is None) and (w is None or np.array_equal(cuts[k].cpu().numpy(), w)), (dh, dw, k)
    ok = _dev(_masks(H, W))
    for bad in (ok[:, :H - 3], ok[:, :, :W - 3], torch.zeros((2, H + 1, W), dtype=torch.bool, device='cuda')):
        with pytest.raises(CsmError):
            ops.cutout_bgra(_dev(img), bad)
    with pytest.raises(CsmError):
        ops.cutout_bgra(img, ok)                                # a host frame
    with pytest.raises(CsmError):
        ops.cutout_bgra(_dev(img), ok.float())
    with pytest.raises(CsmError):
        ops.cutout_bgra(_dev(img), ok, alpha=torch.zeros((H, W + 1), device='cuda'))
    with pytest.raises(ValueError):
        ops.cutout_bgra(_dev(img), ok, pad=-1)
    with pytest.raises(IndexError):
        ops.cutout_bgra(_dev(img), ok, indices=[8])


# ---- surfaces -----------------------------------------------------------------------------------------------------------------
def _read_bgra(path_or_bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else str(path_or_bytes))
    assert im.mode == 'RGBA'
    return np.asarray(im)[..., [2, 1, 0, 3]]


def test_cutouts_and_save_cutouts(tmp_path):
    from animeinsseg.anime_instances import AnimeInstances
    H, W = 75, 90
    img, m = mixed(H, W, 3, 2), _masks(H, W)
    boxes = np.zeros((8, 4), np.float32)
    for inst, frame in ((AnimeInstances(masks=_dev(m), bboxes=_dev(boxes)), _dev(img)), (AnimeInstances(masks=m, bboxes=boxes), img)):
        cuts = inst.cutouts(frame, pad=1)
        assert [c is None for c in cuts] == [True] + [False] * 7
        for k in range(1, 8):
            assert np.array_equal(cuts[k].cpu().numpy(), np_cutout(img, m[k], pad=1))
        assert [tuple(c.shape) for c in inst.cutouts(frame, draw_indices=[5])] == [(H, W, 4)]
    paths = inst.save_cutouts(img, str(tmp_path / "out"), "frame.jpg", pad=1)
    assert [os.path.basename(p) for p in paths] == ['cutout_%03d_frame.jpg.webp' % k for k in range(1, 8)]
    assert sorted(os.listdir(str(tmp_path / "out"))) == [os.path.basename(p) for p in paths]
    for k, p in zip(range(1, 8), paths):
        w = np_cutout(img, m[k], pad=1)
        assert np.array_equal(_read_bgra(p), w)
        assert open(p, 'rb').read() == R.encode(w)
    assert AnimeInstances().cutouts(img) == [] and AnimeInstances().save_cutouts(img, str(tmp_path / "none"), "x") == []


def test_save_cutout_only_writes_one_webp_per_instance(tmp_path):
    """_infer_save_annotations(save_cutout_only=True): cutout_XXX_<name>.webp per instance, the numpy composition of the masks a
    plain infer gives; no JSON; infer() does not forward the flag"""
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    net = AnimeInsSeg('synthetic', default_det_size=96, refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    imgs = [synth.image_u8(160, 192, 50 + k) for k in range(2)]
    plain = net.infer(imgs, pred_score_thr=0.0, max_instances=3, output_type='numpy')
    assert sum(len(p) for p in plain) >= 1
    sd, js = tmp_path / "sd", tmp_path / "pred.json"
    assert net._infer_save_annotations(imgs, 0.0, str(sd), str(js), -1, -1, None, save_cutout_only=True) is None
    assert not js.exists()
    expected = {}
    for k, res in enumerate(plain):
        for j in range(len(res)):
            w = np_cutout(imgs[k], np.asarray(res.masks[j]))
            if w is not None:
                expected['cutout_%03d_%012d.jpg.webp' % (j, k)] = w
    assert expected and sorted(os.listdir(str(sd))) == sorted(expected)
    for nm, w in expected.items():
        assert np.array_equal(_read_bgra(sd / nm), w)
    via = tmp_path / "via_infer"
    net.infer(imgs, save_annotation=str(tmp_path / "a.json"), save_dir=str(via), save_cutout_only=True, pred_score_thr=0.0, max_instances=3)
    assert (tmp_path / "a.json").exists() and os.listdir(str(via)) == []


def test_imwrite_webp(tmp_path):
    from utils.io_utils import imwrite
    for nm in ('list-33x17', 'block-17x15', 'bordered-bgra'):
        a = image(nm)
        p1, p2 = str(tmp_path / "sub" / (nm + ".webp")), str(tmp_path / (nm + ".WEBP"))
        assert imwrite(_dev(a), p1) is True and imwrite(a, p2) is True
        assert open(p1, 'rb').read() == open(p2, 'rb').read() == want(nm)
        check_file(open(p1, 'rb').read(), a)
    with pytest.raises(ValueError):
        imwrite(image('bordered-bgra'), str(tmp_path / "a.png"))     # four channels stay refused everywhere else
    with pytest.raises(ValueError):
        imwrite(image('bordered-bgra'), str(tmp_path / "a.jpg"))
    with pytest.raises(ValueError):
        imwrite(np.zeros((4, 4, 2), np.uint8), str(tmp_path / "b.webp"))
    with pytest.raises(ValueError):
        imwrite(image('block-17x15'), str(tmp_path / "a.tiff"))


def test_get_cutout(monkeypatch):
    monkeypatch.setenv("CSM_SYNTHETIC_WEIGHTS", "1")
    from animeinsseg.models.animeseg_refine import get_cutout, get_mask, load_refinenet
    from cartoonsegmentation_amd import synth
    model = load_refinenet('animeseg')
    for (H, W), s in (((150, 97), 128),):
        rgb = synth.image_u8(H, W, 8)
        p = get_mask(model, rgb, use_amp=True, s=s)[..., 0]
        got = get_cutout(model, rgb, use_amp=True, s=s)
        assert got.dtype == np.uint8 and got.shape == (H, W, 4)
        a = (np.clip(p, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)     # the reference's mask * 255 -> uint8
        assert np.array_equal(got[..., 3], a) and 0 < a.mean() < 255
        assert np.array_equal(got[..., :3], np.where((a > 0)[..., None], rgb, 0))
        assert np.array_equal(get_cutout(model, torch.from_numpy(rgb).cuda(), s=s), got)
