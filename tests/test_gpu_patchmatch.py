"""GPU: the HIP PatchMatch (csrc/patchmatch.hip) is byte-identical to its numpy restatement (tests/patchmatch_restatement.py,
contract DESIGN.md §4.5) through ops.patchmatch_inpaint, the drop-in animeinsseg.inpainting.patch_match and
KenBurnsPipeline(inpaint_type='patchmatch')."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchmatch_restatement as R  # noqa: E402
from test_patchmatch import stripes, textured  # noqa: E402


def _masks(H, W, kind):
    m = np.zeros((H, W), np.uint8)
    if kind == 'rect':
        m[H // 4:H // 2, W // 3:W // 3 + W // 4] = 1
    elif kind == 'border':                           # two holes touching all four borders
        m[:H // 5, W // 2:] = 1
        m[H - H // 4:, :W // 3] = 7
        m[H // 3:H // 2, :3] = 255
    elif kind == 'most':                             # most of the frame: only a band on the left is known
        m[:, W // 4:] = 1
    elif kind == 'blobs':
        yy, xx = np.mgrid[:H, :W]
        m[np.hypot(yy - 0.3 * H, xx - 0.6 * W) < 0.18 * min(H, W)] = 1
        m[np.hypot(yy - 0.7 * H, xx - 0.25 * W) < 0.12 * min(H, W)] = 1
    return m


def _gmask(H, W):
    g = np.zeros((H, W), np.uint8)
    g[H - H // 3:, W - W // 3:] = 1
    return g


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _both(img, m, g, p, seed=0):
    from cartoonsegmentation_amd import ops
    got = ops.patchmatch_inpaint(_dev(img), _dev(m), _dev(g), patch_size=p, seed=seed).cpu().numpy()
    return got, R.patchmatch_inpaint(img, m, g, patch_size=p, seed=seed)


@pytest.mark.parametrize("H,W", [(37, 53), (64, 48), (96, 128)])
@pytest.mark.parametrize("p", [3, 5, 15])
def test_op_is_byte_identical_to_the_restatement(H, W, p):
    img = textured(H, W, H + p)
    for kind in ('rect', 'border', 'blobs', 'most'):
        for g in (None, _gmask(H, W)):
            got, want = _both(img, _masks(H, W, kind), g, p, seed=H * W + p)
            assert got.dtype == np.uint8 and got.shape == (H, W, 3)
            assert np.array_equal(got, want), (H, W, p, kind, g is not None, int((got != want).any(-1).sum()))


def test_stripes_mask_shapes_and_seeds():
    from cartoonsegmentation_amd import ops
    img = stripes(64, 96)
    m = _masks(64, 96, 'rect')
    for p in (3, 7):
        for seed in (0, 1, 0xDEADBEEF):
            got, want = _both(img, m, None, p, seed)
            assert np.array_equal(got, want), (p, seed)
    a = ops.patchmatch_inpaint(_dev(img), _dev(m[..., None]), patch_size=5, seed=3)       # [H,W,1]
    b = ops.patchmatch_inpaint(_dev(img), _dev(m.astype(bool)), patch_size=5, seed=3)     # bool
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), R.patchmatch_inpaint(img, m, patch_size=5, seed=3))


def test_empty_mask_and_no_valid_source_return_the_input():
    from cartoonsegmentation_amd import ops
    img = textured(37, 53, 1)
    d = _dev(img)
    out = ops.patchmatch_inpaint(d, _dev(np.zeros((37, 53), np.uint8)), patch_size=3)
    assert torch.equal(out, d) and out.data_ptr() != d.data_ptr()
    m = np.ones((37, 53), np.uint8)
    m[::4, ::4] = 0
    got, want = _both(img, m, None, 5)
    assert np.array_equal(got, want) and np.array_equal(got, img)
    g = np.ones((37, 53), np.uint8)                  # every pixel excluded: no valid source
    got, want = _both(img, _masks(37, 53, 'rect'), g, 3)
    assert np.array_equal(got, want) and np.array_equal(got, img)


def test_repeated_calls_agree_bit_for_bit():
    from cartoonsegmentation_amd import ops
    img, m = _dev(textured(96, 128, 2)), _dev(_masks(96, 128, 'blobs'))
    a = ops.patchmatch_inpaint(img, m, patch_size=5, seed=11)
    for _ in range(3):
        assert torch.equal(a, ops.patchmatch_inpaint(img, m, patch_size=5, seed=11))


def test_op_argument_errors():
    from cartoonsegmentation_amd import _lib, ops
    img = _dev(textured(20, 20, 0))
    with pytest.raises(ValueError):
        ops.patchmatch_inpaint(img, _dev(np.ones((20, 20), np.uint8)), patch_size=21)
    with pytest.raises(ValueError):
        ops.patchmatch_inpaint(img, _dev(np.ones((20, 20), np.uint8)), patch_size=4)
    with pytest.raises(_lib.CsmError):
        ops.patchmatch_inpaint(img, _dev(np.ones((20, 21), np.uint8)), patch_size=3)
    with pytest.raises(_lib.CsmError):
        ops.patchmatch_inpaint(img, torch.ones((20, 20), dtype=torch.uint8), patch_size=3)


def test_dropin_inpaint_matches_the_restatement():
    from PIL import Image
    from animeinsseg.inpainting import patch_match
    img = textured(64, 48, 8)
    m = _masks(64, 48, 'blobs')
    g = _gmask(64, 48)
    patch_match.set_random_seed(5)
    try:
        out = patch_match.inpaint(img, m, global_mask=g, patch_size=3)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8
        assert np.array_equal(out, R.patchmatch_inpaint(img, m, g, patch_size=3, seed=5))
        assert np.array_equal(patch_match.inpaint(Image.fromarray(img), Image.fromarray(m), global_mask=g, patch_size=3), out)
        white = img.copy()
        white[m > 0] = 255                           # mask=None: the purely white pixels are the holes
        assert np.array_equal(patch_match.inpaint(white, patch_size=3), R.patchmatch_inpaint(white, m, patch_size=3, seed=5))
    finally:
        patch_match.set_random_seed(0)
    assert np.array_equal(patch_match.inpaint(img, m), R.patchmatch_inpaint(img, m, patch_size=15, seed=0))


# ---- Ken Burns -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kb():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    H, W = 320, 384
    kw = dict(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False, depth_field=False,
              focal=W / 2.0, num_frame=3, mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(KenBurnsConfig(**kw))
    pm = KenBurnsPipeline(KenBurnsConfig(inpaint_type='patchmatch', **kw))
    img = synth.image_u8(H, W, 11)
    from test_gpu_kenburns import _two_instances     # a disc and a bar lifted to planes: every view disoccludes background
    return pipe, pm, img, _two_instances(H, W)


def _shift(pipe, kc):
    from cartoonsegmentation_amd import ops
    W, H = kc['intWidth'], kc['intHeight']
    oF = {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(math.floor(0.97 * W)), 'intCropHeight': int(math.floor(0.97 * H))}
    oT = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': oF}, kc)
    d_from = kc['objDepthrange'][0]
    s = ops.shift_vector({'fltShiftU': oT['fltCenterU'] - W / 2.0, 'fltShiftV': oT['fltCenterV'] - H / 2.0, 'fltDepthFrom': d_from,
                          'fltDepthTo': d_from * (oT['intCropWidth'] / max(oF['intCropWidth'], oT['intCropWidth']))}, kc)
    return 1.1 * torch.tensor(s, dtype=torch.float32).view(1, 3, 1).cuda()


def _inpaint_once(pipe, kc, shift):
    """one KenBurnsPipeline.inpaint pass from the raw cloud (process_kenburns' initial state)"""
    kc.inpainted_img = kc['tenRawImage'].view(1, 3, -1)
    kc['tenInpaDisparity'] = kc['tenRawDisparity'].view(1, 1, -1)
    kc['tenInpaDepth'] = kc['tenRawDepth'].view(1, 1, -1)
    kc['tenInpaPoints'] = kc['tenRawPoints'].view(1, 3, -1)
    o = pipe.inpaint(shift, None, kc)
    kc._inpaint_shared = None
    return o, {k: v.clone() for k, v in (('img', kc.inpainted_img), ('disp', kc['tenInpaDisparity']), ('depth', kc['tenInpaDepth']),
                                         ('pts', kc['tenInpaPoints']))}


def test_kenburns_patchmatch_inpaint_matches_gridnet_then_restatement(kb):
    pipe, pm, img, inst = kb
    assert pm.inpaint_type == 'patchmatch' and pipe.inpaint_type == 'default'
    kc = pipe.generate_kenburns_config(img, instances=inst)
    shift = _shift(pipe, kc)
    o_d, app_d = _inpaint_once(pipe, kc, shift)
    o_p, app_p = _inpaint_once(pm, kc, shift)
    H, W = kc['intHeight'], kc['intWidth']
    grid = o_d['tenImage'][0].cpu().numpy()
    u8 = (grid * 255).astype(np.uint8).transpose(1, 2, 0)                               # kenburns_effect.py:497-499
    hole = o_d['tenExisting'][0, 0].cpu().numpy() == 0.0
    assert o_d['segmasks'] is not None
    mask = (hole | (o_d['segmasks'][0, 0].cpu().numpy() > 0)).astype(np.uint8)
    assert 0 < hole.sum() and mask.sum() > hole.sum()
    want = R.patchmatch_inpaint(u8, mask, patch_size=3, seed=0)
    want_f = want.transpose(2, 0, 1)[None].astype(np.float32) * (1.0 / 255.0)           # :501
    assert np.array_equal(o_p['tenImage'].cpu().numpy(), want_f)
    assert torch.equal(o_p['tenExisting'], o_d['tenExisting'])
    n0 = kc['tenRawPoints'].shape[2]
    assert np.array_equal(app_p['img'][:, :, n0:].cpu().numpy(), want_f.reshape(1, 3, -1)[:, :, hole.reshape(-1)])
    assert torch.equal(app_p['img'][:, :, :n0], app_d['img'][:, :, :n0])
    for k in ('disp', 'depth', 'pts'):                                                   # the GridNet's, untouched
        assert torch.equal(app_p[k], app_d[k]), k
    assert torch.equal(o_p['tenDisparity'], o_d['tenDisparity'])
    assert app_p['img'].shape == app_d['img'].shape and H * W > 0


def test_kenburns_patchmatch_autozoom_frames(kb):
    pipe, pm, img, inst = kb
    kc = pm.generate_kenburns_config(img, instances=inst)
    frames = pm.autozoom(kc)
    assert len(frames) == kc.num_frame
    for f in frames:
        f = f.cpu().numpy() if hasattr(f, 'cpu') else np.asarray(f)
        assert f.shape == (kc['intHeight'], kc['intWidth'], 3) and f.dtype == np.uint8


def test_kenburns_inpaint_types(kb):
    pipe, pm, img, inst = kb
    assert pm.inpaint_type == 'patchmatch' and pm._inpaint_ws is not None       # the GridNet weights load for patchmatch too
    pipe.set_inpainting('patchmatch')
    try:
        assert pipe.inpaint_type == 'patchmatch'
        with pytest.raises(NotImplementedError):
            pipe.set_inpainting('ldm')
    finally:
        pipe.set_inpainting('default')
    assert pipe.inpaint_type == 'default'
