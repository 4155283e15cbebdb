"""CPU: the PatchMatch inpainting contract on its numpy restatement, and the host surface of the drop-in
animeinsseg.inpainting.patch_match.  The GPU tests (test_gpu_patchmatch.py) hold the HIP library byte-identical to the restatement."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchmatch_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def stripes(H, W):
    """period-8 vertical stripes, two colours"""
    x = np.arange(W)
    img = np.empty((H, W, 3), np.uint8)
    img[..., 0] = np.where(x % 8 < 4, 30, 200)[None, :]
    img[..., 1] = 255 - img[..., 0]
    img[..., 2] = 90
    return img


def textured(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    base = np.stack([(x * 5) % 256, (y * 7) % 256, ((x + y) * 3) % 256], -1)
    return np.clip(base + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)


def test_constant_image_fills_with_the_constant():
    img = np.full((40, 56, 3), (17, 140, 233), np.uint8)
    for p in (3, 5, 15):
        out = R.patchmatch_inpaint(img, _rect(40, 56, 10, 25, 12, 40), patch_size=p)
        assert np.array_equal(out, img), p


def test_two_colour_image_fills_from_its_own_region_only():
    H, W, p = 48, 64, 5
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :32] = (200, 30, 10)
    img[:, 32:] = (10, 60, 220)
    m = _rect(H, W, 18, 30, 10, 20)                  # more than p from the colour edge and from the frame
    out = R.patchmatch_inpaint(img, m, patch_size=p)
    assert (out[m > 0] == (200, 30, 10)).all()


def test_stripe_texture_is_reproduced_in_the_hole():
    """period-8 stripes: the hole is continued in phase on every pixel (pinned from the restatement: 1.0 at each size)"""
    for H, W, p, hole in ((48, 64, 3, (16, 28, 21, 34)), (48, 64, 5, (16, 28, 21, 34)), (64, 96, 15, (20, 40, 30, 55))):
        img = stripes(H, W)
        m = _rect(H, W, *hole)
        out = R.patchmatch_inpaint(img, m, patch_size=p)
        frac = (out[m > 0] == img[m > 0]).all(-1).mean()
        assert frac >= 0.95 and frac == 1.0, (H, W, p, frac)


def test_known_pixels_never_change_and_fill_stays_in_the_source_range():
    H, W, p = 45, 61, 5
    img = textured(H, W, 3)
    m = np.zeros((H, W), np.uint8)
    m[5:20, 8:30] = 1
    m[30:44, 40:61] = 1                              # touches the bottom and right borders
    out = R.patchmatch_inpaint(img, m, patch_size=p, seed=9)
    known = m == 0
    assert np.array_equal(out[known], img[known])
    lv = R.build_pyramid(img, m > 0, np.zeros((H, W), bool), p)
    r = p // 2
    src = R._window_any(lv[0]['valid'], r)           # every pixel inside some valid source window
    lo, hi = img[src].min(0), img[src].max(0)
    assert (out[m > 0] >= lo).all() and (out[m > 0] <= hi).all()


def test_global_mask_region_never_appears_in_the_fill():
    H, W, p = 48, 64, 3
    img = textured(H, W, 4)
    img[30:44, 4:20] = (255, 0, 255)                 # a uniquely coloured region
    g = _rect(H, W, 30, 44, 4, 20)
    assert ((img == (255, 0, 255)).all(-1) == (g > 0)).all()
    m = _rect(H, W, 8, 24, 30, 50)
    free = R.patchmatch_inpaint(img, m, patch_size=p)
    out = R.patchmatch_inpaint(img, m, global_mask=g, patch_size=p)
    fill = out[m > 0].astype(int)
    assert not ((fill[:, 0] > 200) & (fill[:, 1] < 60) & (fill[:, 2] > 200)).any()
    assert np.array_equal(out[m == 0], img[m == 0]) and not np.array_equal(free, out)


def test_same_seed_same_bytes_and_the_seed_matters():
    img, m = textured(40, 52, 5), _rect(40, 52, 12, 28, 14, 36)
    a = R.patchmatch_inpaint(img, m, patch_size=3, seed=1)
    assert np.array_equal(a, R.patchmatch_inpaint(img, m, patch_size=3, seed=1))
    assert not np.array_equal(a, R.patchmatch_inpaint(img, m, patch_size=3, seed=2))


def test_empty_mask_and_no_valid_source_return_the_input():
    img = textured(37, 53, 6)
    out = R.patchmatch_inpaint(img, np.zeros((37, 53, 1), np.uint8), patch_size=5)
    assert np.array_equal(out, img) and out is not img
    m = np.ones((37, 53), np.uint8)
    m[::4, ::4] = 0                                  # no 5x5 window free of holes
    assert np.array_equal(R.patchmatch_inpaint(img, m, patch_size=5), img)


def test_restatement_shape_rules():
    img = np.zeros((14, 40, 3), np.uint8)
    with pytest.raises(ValueError):
        R.patchmatch_inpaint(img, np.ones((14, 40), np.uint8), patch_size=15)     # smaller than the patch
    for p in (1, 4, 17):
        with pytest.raises(ValueError):
            R.patchmatch_inpaint(np.zeros((40, 40, 3), np.uint8), np.ones((40, 40), np.uint8), patch_size=p)
    assert R.max_levels(1024, 1024, 3) == 9 and R.max_levels(37, 53, 15) == 2 and R.max_levels(29, 53, 15) == 1 and R.max_levels(96, 128, 5) == 5


def test_hash_is_the_stated_lowbias32_chain():
    """the counter hash both sides compute (pinned values: a change of the chain changes every fill)"""
    px = np.array([0, 1, 12345], np.uint32)
    got = R.rng(7, 2, 3, 1, px, 5).tolist()
    h = R._mix32(7 ^ 0x9E3779B9)
    for v in (2, 3, 1):
        h = R._mix32(h ^ v)
    assert got == [R._mix32(R._mix32(h ^ int(q)) ^ 5) for q in px]
    assert R.rng(0, 0, 0, R.INIT_PASS, np.array([0], np.uint32), 0).dtype == np.uint32


# ---- drop-in surface -------------------------------------------------------------------------------------------------------
def test_reference_import_surface_and_signatures():
    from animeinsseg.inpainting import patch_match
    from animeinsseg.inpainting.patch_match import inpaint, inpaint_regularity, set_random_seed, set_verbose  # noqa: F401
    assert patch_match.__all__ == ['set_random_seed', 'set_verbose', 'inpaint', 'inpaint_regularity']
    sig = inspect.signature(patch_match.inpaint).parameters
    assert list(sig) == ['image', 'mask', 'global_mask', 'patch_size']
    assert sig['mask'].default is None and sig['global_mask'].kind is inspect.Parameter.KEYWORD_ONLY and sig['patch_size'].default == 15
    sig = inspect.signature(patch_match.inpaint_regularity).parameters
    assert list(sig) == ['image', 'mask', 'ijmap', 'global_mask', 'patch_size', 'guide_weight']
    assert sig['guide_weight'].default == 0.25
    assert list(inspect.signature(set_random_seed).parameters) == ['seed']
    assert list(inspect.signature(set_verbose).parameters) == ['verbose']
    with pytest.raises(NotImplementedError):
        inpaint_regularity(np.zeros((8, 8, 3), np.uint8), None, np.zeros((8, 8, 3), np.float32))


def test_import_loads_no_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from animeinsseg.inpainting import patch_match\n"
            "from cartoonsegmentation_amd import _lib\n"
            "assert _lib._lib is None\n"
            "patch_match.set_random_seed(3); patch_match.set_verbose(True)\n"
            "assert patch_match._seed == 3 and _lib._lib is None\n" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_argument_handling_of_the_reference():
    from PIL import Image
    from animeinsseg.inpainting.patch_match import _checked_arguments
    img = textured(20, 24, 7)
    img[3:6, 4:9] = 255
    img[10, 10] = (255, 255, 254)
    im, m, g = _checked_arguments(img, None, None)
    assert m.shape == (20, 24, 1) and m.dtype == np.uint8 and g is None
    assert m[..., 0].sum() == 15 and m[3:6, 4:9].all() and m[10, 10, 0] == 0     # purely white pixels only
    im2, m2, g2 = _checked_arguments(Image.fromarray(img), Image.fromarray(m[..., 0] * 255), m[..., 0])
    assert np.array_equal(im2, img) and m2.shape == (20, 24, 1) and g2.shape == (20, 24, 1)
    for bad in (img.astype(np.float32), img[..., :2], img[..., 0]):
        with pytest.raises(AssertionError):
            _checked_arguments(bad, None, None)
    for bad in (m[..., 0].astype(bool), m[..., 0].astype(np.float32), np.zeros((20, 24, 2), np.uint8)):
        with pytest.raises(AssertionError):
            _checked_arguments(img, bad, None)
        with pytest.raises(AssertionError):
            _checked_arguments(img, None, bad)


def test_op_refuses_cpu_tensors():
    import torch
    from cartoonsegmentation_amd import _lib, ops
    with pytest.raises(_lib.CsmError):
        ops.patchmatch_inpaint(torch.zeros((16, 16, 3), dtype=torch.uint8), torch.zeros((16, 16), dtype=torch.uint8))


def test_pipeline_accepts_patchmatch_and_still_refuses_ldm():
    """set_inpainting on a bare pipeline whose inpaint weights are already loaded: no GPU, no checkpoint needed"""
    from cartoonsegmentation_amd.kenburns import KenBurnsPipeline
    pipe = KenBurnsPipeline.__new__(KenBurnsPipeline)
    ws = object()
    pipe._inpaint_ws = ws
    pipe.set_inpainting('patchmatch')
    assert pipe.inpaint_type == 'patchmatch' and pipe._inpaint_ws is ws          # the GridNet weights stay: it runs first
    pipe.set_inpainting('default')
    assert pipe.inpaint_type == 'default'
    for bad in ('ldm', 'PatchMatch', 'telea'):
        with pytest.raises(NotImplementedError):
            pipe.set_inpainting(bad)
    assert pipe.inpaint_type == 'default'
