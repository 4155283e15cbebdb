"""CPU: host side of refine_method='animeseg' (reference animeinsseg/__init__.py:78-115, animeseg_refine/__init__.py:154-188): the
letterbox size rule, the /255 of the input canvas, the checkpoint layouts, the drop-in import surface, and the glue restated with the
oracle's resamplers against the fixture made from the reference's own text (tests/golden/make_golden_animeseg.py)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["pin_animeseg_64x48", "pin_animeseg_40x64"]


def _reference_size_rule(input_img_shape, s):
    """the text of get_mask :170-174, verbatim apart from the function frame"""
    h0, w0 = h, w = input_img_shape[0], input_img_shape[1]
    if h > w:
        h, w = s, int(s * w / h)
    else:
        h, w = int(s * h / w), s
    return h, w


def test_letterbox_size_rule_is_the_reference_text():
    from cartoonsegmentation_amd.segmentation import animeseg_size
    shapes = [(64, 48), (40, 64), (333, 517), (1024, 828), (828, 1024), (1080, 1920), (720, 720), (1, 1), (7, 3), (3, 7),
              (1001, 999), (999, 1001), (719, 1280), (1280, 719), (2160, 3840), (3, 1000)]
    g = np.random.default_rng(0)
    shapes += [tuple(int(v) for v in g.integers(1, 4000, 2)) for _ in range(400)]
    truncation_differs = 0
    for s in (64, 256, 640, 720, 1024):
        for H, W in shapes:
            want = _reference_size_rule((H, W), s)
            if min(want) < 1:
                with pytest.raises(Exception, match="aspect ratio"):
                    animeseg_size(H, W, s)
                continue
            assert animeseg_size(H, W, s) == want, (H, W, s)
            short = s * min(H, W) / max(H, W)
            truncation_differs += int(round(short)) != int(short)
    assert truncation_differs > 50                    # the sweep holds many shapes where rounding would give another size


def test_div255_fp32_equals_the_float64_quotient_for_every_byte():
    """the canvas holds np.float32(u8 / 255) (float64 quotient stored as float32); the kernel divides in fp32"""
    v = np.arange(256, dtype=np.uint8)
    ref = (v / 255).astype(np.float32)
    assert (v / 255).dtype == np.float64
    assert np.array_equal(v.astype(np.float32) / np.float32(255.0), ref)


def _isnet_names():
    """ISNetDIS(in_ch=3) parameters the lowering reads, with their closed-form values"""
    from cartoonsegmentation_amd.nets import build_isnet
    from cartoonsegmentation_amd.weights import SynthWeights
    src, rec = SynthWeights('animeseg.'), {}

    class Rec:
        def get(self, name, shape, kind):
            rec[name] = src.get(name, shape, kind)
            return rec[name]
    build_isnet(Rec(), 1, 32, 32, in_ch=3)
    return rec


def test_checkpoint_layouts(tmp_path):
    from cartoonsegmentation_amd.nets import build_isnet
    from cartoonsegmentation_amd.segmentation import load_animeseg_weights
    from cartoonsegmentation_amd.weights import SynthWeights
    rec = _isnet_names()
    bare = {k: torch.from_numpy(v.copy()) for k, v in rec.items()}
    bare['conv_in.num_batches_tracked'] = torch.tensor(0)           # extra entries of a real state dict are ignored
    flat = {'net.' + k: v for k, v in bare.items()}
    flat.update({'gt_encoder.conv_in.weight': torch.full((16, 1, 3, 3), 7.0), 'gt_encoder.conv_in.bias': torch.zeros(16)})
    lightning = {'epoch': 3, 'global_step': 99, 'pytorch-lightning_version': '1.9.0', 'state_dict': flat}
    ref = build_isnet(SynthWeights('animeseg.'), 1, 32, 32, in_ch=3).serialise(oracle=False)[2]
    for tag, blob in (('bare', bare), ('flat', flat), ('lightning', lightning)):
        p = tmp_path / ('%s.ckpt' % tag)
        torch.save(blob, p)
        ws = load_animeseg_weights(str(p))
        assert not any(k.startswith(('net.', 'gt_encoder.')) for k in ws.sd), tag
        w = build_isnet(ws, 1, 32, 32, in_ch=3).serialise(oracle=False)[2]
        assert np.array_equal(w, ref), tag
    with pytest.raises(FileNotFoundError):
        load_animeseg_weights(str(tmp_path / 'missing.ckpt'))
    assert isinstance(load_animeseg_weights(str(tmp_path / 'missing.ckpt'), synthetic=True), SynthWeights)
    assert load_animeseg_weights(str(tmp_path / 'missing.ckpt'), synthetic=True).prefix == 'animeseg.'


def test_refine_method_and_import_surface():
    from animeinsseg import VALID_REFINEMETHODS
    from animeinsseg.models.animeseg_refine import AnimeSegmentation, get_mask, load_refinenet
    import inspect
    assert 'animeseg' in VALID_REFINEMETHODS and {'refinenet_isnet', 'none'} <= VALID_REFINEMETHODS
    assert list(inspect.signature(get_mask).parameters) == ['model', 'input_img', 'use_amp', 's']
    assert inspect.signature(get_mask).parameters['s'].default == 640
    assert list(inspect.signature(load_refinenet).parameters) == ['refine_method', 'device']
    assert callable(AnimeSegmentation)
    with pytest.raises(NotImplementedError):
        load_refinenet('refinenet_isnet')


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def restated_prepare(img_bgr, s, bgr_to_rgb):
    """letterbox of get_mask with the oracle's cv2 INTER_LINEAR u8 resize -> [1,3,s,s]"""
    from cartoonsegmentation_amd.segmentation import animeseg_size
    from oracle import segment as oseg
    H, W = img_bgr.shape[:2]
    h, w = animeseg_size(H, W, s)
    r = np.empty((h, w, 3), np.uint8)
    oseg.lib().orc_resize_u8_linear(_p(np.ascontiguousarray(img_bgr)), ctypes.c_int(H), ctypes.c_int(W), ctypes.c_int(3),
                                    ctypes.c_int(h), ctypes.c_int(w), _p(r))
    if bgr_to_rgb:
        r = r[..., ::-1]
    x = np.zeros((1, 3, s, s), np.float32)
    ph, pw = s - h, s - w
    x[0, :, ph // 2:ph // 2 + h, pw // 2:pw // 2 + w] = (r / 255).astype(np.float32).transpose(2, 0, 1)
    return x


def restated_prob(prob_plane, H0, W0):
    """crop of the s x s sigmoid plane + the oracle's cv2 float INTER_LINEAR back to (H0, W0)"""
    from cartoonsegmentation_amd.segmentation import animeseg_size
    from oracle import segment as oseg
    s = prob_plane.shape[-1]
    h, w = animeseg_size(H0, W0, s)
    ph, pw = s - h, s - w
    crop = np.ascontiguousarray(prob_plane[ph // 2:ph // 2 + h, pw // 2:pw // 2 + w], np.float32)
    out = np.empty((H0, W0), np.float32)
    oseg.lib().orc_resize_f32_linear(_p(crop), ctypes.c_int(h), ctypes.c_int(w), ctypes.c_int(1), ctypes.c_int(H0), ctypes.c_int(W0),
                                     _p(out))
    return out


def restated_select(masks, fg):
    """animeseg_refine :96-105 with fg[:Hm, :Wm] (detector masks can be smaller than the frame), in integers"""
    k, Hm, Wm = masks.shape
    f = fg[:Hm, :Wm]
    out = masks.copy()
    for i in range(k):
        ao, ar = int(masks[i].sum()), int((masks[i] & f).sum())
        if 10 * ar > 3 * ao:
            out[i] = masks[i] & f
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_glue_restated_against_the_reference_fixture(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    img, s = d['img'], int(d['s'])
    H, W = img.shape[:2]
    assert np.array_equal(restated_prepare(img, s, True), d['x'])
    logits = ((d['logits_raw'] - np.float32(d['centre'])) / np.float32(d['scale'])).astype(np.float32)
    prob = restated_prob(torch.from_numpy(logits).sigmoid().numpy()[0, 0], H, W)     # the sigmoid the reference called
    assert np.array_equal(prob, d['prob'])
    out = restated_select(d['masks_in'], prob > 0.5)
    assert np.array_equal(out, d['masks_out'])
    # the fixture's instances: refined, kept, ratio exactly 0.3 (kept), 0.31 (refined), empty (kept)
    assert [bool(np.array_equal(o, m)) for o, m in zip(d['masks_out'], d['masks_in'])][:5] == [False, True, True, False, True]


def test_integer_select_rule_equals_the_float64_rule():
    """10 * ar > 3 * ao  ==  ar / ao > 0.3 (float64, nan for 0/0) -- exhaustively for small areas, sampled for frame-sized ones"""
    for ao in range(0, 400):
        for ar in range(0, ao + 1):
            with np.errstate(invalid='ignore'):
                ref = bool(np.float64(ar) / np.float64(ao) > 0.3) if ao else False
            assert (10 * ar > 3 * ao) == ref, (ar, ao)
    g = np.random.default_rng(1)
    for ao in list(g.integers(1, 4096 * 4096, 2000)) + [10 * 1024 * 1024, 3840 * 2160]:
        ao = int(ao)
        for ar in {(3 * ao) // 10 - 1, (3 * ao) // 10, (3 * ao) // 10 + 1, -(-3 * ao // 10)}:
            if 0 <= ar <= ao:
                assert (10 * ar > 3 * ao) == (ar / ao > 0.3), (ar, ao)
