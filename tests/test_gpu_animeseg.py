"""GPU: refine_method='animeseg' (reference animeinsseg/__init__.py:78-115, animeseg_refine/__init__.py:154-188) on the MI355X --
the three glue kernels bit-exact against the CPU restatement (tests/test_animeseg_host.py, oracle/post_oracle.c resamplers), the
ISNet-IS program against the oracle interpreter and the reference fixture, and AnimeInsSeg.infer / get_mask / KenBurnsPipeline
against the CPU chain oracle/segment.detect -> restated refine with the oracle ISNet-IS."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("animeseg_host_restated", os.path.join(HERE, "test_animeseg_host.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)

SHAPES = [(64, 48), (40, 64), (333, 517), (1024, 828), (828, 1024), (1080, 1920), (720, 720)]
SIZES = [64, 256, 720]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _orc_sigmoid(x):
    from oracle import segment as oseg
    f = oseg.lib().orc_sigmoid_scalar
    return np.array([f(float(v)) for v in x.ravel()], np.float32).reshape(x.shape)


def _prepare(img, s, bgr):
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, ptr, stream_ptr
    from cartoonsegmentation_amd.segmentation import animeseg_size
    L = _lib.load()
    H, W = img.shape[:2]
    h, w = animeseg_size(H, W, s)
    img_d = dev(img)
    x = torch.full((1, 3, s, s), float('nan'), device='cuda')
    check(L.csm_animeseg_prepare(ptr(img_d), i32(H), i32(W), i32(h), i32(w), i32(s), i32(bgr), ptr(x), stream_ptr()), "prepare")
    return x


def _mask(logits_d, s, H0, W0, thr=0.5):
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, f32, i32, ptr, stream_ptr
    from cartoonsegmentation_amd.segmentation import animeseg_size
    L = _lib.load()
    h, w = animeseg_size(H0, W0, s)
    prob = torch.full((H0, W0), float('nan'), device='cuda')
    fg = torch.full((H0, W0), 7, dtype=torch.uint8, device='cuda')
    check(L.csm_animeseg_mask(ptr(logits_d), i32(s), i32(h), i32(w), i32(H0), i32(W0), f32(thr), ptr(prob), ptr(fg), stream_ptr()),
          "mask")
    return prob.cpu().numpy(), fg.cpu().numpy()


@pytest.mark.parametrize("s", SIZES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_prepare_bit_exact(H, W, s):
    from cartoonsegmentation_amd import synth
    img = synth.image_u8(H, W, H + W)
    for bgr in (0, 1):
        x = _prepare(img, s, bgr).cpu().numpy()
        assert np.array_equal(x, host.restated_prepare(img, s, bgr)), bgr


@pytest.mark.parametrize("s", SIZES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_prob_and_fg_bit_exact(H, W, s):
    logits = np.random.default_rng(H * W + s).normal(0, 3, (s, s)).astype(np.float32)
    prob, fg = _mask(dev(logits), s, H, W)
    want = host.restated_prob(_orc_sigmoid(logits), H, W)
    assert np.array_equal(prob, want)
    assert np.array_equal(fg, (want > 0.5).astype(np.uint8))
    assert 0.2 < fg.mean() < 0.8


def _select(masks, fg):
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, ptr, stream_ptr
    L = _lib.load()
    k, Hm, Wm = masks.shape
    m = dev(masks.astype(np.uint8))
    f = dev(fg.astype(np.uint8))
    counts = torch.empty(2 * k, dtype=torch.int32, device='cuda')
    check(L.csm_animeseg_select(ptr(m), i32(k), i32(Hm), i32(Wm), ptr(f), i32(fg.shape[1]), ptr(counts), stream_ptr()), "select")
    return m.cpu().numpy().astype(bool)


@pytest.mark.parametrize("H0,W0,dh,dw", [(64, 48, 0, 0), (333, 517, 2, 1), (1024, 1024, 1, 2), (1080, 1920, 0, 0)])
def test_select_exact(H0, W0, dh, dw):
    """masks up to 2 px smaller than the frame (top-left slice), ratio exactly 0.3 (kept), just above it, empty, full, random"""
    g = np.random.default_rng(H0 + W0)
    Hm, Wm = H0 - dh, W0 - dw
    yy, xx = np.mgrid[0:H0, 0:W0]
    fg = ((yy - H0 * 0.5) / (H0 * 0.4)) ** 2 + ((xx - W0 * 0.5) / (W0 * 0.3)) ** 2 < 1
    F, B = np.argwhere(fg[:Hm, :Wm]), np.argwhere(~fg[:Hm, :Wm])
    masks = np.zeros((8, Hm, Wm), bool)
    for k, (nf, nb) in enumerate([(3, 7), (30, 70), (31, 69), (300, 700), (299, 701), (0, 50)]):
        for i in np.concatenate([F[g.choice(len(F), nf, replace=False)], B[g.choice(len(B), nb, replace=False)]]):
            masks[k, i[0], i[1]] = True
    masks[6] = True                                                  # masks[7] stays empty
    masks[5] |= g.random((Hm, Wm)) < 0.5
    want = host.restated_select(masks, fg)
    assert np.array_equal(_select(masks, fg), want)
    kept = [np.array_equal(a, b) for a, b in zip(want, masks)]
    assert kept[0] and kept[1] and not kept[2] and kept[3] and not kept[6] and kept[7]


def test_isnet_is_program_vs_oracle_and_fixture():
    from cartoonsegmentation_amd.nets import build_isnet
    from cartoonsegmentation_amd.runtime import CompiledProgram
    from cartoonsegmentation_amd.weights import SynthWeights
    from cartoonsegmentation_amd import synth
    from oracle import nets as onets
    ws = SynthWeights('animeseg.')
    s = 720
    xs = torch.cat([_prepare(synth.image_u8(1024, 828, 3), s, 1), _prepare(synth.image_u8(720, 1280, 4), s, 1)]).cpu().numpy()
    outs = {}
    for n in (1, 2):
        prog = build_isnet(ws, n, s, s, in_ch=3)
        y = torch.full((n, 1, s, s), float('nan'), device='cuda')
        CompiledProgram(prog, torch.device('cuda')).run(dev(xs[:n]), y)
        outs[n] = y.cpu().numpy()
        yo = np.zeros((n, 1, s, s), np.float32)
        onets.run_program(prog, [np.ascontiguousarray(xs[:n]), yo])
        assert np.array_equal(outs[n], yo), n
    assert np.array_equal(outs[2][:1], outs[1])
    y1b = torch.empty((1, 1, s, s), device='cuda')
    CompiledProgram(build_isnet(ws, 1, s, s, in_ch=3), torch.device('cuda')).run(dev(xs[1:2]), y1b)
    assert np.array_equal(outs[2][1:], y1b.cpu().numpy())
    for name in host.FIXTURES:                                       # against the reference module's own logits
        d = np.load(os.path.join(HERE, "golden", name + ".npz"))
        y = torch.empty((1, 1, 64, 64), device='cuda')
        CompiledProgram(build_isnet(ws, 1, 64, 64, in_ch=3), torch.device('cuda')).run(dev(d['x']), y)
        assert np.abs(y.cpu().numpy() - d['logits_raw']).max() <= 2e-4 * float(np.abs(d['logits_raw']).max())


@pytest.mark.parametrize("name", host.FIXTURES)
def test_glue_kernels_vs_reference_fixture(name):
    """the fixture's letterbox bit-exact; prob within the sigmoid's ulps of the reference's torch.sigmoid; the select exact"""
    d = np.load(os.path.join(HERE, "golden", name + ".npz"))
    img, s = d['img'], int(d['s'])
    H, W = img.shape[:2]
    assert np.array_equal(_prepare(img, s, 1).cpu().numpy(), d['x'])
    logits = ((d['logits_raw'] - np.float32(d['centre'])) / np.float32(d['scale'])).astype(np.float32)
    prob, fg = _mask(dev(logits[0, 0]), s, H, W)
    assert np.abs(prob - d['prob']).max() <= 1e-6
    assert np.array_equal(fg.astype(bool), d['prob'] > 0.5)          # (no fixture pixel lies within 1e-6 of 0.5)
    assert np.array_equal(_select(d['masks_in'], fg.astype(bool)), d['masks_out'])


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _shifted_ckpt(tmp_path, img, s):
    """the closed-form ISNet-IS weights put d1 far below 0 (fg empty: every instance kept).  A checkpoint whose side1 bias is moved
    by the median logit of this frame makes the foreground cover about half of it, so the select really refines."""
    from cartoonsegmentation_amd.nets import build_isnet
    from cartoonsegmentation_amd.runtime import CompiledProgram
    from cartoonsegmentation_amd.segmentation import animeseg_size
    rec = host._isnet_names()
    H, W = img.shape[:2]
    h, w = animeseg_size(H, W, s)
    from cartoonsegmentation_amd.weights import SynthWeights
    y = torch.empty((1, 1, s, s), device='cuda')
    CompiledProgram(build_isnet(SynthWeights('animeseg.'), 1, s, s, in_ch=3), torch.device('cuda')).run(_prepare(img, s, 1), y)
    crop = y.cpu().numpy()[0, 0, (s - h) // 2:(s - h) // 2 + h, (s - w) // 2:(s - w) // 2 + w]
    sd = {k: torch.from_numpy(v.copy()) for k, v in rec.items()}
    sd['side1.bias'] -= float(np.median(crop))
    p = str(tmp_path / ('isnetis_%dx%d_%d.ckpt' % (H, W, s)))
    torch.save({'net.' + k: v for k, v in sd.items()}, p)
    return p, sd


def _cpu_chain(img, det_S, s, sd, max_instances):
    from cartoonsegmentation_amd.nets import build_isnet, build_rtmdet
    from cartoonsegmentation_amd.weights import StateDictWeights, SynthWeights
    from oracle import nets as onets
    from oracle import segment as oseg
    rp, cfg = build_rtmdet(SynthWeights('rtmdet.'), 1, det_S, det_S)
    cfg.max_per_img = max_instances
    d = oseg.detect(img, rp, cfg, det_S, pred_score_thr=0.3)
    assert d['n'] > 0
    H, W = img.shape[:2]
    x = host.restated_prepare(img, s, True)
    y = np.zeros((1, 1, s, s), np.float32)
    onets.run_program(build_isnet(StateDictWeights(sd), 1, s, s, in_ch=3), [x, y])
    fg = host.restated_prob(_orc_sigmoid(y[0, 0]), H, W) > 0.5
    return d, fg, host.restated_select(d['masks'].astype(bool), fg)


@pytest.mark.parametrize("H,W,det_S,s", [(96, 128, 64, 64), (128, 96, 64, 80), (67, 101, 64, 64), (64, 130, 64, 48),
                                         (1024, 1024, 320, 720)])
def test_infer_matches_cpu_chain(tmp_path, H, W, det_S, s):
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    img = synth.image_u8(H, W, 5)
    ckpt, sd = _shifted_ckpt(tmp_path, img, s)
    net = AnimeInsSeg('synthetic', default_det_size=det_S,
                      refine_kwargs={'refine_method': 'animeseg', 'refine_size': s, 'refinenet_ckpt': ckpt})
    inst = net.infer(img, pred_score_thr=0.3, max_instances=3, output_type='numpy')
    d, fg, want = _cpu_chain(img, det_S, s, sd, 3)
    assert 0.2 < fg.mean() < 0.8
    assert d['n'] == len(inst) and np.array_equal(d['scores'], inst.scores) and np.array_equal(d['bboxes'], inst.bboxes)
    assert inst.masks.dtype == np.bool_ and np.array_equal(inst.masks, want)
    if (H, W) == (64, 130):
        assert inst.masks.shape[1:] == (64, 128)                    # detector masks 2 px narrower than the frame: fg[:, :128]
    t = net.infer(img, pred_score_thr=0.3, max_instances=3)          # tensor output: a bool tensor on the device
    assert t.is_cuda and t.masks.dtype == torch.bool and np.array_equal(t.masks.cpu().numpy(), want)


def test_batched_frames_equal_single_frames(tmp_path):
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    imgs = [synth.image_u8(96, 128, 20 + i) for i in range(5)] + [np.full((96, 128, 3), 128, np.uint8)]
    ckpt, _ = _shifted_ckpt(tmp_path, imgs[0], 64)
    net = AnimeInsSeg('synthetic', default_det_size=64,
                      refine_kwargs={'refine_method': 'animeseg', 'refine_size': 64, 'refinenet_ckpt': ckpt})
    net.refine_batch = 2                                              # chunks of 2 frames per ISNet-IS run
    for out_type in ('tensor', 'numpy'):
        many = net.infer(imgs, pred_score_thr=0.3, max_instances=3, output_type=out_type)
        for img, m in zip(imgs, many):
            one = net.infer(img, pred_score_thr=0.3, max_instances=3, output_type=out_type)
            assert len(one) == len(m)
            if len(one):
                a, b = (one.masks, m.masks) if out_type == 'numpy' else (one.masks.cpu().numpy(), m.masks.cpu().numpy())
                assert np.array_equal(a, b) and np.array_equal(np.asarray(one.scores if out_type == 'numpy' else one.scores.cpu()),
                                                                np.asarray(m.scores if out_type == 'numpy' else m.scores.cpu()))
    assert any(not i.is_empty for i in many)


def test_get_mask_and_forward(monkeypatch):
    monkeypatch.setenv("CSM_SYNTHETIC_WEIGHTS", "1")
    from animeinsseg.models.animeseg_refine import AnimeSegmentation, get_mask, load_refinenet
    from cartoonsegmentation_amd import synth
    from cartoonsegmentation_amd.nets import build_isnet
    from cartoonsegmentation_amd.weights import SynthWeights
    from oracle import nets as onets
    model = load_refinenet('animeseg')
    assert isinstance(model, AnimeSegmentation)
    for (H, W), s in (((64, 48), 64), ((150, 97), 128)):
        rgb = synth.image_u8(H, W, 8)
        p = get_mask(model, rgb, use_amp=True, s=s)
        assert p.dtype == np.float32 and p.shape == (H, W, 1)
        x = _prepare(rgb, s, 0)
        y = model.logits(x)
        prob, _ = _mask(y, s, H, W)
        assert np.array_equal(p[..., 0], prob)                       # get_mask == the prob kernel on the net's logits
        yo = np.zeros((1, 1, s, s), np.float32)
        onets.run_program(build_isnet(SynthWeights('animeseg.'), 1, s, s, in_ch=3), [host.restated_prepare(rgb, s, False), yo])
        assert np.array_equal(p[..., 0], host.restated_prob(_orc_sigmoid(yo[0, 0]), H, W))
        f = model(x)                                                 # AnimeSegmentation.forward: sigmoid(d1) [n,1,s,s]
        assert f.shape == (1, 1, s, s) and np.array_equal(f.cpu().numpy(), _orc_sigmoid(yo))


def test_kenburns_pipeline_uses_the_animeseg_refine(tmp_path):
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    H, W = 320, 384                                                   # the depth statistics crop 128 px off every side
    img = synth.image_u8(H, W, 12)
    ckpt, _ = _shifted_ckpt(tmp_path, img, 64)
    kw = {'refine_method': 'animeseg', 'refine_size': 64, 'refinenet_ckpt': ckpt}
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False,
                         depth_field=False, focal=W / 2.0, num_frame=3, mask_refine_kwargs=kw)
    pipe = KenBurnsPipeline(cfg)
    pipe.animeinsseg.set_detect_size(96)
    pipe.max_instances = 3
    kc = pipe.generate_kenburns_config(img)
    net = AnimeInsSeg('synthetic', default_det_size=96, refine_kwargs=kw)
    want = net.infer(img, pred_score_thr=cfg.pred_score_thr, max_instances=3)
    none = net.infer(img, pred_score_thr=cfg.pred_score_thr, max_instances=3, refine_kwargs={'refine_method': 'none'})
    got = kc.instances
    assert len(got) == len(want) > 0
    assert np.array_equal(got.masks.cpu().numpy(), want.masks.cpu().numpy())
    assert np.array_equal(got.bboxes.cpu().numpy(), want.bboxes.cpu().numpy())
    assert not np.array_equal(want.masks.cpu().numpy(), none.masks.cpu().numpy())   # the refine changed something
