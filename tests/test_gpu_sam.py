"""GPU: Segment Anything on libcsm355 (nets/sam.py, csrc/sam.hip, cartoonsegmentation_amd/sam.py) against the float64 restatement
(tests/sam_restatement.py, itself pinned against transformers' SamModel by tests/test_sam.py) on the same seeded weights.

Tolerances: 1e-4 relative in max-norm for whole programs (the project's tolerance for reduced-size transformer programs,
tests/test_gpu_dpt_beit.py); 1e-5 for one attention op against float64 (the reductions' tolerance of include/csm355.h)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sam_cases as C  # noqa: E402
import sam_e2e_cases as E  # noqa: E402
import sam_restatement as R  # noqa: E402
from cartoonsegmentation_amd import program as P  # noqa: E402
from cartoonsegmentation_amd.nets import sam as S  # noqa: E402
from cartoonsegmentation_amd.weights import StateDictWeights, SynthWeights  # noqa: E402


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _run(prog, ins, out_shapes):
    from cartoonsegmentation_amd.runtime import CompiledProgram
    outs = [torch.full(s, float('nan'), dtype=torch.float32, device='cuda') for s in out_shapes]
    CompiledProgram(prog, 'cuda').run(*[torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in ins], *outs)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


# ---- (a) the image encoder ---------------------------------------------------------------------------------------------------------------------
ENC = dict(out_chans=32, dec_mlp=64, iou_hidden=32, patch=16)
ENCODER_CASES = [
    ('A', C.CFG_A, 1),
    ('B', C.CFG_B, 1),
    ('one-window', dict(ENC, embed=64, depth=2, heads=2, global_blocks=(1,), window=7, image=112, mlp_dim=128), 1),       # d = 32, no padding
    ('23x23-d80', dict(ENC, embed=160, depth=2, heads=2, global_blocks=(1,), window=14, image=368, mlp_dim=320), 2),      # 196 / 529 tokens, ViT-H's d
    ('64x64', dict(ENC, embed=128, depth=2, heads=2, global_blocks=(1,), window=14, image=1024, mlp_dim=256), 1),         # the real token counts
]


@pytest.mark.parametrize("name,kw,n", ENCODER_CASES, ids=[c[0] for c in ENCODER_CASES])
def test_encoder_hip_vs_float64(name, kw, n):
    cfg = S.SamConfig(**kw)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), 20 + len(name))
    x = np.random.default_rng(30 + n).standard_normal((n, 3, cfg.image, cfg.image)).astype(np.float32)
    ref = R.Model(sd, cfg).encoder(torch.as_tensor(x.astype(np.float64))).numpy()
    got, = _run(S.build_sam_encoder(StateDictWeights(sd), cfg, n), [x], [(n, cfg.out_chans, cfg.grid, cfg.grid)])
    err = _rel(got, ref)
    print(name, 'encoder rel err', err)
    assert err < 1e-4


# ---- (b) the attention op by itself ------------------------------------------------------------------------------------------------------------
def _attention_ref(qkv, heads, d, gh, gw, rh, rw):
    """float64: q is the pre-scaled one the op receives; the bias multiplies the unscaled q = q_s sqrt(d)"""
    n, N = qkv.shape[0], gh * gw
    t = torch.as_tensor(qkv.astype(np.float64)).reshape(n, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    a = q @ k.transpose(-2, -1)
    qu = (q * np.sqrt(float(d))).reshape(n, heads, gh, gw, d)
    iy = torch.arange(gh)[:, None] - torch.arange(gh)[None, :] + gh - 1
    ix = torch.arange(gw)[:, None] - torch.arange(gw)[None, :] + gw - 1
    bh = torch.einsum('bnhwc,hkc->bnhwk', qu, torch.as_tensor(rh.astype(np.float64))[iy])
    bw = torch.einsum('bnhwc,wkc->bnhwk', qu, torch.as_tensor(rw.astype(np.float64))[ix])
    a = (a.reshape(n, heads, gh, gw, gh, gw) + bh[..., :, None] + bw[..., None, :]).reshape(n, heads, N, N)
    return (torch.softmax(a, -1) @ v).transpose(1, 2).reshape(n, N, heads * d).numpy()


def _attention_prog(n, gh, gw, heads, d, rh, rw):
    p = P.Program("attention_relpos")
    x = p.ext_nchw(n, 3 * heads * d, gh, gw)
    y = p.ext_nchw(n, heads * d, gh, gw)
    p.to_nchw(p.attention_relpos(p.to_nhwc(x), heads, (gh, gw), rh, rw), y)
    p.plan()
    return p


@pytest.mark.parametrize("g", [3, 14, 23])
@pytest.mark.parametrize("d", [32, 64, 80])
def test_attention_relpos_vs_float64(g, d):
    n, heads, N = 2, 2, g * g
    rng = np.random.default_rng(100 * g + d)
    qkv = rng.standard_normal((n, N, 3 * heads * d)).astype(np.float32)
    qkv[..., :heads * d] *= np.float32(d) ** np.float32(-0.5)
    rh, rw = (rng.standard_normal((2 * g - 1, d)) / np.sqrt(d)).astype(np.float32), (rng.standard_normal((2 * g - 1, d)) / np.sqrt(d)).astype(np.float32)
    ref = _attention_ref(qkv, heads, d, g, g, rh, rw)
    x = qkv.reshape(n, g, g, -1).transpose(0, 3, 1, 2)
    got, = _run(_attention_prog(n, g, g, heads, d, rh, rw), [x], [(n, heads * d, g, g)])
    err = _rel(got.transpose(0, 2, 3, 1).reshape(n, N, -1), ref)
    print('N', N, 'd', d, 'rel err', err)
    assert err < 1e-5


@pytest.mark.parametrize("g,d", [(3, 32), (14, 64), (23, 32)])
def test_attention_relpos_with_zero_tables_equals_plain_attention(g, d):
    n, heads, N = 2, 2, g * g
    qkv = np.random.default_rng(7 * g + d).standard_normal((n, N, 3 * heads * d)).astype(np.float32)
    qkv[..., :heads * d] *= np.float32(d) ** np.float32(-0.5)
    zero = np.zeros((2 * g - 1, d), np.float32)
    got, = _run(_attention_prog(n, g, g, heads, d, zero, zero), [qkv.reshape(n, g, g, -1).transpose(0, 3, 1, 2)], [(n, heads * d, g, g)])
    p = P.Program("attention")
    x = p.ext_nchw(n, 3 * heads * d, N, 1)
    y = p.ext_nchw(n, heads * d, N, 1)
    p.to_nchw(p.attention(p.to_nhwc(x), heads), y)
    p.plan()
    plain, = _run(p, [qkv.transpose(0, 2, 1)[..., None]], [(n, heads * d, N, 1)])
    assert _rel(got.reshape(n, heads * d, N), plain.reshape(n, heads * d, N)) < 1e-6


# ---- (c) cross-attention -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nk", [(7, 49), (49, 7), (7, 4096)])
@pytest.mark.parametrize("d", [16, 32])
def test_cross_attention_vs_float64(nq, nk, d):
    n, heads = 2, 4
    rng = np.random.default_rng(nq * 13 + nk + d)
    q = (rng.standard_normal((n, nq, heads * d)) * d ** -0.5).astype(np.float32)
    kv = rng.standard_normal((n, nk, 2 * heads * d)).astype(np.float32)
    sp = lambda t, m: torch.as_tensor(t.astype(np.float64)).reshape(n, m, heads, d).transpose(1, 2)      # noqa: E731
    a = torch.softmax(sp(q, nq) @ sp(kv[..., :heads * d], nk).transpose(-2, -1), -1)
    ref = (a @ sp(kv[..., heads * d:], nk)).transpose(1, 2).reshape(n, nq, heads * d).numpy()
    p = P.Program("cross_attention")
    qe, ke, oe = p.ext_nchw(n, heads * d, nq, 1), p.ext_nchw(n, 2 * heads * d, nk, 1), p.ext_nchw(n, heads * d, nq, 1)
    p.to_nchw(p.cross_attention(p.to_nhwc(qe), p.to_nhwc(ke), heads), oe)
    p.plan()
    got, = _run(p, [q.transpose(0, 2, 1)[..., None], kv.transpose(0, 2, 1)[..., None]], [(n, heads * d, nq, 1)])
    err = _rel(got[..., 0].transpose(0, 2, 1), ref)
    print(nq, nk, d, 'rel err', err)
    assert err < 1e-5


# ---- (d) the whole model: low-res logits and IoU predictions -----------------------------------------------------------------------------------
def _sam(kw, seed, **opts):
    from cartoonsegmentation_amd.sam import Sam
    cfg = S.SamConfig(**kw)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), seed)
    return Sam(StateDictWeights(sd), 'cuda', cfg=cfg, **opts), R.Model(sd, cfg), cfg


@pytest.mark.parametrize("kw,boxes,seed", [(C.CFG_A, C.BOXES_A, C.SEED_A), (C.CFG_B, C.BOXES_B, C.SEED_B)], ids=['A', 'B'])
def test_full_model_hip_vs_float64(kw, boxes, seed):
    sam, ref, cfg = _sam(kw, seed)
    x = np.random.default_rng(seed + 10).standard_normal((1, 3, cfg.image, cfg.image)).astype(np.float32)
    rl, ri = ref.forward(torch.as_tensor(x.astype(np.float64)), boxes)
    sam.set_prepared(torch.from_numpy(x).cuda())
    low, iou = sam.low_res(boxes, frame='model')
    el, ei = _rel(low.cpu().numpy(), rl.numpy()), _rel(iou.cpu().numpy(), ri.numpy())
    print('logits', el, 'iou', ei)
    assert el < 1e-4 and ei < 1e-4


def test_full_model_hip_vs_recorded_sam_model_outputs():
    """the fixture holds transformers SamModel's float64 outputs: this path needs neither transformers nor the restatement"""
    z = np.load(C.GOLDEN)
    sam, _, cfg = _sam(C.CFG_A, int(z['seed']))
    sam.set_prepared(torch.from_numpy(C.prepared(z['image_u8']).astype(np.float32)).cuda())
    low, iou = sam.low_res(z['boxes'], frame='model')
    assert _rel(low.cpu().numpy(), z['low_res_logits']) < 1e-4 and _rel(iou.cpu().numpy(), z['iou']) < 1e-4


# ---- (e) masks end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CASES, ids=[c['name'] for c in E.CASES])
def test_apply_sam_masks_end_to_end(case):
    from cartoonsegmentation_amd.sam import apply_sam
    logits, riou = E.reference(case)
    logits = logits.numpy()
    for k in range(logits.shape[0]):                                   # the premise, on the restatement alone
        assert (np.abs(logits[k]) <= 1e-4 * np.abs(logits[k]).max()).mean() <= 0.005
    sam, _, cfg = _sam(C.CFG_A, case['seed'])
    img = C.image_u8(case['h'], case['w'], case['img_seed'])
    masks = apply_sam(img, case['boxes'], sam=sam)
    assert masks.dtype == np.bool_ and masks.shape == logits.shape
    for k in range(logits.shape[0]):
        sure = np.abs(logits[k]) > 1e-4 * np.abs(logits[k]).max()
        assert np.array_equal(masks[k][sure], (logits[k] > 0)[sure]), (case['name'], k, int((masks[k] != (logits[k] > 0))[sure].sum()))
    # one call == chunks of one; device results; IoU predictions
    whole, iou = sam.predict_boxes(case['boxes'])
    assert whole.is_cuda and whole.dtype == torch.bool and np.array_equal(whole.cpu().numpy(), masks)
    assert _rel(iou.cpu().numpy(), riou.numpy()) < 1e-4
    one = type(sam)(sam.ws, 'cuda', cfg=cfg, scratch_bytes=1)
    assert one.chunk_size(3) == 1
    m1, i1 = one.set_image(torch.from_numpy(img).cuda()).predict_boxes(torch.tensor(case['boxes'], dtype=torch.int32, device='cuda'))
    assert torch.equal(m1, whole) and torch.equal(i1, iou) and list(one._decoders) == [1]
    # no boxes: empty results
    m0, i0 = sam.predict_boxes([])
    assert tuple(m0.shape) == (0, case['h'], case['w']) and m0.dtype == torch.bool and tuple(i0.shape) == (0,)
    assert apply_sam(img, [], sam=sam).shape == (0, case['h'], case['w'])


def test_decoder_program_cache_is_bounded():
    sam, _, cfg = _sam(C.CFG_A, 3, max_programs=2)
    sam.set_image(C.image_u8(80, 100, 5))
    first, _ = sam.predict_boxes([[5, 5, 60, 60]])
    sam.predict_boxes([[5, 5, 60, 60], [10, 20, 90, 70]])
    sam.predict_boxes([[5, 5, 60, 60], [10, 20, 90, 70], [1, 2, 30, 40]])
    assert list(sam._decoders) == [2, 3] and sam.evictions == 1
    again, _ = sam.predict_boxes([[5, 5, 60, 60]])
    assert torch.equal(first, again) and len(sam._decoders) == 2


# ---- (f) KenBurnsPipeline(detector='sam') --------------------------------------------------------------------------------------------------------
def test_kenburns_pipeline_with_detector_sam(monkeypatch):
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from cartoonsegmentation_amd import kenburns as K, synth
    from cartoonsegmentation_amd.sam import Sam
    tiny = S.SamConfig(**C.CFG_A)
    built = []
    monkeypatch.setattr(K, 'Sam', lambda path, device=None: built.append(path) or Sam(SynthWeights('sam.'), device, cfg=tiny))
    cfg = K.KenBurnsConfig(detector='sam', det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False,
                           depth_field=False, focal=160.0, num_frame=3, pred_score_thr=0.01, mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = K.KenBurnsPipeline(cfg)
    assert built == ['models/sam/sam_vit_h_4b8939.pth'] and pipe.detector == 'sam' and isinstance(pipe.sam, Sam)
    pipe.max_instances = 3
    pipe.animeinsseg.set_detect_size(96)
    img = synth.image_u8(288, 320, 21)                                  # (the pipeline's depth-range crop needs more than 256 x 256)
    det = pipe.animeinsseg.infer(img, cfg.pred_score_thr, None, output_type='tensor', max_instances=3)
    assert not det.is_empty
    inst, _ = pipe.run_instance_segmentation(img)
    assert torch.equal(inst.bboxes, det.bboxes) and torch.equal(inst.scores, det.scores)
    xyxy = det.bboxes.to(torch.int32).clone()
    xyxy[:, 2:] += xyxy[:, :2]
    want, _ = pipe.sam.set_image(img).predict_boxes(xyxy)
    assert inst.masks.is_cuda and inst.masks.dtype == torch.bool and torch.equal(inst.masks, want)
    kc = pipe.generate_kenburns_config(img)
    assert kc['intHeight'] == 288 and kc['intWidth'] == 320 and torch.isfinite(kc['tenRawDisparity']).all()
    pipe.cfg.pred_score_thr = 2.0                                       # nothing passes: an empty AnimeInstances, SAM is not run
    empty, _ = pipe.run_instance_segmentation(img)
    assert empty.is_empty and len(empty) == 0
