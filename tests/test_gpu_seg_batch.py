"""GPU: the batched segmentation glue of a step (csrc/maskhead.hip: csm_nms_batch, csm_det_masks_batch, csm_refine_prepare_many, one
csm_refine_threshold launch per ISNet chunk) against the per-item calls it replaces, and the whole batched path against
CSM_SEG_GLUE_BATCH=0.  Every comparison is exact (torch.equal): the batched entry points run the per-item kernels with the frame
or the item as a grid dimension."""
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT = -7


def _L():
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def _args():
    from cartoonsegmentation_amd._lib import check, f32, i32, i64, ptr, stream_ptr
    return check, f32, i32, i64, ptr, stream_ptr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
NMS_NB, NMS_K, NMS_KEEP, NMS_THR = 3, 96, 5, 0.6


def _nms_boxes():
    """image 0: three clusters of 32 heavily overlapping boxes (80 px wide, centres jittered by up to 2 px: IoU > 0.8) -> 3 kept, fewer than
    max_keep; image 1: 96 disjoint boxes -> exactly max_keep kept; image 2: zero-area boxes (no box suppresses another: 0 > thr * 0
    is false) -> max_keep kept.  Labels: image 0 by cluster (two clusters share a label, so the kept count stays 3), others j % 3."""
    rng = np.random.default_rng(11)
    boxes = np.zeros((NMS_NB, NMS_K, 4), np.float32)
    centres = np.array([(100, 100), (300, 120), (200, 400)], np.float32)
    cl = rng.integers(0, 3, NMS_K)
    cl[:3] = (0, 1, 2)
    c = centres[cl] + rng.uniform(-2, 2, (NMS_K, 2)).astype(np.float32)
    boxes[0] = np.concatenate([c - 40, c + 40], 1)
    j = np.arange(NMS_K)
    x0, y0 = (j % 12) * 50.0, (j // 12) * 50.0
    boxes[1] = np.stack([x0, y0, x0 + 40, y0 + 40], 1)
    p = rng.uniform(0, 500, (NMS_K, 2)).astype(np.float32)
    p[1] = p[0]                                                       # two coincident points as well
    boxes[2] = np.concatenate([p, p], 1)
    labels = np.stack([np.where(cl == 2, 1, 0), j % 3, j % 3]).astype(np.float32)
    return boxes, labels * np.float32(boxes.max() + 1)


@pytest.mark.parametrize("with_classes", [False, True])
def test_nms_batch_equals_nms_per_image(with_classes):
    check, f32, i32, i64, ptr, stream_ptr = _args()
    L = _L()
    boxes, offs = _nms_boxes()
    boxes_d, offs_d = _dev(boxes), (_dev(offs) if with_classes else None)
    keep = torch.full((NMS_NB, NMS_KEEP), SENT, dtype=torch.int32, device='cuda')
    nk = torch.full((NMS_NB,), SENT, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.csm_nms_batch_scratch_bytes(i32(NMS_NB), i32(NMS_K)), dtype=torch.uint8, device='cuda')
    check(L.csm_nms_batch(ptr(boxes_d), ptr(offs_d), i32(NMS_NB), i32(NMS_K), f32(NMS_THR), i32(NMS_KEEP), ptr(keep), ptr(nk),
                          ptr(scratch), stream_ptr()), "nms_batch")
    keep1 = torch.full((NMS_NB, NMS_KEEP), SENT, dtype=torch.int32, device='cuda')
    nk1 = torch.full((NMS_NB,), SENT, dtype=torch.int32, device='cuda')
    scr1 = torch.empty(L.csm_nms_scratch_bytes(i32(NMS_K)), dtype=torch.uint8, device='cuda')
    for b in range(NMS_NB):
        check(L.csm_nms(ptr(boxes_d[b]), ptr(None if offs_d is None else offs_d[b]), i32(NMS_K), f32(NMS_THR), i32(NMS_KEEP),
                        ptr(keep1[b]), ptr(nk1[b:b + 1]), ptr(scr1), stream_ptr()), "nms")
    assert torch.equal(nk, nk1) and torch.equal(keep, keep1)
    assert nk.tolist() == [3, NMS_KEEP, NMS_KEEP]                      # the cases are what they are meant to be
    assert (keep[0, 3:] == SENT).all()


# ---- detector masks ----------------------------------------------------------------------------------------------------------------
DM_H = DM_W = 12
DM_STRIDE, DM_LD, DM_NB, DM_M, DM_NK, DM_G = 8, 8, 3, 4, (2, 0, 3), 169


@pytest.mark.parametrize("shape", [(150, 150, 150, 150), (131, 133, 129, 130), (100, 104, 100, 104)], ids=lambda s: "x".join(map(str, s)))
def test_det_masks_batch_equals_the_per_frame_calls(shape):
    """8 prototypes on 12 x 12 at stride 8, three frames with n_k = (2, 0, 3) of 4 slots each.  Shapes (rh2, rw2, oh, ow): no crop
    (byte stores: ow % 4 != 0), oh < rh2 and ow < rw2 (the crop), and ow % 4 == 0 (32-bit stores).  The masks block, the boxes block
    (truncation toward zero, also of negative coordinates) and the sentinel tail behind both equal the per-frame results."""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    L = _L()
    rh2, rw2, oh, ow = shape
    rng = np.random.default_rng(5)
    h, w, nb, M = DM_H, DM_W, DM_NB, DM_M
    feat = _dev(rng.standard_normal((nb, h, w, DM_LD)).astype(np.float32))
    kernels = _dev((rng.standard_normal((nb, M, DM_G)) * 0.5).astype(np.float32))
    pri = np.zeros((nb, M, 4), np.float32)
    pri[..., :2] = rng.integers(0, 12, (nb, M, 2)) * DM_STRIDE
    pri[..., 2:] = DM_STRIDE
    priors = _dev(pri)
    bx = rng.uniform(-20, 160, (nb, M, 4)).astype(np.float32)
    bx[0, 0] = (-3.7, -0.2, 17.9, 150.5)
    boxes = _dev(bx)
    total = sum(DM_NK)
    logits = torch.empty((total, h, w), dtype=torch.float32, device='cuda')
    masks = torch.full((total + 1, oh, ow), 0xA5, dtype=torch.uint8, device='cuda')
    bout = torch.full((total + 1, 4), SENT, dtype=torch.int32, device='cuda')
    check(L.csm_det_masks_batch(ptr(feat), i64(h * w * DM_LD), i32(DM_LD), i32(h), i32(w), i32(8), i32(8), ptr(kernels), ptr(priors),
                                ptr(boxes), i32(nb), i32(M), (ctypes.c_int * nb)(*DM_NK), i32(DM_STRIDE), i32(DM_STRIDE), i32(rh2), i32(rw2),
                                i32(oh), i32(ow), f32(0.5), ptr(logits), ptr(masks), ptr(bout), stream_ptr()), "det_masks_batch")
    ref_m = torch.full((total + 1, oh, ow), 0xA5, dtype=torch.uint8, device='cuda')
    ref_b = torch.full((total + 1, 4), SENT, dtype=torch.int32, device='cuda')
    s = 0
    for k, n in enumerate(DM_NK):
        if not n:
            continue
        lg = torch.empty((n, h, w), dtype=torch.float32, device='cuda')
        check(L.csm_maskhead_logits(ptr(feat[k]), i32(DM_LD), i32(h), i32(w), i32(8), i32(8), ptr(kernels[k, :n].contiguous()),
                                    ptr(priors[k, :n].contiguous()), i32(n), i32(DM_STRIDE), ptr(lg), stream_ptr()), "maskhead")
        check(L.csm_mask_resize_threshold(ptr(lg), i32(n), i32(h), i32(w), i32(DM_STRIDE), i32(rh2), i32(rw2), i32(oh), i32(ow), f32(0.5),
                                          ptr(ref_m[s:s + n]), stream_ptr()), "mask_resize")
        assert torch.equal(logits[s:s + n], lg)
        b = boxes[k, :n].to(torch.int32)                               # AnimeInsSeg._instances_from
        b[:, 2:] -= b[:, :2]
        ref_b[s:s + n] = b
        s += n
    assert torch.equal(masks, ref_m) and torch.equal(bout, ref_b)
    assert bout[0].tolist() == [-3, 0, 20, 150]
    assert 0 < int(ref_m[:total].sum()) < total * oh * ow              # both values occur


def test_det_masks_batch_without_detections_launches_nothing():
    check, f32, i32, i64, ptr, stream_ptr = _args()
    masks = torch.full((4,), 0xA5, dtype=torch.uint8, device='cuda')
    check(_L().csm_det_masks_batch(ptr(None), i64(0), i32(8), i32(12), i32(12), i32(8), i32(8), ptr(None), ptr(None), ptr(None), i32(2),
                                   i32(4), (ctypes.c_int * 2)(0, 0), i32(8), i32(8), i32(2), i32(2), i32(2), i32(2), f32(0.5), ptr(None),
                                   ptr(masks), ptr(None), stream_ptr()), "det_masks_batch")
    assert (masks.cpu().numpy() == 0xA5).all()


# ---- ISNet refine glue -------------------------------------------------------------------------------------------------------------
RF_H, RF_W, RF_HM, RF_WM, RF_T, RF_COUNTS = 37, 53, 36, 52, 24, (2, 0, 3)


def test_refine_prepare_many_equals_prepare_batch_per_item():
    """three 37 x 53 images, masks of 36 x 52 (one pixel smaller, as detector masks can be), T = 24, five items spread (2, 0, 3)"""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    from cartoonsegmentation_amd.segmentation import scaledown_size
    L = _L()
    rng = np.random.default_rng(3)
    H, W, Hm, Wm, T = RF_H, RF_W, RF_HM, RF_WM, RF_T
    rh, rw = scaledown_size(H, W, T)
    rhm, rwm = scaledown_size(Hm, Wm, T)
    assert (rh, rw) == (17, 24) and rhm <= T and rwm <= T
    imgs = [_dev(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in RF_COUNTS]
    masks = [_dev((rng.uniform(size=(max(n, 1), Hm, Wm)) > 0.5).astype(np.uint8)) for n in RF_COUNTS]
    items = [(j, k) for j, n in enumerate(RF_COUNTS) for k in range(n)]
    n = len(items)
    batch = torch.full((n + 1, 4, T, T), float('nan'), device='cuda')
    VP = ctypes.c_void_p * n
    check(L.csm_refine_prepare_many(VP(*[imgs[j].data_ptr() for j, _ in items]), VP(*[masks[j][k].data_ptr() for j, k in items]),
                                    i32(n), i32(H), i32(W), i32(rh), i32(rw), i32(Hm), i32(Wm), i32(rhm), i32(rwm), i32(T), ptr(batch),
                                    stream_ptr()), "refine_prepare_many")
    ref = torch.full((n + 1, 4, T, T), float('nan'), device='cuda')
    for i, (j, k) in enumerate(items):
        check(L.csm_refine_prepare_batch(ptr(imgs[j]), ptr(masks[j][k:k + 1]), i32(1), i32(H), i32(W), i32(rh), i32(rw), i32(Hm), i32(Wm),
                                         i32(rhm), i32(rwm), i32(T), ptr(ref[i:i + 1]), stream_ptr()), "refine_prepare")
    assert torch.equal(batch[:n], ref[:n]) and not torch.isnan(batch[:n]).any()
    assert torch.isnan(batch[n]).all()
    assert float(batch[:n, 3].max()) > 0 and float(batch[:n, :3].max()) > 0


def test_one_refine_threshold_launch_equals_one_launch_per_item():
    """n = 5 into one block vs five n = 1 launches: T = 24, crop (17, 24), output 37 x 53; logits that are exactly 0 and exactly
    logit(thr) among them"""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    L = _L()
    T, ch, cw, H, W, n, thr = RF_T, 17, 24, RF_H, RF_W, 5, 0.3
    rng = np.random.default_rng(9)
    lg = rng.standard_normal((n, 1, T, T)).astype(np.float32) * 2
    flat = lg.reshape(-1)
    flat[rng.integers(0, flat.size, 200)] = 0.0
    flat[rng.integers(0, flat.size, 200)] = np.float32(math.log(thr / (1 - thr)))
    lg[0, 0, :4, :4] = np.float32(math.log(thr / (1 - thr)))          # a flat patch at the threshold itself
    logits = _dev(lg)
    block = torch.full((n + 1, H, W), 0xA5, dtype=torch.uint8, device='cuda')
    check(L.csm_refine_threshold(ptr(logits), i32(n), i32(T), i32(T), i32(ch), i32(cw), i32(H), i32(W), f32(thr), ptr(block), stream_ptr()),
          "refine_threshold")
    ref = torch.full((n + 1, H, W), 0xA5, dtype=torch.uint8, device='cuda')
    for i in range(n):
        check(L.csm_refine_threshold(ptr(logits[i:i + 1]), i32(1), i32(T), i32(T), i32(ch), i32(cw), i32(H), i32(W), f32(thr),
                                     ptr(ref[i:i + 1]), stream_ptr()), "refine_threshold")
    assert torch.equal(block, ref)
    got = block[:n].cpu().numpy()
    assert ((got == 0) | (got == 1)).all() and 0 < got.sum() < got.size


# ---- the whole batched path ----------------------------------------------------------------------------------------------------------
def test_env_switch_selects_the_per_item_calls(monkeypatch):
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from cartoonsegmentation_amd.segmentation import AnimeInsSeg
    monkeypatch.setenv("CSM_SEG_GLUE_BATCH", "0")
    assert AnimeInsSeg('synthetic', refine_kwargs={'refine_method': 'none'}).seg_glue_batch is False
    monkeypatch.delenv("CSM_SEG_GLUE_BATCH")
    assert AnimeInsSeg('synthetic', refine_kwargs={'refine_method': 'none'}).seg_glue_batch is True


def test_batched_glue_equals_the_per_item_path():
    """generate_kenburns_configs of the pipeline of test_batched_configs_match_single_frame_path (three 320 x 320 synthetic frames, det
    96, refine 64, LeReS 96, two instances at most) with the batched glue and with the per-item calls (what CSM_SEG_GLUE_BATCH=0
    sets): instance counts, masks, boxes (dtype too), scores, depth, points and depth range are equal.  (The synthetic detector scores
    every prior about 0.49, so no seed gives a frame without an instance; the empty frame of a run is covered by n_k = (2, 0, 3) in the
    tests above.)"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    imgs = [synth.image_u8(320, 320, 31 + k) for k in range(3)]
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False, focal=160.0,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    pipe.max_instances, pipe.overlap_depth = 2, False
    pipe.animeinsseg.set_detect_size(96)
    assert pipe.animeinsseg.seg_glue_batch is True
    new = pipe.generate_kenburns_configs(imgs)
    pipe.animeinsseg.seg_glue_batch = False
    old = pipe.generate_kenburns_configs(imgs)
    assert sum(len(k.instances) for k in new) > 0
    for ko, kn in zip(old, new):
        io, inn = ko.instances, kn.instances
        assert len(io) == len(inn)
        if len(io):
            assert inn.masks.dtype == io.masks.dtype == torch.bool and torch.equal(io.masks, inn.masks)
            assert inn.bboxes.dtype == io.bboxes.dtype == torch.int32 and torch.equal(io.bboxes, inn.bboxes)
            assert inn.scores.dtype == io.scores.dtype and torch.equal(io.scores, inn.scores)
            assert set(np.unique(inn.masks.view(torch.uint8).cpu().numpy()).tolist()) <= {0, 1}
        assert torch.equal(ko['tenRawDepth'], kn['tenRawDepth']) and torch.equal(ko['tenRawPoints'], kn['tenRawPoints'])
        assert ko['objDepthrange'] == kn['objDepthrange']
