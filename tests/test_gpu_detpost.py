"""GPU: the detector post-processing kernels one by one (csrc/maskhead.hip: csm_nms, csm_mask_resize_threshold, csm_maskhead_logits,
csm_det_preprocess, csm_pack_mask_bits; csrc/detdecode.hip: csm_det_decode / csm_det_gather in a chain with csm_nms at the shipped size)
against the plain float64 references of tests/detpost_cases.py and against the oracle, at the edge shapes listed there.
tests/test_detpost_references.py proves the same cases (and the property each exists for) on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detpost_cases as C  # noqa: E402
from test_detpost_references import mask_compare, maskhead_oracle_errors  # noqa: E402

CSM_ERR_ARG = 1
SENT = -7


def _L():
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _args():
    from cartoonsegmentation_amd._lib import check, f32, i32, i64, ptr, stream_ptr
    return check, f32, i32, i64, ptr, stream_ptr


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
def _hip_nms(boxes_d, offs_d, n, thr, max_keep, scratch):
    """-> (n_keep, keep buffer [max_keep + 8] pre-filled with SENT)"""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    keep = torch.full((max_keep + 8,), SENT, dtype=torch.int32, device='cuda')
    nk = torch.full((1,), SENT, dtype=torch.int32, device='cuda')
    check(_L().csm_nms(ptr(boxes_d), ptr(offs_d), i32(n), f32(thr), i32(max_keep), ptr(keep), ptr(nk), ptr(scratch), stream_ptr()), "nms")
    return int(nk.item()), keep.cpu().numpy()


@pytest.mark.parametrize("with_classes", [False, True])
@pytest.mark.parametrize("n", C.NMS_SIZES)
def test_nms_equals_the_greedy_float64_loop(n, with_classes):
    """k_nms_mask + k_nms_scan on exact inputs (fp32 and float64 take the same decision on every pair): n_keep and keep[:n_keep] are
    the reference's for every max_keep, entries past n_keep keep their sentinel; the suppression bitmap equals the float64 pair matrix.  Lists with clusters over many words, the A/B/C chain in
    three words, IoU == thr on boxes 63 / 64, twins with different labels, the zero-box tail of the decode (test_detpost_references.py)."""
    from oracle import segment as oseg
    case = C.nms_case(n, with_classes)
    boxes_d = _dev(case['boxes']) if n else None
    offs_d = _dev(case['offsets']) if with_classes and n else None
    scratch = torch.empty(_L().csm_nms_scratch_bytes(ctypes.c_int(max(n, 1))), dtype=torch.uint8, device='cuda')
    for thr in C.NMS_THRS:
        for max_keep in C.nms_max_keeps(n):
            ref = C.nms_reference(case['boxes'], case['offsets'], thr, max_keep)
            nk, keep = _hip_nms(boxes_d, offs_d, n, thr, max_keep, scratch)
            assert nk == min(len(ref), max_keep) == len(ref), (n, with_classes, thr, max_keep, nk, len(ref))
            assert np.array_equal(keep[:nk], ref), (n, with_classes, thr, max_keep)
            assert (keep[nk:] == SENT).all()
            assert np.array_equal(keep[:nk], oseg.nms(case['boxes'], case['offsets'], thr, max_keep))
        # k_nms_mask's bitmap itself: row i, bit j of word j / 64 <=> j > i and box i would suppress box j; every pair, also those the
        # greedy scan never consults (a box's own bit and the bits past n stay clear)
        if n and (n <= 1000 or thr == C.NMS_THRS[0]):
            words = (n + 63) // 64
            bits = np.unpackbits(scratch[:n * words * 8].cpu().numpy().reshape(n, words * 8), axis=1, bitorder='little')
            assert not bits[:, n:].any()
            assert np.array_equal(bits[:, :n].astype(bool), C.nms_pair_matrix(case['boxes'], case['offsets'], thr))


def test_nms_rejects_bad_sizes_without_a_launch():
    _, f32, i32, _, ptr, stream_ptr = _args()
    L = _L()
    boxes = torch.zeros((8, 4), device='cuda')
    keep = torch.full((16,), SENT, dtype=torch.int32, device='cuda')
    nk = torch.full((1,), SENT, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.csm_nms_scratch_bytes(ctypes.c_int(8)), dtype=torch.uint8, device='cuda')
    # n = 4097 with an 8-box buffer: a launch would read out of bounds, the argument check must come first
    assert L.csm_nms(ptr(boxes), ptr(None), i32(4097), f32(0.5), i32(4), ptr(keep), ptr(nk), ptr(scratch), stream_ptr()) == CSM_ERR_ARG
    assert L.csm_nms(ptr(boxes), ptr(None), i32(8), f32(0.5), i32(0), ptr(keep), ptr(nk), ptr(scratch), stream_ptr()) == CSM_ERR_ARG
    torch.cuda.synchronize()
    assert int(nk.item()) == SENT and (keep.cpu().numpy() == SENT).all()


# ---- mask resize + threshold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MASK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_mask_resize_threshold_equals_oracle_and_float64_torch(case):
    """k_mask_resize_threshold: byte-identical to the oracle; equal to torch's own float64 interpolate -> interpolate -> crop ->
    sigmoid > thr on every pixel further than 1e-4 from thr (at most 0.5 % of a case's pixels are that close: a condition of the
    inputs, asserted on the CPU as well); nothing written past the n * oh * ow bytes."""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    from oracle import segment as oseg
    h, w, rh, rw, oh, ow, thr, n = case
    logits = C.mask_logits(case)
    out = torch.full((n * oh * ow + ow,), 0xA5, dtype=torch.uint8, device='cuda')                  # one extra row
    logits_d = _dev(logits) if n else None
    check(_L().csm_mask_resize_threshold(ptr(logits_d), i32(n), i32(h), i32(w), i32(C.MASK_UP), i32(rh), i32(rw),
                                         i32(oh), i32(ow), f32(thr), ptr(out), stream_ptr()), "mask_resize")
    got = out.cpu().numpy()
    assert (got[n * oh * ow:] == 0xA5).all()
    if n == 0:
        return
    got = got[:n * oh * ow].reshape(n, oh, ow)
    assert np.array_equal(got, oseg.mask_resize_threshold(logits, C.MASK_UP, rh, rw, oh, ow, thr))
    bad, excluded = mask_compare(got, logits, case)
    assert excluded <= C.MASK_EXCLUDED_CAP
    assert bad == 0


# ---- mask head -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maskhead_bound():
    return 4.0 * max(maskhead_oracle_errors().values())


@pytest.mark.parametrize("hw", C.MASKHEAD_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("ld", C.MASKHEAD_LDS)
def test_maskhead_logits_at_a_channel_pitch(ld, hw, maskhead_bound):
    """k_maskhead reading 8 prototype channels out of a buffer of channel pitch ld (production passes the workspace buffer's pitch):
    bit-exact against the oracle, and against float64 within 4 x the oracle's own largest error over these cases (measured on the CPU:
    2.7e-7 of a case's largest |logit|, so the bound is 1.1e-6); the logits buffer is written for n * h * w floats and no further."""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    from oracle import segment as oseg
    assert 0.0 < maskhead_bound < 1e-5
    for n in C.MASKHEAD_NS:
        k = C.maskhead_case(ld, hw, n)
        h, w = hw
        wide = _dev(k['wide'])
        feat_ptr = ctypes.c_void_p(wide.data_ptr() + 4 * k['c0'])
        out = torch.full((n * h * w + 64,), float('nan'), device='cuda')
        ker, pri = (_dev(k['kernels']), _dev(k['priors'])) if n else (None, None)
        check(_L().csm_maskhead_logits(feat_ptr, i32(ld), i32(h), i32(w), i32(8), i32(8), ptr(ker), ptr(pri), i32(n),
                                       i32(C.MASKHEAD_FEAT_STRIDE), ptr(out), stream_ptr()), "maskhead")
        got = out.cpu().numpy()
        assert np.isnan(got[n * h * w:]).all()
        got = got[:n * h * w].reshape(n, h, w)
        assert np.array_equal(got, oseg.maskhead_logits(k['wide'], k['kernels'], k['priors'], C.MASKHEAD_FEAT_STRIDE, c0=k['c0']))
        ref = C.maskhead_reference(k['wide'][..., k['c0']:k['c0'] + 8], k['kernels'], k['priors'], C.MASKHEAD_FEAT_STRIDE)
        assert C.maskhead_rel_err(got, ref) <= maskhead_bound


# ---- detector preprocess -----------------------------------------------------------------------------------------------------------
PRE = C.preprocess_cases()


@pytest.mark.parametrize("case", PRE, ids=[c[0] for c in PRE])
def test_det_preprocess_equals_oracle_and_float64(case):
    """k_det_preprocess: byte-exact against the oracle; within one grey level (1 / std[c]) of the float64 statement (bilinear at cv2's
    half-pixel centres, clamped edges, rounded to a grey level, normalised, pad outside (rh, rw))"""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    from oracle import segment as oseg
    name, img, rh, rw, S_h, S_w = case
    H, W = img.shape[:2]
    out = torch.full((3 * S_h * S_w + S_w,), float('nan'), device='cuda')
    mean, std = (ctypes.c_float * 3)(*C.DetNorm.mean), (ctypes.c_float * 3)(*C.DetNorm.std)
    img_d = _dev(img)
    check(_L().csm_det_preprocess(ptr(img_d), i32(H), i32(W), i32(rh), i32(rw), i32(S_h), i32(S_w), mean, std, f32(C.DetNorm.pad_value),
                                  ptr(out), stream_ptr()), "det_preprocess")
    got = out.cpu().numpy()
    assert np.isnan(got[3 * S_h * S_w:]).all()
    got = got[:3 * S_h * S_w].reshape(1, 3, S_h, S_w)
    assert np.array_equal(got, oseg.det_preprocess(img, (S_h, S_w), C.DetNorm, rh, rw))
    d = np.abs(got.astype(np.float64) - C.preprocess_reference(img, rh, rw, S_h, S_w))[0]
    assert (d <= C.preprocess_bound()).all()


# ---- bit packing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PACK_SIZES)
def test_pack_mask_bits_at_every_misalignment(n):
    """k_pack_bits == np.packbits(m != 0, bitorder='little') with the input at byte offsets 0..7 of a larger buffer (8-byte loads only
    at offset 0) and byte values {0, 1, 2, 128, 255}; the byte after the output survives"""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    m = C.pack_case(n)
    ref = C.pack_reference(m)
    nb = (n + 7) // 8
    for k in range(8):
        buf = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() % 8 == 0
        buf[k:k + n] = _dev(m)
        out = torch.full((nb + 1,), 0x5A, dtype=torch.uint8, device='cuda')
        check(_L().csm_pack_mask_bits(ctypes.c_void_p(buf.data_ptr() + k), i64(n), ptr(out), stream_ptr()), "pack_mask_bits")
        got = out.cpu().numpy()
        assert np.array_equal(got[:nb], ref), (n, k)
        assert got[nb] == 0x5A


# ---- decode -> NMS -> gather at the shipped size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3])
def test_decode_nms_gather_chain_at_the_shipped_size(nc):
    """csm_det_decode -> csm_nms (iou 0.6, max_keep 100) -> csm_det_gather on 80x80 / 40x40 / 20x20 head maps with nms_pre 1000 (K = 2400
    slots for one class, 3000 for three), clustered boxes and a level short of candidates, against the numpy statement of mmdet's decode
    followed by the reference NMS in np.float32 (the boxes are not exact here, so the reference takes its decisions in the kernel's type).
    The kept list is the reference's valid detections first, then score -1 slots in slot order."""
    check, f32, i32, i64, ptr, stream_ptr = _args()
    L = _L()
    P, hw, strides = C.CHAIN, C.CHAIN_HW, C.CHAIN_STRIDES
    k = C.chain_case(nc)
    G, M, nl = P['G'], P['max_keep'], 3
    sc, bx, sr, lb, _ = C.decode_reference(k['cls'], k['reg'], hw, strides, nc, P['nms_pre'], P['score_thr'], P['det'], P['det'],
                                           P['scale'], P['scale'], P['min_box'])
    n = len(sc)
    cls_d, reg_d, kern_d = [[_dev(a[None]) for a in k[key]] for key in ('cls', 'reg', 'kern')]
    vp = ctypes.c_void_p * nl
    cp_, rp_, kp_ = vp(*[t.data_ptr() for t in cls_d]), vp(*[t.data_ptr() for t in reg_d]), vp(*[t.data_ptr() for t in kern_d])
    level_hw = (ctypes.c_int * 6)(*[v for h, w in hw for v in (h, w)])
    st = (ctypes.c_int * 3)(*strides)
    lds3 = (ctypes.c_int * 9)(*[v for _ in range(3) for v in (nc, 4, G)])
    K = L.csm_det_decode_slots(level_hw, i32(nl), i32(nc), i32(P['nms_pre']))
    assert K == (2400 if nc == 1 else 3000) and n < K
    scores = torch.empty((1, K), device='cuda'); boxes = torch.empty((1, K, 4), device='cuda')
    src = torch.empty((1, K), dtype=torch.int32, device='cuda'); labels = torch.empty((1, K), dtype=torch.int32, device='cuda')
    offs = torch.empty((1, K), device='cuda') if nc > 1 else None
    scratch = torch.empty(L.csm_det_decode_scratch_bytes(i32(1), i32(K)), dtype=torch.uint8, device='cuda')
    sfx = float(np.float32(P['scale']))
    check(L.csm_det_decode(cp_, rp_, level_hw, st, lds3, i32(nl), i32(1), i32(nc), f32(P['score_thr']), i32(P['nms_pre']), f32(P['det']),
                           f32(P['det']), f32(sfx), f32(sfx), f32(P['min_box']), i32(K), ptr(scores), ptr(boxes), ptr(src), ptr(labels),
                           ptr(offs), ptr(scratch), stream_ptr()), "det_decode")
    got_s, got_b = scores[0].cpu().numpy(), boxes[0].cpu().numpy()
    assert np.array_equal(got_s[:n], sc) and (got_s[n:] == -1.0).all()
    assert np.array_equal(got_b[:n], bx) and not got_b[n:].any()
    assert np.array_equal(src[0, :n].cpu().numpy(), sr) and np.array_equal(labels[0, :n].cpu().numpy(), lb)
    ref_offs = None
    if nc > 1:
        ref_offs = (lb.astype(np.float32) * (np.float32(bx.max()) + np.float32(1))).astype(np.float32)
        assert np.array_equal(offs[0, :n].cpu().numpy(), ref_offs)
    # reference NMS in fp32 over the candidates; the trailing slots are zero boxes, which neither suppress nor are suppressed, so the
    # scan runs on into them until max_keep: valid entries first
    valid_keep = C.nms_reference(bx, ref_offs, P['iou'], K, np.float32)
    assert len(valid_keep) < 0.1 * n and len(valid_keep) < M                                     # NMS removes most candidates
    ref_keep = np.concatenate([valid_keep, np.arange(n, K)])[:M].astype(np.int32)
    if nc == 1:
        assert np.array_equal(ref_keep, C.nms_reference(np.concatenate([bx, np.zeros((K - n, 4), np.float32)]), None, P['iou'], M, np.float32))
    keep = torch.full((1, M + 8), SENT, dtype=torch.int32, device='cuda')
    nk = torch.full((1,), SENT, dtype=torch.int32, device='cuda')
    nscr = torch.empty(L.csm_nms_scratch_bytes(i32(K)), dtype=torch.uint8, device='cuda')
    check(L.csm_nms(ptr(boxes[0]), ptr(None if offs is None else offs[0]), i32(K), f32(P['iou']), i32(M), ptr(keep[0]), ptr(nk), ptr(nscr),
                    stream_ptr()), "nms")
    got_keep = keep[0].cpu().numpy()
    assert int(nk.item()) == len(ref_keep) == M
    assert np.array_equal(got_keep[:M], ref_keep) and (got_keep[M:] == SENT).all()
    keep_m = keep[:, :M].contiguous()
    ks, kb, kl = torch.empty((1, M), device='cuda'), torch.empty((1, M, 4), device='cuda'), torch.empty((1, M), dtype=torch.int32, device='cuda')
    kp, kk = torch.empty((1, M, 4), device='cuda'), torch.empty((1, M, G), device='cuda')
    check(L.csm_det_gather(kp_, level_hw, st, lds3, i32(nl), i32(1), i32(K), i32(M), i32(G), ptr(keep_m), ptr(scores), ptr(boxes), ptr(src),
                           ptr(labels), ptr(ks), ptr(kb), ptr(kl), ptr(kp), ptr(kk), stream_ptr()), "det_gather")
    nv = len(valid_keep)
    ks, kb, kl, kp, kk = (t[0].cpu().numpy() for t in (ks, kb, kl, kp, kk))
    assert np.array_equal(ks[:nv], sc[valid_keep]) and (ks[nv:] == -1.0).all()
    assert np.array_equal(kb[:nv], bx[valid_keep]) and not kb[nv:].any()
    assert np.array_equal(kl[:nv], lb[valid_keep])
    prior0 = np.cumsum([0] + [h * w for h, w in hw])
    kern_flat = np.concatenate([a.reshape(-1, G) for a in k['kern']])
    pri_all = np.concatenate([np.stack([(np.arange(h * w) % w) * s, (np.arange(h * w) // w) * s, np.full(h * w, s), np.full(h * w, s)], 1)
                              for (h, w), s in zip(hw, strides)]).astype(np.float32)
    assert prior0[-1] == len(kern_flat) == len(pri_all)
    assert np.array_equal(kk[:nv], kern_flat[sr[valid_keep]])
    assert np.array_equal(kp[:nv], pri_all[sr[valid_keep]])
