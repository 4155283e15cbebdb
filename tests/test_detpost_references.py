"""CPU: the oracle of the detector post-processing (oracle/segment.py over oracle/post_oracle.c) against the plain float64 references
of tests/detpost_cases.py, on every case the GPU tests use -- and, for every case, the property the case exists for (suppressed share,
chain in three words, exact-threshold pair, excluded share of the mask comparison, grey-level bound).  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detpost_cases as C  # noqa: E402

from oracle import segment as oseg  # noqa: E402


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_classes", [False, True])
@pytest.mark.parametrize("n", C.NMS_SIZES)
def test_nms_oracle_equals_the_greedy_float64_loop_and_the_case_has_its_layouts(n, with_classes):
    case = C.nms_case(n, with_classes)
    boxes, offs, plants = case['boxes'], case['offsets'], case['plants']
    assert boxes.shape == (n, 4) and (offs is None) == (not with_classes)
    if with_classes and n:
        assert np.array_equal(offs, case['labels'] * (boxes.max() + 1)) and offs.max() <= 2 * 1024
    # which layouts a list of this length must hold
    if n >= 63:
        assert 'exact_0.5' in plants
    if n >= 129:
        assert {'chain', 'twins', 'above_0.5', 'exact_0.625'} <= set(plants)
    if n >= 1000:
        assert {'tail', 'above_0.625'} <= set(plants)
    for thr in C.NMS_THRS:
        full = C.nms_reference(boxes, offs, thr, n + 5)
        kept = set(full.tolist())
        if n <= 1000:                                                                    # the pair matrix drives the same greedy result
            sup, dead, walk = C.nms_pair_matrix(boxes, offs, thr), np.zeros(n, bool), []
            for i in range(n):
                if not dead[i]:
                    walk.append(i)
                    dead |= sup[i]
            assert walk == full.tolist() and not np.tril(sup).any()
        for max_keep in C.nms_max_keeps(n):
            ref = C.nms_reference(boxes, offs, thr, max_keep)
            assert np.array_equal(ref, full[:max_keep])                                  # stopping early == a prefix of the full run
            got = oseg.nms(boxes, offs, thr, max_keep)
            assert len(got) == min(len(full), max_keep) and np.array_equal(got, ref), (n, with_classes, thr, max_keep)
        # (a) clusters: more than half of ALL boxes are suppressed
        if n >= 63:
            assert n - len(full) > n / 2, (n, len(full))
        # (b) chain: A suppresses B, B would suppress C, A does not; three different words; C is kept
        if 'chain' in plants:
            a, b, c = plants['chain']
            assert len({a // 64, b // 64, c // 64}) == 3
            assert C.nms_suppresses(boxes[a], boxes[b], thr) and C.nms_suppresses(boxes[b], boxes[c], thr)
            assert not C.nms_suppresses(boxes[a], boxes[c], thr)
            assert a in kept and b not in kept and c in kept
        # (c) IoU exactly thr is kept (strict >), the smallest step above it is suppressed
        for name in ('exact_%s' % thr, 'above_%s' % thr):
            if name in plants:
                i, j = plants[name]
                bi, bj = boxes[i].astype(np.float64), boxes[j].astype(np.float64)
                inter = (min(bi[2], bj[2]) - max(bi[0], bj[0])) * (min(bi[3], bj[3]) - max(bi[1], bj[1]))
                union = (bi[2] - bi[0]) * (bi[3] - bi[1]) + (bj[2] - bj[0]) * (bj[3] - bj[1]) - inter
                assert i in kept
                if name.startswith('exact'):
                    assert inter == thr * union and j in kept
                else:
                    assert thr * union < inter <= thr * union + 0.5 and j not in kept
        if n >= 65:
            assert plants['exact_0.5'] == (63, 64)                                           # across the first word boundary
        # (d) identical boxes, labels 0 and 2: both kept with class offsets, one without
        if 'twins' in plants:
            i, j = plants['twins']
            assert np.array_equal(boxes[i], boxes[j]) and case['labels'][i] != case['labels'][j]
            assert i in kept and (j in kept) == with_classes
        # (e) decode form: the zero boxes of the last third are all kept and suppress nothing
        if 'tail' in plants:
            t0, t1 = plants['tail']
            assert t1 == n and t0 == n - n // 3 and not boxes[t0:].any()
            assert set(range(t0, t1)) <= kept
            assert np.array_equal(full[full < t0], C.nms_reference(boxes[:t0], None if offs is None else offs[:t0], thr, n + 5))


def test_nms_case_list_covers_every_layout():
    have = set()
    for n in C.NMS_SIZES:
        have |= set(C.nms_case(n, True)['plants'])
    assert have == {'chain', 'exact_0.5', 'above_0.5', 'exact_0.625', 'above_0.625', 'twins', 'tail'}
    assert C.nms_case(2, False)['plants'] == {'exact_0.5': (0, 1)}
    assert len(C.nms_case(4096, True)['boxes']) == 4096                                  # all 64 lanes own a word


# ---- mask resize + threshold -----------------------------------------------------------------------------------------------------
def mask_compare(mask_u8, logits, case):
    """-> (mismatches outside the excluded band, excluded share)"""
    h, w, rh, rw, oh, ow, thr, n = case
    prob = C.mask_reference_prob(logits, C.MASK_UP, rh, rw, oh, ow)
    assert prob.shape == (n, oh, ow)
    sure = np.abs(prob - thr) > C.MASK_EPS
    return int(((mask_u8 != 0) != (prob > thr))[sure].sum()), 1.0 - sure.mean()


def test_mask_case_list_covers_the_store_paths():
    ows = [c[5] for c in C.MASK_CASES]
    assert {o % 4 for o in ows} == {0, 1, 2, 3} and max(ows) > 1024
    assert sum(1 for c in C.MASK_CASES if c[6] == 0.3) == 2 and any(c[7] == 0 for c in C.MASK_CASES)
    assert any(c[2] == c[3] == max(c[4], c[5]) for c in C.MASK_CASES)                    # the box-prompt form
    assert any((c[0] * C.MASK_UP, c[1] * C.MASK_UP) == (c[2], c[3]) for c in C.MASK_CASES)   # identity second resize


@pytest.mark.parametrize("case", C.MASK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_mask_resize_threshold_oracle_equals_float64_torch(case):
    """measured: the oracle mismatches nowhere outside the excluded band, and the band holds at most 0.103 % of a case's pixels
    (cap 0.5 %: a condition of the inputs)"""
    h, w, rh, rw, oh, ow, thr, n = case
    logits = C.mask_logits(case)
    got = oseg.mask_resize_threshold(logits, C.MASK_UP, rh, rw, oh, ow, thr)
    assert got.shape == (n, oh, ow) and got.dtype == np.uint8
    if n == 0:
        return
    assert set(np.unique(got).tolist()) <= {0, 1}
    bad, excluded = mask_compare(got, logits, case)
    print("mask case %s: excluded share %.5f %%, mismatches %d" % (case, 100 * excluded, bad))
    assert excluded <= C.MASK_EXCLUDED_CAP
    assert bad == 0


# ---- mask head -----------------------------------------------------------------------------------------------------------------------
def maskhead_oracle_errors():
    """relative error (C.maskhead_rel_err) of the oracle against float64 on every mask-head case"""
    errs = {}
    for ld in C.MASKHEAD_LDS:
        for hw in C.MASKHEAD_HW:
            for n in C.MASKHEAD_NS:
                k = C.maskhead_case(ld, hw, n)
                got = oseg.maskhead_logits(k['wide'], k['kernels'], k['priors'], C.MASKHEAD_FEAT_STRIDE, c0=k['c0'])
                ref = C.maskhead_reference(k['wide'][..., k['c0']:k['c0'] + 8], k['kernels'], k['priors'], C.MASKHEAD_FEAT_STRIDE)
                assert got.shape == ref.shape == (n, hw[0], hw[1])
                errs[(ld, hw, n)] = C.maskhead_rel_err(got, ref)
    return errs


def test_maskhead_oracle_against_float64():
    """measured: largest relative error of the fp32 fmaf-chain oracle against float64 over the 45 cases = 2.7e-7 (|error| over the
    case's largest |logit|).  Three layers of at most 10 fp32 fmaf steps each: a few ulp (6e-8 each) of the largest logit."""
    errs = maskhead_oracle_errors()
    worst = max(errs.values())
    print("maskhead: largest relative error of the oracle against float64 = %.3e" % worst)
    assert 0.0 < worst <= 32 * 2.0 ** -24                     # 3 layers x <= 10 steps, half an ulp each, relative to the largest logit
    # the channel pitch matters: the slice of the wide buffer gives the contiguous copy's result, bit for bit
    k = C.maskhead_case(40, (20, 33), 5)
    sl = np.ascontiguousarray(k['wide'][..., k['c0']:k['c0'] + 8])
    assert np.array_equal(oseg.maskhead_logits(sl, k['kernels'], k['priors'], 8),
                          oseg.maskhead_logits(k['wide'], k['kernels'], k['priors'], 8, c0=k['c0']))
    assert not np.array_equal(oseg.maskhead_logits(sl, k['kernels'], k['priors'], 8), oseg.maskhead_logits(k['wide'], k['kernels'], k['priors'], 8))
    assert len({float(p[2]) for p in k['priors']}) == 3      # priors of all three strides


# ---- detector preprocess -----------------------------------------------------------------------------------------------------------
PRE = C.preprocess_cases()


def test_preprocess_case_list():
    names = {c[0] for c in PRE}
    assert len(names) == len(PRE)
    assert {c[5] for c in PRE} >= {64, 257, 1024} and any(c[4] != c[5] for c in PRE)
    assert any(c[1].shape[:2] == (1, 1) for c in PRE)
    assert any((c[2], c[3]) == c[1].shape[:2] for c in PRE)                                  # copy branch
    assert any(c[2] < c[4] and c[3] == c[5] for c in PRE) and any(c[3] < c[5] and c[2] == c[4] for c in PRE)
    assert any(c[2] > c[1].shape[0] for c in PRE) and any(c[2] < c[1].shape[0] for c in PRE)  # up and down
    assert any(set(np.unique(c[1]).tolist()) == {0, 255} for c in PRE)


@pytest.mark.parametrize("case", PRE, ids=[c[0] for c in PRE])
def test_det_preprocess_oracle_within_one_grey_level_of_float64(case):
    name, img, rh, rw, S_h, S_w = case
    got = oseg.det_preprocess(img, (S_h, S_w), C.DetNorm, rh, rw)
    ref = C.preprocess_reference(img, rh, rw, S_h, S_w)
    assert got.shape == ref.shape == (1, 3, S_h, S_w)
    d = np.abs(got.astype(np.float64) - ref)[0]
    print("preprocess %s: largest difference %.3f grey levels" % (name, (d * np.asarray(C.DetNorm.std)[:, None, None]).max()))
    assert (d <= C.preprocess_bound()).all()
    pad = (np.float32(C.DetNorm.pad_value) - np.asarray(C.DetNorm.mean, np.float32)) / np.asarray(C.DetNorm.std, np.float32)
    assert np.array_equal(got[0, :, rh:, :], np.broadcast_to(pad[:, None, None], (3, S_h - rh, S_w)))
    assert np.array_equal(got[0, :, :, rw:], np.broadcast_to(pad[:, None, None], (3, S_h, S_w - rw)))
    if (rh, rw) == img.shape[:2]:                              # the copy branch is exact up to the fp32 normalisation
        assert (d[:, :rh, :rw] <= 1e-6).all()


# ---- bit packing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PACK_SIZES)
def test_pack_reference_is_what_the_shard_record_reader_unpacks(n):
    """np.packbits(m != 0, bitorder='little') is the form cartoonsegmentation_amd.shard.read_record decodes on rank 0"""
    from cartoonsegmentation_amd import shard
    m = C.pack_case(n)
    assert set(np.unique(C.pack_case(100003)).tolist()) == set(C.PACK_VALUES.tolist())
    ref = C.pack_reference(m)
    fb, mb, total = shard.record_layout(1, n, 1)
    assert len(ref) == mb == (n + 7) // 8
    rec = torch.zeros(total, dtype=torch.uint8)
    rec[fb:fb + mb] = torch.from_numpy(ref)
    rec[fb + mb:] = torch.tensor([1], dtype=torch.int64).view(torch.uint8)
    _, masks, cnt = shard.read_record(rec, 1, n, 1)
    assert cnt == 1 and np.array_equal(masks[0, 0].numpy(), m != 0)


# ---- the chain's inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3])
def test_chain_case_has_clusters_short_level_and_trailing_slots(nc):
    k = C.chain_case(nc)
    P = C.CHAIN
    sc, bx, sr, lb, n_before = C.decode_reference(k['cls'], k['reg'], C.CHAIN_HW, C.CHAIN_STRIDES, nc, P['nms_pre'], P['score_thr'], P['det'],
                                                  P['det'], P['scale'], P['scale'], P['min_box'])
    slots = sum(min(P['nms_pre'], h * w * nc) for h, w in C.CHAIN_HW)
    assert slots == (2400 if nc == 1 else 3000)
    per_level = [int((c > np.float32(P['score_thr'])).sum()) for c in k['cls']]
    assert per_level[0] > P['nms_pre'] and per_level[2] < min(P['nms_pre'], 400 * nc)    # a top-k cut and a level short of candidates
    n = len(sc)
    assert n < slots and (np.diff(sc) <= 0).all()
    offs = (lb.astype(np.float32) * (bx.max() + np.float32(1))).astype(np.float32) if nc > 1 else None
    full = C.nms_reference(bx, offs, P['iou'], slots, np.float32)
    print("chain nc=%d: %d candidates in %d slots, NMS keeps %d" % (nc, n, slots, len(full)))
    assert len(full) < 0.1 * n                                   # NMS removes most candidates
    assert len(full) < P['max_keep']                             # so the kept list runs on into the score -1 slots
