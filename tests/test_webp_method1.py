"""CPU: the contract of the WebP writer's method 1 (B_PRED macroblocks and per-frame probability updates).  libwebp
(through Pillow) and the project's own decoder restatement (tests/webplossy_restatement.py) decode the files of the restatement
(tests/webp_m1_restatement.py) to exactly the RGB it predicts; the frames reach every new path; the cost table is its formula and no
update is taken that does not pay; the first partition's new bound; argument errors; never worse than method 0 at equal size."""
import functools
import math
import os
import sys

import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_m1_restatement as M  # noqa: E402
import webp_restatement as R  # noqa: E402
import webplossy_restatement as D  # noqa: E402
from test_mjpeg import cartoon, psnr  # noqa: E402
from test_webp import CASES, IDS, MAX_DEFICIT_DB, SHAPES, _host_code, frame, pil_frames, pillow_webp, want  # noqa: E402
from cartoonsegmentation_amd import webpcode  # noqa: E402


@functools.lru_cache(maxsize=None)
def want1(name, quality, v=0):
    """the method-1 restatement's result for frame v of a case of test_webp.SHAPES, computed once and shared"""
    return M.encode_frame(frame(name, v), quality)


@functools.lru_cache(maxsize=None)
def large():
    """the 1024x1024 cartoon frame of the GPU test at quality 90"""
    return M.encode_frame(cartoon(1024, 1024, seed=0), 90)


# ---- pinned by libwebp and by the decoder's restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,quality", CASES, ids=IDS)
def test_libwebp_and_the_decoder_restatement_show_what_method1_reconstructs(name, quality):
    H, W, _ = SHAPES[name]
    r = want1(name, quality)
    data = R.still_file(r['vp8'])
    frames, size, n, _, _ = pil_frames(data)
    assert size == (W, H) and n == 1
    expect = R.decoded_rgb(r, H, W)
    diff = np.argwhere(frames[0] != expect)
    assert diff.size == 0, (name, quality, len(diff), diff[0].tolist())
    bgra, report = D.decode(data)
    assert np.array_equal(bgra[..., 2::-1], expect)
    assert report['has_b'] == bool(r['is_b'].any()) and report['prob_updates'] == sum(r['updated'])
    assert report['bmodes'] == set(r['bmodes'][r['is_b']].ravel().tolist())
    assert report['skipped'] == int(r['skip'].sum()) and report['partitions'] == webpcode.partitions(H) == len(r['parts'])
    assert r['vp8'] == webpcode.vp8_frame(r['first'], r['parts'], W, H)


def test_the_prediction_table_is_the_decoders_predictor():
    """the vectorised ten predictions equal webplossy_restatement.subblock_prediction, mode by mode"""
    rng = np.random.default_rng(11)
    for k in range(200):
        e = rng.integers(0, 256, 13) if k else np.array([0, 255] * 6 + [0])
        ten = M.subblock_predictions(e)
        for mode in range(10):
            assert np.array_equal(ten[mode], D.subblock_prediction(mode, e[4], e[5:13], e[3::-1])), (k, mode)


# ---- coverage: the encoder alone reaches every new path -----------------------------------------------------------------------------
def _carried(r):
    """[mbh,mbw,2]: the (left, above) Y2 context a macroblock reads, by the contract's rule: the flag of the nearest macroblock in
    its row / column that is not B_PRED (0 when that one is skipped, or there is none); and [mbh,mbw,2] whether that macroblock is
    not the immediate neighbour"""
    is_b, skip = r['is_b'], r['skip']
    y2 = r['lev_y2'].any(axis=2) & ~skip & ~is_b
    mbh, mbw = is_b.shape
    ctx, far = np.zeros((mbh, mbw, 2), int), np.zeros((mbh, mbw, 2), bool)
    for y in range(mbh):
        for x in range(mbw):
            k = x - 1
            while k >= 0 and is_b[y, k]:
                k -= 1
            ctx[y, x, 0], far[y, x, 0] = (y2[y, k] if k >= 0 else 0), (x >= 1 and is_b[y, x - 1])
            k = y - 1
            while k >= 0 and is_b[k, x]:
                k -= 1
            ctx[y, x, 1], far[y, x, 1] = (y2[k, x] if k >= 0 else 0), (y >= 1 and is_b[y - 1, x])
    return ctx, far


def test_the_frames_reach_every_new_path():
    r = want1('243x317', 90)
    is_b, skip, bm = r['is_b'], r['skip'], r['bmodes']
    mbh, mbw = is_b.shape
    assert set(bm[is_b].ravel().tolist()) == set(range(10))                                  # all ten sub-block modes
    assert is_b.any() and not is_b.all()                                                     # B_PRED and 16x16 in one frame
    assert any(is_b[y, x] and not is_b[y - 1, x] and not is_b[y, x - 1] for y in range(1, mbh) for x in range(1, mbw))   # implied contexts
    assert is_b[0].any() and is_b[:, -1].any() and is_b[-1, -1]                              # top row, last column, the corner
    assert (is_b & skip).any() and (is_b & ~skip).any()                                      # a skipped B_PRED macroblock
    # a coded 16x16 macroblock whose Y2 context 1 comes from beyond a B_PRED neighbour (whose own mask would say 0), in a row and in a column
    ctx, far = _carried(r)
    coded16 = ~is_b & ~skip
    assert (coded16 & far[..., 0] & (ctx[..., 0] == 1)).any() and (coded16 & far[..., 1] & (ctx[..., 1] == 1)).any()
    assert all(np.any(r['updated'][k * 264:(k + 1) * 264]) for k in range(4))                # updates in all four block types
    for name in ('black', 'white'):
        flat = want1(name, 90)
        assert not any(flat['updated']) and not flat['is_b'].any() and flat['probs'] == R.COEFF_PROBS     # no update at all
    # other frames that mix the two kinds at other sizes and qualities, so that the list does not hang on one frame
    for name, q in (('100x101', 50), ('noise', 90), ('17x33', 50), ('16x1120', 90)):
        b = want1(name, q)['is_b']
        assert b.any() and not b.all(), (name, q)


# ---- the cost table and the update rule -----------------------------------------------------------------------------------------
def test_the_cost_table_is_its_formula():
    assert len(M.PROB_COST) == 255
    assert M.PROB_COST == [int(round(256 * math.log2(256 / p))) for p in range(1, 256)]
    assert M.PROB_COST[127] == 256 and M.PROB_COST[0] == 2048
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cartoonsegmentation_amd', 'csrc',
                               'csm_vp8_tables.h')).read()
    body = header[header.index('kProbCost[255]'):]
    body = body[body.index('{') + 1:body.index('}')]
    assert [int(v) for v in body.replace('\n', ' ').split(',')] == M.PROB_COST            # the device's copy
    body = header[header.index('kBModeProbs[900]'):]
    body = body[body.index('{') + 1:body.index('}')]
    assert [int(v) for v in body.replace('\n', ' ').split(',')] == np.array(D.KF_BMODE_PROBS).ravel().tolist()


def _token_cost(tokens, probs):
    """the cost of a frame's tokens under a table, in 1/256 bit, recounted token by token"""
    return sum(M.bit_cost(probs[i] if i >= 0 else -i, bit) for part in tokens for i, bit in part)


@pytest.mark.parametrize("name,quality", [('243x317', 90), ('100x101', 50), ('noise', 90), ('gradient', 100), ('48x64', 1), ('black', 90)])
def test_an_update_is_never_taken_when_it_does_not_pay(name, quality):
    r = want1(name, quality)
    probs, updated, counts = r['probs'], r['updated'], r['counts']
    price = [8 * 256 + M.bit_cost(R.COEFF_UPDATE_PROBS[i], 1) - M.bit_cost(R.COEFF_UPDATE_PROBS[i], 0) for i in range(1056)]
    # the counts are the frame's tokens
    recount = np.zeros((1056, 2), np.int64)
    for part in r['tokens']:
        for i, bit in part:
            if i >= 0:
                recount[i, bit] += 1
    assert np.array_equal(recount, counts)
    for i in range(1056):
        one = list(R.COEFF_PROBS)
        one[i] = probs[i]
        if updated[i]:                # this entry alone saves more than its flag and value cost
            c0, c1 = int(counts[i, 0]), int(counts[i, 1])
            saving = c0 * (M.bit_cost(R.COEFF_PROBS[i], 0) - M.bit_cost(probs[i], 0)) + c1 * (M.bit_cost(R.COEFF_PROBS[i], 1) - M.bit_cost(probs[i], 1))
            assert saving > price[i] and probs[i] != R.COEFF_PROBS[i], (i, saving, price[i])
        else:
            assert probs[i] == R.COEFF_PROBS[i]
    # and over the whole frame, token by token under both tables
    before, after = _token_cost(r['tokens'], R.COEFF_PROBS), _token_cost(r['tokens'], probs)
    paid = sum(price[i] for i in range(1056) if updated[i])
    print("%s q%d: %d updates, tokens %d -> %d (1/256 bit), paid %d" % (name, quality, sum(updated), before, after, paid))
    assert before - after >= paid and (any(updated) or before == after)
    if any(updated):
        assert before - after > paid


# ---- the first partition's bound -----------------------------------------------------------------------------------------------------
def _first_cap(nmb):
    """csrc/webp.hip's bound for method 1: 7 bits for each of 30 + 1056 * 9 + 9 header pairs and 1 + 1 + 16 * 7 + 3 pairs per
    macroblock, rounded up to bytes, plus 8 for the coder's padding and its held-back byte"""
    return (7 * (30 + 1056 * 9 + 9 + (1 + 1 + 16 * 7 + 3) * nmb) + 7) // 8 + 8


@pytest.mark.parametrize("mbw,mbh", [(1, 1), (3, 2)])
def test_the_worst_first_partition_stays_inside_its_new_segment(mbw, mbh):
    """(after test_webp.test_device_coder_never_writes_past_its_segment) the longest first partition method 1 can write -- every
    probability updated, every macroblock B_PRED with the deepest sub-block mode and the deepest chroma mode -- has no more pairs than
    the bound counts and, through csm_boolenc.h built for the host, fits the segment; streams of that many pairs that move the most
    bits fit too; a segment one byte short sets the flag and nothing behind it is touched"""
    nmb = mbw * mbh
    shape = (mbh, mbw)
    skip = np.zeros(shape, bool)
    skip[0, 0] = True
    pairs = M.first_pairs(127, 31, 0, [1] * 1056, [1] * 1056, skip, np.ones(shape, bool), np.full(shape + (16,), D.B_HU), np.zeros(shape, int),
                          np.full(shape, R.TM_PRED))
    bound = 30 + 1056 * 9 + 9 + 117 * nmb
    assert bound - 1 <= len(pairs) <= bound            # 29 header bits are written; the bound counts 30
    assert max(len(t) for t in M.BMODE_TREE.values()) == 7
    cap = _first_cap(nmb)
    streams = [pairs, [(255, 1)] * bound, [(1, 0)] * bound, [(128, 1)] * bound, [(254, 1), (2, 0)] * (bound // 2)]
    for s in streams:
        expect = R.code_pairs(s)
        need, over, intact, seg = _host_code(s, cap)
        assert need == len(expect) <= cap and over == 0 and intact == 1 and seg[:need] == expect, (len(s), need, cap)
        need, over, intact, seg = _host_code(s, len(expect) - 1)
        assert need == len(expect) and over == 1 and intact == 1 and seg == expect[:-1]
    assert _first_cap(4096) < webpcode.MAX_FIRST_BYTES < _first_cap(8192)       # what the frame tag holds: ops checks the coded size


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_method_argument_errors():
    torch = pytest.importorskip("torch")
    from cartoonsegmentation_amd import _lib, ops
    from cartoonsegmentation_amd._lib import CsmError
    from cartoonsegmentation_amd.kenburns import npyframes2video
    for bad in (2, -1, True, False, 1.0, '1', None):
        with pytest.raises(ValueError):
            webpcode.check_method(bad)
    assert webpcode.check_method(0) == 0 and webpcode.check_method(np.int64(1)) == 1
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for fn in (ops.webp_encode, ops.webp_streams):
        for bad in (2, -1, True, 1.0, '1', None):
            with pytest.raises(ValueError):
                fn(x, method=bad)
        for ok in (0, 1):
            with pytest.raises(CsmError):
                fn(x, method=ok)                                             # a CPU tensor
            with pytest.raises(ValueError):
                fn(x, quality=0, method=ok)
            with pytest.raises(ValueError):
                fn(torch.zeros((16384, 1, 3), dtype=torch.uint8), method=ok)
    for bad in (3, True, None):
        with pytest.raises(ValueError):
            npyframes2video([np.zeros((8, 8, 3), np.uint8)], 'x.webp', method=bad)       # refused before the frames are uploaded
    L = _lib.load()
    for n, H, W in ((1, 1, 1), (3, 100, 101), (75, 1024, 1024)):
        zero, one = L.csm_webp_scratch_bytes_m(n, H, W, 0), L.csm_webp_scratch_bytes_m(n, H, W, 1)
        assert zero == L.csm_webp_scratch_bytes(n, H, W) > 0 and one > zero
        assert L.csm_webp_scratch_bytes_m(n, H, W, 2) == 0 and L.csm_webp_scratch_bytes_m(n, H, W, -1) == 0
        nmb = ((H + 15) // 16) * ((W + 15) // 16)
        extra = (n * _first_cap(nmb) + 15) // 16 * 16 - (n * ((7 * (1100 + 7 * nmb) + 7) // 8 + 8) + 15) // 16 * 16
        assert one - zero >= extra + n * (17 * nmb + 2112 * 4 + 2 * 1056)    # the larger first partitions, the modes, counters and tables
    assert L.csm_webp_scratch_bytes_m(1, 16384, 16, 1) == 0
    for fn, args in ((L.csm_webp_measure_m, (None, 1, 16, 16, 90, 2, None, None, None)), (L.csm_webp_write_m, (1, 16, 16, 2, None, 0, None, None)),
                     (L.csm_webp_stage_m, (1, None, 1, 16, 16, 90, 7, None, None, None))):
        assert fn(*args) != 0                                                # refused before anything is launched


# ---- never worse than method 0 at equal size ------------------------------------------------------------------------------------------
# PSNR (dB, RGB against the source) of the three 243x317 cartoon frames below Pillow's WebP (method 4) at the largest quality whose
# file is not larger than ours, as test_webp.deficit measures it for method 0.  Measured for method 1:
# quality 50: 0.24, 0.17, 0.16; quality 75: 0.19, 0.14, 0.18; quality 90: 0.07, 0.08, 0.02 (method 0: 2.04 .. 0.52).  The bound is the
# largest of them (0.24) rounded up to the next 0.5 dB (0.5) plus 0.5 dB, as §4.12 derived method 0's.
MAX_DEFICIT_M1_DB = 1.0


def _psnr1(v, quality):
    f = frame('243x317', v)
    r = want1('243x317', quality, v)
    return len(R.still_file(r['vp8'])), psnr(R.decoded_rgb(r, 243, 317), f[:, :, ::-1])


def _psnr0(v, quality):
    f = frame('243x317', v)
    r = want('243x317', quality, v)
    return len(R.still_file(r['vp8'])), psnr(R.decoded_rgb(r, 243, 317), f[:, :, ::-1])


@pytest.mark.parametrize("quality", [50, 75, 90])
@pytest.mark.parametrize("v", [0, 1, 2])
def test_never_worse_than_method_0_at_equal_size(v, quality):
    """both are comparisons with method 0's encoder, not with a number: at the same quality number the method-1 file is smaller, and
    at q0 -- the largest method-0 quality whose file is not larger than the method-1 file, found by bisection since method 0's size
    grows with the quality -- method 0's PSNR is not higher.  The deficit against Pillow is printed and held to the caps."""
    f = frame('243x317', v)
    size1, psnr1 = _psnr1(v, quality)
    same0, same0_psnr = _psnr0(v, quality)
    assert size1 < same0, (size1, same0)
    lo, hi = 0, 100                                      # method 0 at quality lo fits (0: none does), at hi + 1 it does not
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _psnr0(v, mid)[0] <= size1:
            lo = mid
        else:
            hi = mid - 1
    assert lo >= 1, "method 0's smallest file is larger than method 1's"
    size0, psnr0 = _psnr0(v, lo)
    assert size0 <= size1 and (lo == 100 or _psnr0(v, lo + 1)[0] > size1)
    for q in range(100, 0, -1):
        theirs = pillow_webp(f, q)
        if len(theirs) <= size1:
            break
    else:
        raise AssertionError("Pillow's smallest file (%d bytes) is larger than ours (%d)" % (len(theirs), size1))
    ref = psnr(pil_frames(theirs)[0][0], f[:, :, ::-1])
    print("frame %d quality %d: method 1 %d B %.2f dB; method 0 at the same quality %d B %.2f dB, at q0 = %d %d B %.2f dB (gain %.2f dB); "
          "Pillow quality %d %d B %.2f dB; deficit %.2f dB" % (v, quality, size1, psnr1, same0, same0_psnr, lo, size0, psnr0, psnr1 - psnr0,
                                                              q, len(theirs), ref, ref - psnr1))
    assert psnr1 >= psnr0, (psnr1, psnr0, lo)
    assert ref - psnr1 <= MAX_DEFICIT_DB
    assert ref - psnr1 <= MAX_DEFICIT_M1_DB
