"""The WebP writer's second coding method restated in numpy / pure Python: method 0's key-frame encoder
(tests/webp_restatement.py) plus B_PRED macroblocks (ten 4x4 predictors, chosen by SSE; 16x16 against B_PRED by an integer
rate-distortion rule) and per-frame coefficient-probability updates.  The transforms, the quantiser, the boolean coder, the 16x16
predictions and the containers are method 0's; the sub-block mode numbering and kf_bmode_probs are the decoder's
(tests/webplossy_restatement.py).  tests/test_webp_method1.py holds this text to libwebp and to the decoder's restatement on every
byte, tests/test_gpu_webp_method1.py holds the device code to these bytes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as R  # noqa: E402
import webplossy_restatement as D  # noqa: E402

# C[p] = round(256 * log2(256 / p)) for p = 1..255: the cost of a decision of probability p / 256 in 1/256 bit; PROB_COST[p - 1]
PROB_COST = [
    2048, 1792, 1642, 1536, 1454, 1386, 1329, 1280, 1236, 1198, 1162, 1130, 1101, 1073, 1048, 1024, 1002, 980, 961, 942, 924, 906, 890, 874, 859, 845, 831, 817, 804, 792, 780, 768,
    757, 746, 735, 724, 714, 705, 695, 686, 676, 668, 659, 650, 642, 634, 626, 618, 611, 603, 596, 589, 582, 575, 568, 561, 555, 548, 542, 536, 530, 524, 518, 512,
    506, 501, 495, 490, 484, 479, 474, 468, 463, 458, 453, 449, 444, 439, 434, 430, 425, 420, 416, 412, 407, 403, 399, 394, 390, 386, 382, 378, 374, 370, 366, 362,
    358, 355, 351, 347, 343, 340, 336, 333, 329, 326, 322, 319, 315, 312, 309, 305, 302, 299, 296, 292, 289, 286, 283, 280, 277, 274, 271, 268, 265, 262, 259, 256,
    253, 250, 247, 245, 242, 239, 236, 234, 231, 228, 226, 223, 220, 218, 215, 212, 210, 207, 205, 202, 200, 197, 195, 193, 190, 188, 185, 183, 181, 178, 176, 174,
    171, 169, 167, 164, 162, 160, 158, 156, 153, 151, 149, 147, 145, 143, 140, 138, 136, 134, 132, 130, 128, 126, 124, 122, 120, 118, 116, 114, 112, 110, 108, 106,
    104, 102, 101, 99, 97, 95, 93, 91, 89, 87, 86, 84, 82, 80, 78, 77, 75, 73, 71, 70, 68, 66, 64, 63, 61, 59, 58, 56, 54, 53, 51, 49,
    48, 46, 44, 43, 41, 40, 38, 36, 35, 33, 32, 30, 28, 27, 25, 24, 22, 21, 19, 18, 16, 15, 13, 12, 10, 9, 7, 6, 4, 3, 1]

RD_SHIFT = 14                      # J = D + ((3 * ac * ac * R) >> RD_SHIFT), R in 1/256 bit (§4.12b records the search)
IMPLIED = (D.B_DC, D.B_VE, D.B_HE, D.B_TM)         # the sub-block mode a 16x16 mode (DC, V, H, TM) stands for in contexts
# the (tree node, bit) decisions of every sub-block mode in the format's sub-block mode tree
BMODE_TREE = {
    D.B_DC: ((0, 0),), D.B_TM: ((0, 1), (1, 0)), D.B_VE: ((0, 1), (1, 1), (2, 0)),
    D.B_HE: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 0)), D.B_RD: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)),
    D.B_VR: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)), D.B_LD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 0)),
    D.B_VL: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)), D.B_HD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)),
    D.B_HU: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1))}


def bit_cost(prob, bit):
    return PROB_COST[(256 - prob if bit else prob) - 1]


# ---- the ten 4x4 predictions at once ----------------------------------------------------------------------------------------------
# The 13 pixels around a sub-block, e[0..3] the left column from the bottom up (L K J I), e[4] the corner X, e[5..12] the row above
# and its continuation to the right (A..H).  Eight of the ten predictors are (a + b + c + d + 2) >> 2 of four of them per pixel:
# avg3(a, b, c) takes (a, b, b, c), avg2(a, b) takes (a, a, b, b), a copy takes the pixel four times.
def _pred_index():
    n = {c: i for i, c in enumerate("LKJIXABCDEFGH")}
    idx = np.zeros((10, 4, 4, 4), np.int64)

    def put(mode, cells, names):
        t = [n[c] for c in names]
        t = (t[0], t[1], t[1], t[2]) if len(t) == 3 else (t[0], t[0], t[1], t[1]) if len(t) == 2 else (t[0],) * 4
        for y, x in cells:
            idx[mode, y, x] = t

    for x in range(4):
        for y in range(4):
            put(D.B_VE, [(y, x)], "XABCDE"[x:x + 3])
            put(D.B_HE, [(y, x)], "XIJKLL"[y:y + 3])
            put(D.B_LD, [(y, x)], "ABCDEFGHH"[x + y:x + y + 3])
            put(D.B_RD, [(y, x)], "LKJIXABCD"[3 + x - y:6 + x - y])
    for cells, names in (([(0, 0), (2, 1)], "XA"), ([(0, 1), (2, 2)], "AB"), ([(0, 2), (2, 3)], "BC"), ([(0, 3)], "CD"),
                         ([(3, 0)], "KJI"), ([(2, 0)], "JIX"), ([(1, 0), (3, 1)], "IXA"), ([(1, 1), (3, 2)], "XAB"),
                         ([(1, 2), (3, 3)], "ABC"), ([(1, 3)], "BCD")):
        put(D.B_VR, cells, names)
    for cells, names in (([(0, 0)], "AB"), ([(0, 1), (2, 0)], "BC"), ([(0, 2), (2, 1)], "CD"), ([(0, 3), (2, 2)], "DE"),
                         ([(1, 0)], "ABC"), ([(1, 1), (3, 0)], "BCD"), ([(1, 2), (3, 1)], "CDE"), ([(1, 3), (3, 2)], "DEF"),
                         ([(2, 3)], "EFG"), ([(3, 3)], "FGH")):
        put(D.B_VL, cells, names)
    for cells, names in (([(0, 0), (1, 2)], "IX"), ([(1, 0), (2, 2)], "JI"), ([(2, 0), (3, 2)], "KJ"), ([(3, 0)], "LK"),
                         ([(0, 3)], "ABC"), ([(0, 2)], "XAB"), ([(0, 1), (1, 3)], "IXA"), ([(1, 1), (2, 3)], "JIX"),
                         ([(2, 1), (3, 3)], "KJI"), ([(3, 1)], "LKJ")):
        put(D.B_HD, cells, names)
    for cells, names in (([(0, 0)], "IJ"), ([(0, 2), (1, 0)], "JK"), ([(1, 2), (2, 0)], "KL"), ([(0, 1)], "IJK"),
                         ([(0, 3), (1, 1)], "JKL"), ([(1, 3), (2, 1)], "KLL"),
                         ([(2, 2), (2, 3), (3, 0), (3, 1), (3, 2), (3, 3)], "L")):
        put(D.B_HU, cells, names)
    return idx


PRED_INDEX = _pred_index()


def subblock_predictions(e):
    """the ten predictions [10,4,4] (in the decoder's mode numbering) from the 13 edge pixels e"""
    p = (e[PRED_INDEX].sum(axis=3) + 2) >> 2
    p[D.B_DC] = (e[0:4].sum() + e[5:9].sum() + 4) >> 3
    p[D.B_TM] = np.clip(e[3::-1, None] + e[None, 5:9] - e[4], 0, 255)
    return p


# ---- the rate side of the 16x16 / B_PRED rule ------------------------------------------------------------------------------------
def level_cost(levels):
    """the coefficient-cost proxy of one block's zigzag-ordered levels, in 1/256 bit: nothing for an empty block; else one bit for
    the block, one for every zero before the last level, and 1 + 2 * bit_length(|v|) for every level v"""
    last = -1
    for i in range(15, -1, -1):
        if levels[i]:
            last = i
            break
    if last < 0:
        return 0
    bits = 1
    for i in range(last + 1):
        v = abs(int(levels[i]))
        bits += 1 + 2 * v.bit_length() if v else 1
    return 256 * bits


def rd_lambda(qi):
    return 3 * R.AC_TABLE[qi] * R.AC_TABLE[qi]


# ---- tokens with their table positions --------------------------------------------------------------------------------------------
def block_tokens(levels, first, kind, ctx, out):
    """R.block_pairs with the position of every probability: appends (index into the 1056 coefficient probabilities, bit), or
    (-probability, bit) for the format's fixed ones; returns 1 if the block has a non-zero level"""
    def at(n, c):
        return ((kind * 8 + R.BANDS[n]) * 3 + c) * 11

    last = -1
    for i in range(15, first - 1, -1):
        if levels[i]:
            last = i
            break
    n = first
    p = at(n, int(ctx))
    out.append((p, int(last >= 0)))
    if last < 0:
        return 0
    while n < 16:
        c = int(levels[n])
        n += 1
        v = abs(c)
        out.append((p + 1, int(v != 0)))
        if v == 0:
            p = at(n, 0)
            continue
        out.append((p + 2, int(v > 1)))
        if v == 1:
            p = at(n, 1)
        else:
            out.append((p + 3, int(v > 4)))
            if v <= 4:
                out.append((p + 4, int(v != 2)))
                if v != 2:
                    out.append((p + 5, int(v == 4)))
            else:
                out.append((p + 6, int(v > 10)))
                if v <= 10:
                    out.append((p + 7, int(v > 6)))
                    if v <= 6:
                        out.append((-159, int(v == 6)))
                    else:
                        out.append((-165, int(v >= 9)))
                        out.append((-145, int(not v & 1)))
                else:
                    if v < 3 + (8 << 1):
                        out += [(p + 8, 0), (p + 9, 0)]
                        v, tab = v - (3 + (8 << 0)), R.CAT3
                    elif v < 3 + (8 << 2):
                        out += [(p + 8, 0), (p + 9, 1)]
                        v, tab = v - (3 + (8 << 1)), R.CAT4
                    elif v < 3 + (8 << 3):
                        out += [(p + 8, 1), (p + 10, 0)]
                        v, tab = v - (3 + (8 << 2)), R.CAT5
                    else:
                        out += [(p + 8, 1), (p + 10, 1)]
                        v, tab = v - (3 + (8 << 3)), R.CAT6
                    for k, pr in enumerate(tab):
                        out.append((-pr, (v >> (len(tab) - 1 - k)) & 1))
            p = at(n, 2)
        out.append((-128, int(c < 0)))
        if n == 16:
            return 1
        out.append((p, int(n <= last)))
        if n > last:
            return 1
    return 1


def adapted_probs(counts):
    """counts [1056][2] of the frame's branch decisions -> (probabilities [1056], update flags [1056])"""
    probs, flags = list(R.COEFF_PROBS), [0] * 1056
    for i in range(1056):
        c0, c1 = int(counts[i][0]), int(counts[i][1])
        if c0 + c1 == 0:
            continue
        old, u = R.COEFF_PROBS[i], R.COEFF_UPDATE_PROBS[i]
        new = min(255, max(1, (255 * c0 + (c0 + c1) // 2) // (c0 + c1)))
        saving = c0 * (PROB_COST[old - 1] - PROB_COST[new - 1]) + c1 * (PROB_COST[255 - old] - PROB_COST[255 - new])
        # an update flag of probability 255 has no entry for its 1: C[256 - 255] = C[1]
        if saving > 8 * 256 + PROB_COST[256 - u - 1] - PROB_COST[u - 1]:
            probs[i], flags[i] = new, 1
    return probs, flags


# ---- the first partition ----------------------------------------------------------------------------------------------------------
def first_pairs(qi, level, log2parts, probs, updated, skip, is_b, bmodes, ymodes, uvmodes):
    """the (probability, bit) pairs of the first partition: the frame header with its probability updates, then per macroblock the
    skip flag, the luma mode (B_PRED: the 16 sub-block modes, each in the context of the modes above and to the left) and the
    chroma mode"""
    out = []

    def bits(value, n):
        out.extend((128, (value >> k) & 1) for k in range(n - 1, -1, -1))

    mbh, mbw = skip.shape
    total, nskip = mbh * mbw, int(np.sum(skip))
    prob_skip = max(1, (total - nskip) * 255 // total)
    bits(0, 3)                        # colour space, clamping needed, no segmentation
    bits(1, 1)                        # simple loop filter
    bits(level, 6)
    bits(0, 4)                        # sharpness, no filter deltas
    bits(log2parts, 2)
    bits(qi, 7)
    bits(0, 6)                        # no quantiser deltas, refresh_entropy_probs 0
    for i in range(1056):
        out.append((R.COEFF_UPDATE_PROBS[i], int(updated[i])))
        if updated[i]:
            bits(int(probs[i]), 8)
    bits(1, 1)                        # mb_no_coeff_skip
    bits(prob_skip, 8)
    for mby in range(mbh):
        for mbx in range(mbw):
            out.append((prob_skip, int(skip[mby, mbx])))
            if is_b[mby, mbx]:
                out.append((R.YMODE_PROBS[0], 0))
                for b in range(16):
                    bx, by = b & 3, b >> 2
                    above = bmodes[mby, mbx, b - 4] if by else (bmodes[mby - 1, mbx, 12 + bx] if mby else D.B_DC)
                    left = bmodes[mby, mbx, b - 1] if bx else (bmodes[mby, mbx - 1, 4 * by + 3] if mbx else D.B_DC)
                    pb = D.KF_BMODE_PROBS[int(above)][int(left)]
                    out.extend((pb[node], bit) for node, bit in BMODE_TREE[int(bmodes[mby, mbx, b])])
            else:
                m = int(ymodes[mby, mbx])
                out += [(R.YMODE_PROBS[0], 1), (R.YMODE_PROBS[1], m >> 1), (R.YMODE_PROBS[3] if m >> 1 else R.YMODE_PROBS[2], m & 1)]
            m = int(uvmodes[mby, mbx])
            out.append((R.UVMODE_PROBS[0], int(m != R.DC_PRED)))
            if m != R.DC_PRED:
                out.append((R.UVMODE_PROBS[1], int(m != R.V_PRED)))
                if m != R.V_PRED:
                    out.append((R.UVMODE_PROBS[2], int(m == R.TM_PRED)))
    return out


# ---- one frame ------------------------------------------------------------------------------------------------------------------
def encode_frame(frame, quality=90):
    """One BGR uint8 frame [H,W,3] -> dict: what R.encode_frame returns ('ymodes' in method 0's numbering, unused where 'is_b'),
    and 'is_b' [mbh,mbw], 'bmodes' [mbh,mbw,16] (the implied mode in 16x16 macroblocks), 'probs' and 'updated' [1056], 'counts'
    [1056,2], 'tokens' (per partition the (index | -probability, bit) list), 'lev_y2' [mbh,mbw,16] the Y2 levels (zeros where
    'is_b')."""
    H, W = frame.shape[:2]
    assert frame.dtype == np.uint8 and frame.shape[2] == 3 and 1 <= H <= R.MAX_SIDE and 1 <= W <= R.MAX_SIDE
    qi = R.quality_to_qi(quality)
    (y1dc, y1ac), (y2dc, y2ac), (uvdc, uvac) = R.quantisers(qi)
    lam = rd_lambda(qi)
    src = R.planes_of(frame)
    Hp, Wp = src[0].shape
    mbh, mbw = Hp // 16, Wp // 16
    # luma with the format's border: row 0 holds 127 (4 columns past the last macroblock too), column 0 holds 129 from row 1 down
    P = np.zeros((Hp + 1, Wp + 5), np.int64)
    P[0, :] = 127
    P[1:, 0] = 129
    rec = [P[1:, 1:Wp + 1], np.zeros_like(src[1]), np.zeros_like(src[2])]
    ymodes, uvmodes = np.zeros((mbh, mbw), np.int64), np.zeros((mbh, mbw), np.int64)
    is_b = np.zeros((mbh, mbw), bool)
    bmodes = np.zeros((mbh, mbw, 16), np.int64)
    inner, skip = np.zeros((mbh, mbw), bool), np.zeros((mbh, mbw), bool)
    lev_y2 = np.zeros((mbh, mbw, 16), np.int64)                      # zigzag order from here on
    lev_y = np.zeros((mbh, mbw, 16, 16), np.int64)
    lev_c = np.zeros((2, mbh, mbw, 4, 16), np.int64)
    zz = R.ZIGZAG
    for mby in range(mbh):
        for mbx in range(mbw):
            ys, xs = slice(16 * mby, 16 * mby + 16), slice(16 * mbx, 16 * mbx + 16)
            s = src[0][ys, xs]
            # the 16x16 candidate, as in method 0
            preds = R.predictions(rec[0], mbx, mby, 16)
            m = int(np.argmin(((preds - s) ** 2).sum(axis=(1, 2))))
            coef = R.fdct(R._blocks(s - preds[m]))
            l2, q2 = R.quantise(R.fwht(coef[:, 0]), y2dc, y2ac)
            dcs = R.iwht(l2 * q2)
            ly, qy = R.quantise(coef, y1ac, y1ac)
            ly[:, 0] = 0
            deq = ly * qy
            deq[:, 0] = dcs
            rec16 = np.clip(preds[m] + R._unblocks(R.idct(deq)), 0, 255)
            l2, ly = l2[zz], ly[:, zz]
            # the B_PRED candidate: 16 sub-blocks in raster order, each reconstructed before the next predicts from it
            x0, y0 = 16 * mbx, 16 * mby
            nb = np.zeros((17, 21), np.int64)
            nb[0] = P[y0, x0:x0 + 21]
            if mby and mbx == mbw - 1:
                nb[0, 17:] = nb[0, 16]
            nb[1:, 0] = P[y0 + 1:y0 + 17, x0]
            nb[[4, 8, 12], 17:] = nb[0, 17:]
            lb, bm = np.zeros((16, 16), np.int64), [0] * 16
            for b in range(16):
                yy, xx = 1 + 4 * (b >> 2), 1 + 4 * (b & 3)
                e = np.concatenate([nb[yy:yy + 4, xx - 1][::-1], nb[yy - 1, xx - 1:xx + 8]])
                sb = s[yy - 1:yy + 3, xx - 1:xx + 3]
                pr = subblock_predictions(e)
                bm[b] = int(np.argmin(((pr - sb) ** 2).sum(axis=(1, 2))))          # the first of equal minima
                lv, q = R.quantise(R.fdct((sb - pr[bm[b]])[None]), y1dc, y1ac)
                nb[yy:yy + 4, xx:xx + 4] = np.clip(pr[bm[b]] + R.idct(lv * q)[0], 0, 255)
                lb[b] = lv[0][zz]
            recb = nb[1:, 1:17]
            # the rule: distortion of the reconstruction plus lambda times (mode bits + level proxy); ties go to 16x16
            r16 = bit_cost(R.YMODE_PROBS[0], 1) + bit_cost(R.YMODE_PROBS[1], m >> 1) + \
                bit_cost(R.YMODE_PROBS[3] if m >> 1 else R.YMODE_PROBS[2], m & 1) + level_cost(l2) + sum(level_cost(v) for v in ly)
            rb = bit_cost(R.YMODE_PROBS[0], 0) + sum(level_cost(v) for v in lb)
            for b in range(16):
                bx, by = b & 3, b >> 2
                above = bm[b - 4] if by else (bmodes[mby - 1, mbx, 12 + bx] if mby else D.B_DC)
                left = bm[b - 1] if bx else (bmodes[mby, mbx - 1, 4 * by + 3] if mbx else D.B_DC)
                pb = D.KF_BMODE_PROBS[int(above)][int(left)]
                rb += sum(bit_cost(pb[node], bit) for node, bit in BMODE_TREE[bm[b]])
            j16 = int(((rec16 - s) ** 2).sum()) + ((lam * r16) >> RD_SHIFT)
            jb = int(((recb - s) ** 2).sum()) + ((lam * rb) >> RD_SHIFT)
            ymodes[mby, mbx] = m
            if jb < j16:
                is_b[mby, mbx] = True
                bmodes[mby, mbx] = bm
                rec[0][ys, xs] = recb
                lev_y[mby, mbx] = lb
                luma_any = bool(lb.any())
            else:
                bmodes[mby, mbx] = IMPLIED[m]
                rec[0][ys, xs] = rec16
                lev_y2[mby, mbx], lev_y[mby, mbx] = l2, ly
                luma_any = bool(l2.any() or ly.any())
            ys, xs = slice(8 * mby, 8 * mby + 8), slice(8 * mbx, 8 * mbx + 8)
            pu, pv = R.predictions(rec[1], mbx, mby, 8), R.predictions(rec[2], mbx, mby, 8)
            sse = ((pu - src[1][ys, xs]) ** 2).sum(axis=(1, 2)) + ((pv - src[2][ys, xs]) ** 2).sum(axis=(1, 2))
            m = int(np.argmin(sse))
            uvmodes[mby, mbx] = m
            for c, pred in ((0, pu[m]), (1, pv[m])):
                lc, qc = R.quantise(R.fdct(R._blocks(src[1 + c][ys, xs] - pred)), uvdc, uvac)
                rec[1 + c][ys, xs] = np.clip(pred + R._unblocks(R.idct(lc * qc)), 0, 255)
                lev_c[c, mby, mbx] = lc[:, zz]
            chroma_any = bool(lev_c[:, mby, mbx].any())
            skip[mby, mbx] = not (luma_any or chroma_any)
            # a decoder filters the inner edges of every B_PRED macroblock; of the others as in method 0
            inner[mby, mbx] = is_b[mby, mbx] or bool(ly.any() or dcs.any() or chroma_any)
    # tokens: macroblock row r goes to partition r % parts; the Y2 context is carried past B_PRED macroblocks
    log2parts = min(3, mbh.bit_length() - 1)
    nparts = 1 << log2parts
    tokens = [[] for _ in range(nparts)]
    top_y, top_c, top_y2 = np.zeros(4 * mbw, np.int64), np.zeros((2, 2 * mbw), np.int64), np.zeros(mbw, np.int64)
    for mby in range(mbh):
        out = tokens[mby % nparts]
        left_y, left_c, left_y2 = np.zeros(4, np.int64), np.zeros((2, 2), np.int64), 0
        for mbx in range(mbw):
            b_pred = is_b[mby, mbx]
            if skip[mby, mbx]:
                left_y[:], left_c[:] = 0, 0
                top_y[4 * mbx:4 * mbx + 4], top_c[:, 2 * mbx:2 * mbx + 2] = 0, 0
                if not b_pred:
                    left_y2 = top_y2[mbx] = 0
                continue
            if not b_pred:
                left_y2 = top_y2[mbx] = block_tokens(lev_y2[mby, mbx], 0, 1, left_y2 + top_y2[mbx], out)
            for by in range(4):
                for bx in range(4):
                    nz = block_tokens(lev_y[mby, mbx, 4 * by + bx], 0 if b_pred else 1, 3 if b_pred else 0,
                                      left_y[by] + top_y[4 * mbx + bx], out)
                    left_y[by] = top_y[4 * mbx + bx] = nz
            for c in range(2):
                for by in range(2):
                    for bx in range(2):
                        nz = block_tokens(lev_c[c, mby, mbx, 2 * by + bx], 0, 2, left_c[c, by] + top_c[c, 2 * mbx + bx], out)
                        left_c[c, by] = top_c[c, 2 * mbx + bx] = nz
    counts = np.zeros((1056, 2), np.int64)
    for part in tokens:
        for i, bit in part:
            if i >= 0:
                counts[i, bit] += 1
    probs, updated = adapted_probs(counts)
    parts = [R.code_pairs([(probs[i] if i >= 0 else -i, bit) for i, bit in part]) for part in tokens]
    level = R.filter_level(qi)
    first = R.code_pairs(first_pairs(qi, level, log2parts, probs, updated, skip, is_b, bmodes, ymodes, uvmodes))
    return {'vp8': R.vp8_frame(first, parts, W, H), 'first': first, 'parts': parts, 'ymodes': ymodes, 'uvmodes': uvmodes,
            'is_b': is_b, 'bmodes': bmodes, 'planes': (np.array(rec[0]), rec[1], rec[2]), 'inner': inner, 'level': level,
            'skip': skip, 'probs': probs, 'updated': updated, 'counts': counts, 'tokens': tokens, 'lev_y2': lev_y2}


def encode(frames, quality=90):
    """the still .webp file of every frame"""
    return [R.still_file(encode_frame(f, quality)['vp8']) for f in frames]


def encode_animation(frames, quality=90, fps=25, loop=0, order=None):
    H, W = frames[0].shape[:2]
    return R.animation_file([encode_frame(f, quality)['vp8'] for f in frames], W, H, fps, loop, order)
