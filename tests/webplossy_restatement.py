"""The lossy WebP decoder's contract restated in pure Python / numpy: a VP8 key-frame decoder (RFC 6386) and the
ALPH chunk's decoder, written from the format and not from the kernels, in the order a reader of the RFC would write them: whole
frame parsed to symbols first, then reconstruction in raster order, then the loop filter in raster order, then libwebp's chroma
upsampling and colour conversion.  tests/test_webplossy.py holds this text to libwebp (Pillow) on every decoded byte and the device
code (csrc/webplossy.hip) to the same files.

    parse(vp8)           the frame's symbols: header fields, per-macroblock modes and quantised levels (what a transcoder needs)
    decode(file)         (B, G, R, A uint8 [H,W,4], report); report says what the file held (modes, segments, partitions, ...)
    container(file)      the VP8 and ALPH chunks of a still file

The tables shared with the writer's restatement (coefficient probabilities, quantiser steps, zigzag, bands) come from there."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as E  # noqa: E402
import webpdec_restatement as LL  # noqa: E402

# sub-block modes, numbered as the leaves of the format's mode tree from left to right
B_DC, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU = range(10)
DC_PRED, TM_PRED, V_PRED, H_PRED = 0, 1, 2, 3                 # whole-block modes, numbered like the sub-block modes they imply

# key-frame sub-block mode probabilities [mode above][mode to the left][tree node], modes in the numbering above
KF_BMODE_PROBS = np.array([
    231, 120, 48, 89, 115, 113, 120, 152, 112, 152, 179, 64, 126, 170, 118, 46, 70, 95, 175, 69, 143, 80, 85, 82, 72, 155, 103, 56, 58, 10, 171, 218, 189, 17, 13, 152, 114, 26, 17, 163, 44, 195, 21, 10, 173,
    121, 24, 80, 195, 26, 62, 44, 64, 85, 144, 71, 10, 38, 171, 213, 144, 34, 26, 170, 46, 55, 19, 136, 160, 33, 206, 71, 63, 20, 8, 114, 114, 208, 12, 9, 226, 81, 40, 11, 96, 182, 84, 29, 16, 36,
    134, 183, 89, 137, 98, 101, 106, 165, 148, 72, 187, 100, 130, 157, 111, 32, 75, 80, 66, 102, 167, 99, 74, 62, 40, 234, 128, 41, 53, 9, 178, 241, 141, 26, 8, 107, 74, 43, 26, 146, 73, 166, 49, 23, 157,
    65, 38, 105, 160, 51, 52, 31, 115, 128, 104, 79, 12, 27, 217, 255, 87, 17, 7, 87, 68, 71, 44, 114, 51, 15, 186, 23, 47, 41, 14, 110, 182, 183, 21, 17, 194, 66, 45, 25, 102, 197, 189, 23, 18, 22,
    88, 88, 147, 150, 42, 46, 45, 196, 205, 43, 97, 183, 117, 85, 38, 35, 179, 61, 39, 53, 200, 87, 26, 21, 43, 232, 171, 56, 34, 51, 104, 114, 102, 29, 93, 77, 39, 28, 85, 171, 58, 165, 90, 98, 64,
    34, 22, 116, 206, 23, 34, 43, 166, 73, 107, 54, 32, 26, 51, 1, 81, 43, 31, 68, 25, 106, 22, 64, 171, 36, 225, 114, 34, 19, 21, 102, 132, 188, 16, 76, 124, 62, 18, 78, 95, 85, 57, 50, 48, 51,
    193, 101, 35, 159, 215, 111, 89, 46, 111, 60, 148, 31, 172, 219, 228, 21, 18, 111, 112, 113, 77, 85, 179, 255, 38, 120, 114, 40, 42, 1, 196, 245, 209, 10, 25, 109, 88, 43, 29, 140, 166, 213, 37, 43, 154,
    61, 63, 30, 155, 67, 45, 68, 1, 209, 100, 80, 8, 43, 154, 1, 51, 26, 71, 142, 78, 78, 16, 255, 128, 34, 197, 171, 41, 40, 5, 102, 211, 183, 4, 1, 221, 51, 50, 17, 168, 209, 192, 23, 25, 82,
    138, 31, 36, 171, 27, 166, 38, 44, 229, 67, 87, 58, 169, 82, 115, 26, 59, 179, 63, 59, 90, 180, 59, 166, 93, 73, 154, 40, 40, 21, 116, 143, 209, 34, 39, 175, 47, 15, 16, 183, 34, 223, 49, 45, 183,
    46, 17, 33, 183, 6, 98, 15, 32, 183, 57, 46, 22, 24, 128, 1, 54, 17, 37, 65, 32, 73, 115, 28, 128, 23, 128, 205, 40, 3, 9, 115, 51, 192, 18, 6, 223, 87, 37, 9, 115, 59, 77, 64, 21, 47,
    104, 55, 44, 218, 9, 54, 53, 130, 226, 64, 90, 70, 205, 40, 41, 23, 26, 57, 54, 57, 112, 184, 5, 41, 38, 166, 213, 30, 34, 26, 133, 152, 116, 10, 32, 134, 39, 19, 53, 221, 26, 114, 32, 73, 255,
    31, 9, 65, 234, 2, 15, 1, 118, 73, 75, 32, 12, 51, 192, 255, 160, 43, 51, 88, 31, 35, 67, 102, 85, 55, 186, 85, 56, 21, 23, 111, 59, 205, 45, 37, 192, 55, 38, 70, 124, 73, 102, 1, 34, 98,
    125, 98, 42, 88, 104, 85, 117, 175, 82, 95, 84, 53, 89, 128, 100, 113, 101, 45, 75, 79, 123, 47, 51, 128, 81, 171, 1, 57, 17, 5, 71, 102, 57, 53, 41, 49, 38, 33, 13, 121, 57, 73, 26, 1, 85,
    41, 10, 67, 138, 77, 110, 90, 47, 114, 115, 21, 2, 10, 102, 255, 166, 23, 6, 101, 29, 16, 10, 85, 128, 101, 196, 26, 57, 18, 10, 102, 102, 213, 34, 20, 43, 117, 20, 15, 36, 163, 128, 68, 1, 26,
    102, 61, 71, 37, 34, 53, 31, 243, 192, 69, 60, 71, 38, 73, 119, 28, 222, 37, 68, 45, 128, 34, 1, 47, 11, 245, 171, 62, 17, 19, 70, 146, 85, 55, 62, 70, 37, 43, 37, 154, 100, 163, 85, 160, 1,
    63, 9, 92, 136, 28, 64, 32, 201, 85, 75, 15, 9, 9, 64, 255, 184, 119, 16, 86, 6, 28, 5, 64, 255, 25, 248, 1, 56, 8, 17, 132, 137, 255, 55, 116, 128, 58, 15, 20, 82, 135, 57, 26, 121, 40,
    164, 50, 31, 137, 154, 133, 25, 35, 218, 51, 103, 44, 131, 131, 123, 31, 6, 158, 86, 40, 64, 135, 148, 224, 45, 183, 128, 22, 26, 17, 131, 240, 154, 14, 1, 209, 45, 16, 21, 91, 64, 222, 7, 1, 197,
    56, 21, 39, 155, 60, 138, 23, 102, 213, 83, 12, 13, 54, 192, 255, 68, 47, 28, 85, 26, 85, 85, 128, 128, 32, 146, 171, 18, 11, 7, 63, 144, 171, 4, 4, 246, 35, 27, 10, 146, 174, 171, 12, 26, 128,
    190, 80, 35, 99, 180, 80, 126, 54, 45, 85, 126, 47, 87, 176, 51, 41, 20, 32, 101, 75, 128, 139, 118, 146, 116, 128, 85, 56, 41, 15, 176, 236, 85, 37, 9, 62, 71, 30, 17, 119, 118, 255, 17, 18, 138,
    101, 38, 60, 138, 55, 70, 43, 26, 142, 146, 36, 19, 30, 171, 255, 97, 27, 20, 138, 45, 61, 62, 219, 1, 81, 188, 64, 32, 41, 20, 117, 151, 142, 20, 21, 163, 112, 19, 12, 61, 195, 128, 48, 4, 24,
], np.int64).reshape(10, 10, 9).tolist()

CATS = [E.CAT3, E.CAT4, E.CAT5, E.CAT6]


class Corrupt(ValueError):
    pass


# ---- the boolean decoder --------------------------------------------------------------------------------------------------------
class BoolDecoder:
    """The format's boolean decoder, one input byte at a time and only when the next decision needs it, so that `pos` is the
    number of bytes the decisions so far depend on.  Bytes past the end read as zero and set `past`."""

    def __init__(self, data):
        self.data, self.pos, self.value, self.range, self.bits, self.past = data, 0, 0, 255, -8, False

    def bit(self, prob):
        while self.bits < 0:
            if self.pos < len(self.data):
                self.value = (self.value << 8) | self.data[self.pos]
            else:
                self.value <<= 8
                self.past = True
            self.pos += 1
            self.bits += 8
        split = 1 + (((self.range - 1) * prob) >> 8)
        if (self.value >> self.bits) >= split:
            self.value -= split << self.bits
            self.range -= split
            b = 1
        else:
            self.range = split
            b = 0
        while self.range < 128:
            self.range <<= 1
            self.bits -= 1
        return b

    def used(self):
        """the bytes that hold the bits shifted out so far and the 8 behind them"""
        return min(len(self.data), (8 * self.pos - 8 - self.bits + 15) >> 3)

    def literal(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit(128)
        return v

    def signed(self, n):
        v = self.literal(n)
        return -v if self.bit(128) else v

    def optional_signed(self, n):
        return self.signed(n) if self.bit(128) else 0


# ---- the frame's symbols ----------------------------------------------------------------------------------------------------------
def _s16(v):
    return ((int(v) + 32768) & 65535) - 32768


def read_header(d):
    h = {'colour_space': d.literal(1), 'clamp': d.literal(1)}
    h['segmentation'] = d.literal(1)
    h['update_map'] = h['update_data'] = 0
    h['absolute'] = 1                      # what libwebp starts from: a map without a data update means quantiser 0 and level 0, absolute
    h['seg_quant'], h['seg_level'], h['seg_probs'] = [0] * 4, [0] * 4, [255] * 3
    if h['segmentation']:
        h['update_map'], h['update_data'] = d.literal(1), d.literal(1)
        if h['update_data']:
            h['absolute'] = d.literal(1)
            h['seg_quant'] = [d.optional_signed(7) for _ in range(4)]
            h['seg_level'] = [d.optional_signed(6) for _ in range(4)]
        if h['update_map']:
            h['seg_probs'] = [d.literal(8) if d.literal(1) else 255 for _ in range(3)]
    h['simple'], h['level'], h['sharpness'] = d.literal(1), d.literal(6), d.literal(3)
    h['lf_delta'] = d.literal(1)
    h['ref_lf_delta'], h['mode_lf_delta'], h['lf_delta_update'] = [0] * 4, [0] * 4, 0
    if h['lf_delta']:
        h['lf_delta_update'] = d.literal(1)
        if h['lf_delta_update']:
            h['ref_lf_delta'] = [d.optional_signed(6) for _ in range(4)]
            h['mode_lf_delta'] = [d.optional_signed(6) for _ in range(4)]
    h['log2parts'] = d.literal(2)
    h['qi'] = d.literal(7)
    h['qdelta'] = [d.optional_signed(4) for _ in range(5)]          # y1 dc, y2 dc, y2 ac, uv dc, uv ac
    h['refresh_entropy'] = d.literal(1)
    probs, updates = list(E.COEFF_PROBS), 0
    for i, up in enumerate(E.COEFF_UPDATE_PROBS):
        if d.bit(up):
            probs[i] = d.literal(8)
            updates += 1
    h['probs'], h['prob_updates'] = np.array(probs, np.int64).reshape(4, 8, 3, 11).tolist(), updates
    h['use_skip'] = d.literal(1)
    h['prob_skip'] = d.literal(8) if h['use_skip'] else 0
    return h


def read_bmode(d, p):
    if not d.bit(p[0]):
        return B_DC
    if not d.bit(p[1]):
        return B_TM
    if not d.bit(p[2]):
        return B_VE
    if not d.bit(p[3]):
        if not d.bit(p[4]):
            return B_HE
        return B_VR if d.bit(p[5]) else B_RD
    if not d.bit(p[6]):
        return B_LD
    if not d.bit(p[7]):
        return B_VL
    return B_HU if d.bit(p[8]) else B_HD


def read_block(d, probs, kind, ctx, first, cats):
    """one block's tokens -> (levels [16] in zigzag positions, the position behind the last token read)"""
    lev = [0] * 16
    n = first
    p = probs[kind][E.BANDS[n]][ctx]
    while n < 16:
        if not d.bit(p[0]):
            return lev, n
        while not d.bit(p[1]):
            n += 1
            if n == 16:
                return lev, 16
            p = probs[kind][E.BANDS[n]][0]
        nxt = probs[kind][E.BANDS[n + 1]]
        if not d.bit(p[2]):
            v, p = 1, nxt[1]
        else:
            if not d.bit(p[3]):
                v = 2 if not d.bit(p[4]) else 3 + d.bit(p[5])
            elif not d.bit(p[6]):
                if not d.bit(p[7]):
                    v = 5 + d.bit(159)
                else:
                    v = 7 + 2 * d.bit(165)
                    v += d.bit(145)
                cats.add(1 if v < 7 else 2)
            else:
                b1 = d.bit(p[8])
                cat = 2 * b1 + d.bit(p[9 + b1])
                v = 0
                for pr in CATS[cat]:
                    v = 2 * v + d.bit(pr)
                v += 3 + (8 << cat)
                cats.add(3 + cat)
            p = nxt[2]
        lev[n] = -v if d.bit(128) else v
        n += 1
    return lev, 16


def split_frame(vp8):
    """the plain bytes of a key frame: (width, height, version, the first partition's bytes, the offset behind them)"""
    if len(vp8) < 10:
        raise Corrupt("a frame of %d bytes" % len(vp8))
    tag = vp8[0] | vp8[1] << 8 | vp8[2] << 16
    if tag & 1 or not (tag >> 4) & 1 or (tag >> 1) & 7 > 3:
        raise Corrupt("not a shown key frame")
    if vp8[3:6] != b'\x9d\x01\x2a':
        raise Corrupt("start code")
    w, h = struct.unpack('<HH', vp8[6:10])
    if (w | h) >> 14:
        raise Corrupt("scaling")
    size = tag >> 5
    if 10 + size > len(vp8):
        raise Corrupt("first partition")
    return w, h, (tag >> 1) & 7, vp8[10:10 + size], 10 + size


def parse(vp8):
    """The symbols of a key frame.  Returns a dict: 'width', 'height', 'version', 'header' (read_header), and per macroblock
    [mbh][mbw]: 'segment', 'skip', 'is_b', 'ymode', 'bmodes' ([16]), 'uvmode', 'levels' ([25][16] quantised levels in zigzag
    positions: 16 luma, 4 U, 4 V, Y2), 'ends' ([25], the position behind each block's last token); 'used': bytes read of the
    first partition and of every token partition; 'past': any read behind a partition's end; 'cats': token categories met."""
    vp8 = bytes(vp8)
    W, H, version, first, p = split_frame(vp8)
    d = BoolDecoder(first)
    hdr = read_header(d)
    nparts = 1 << hdr['log2parts']
    if p + 3 * (nparts - 1) > len(vp8):
        raise Corrupt("partition sizes")
    sizes = [int.from_bytes(vp8[p + 3 * i:p + 3 * i + 3], 'little') for i in range(nparts - 1)]
    p += 3 * (nparts - 1)
    parts = []
    for s in sizes:
        parts.append(vp8[p:p + s])                                  # a size past the end gives a short partition, as libwebp takes it
        p += s
    parts.append(vp8[p:])
    toks = [BoolDecoder(b) for b in parts]
    mbw, mbh = (W + 15) >> 4, (H + 15) >> 4
    out = {'width': W, 'height': H, 'version': version, 'header': hdr, 'mbw': mbw, 'mbh': mbh, 'nparts': nparts, 'cats': set()}
    mbs = [[None] * mbw for _ in range(mbh)]
    top_modes = [B_DC] * (4 * mbw)
    top_nz = [[0] * 9 for _ in range(mbw)]                           # 4 luma, 2 U, 2 V, Y2
    probs = hdr['probs']
    for mby in range(mbh):
        t = toks[mby & (nparts - 1)]
        left_modes, left_nz = [B_DC] * 4, [0] * 9
        for mbx in range(mbw):
            m = {'segment': 0}
            if hdr['update_map']:
                sp = hdr['seg_probs']
                m['segment'] = (2 + d.bit(sp[2])) if d.bit(sp[0]) else d.bit(sp[1])
            m['skip'] = d.bit(hdr['prob_skip']) if hdr['use_skip'] else 0
            m['is_b'] = 1 - d.bit(145)
            if m['is_b']:
                bm = []
                for by in range(4):
                    for bx in range(4):
                        mode = read_bmode(d, KF_BMODE_PROBS[top_modes[4 * mbx + bx]][left_modes[by]])
                        top_modes[4 * mbx + bx] = left_modes[by] = mode
                        bm.append(mode)
                m['bmodes'], m['ymode'] = bm, -1
            else:
                ym = (TM_PRED if d.bit(128) else H_PRED) if d.bit(156) else (V_PRED if d.bit(163) else DC_PRED)
                m['ymode'], m['bmodes'] = ym, [ym] * 16
                top_modes[4 * mbx:4 * mbx + 4] = [ym] * 4
                left_modes = [ym] * 4
            m['uvmode'] = DC_PRED if not d.bit(142) else V_PRED if not d.bit(114) else TM_PRED if d.bit(183) else H_PRED
            levels, ends = [[0] * 16 for _ in range(25)], [0] * 25
            tn = top_nz[mbx]
            if m['skip']:
                for k in range(8):
                    tn[k] = left_nz[k] = 0
                if not m['is_b']:
                    tn[8] = left_nz[8] = 0
            else:
                first_pos, kind = 0, 3
                if not m['is_b']:
                    levels[24], ends[24] = read_block(t, probs, 1, tn[8] + left_nz[8], 0, out['cats'])
                    tn[8] = left_nz[8] = int(ends[24] > 0)
                    first_pos, kind = 1, 0
                for by in range(4):
                    for bx in range(4):
                        k = 4 * by + bx
                        levels[k], ends[k] = read_block(t, probs, kind, tn[bx] + left_nz[by], first_pos, out['cats'])
                        tn[bx] = left_nz[by] = int(ends[k] > first_pos)
                for c in range(2):
                    for by in range(2):
                        for bx in range(2):
                            k = 16 + 4 * c + 2 * by + bx
                            levels[k], ends[k] = read_block(t, probs, 2, tn[4 + 2 * c + bx] + left_nz[4 + 2 * c + by], 0, out['cats'])
                            tn[4 + 2 * c + bx] = left_nz[4 + 2 * c + by] = int(ends[k] > 0)
            m['levels'], m['ends'] = levels, ends
            mbs[mby][mbx] = m
    out['mbs'] = mbs
    out['used'] = [d.used()] + [t.used() for t in toks]
    out['past'] = d.past or any(t.past for t in toks)
    out['part_sizes'] = [len(first)] + [len(b) for b in parts]
    return out


# ---- quantisers and filter strengths -----------------------------------------------------------------------------------------------
def _clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def segment_quantisers(hdr):
    """per segment ((y1 dc, y1 ac), (y2 dc, y2 ac), (uv dc, uv ac)) and the quantiser index itself"""
    out = []
    for s in range(4):
        q = hdr['qi']
        if hdr['segmentation']:
            q = hdr['seg_quant'][s] + (0 if hdr['absolute'] else hdr['qi'])
        dq = hdr['qdelta']
        y2ac = (E.AC_TABLE[_clip(q + dq[2], 0, 127)] * 101581) >> 16
        out.append(((E.DC_TABLE[_clip(q + dq[0], 0, 127)], E.AC_TABLE[_clip(q, 0, 127)]),
                    (2 * E.DC_TABLE[_clip(q + dq[1], 0, 127)], max(8, y2ac)),
                    (E.DC_TABLE[_clip(q + dq[3], 0, 117)], E.AC_TABLE[_clip(q + dq[4], 0, 127)]), q))
    return out


def filter_strength(hdr, segment, is_b):
    """(limit, inner limit, hev threshold) of a macroblock; limit 0: not filtered"""
    level = hdr['level']
    if hdr['segmentation']:
        level = hdr['seg_level'][segment] + (0 if hdr['absolute'] else hdr['level'])
    if hdr['lf_delta']:
        level += hdr['ref_lf_delta'][0]
        if is_b:
            level += hdr['mode_lf_delta'][0]
    level = _clip(level, 0, 63)
    if level == 0:
        return 0, 0, 0
    inner = level
    if hdr['sharpness'] > 0:
        inner >>= 2 if hdr['sharpness'] > 4 else 1
        inner = min(inner, 9 - hdr['sharpness'])
    inner = max(inner, 1)
    return 2 * level + inner, inner, 2 if level >= 40 else 1 if level >= 15 else 0


# ---- reconstruction ---------------------------------------------------------------------------------------------------------------
def _avg3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def _avg2(a, b):
    return (a + b + 1) >> 1


def subblock_prediction(mode, X, T, Lf):
    """4x4 prediction [row][column] from the pixel above-left X, the 8 above and above-right T, the 4 to the left Lf"""
    A, B, C, D, Ee, F, G, Hh = (int(v) for v in T)
    I, J, K, L = (int(v) for v in Lf)
    X = int(X)
    p = np.zeros((4, 4), np.int64)
    if mode == B_DC:
        p[:] = (A + B + C + D + I + J + K + L + 4) >> 3
    elif mode == B_TM:
        p[:] = np.clip(np.array([I, J, K, L])[:, None] + np.array([A, B, C, D])[None, :] - X, 0, 255)
    elif mode == B_VE:
        p[:] = [_avg3(X, A, B), _avg3(A, B, C), _avg3(B, C, D), _avg3(C, D, Ee)]
    elif mode == B_HE:
        p[:] = np.array([_avg3(X, I, J), _avg3(I, J, K), _avg3(J, K, L), _avg3(K, L, L)])[:, None]
    elif mode == B_LD:
        t = [A, B, C, D, Ee, F, G, Hh, Hh]
        for y in range(4):
            for x in range(4):
                p[y, x] = _avg3(t[x + y], t[x + y + 1], t[x + y + 2])
    elif mode == B_RD:
        e = [L, K, J, I, X, A, B, C, D]
        for y in range(4):
            for x in range(4):
                p[y, x] = _avg3(e[3 + x - y], e[4 + x - y], e[5 + x - y])
    elif mode == B_VR:
        p[0, 0] = p[2, 1] = _avg2(X, A)
        p[0, 1] = p[2, 2] = _avg2(A, B)
        p[0, 2] = p[2, 3] = _avg2(B, C)
        p[0, 3] = _avg2(C, D)
        p[3, 0] = _avg3(K, J, I)
        p[2, 0] = _avg3(J, I, X)
        p[1, 0] = p[3, 1] = _avg3(I, X, A)
        p[1, 1] = p[3, 2] = _avg3(X, A, B)
        p[1, 2] = p[3, 3] = _avg3(A, B, C)
        p[1, 3] = _avg3(B, C, D)
    elif mode == B_VL:
        p[0, 0] = _avg2(A, B)
        p[0, 1] = p[2, 0] = _avg2(B, C)
        p[0, 2] = p[2, 1] = _avg2(C, D)
        p[0, 3] = p[2, 2] = _avg2(D, Ee)
        p[1, 0] = _avg3(A, B, C)
        p[1, 1] = p[3, 0] = _avg3(B, C, D)
        p[1, 2] = p[3, 1] = _avg3(C, D, Ee)
        p[1, 3] = p[3, 2] = _avg3(D, Ee, F)
        p[2, 3] = _avg3(Ee, F, G)
        p[3, 3] = _avg3(F, G, Hh)
    elif mode == B_HD:
        p[0, 0] = p[1, 2] = _avg2(I, X)
        p[1, 0] = p[2, 2] = _avg2(J, I)
        p[2, 0] = p[3, 2] = _avg2(K, J)
        p[3, 0] = _avg2(L, K)
        p[0, 3] = _avg3(A, B, C)
        p[0, 2] = _avg3(X, A, B)
        p[0, 1] = p[1, 3] = _avg3(I, X, A)
        p[1, 1] = p[2, 3] = _avg3(J, I, X)
        p[2, 1] = p[3, 3] = _avg3(K, J, I)
        p[3, 1] = _avg3(L, K, J)
    else:
        p[0, 0] = _avg2(I, J)
        p[0, 2] = p[1, 0] = _avg2(J, K)
        p[1, 2] = p[2, 0] = _avg2(K, L)
        p[0, 1] = _avg3(I, J, K)
        p[0, 3] = p[1, 1] = _avg3(J, K, L)
        p[1, 3] = p[2, 1] = _avg3(K, L, L)
        p[2, 2] = p[2, 3] = p[3, 0] = p[3, 1] = p[3, 2] = p[3, 3] = L
    return p


def block_prediction(P, x0, y0, size, mode):
    """whole-block prediction on the bordered plane P (row 0 holds 127, column 0 holds 129; pixel (x, y) is P[y + 1, x + 1])"""
    top, left, tl = P[y0, x0 + 1:x0 + 1 + size], P[y0 + 1:y0 + 1 + size, x0], P[y0, x0]
    if mode == DC_PRED:
        sh = 3 if size == 8 else 4
        if x0 and y0:
            dc = (top.sum() + left.sum() + size) >> (sh + 1)
        elif y0:
            dc = (top.sum() + (size >> 1)) >> sh
        elif x0:
            dc = (left.sum() + (size >> 1)) >> sh
        else:
            dc = 128
        return np.full((size, size), dc, np.int64)
    if mode == V_PRED:
        return np.broadcast_to(top, (size, size))
    if mode == H_PRED:
        return np.broadcast_to(left[:, None], (size, size))
    return np.clip(left[:, None] + top[None, :] - tl, 0, 255)


def _dequant(levels, dc, ac):
    """zigzag-positioned levels -> raster-ordered coefficients, kept in 16 bits as the format's decoders keep them"""
    c = np.zeros(16, np.int64)
    for n, v in enumerate(levels):
        if v:
            c[E.ZIGZAG[n]] = _s16(v * (dc if n == 0 else ac))
    return c


def _bordered(h, w):
    P = np.zeros((h + 1, w + 1), np.int64)
    P[0, :] = 127
    P[1:, 0] = 129
    return P


def reconstruct(f, report):
    """the unfiltered planes (bordered) and per macroblock the coefficients [25,16] and the inner-edge flag"""
    hdr, mbw, mbh = f['header'], f['mbw'], f['mbh']
    quants = segment_quantisers(hdr)
    Y, U, V = _bordered(16 * mbh, 16 * mbw), _bordered(8 * mbh, 8 * mbw), _bordered(8 * mbh, 8 * mbw)
    coefs = np.zeros((mbh, mbw, 25, 16), np.int64)
    inner = np.zeros((mbh, mbw), bool)
    for mby in range(mbh):
        for mbx in range(mbw):
            m = f['mbs'][mby][mbx]
            (y1dc, y1ac), (y2dc, y2ac), (uvdc, uvac), qidx = quants[m['segment']]
            report['segment_qi'].add(qidx)
            report['segments'].add(m['segment'])
            c = coefs[mby, mbx]
            nonzero = False
            if not m['skip']:
                for k in range(16):
                    c[k] = _dequant(m['levels'][k], y1dc, y1ac)
                for k in range(16, 24):
                    c[k] = _dequant(m['levels'][k], uvdc, uvac)
                if not m['is_b']:
                    c[24] = _dequant(m['levels'][24], y2dc, y2ac)
                    dcs = E.iwht(c[24])
                    c[:16, 0] = [_s16(v) for v in dcs]
                for k in range(24):
                    e = m['ends'][k]
                    nonzero = nonzero or e > 1 or (c[k, 0] != 0 if k < 16 else e > 0)
            else:
                report['skipped'] += 1
            # an inner edge is filtered in a sub-block macroblock, and wherever a coefficient was coded
            inner[mby, mbx] = bool(m['is_b'] or nonzero)
            x0, y0 = 16 * mbx, 16 * mby
            if m['is_b']:
                if mby == 0:
                    tr = np.full(4, 127, np.int64)
                elif mbx == mbw - 1:
                    tr = np.full(4, Y[y0, x0 + 16], np.int64)
                else:
                    tr = Y[y0, x0 + 17:x0 + 21].copy()
                for by in range(4):
                    for bx in range(4):
                        xx, yy = x0 + 4 * bx, y0 + 4 * by
                        T = np.concatenate([Y[yy, xx + 1:xx + 5], tr if bx == 3 else Y[yy, xx + 5:xx + 9]])
                        mode = m['bmodes'][4 * by + bx]
                        report['bmodes'].add(mode)
                        pred = subblock_prediction(mode, Y[yy, xx], T, Y[yy + 1:yy + 5, xx])
                        Y[yy + 1:yy + 5, xx + 1:xx + 5] = np.clip(pred + E.idct(c[4 * by + bx])[0], 0, 255)
            else:
                report['ymodes'].add(m['ymode'])
                pred = block_prediction(Y, x0, y0, 16, m['ymode'])
                Y[y0 + 1:y0 + 17, x0 + 1:x0 + 17] = np.clip(pred + E._unblocks(E.idct(c[:16])), 0, 255)
            report['uvmodes'].add(m['uvmode'])
            x0, y0 = 8 * mbx, 8 * mby
            for P, k0 in ((U, 16), (V, 20)):
                pred = block_prediction(P, x0, y0, 8, m['uvmode'])
                P[y0 + 1:y0 + 9, x0 + 1:x0 + 9] = np.clip(pred + E._unblocks(E.idct(c[k0:k0 + 4])), 0, 255)
    return (Y, U, V), coefs, inner


# ---- the loop filter --------------------------------------------------------------------------------------------------------------
def _edge(P, pos, lo, hi, vertical):
    """views of the 8 lines of pixels across an edge: p3, p2, p1, p0, q0, q1, q2, q3; a vertical edge stands left of column `pos`"""
    if vertical:
        return [P[lo:hi, pos + k] for k in range(-4, 4)]
    return [P[pos + k, lo:hi] for k in range(-4, 4)]


def _common(p1, p0, q0, q1, use_outer):
    """the filters' shared term: three times the step across the edge, plus the clamped outer difference where it is used"""
    return 3 * (q0 - p0) + (np.clip(p1 - q1, -128, 127) if use_outer else 0)


def filter_simple(v, limit):
    p1, p0, q0, q1 = (t.copy() for t in v[2:6])
    on = 4 * np.abs(p0 - q0) + np.abs(p1 - q1) <= 2 * limit + 1
    a = _common(p1, p0, q0, q1, True)
    f1, f2 = np.clip((a + 4) >> 3, -16, 15), np.clip((a + 3) >> 3, -16, 15)
    v[3][...] = np.where(on, np.clip(p0 + f2, 0, 255), p0)
    v[4][...] = np.where(on, np.clip(q0 - f1, 0, 255), q0)


def filter_normal(v, limit, inner_limit, hev_thr, mb_edge):
    p3, p2, p1, p0, q0, q1, q2, q3 = (t.copy() for t in v)
    on = 4 * np.abs(p0 - q0) + np.abs(p1 - q1) <= 2 * limit + 1
    for a, b in ((p3, p2), (p2, p1), (p1, p0), (q3, q2), (q2, q1), (q1, q0)):
        on &= np.abs(a - b) <= inner_limit
    hev = (np.abs(p1 - p0) > hev_thr) | (np.abs(q1 - q0) > hev_thr)
    # high edge variance: only the two pixels at the edge move
    a = _common(p1, p0, q0, q1, True)
    f1, f2 = np.clip((a + 4) >> 3, -16, 15), np.clip((a + 3) >> 3, -16, 15)
    h_p0, h_q0 = np.clip(p0 + f2, 0, 255), np.clip(q0 - f1, 0, 255)
    new = [p3, p2, p1, p0, q0, q1, q2, q3]
    if mb_edge:
        w = np.clip(a, -128, 127)
        a1, a2, a3 = (27 * w + 63) >> 7, (18 * w + 63) >> 7, (9 * w + 63) >> 7
        low = [p3, np.clip(p2 + a3, 0, 255), np.clip(p1 + a2, 0, 255), np.clip(p0 + a1, 0, 255),
               np.clip(q0 - a1, 0, 255), np.clip(q1 - a2, 0, 255), np.clip(q2 - a3, 0, 255), q3]
    else:
        a = _common(p1, p0, q0, q1, False)
        f1, f2 = np.clip((a + 4) >> 3, -16, 15), np.clip((a + 3) >> 3, -16, 15)
        f3 = (f1 + 1) >> 1
        low = [p3, p2, np.clip(p1 + f3, 0, 255), np.clip(p0 + f2, 0, 255), np.clip(q0 - f1, 0, 255), np.clip(q1 - f3, 0, 255), q2, q3]
    high = [p3, p2, p1, h_p0, h_q0, q1, q2, q3]
    for k in range(1, 7):
        v[k][...] = np.where(on, np.where(hev, high[k], low[k]), new[k])


def loop_filter(f, planes, inner, report):
    """in place on the bordered planes, macroblocks in raster order"""
    hdr = f['header']
    report['filter'] = 'none' if hdr['level'] == 0 else 'simple' if hdr['simple'] else 'normal'
    if hdr['level'] == 0:                                           # the frame's level switches the filter off, whatever the segments say
        return
    Y, U, V = planes
    for mby in range(f['mbh']):
        for mbx in range(f['mbw']):
            m = f['mbs'][mby][mbx]
            limit, ilimit, hev = filter_strength(hdr, m['segment'], m['is_b'])
            if limit == 0:
                continue
            report['hev'].add(hev)
            report['filter_levels'].add((limit - ilimit) // 2)
            todo = [(Y, 16, 16 * mbx + 1, 16 * mby + 1, (4, 8, 12))]
            if not hdr['simple']:
                todo += [(U, 8, 8 * mbx + 1, 8 * mby + 1, (4,)), (V, 8, 8 * mbx + 1, 8 * mby + 1, (4,))]
            for vertical in (True, False):
                for P, size, x0, y0, inners in todo:
                    at, lo = (x0, y0) if vertical else (y0, x0)
                    if (mbx if vertical else mby) > 0:
                        e = _edge(P, at, lo, lo + size, vertical)
                        filter_simple(e, limit + 4) if hdr['simple'] else filter_normal(e, limit + 4, ilimit, hev, True)
                    if inner[mby, mbx]:
                        for k in inners:
                            e = _edge(P, at + k, lo, lo + size, vertical)
                            filter_simple(e, limit) if hdr['simple'] else filter_normal(e, limit, ilimit, hev, False)


# ---- alpha --------------------------------------------------------------------------------------------------------------------------
def decode_alpha(alph, W, H, report):
    """the ALPH chunk's plane [H,W] uint8"""
    if len(alph) < 1:
        raise Corrupt("an empty ALPH chunk")
    head = alph[0]
    comp, filt, pre = head & 3, (head >> 2) & 3, (head >> 4) & 3
    if comp > 1 or head >> 6:
        raise Corrupt("ALPH header")
    report['alph'] = (comp, filt, pre)
    if comp == 0:
        if len(alph) - 1 < W * H:
            raise Corrupt("a short ALPH chunk")
        d = np.frombuffer(alph, np.uint8, W * H, 1).reshape(H, W).astype(np.int64)
    else:
        bits = 0x2f | (W - 1) << 8 | (H - 1) << 22                     # the five header bytes a VP8L file would begin with
        argb, _ = LL.decode_payload(bits.to_bytes(5, 'little') + bytes(alph[1:]))
        d = ((argb >> 8) & 255).astype(np.int64)
    if filt == 0:
        return d.astype(np.uint8)
    a = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if x == 0 and y == 0:
                pred = 0
            elif y == 0 or (filt == 1 and x > 0):
                pred = a[y, x - 1]
            elif x == 0 or filt == 2:
                pred = a[y - 1, x]
            else:
                pred = _clip(a[y, x - 1] + a[y - 1, x] - a[y - 1, x - 1], 0, 255)
            a[y, x] = (d[y, x] + pred) & 255
    return a.astype(np.uint8)


# ---- files --------------------------------------------------------------------------------------------------------------------------
def container(data):
    """(VP8 chunk, ALPH chunk or None) of a still file: a plain walk over the RIFF chunks"""
    data = bytes(data)
    assert data[:4] == b'RIFF' and data[8:12] == b'WEBP'
    p, end = 12, 8 + struct.unpack('<I', data[4:8])[0]
    vp8 = alph = None
    while p + 8 <= end and vp8 is None:
        kind, n = data[p:p + 4], struct.unpack('<I', data[p + 4:p + 8])[0]
        if kind == b'VP8 ':
            vp8 = data[p + 8:p + 8 + n]
        elif kind == b'ALPH':
            alph = data[p + 8:p + 8 + n]
        p += 8 + n + (n & 1)
    if vp8 is None:
        raise Corrupt("no VP8 chunk")
    return vp8, alph


def new_report():
    return {'ymodes': set(), 'bmodes': set(), 'uvmodes': set(), 'segments': set(), 'segment_qi': set(), 'skipped': 0, 'hev': set(),
            'filter_levels': set(), 'alph': None}


def decode_vp8(vp8, report=None):
    """(R, G, B uint8 [H,W,3], report, the parsed frame, the coefficients [mbh,mbw,25,16])"""
    report = new_report() if report is None else report
    f = parse(vp8)
    if f['past']:
        raise Corrupt("a partition ended early")
    hdr = f['header']
    planes, coefs, inner = reconstruct(f, report)
    loop_filter(f, planes, inner, report)
    report.update(partitions=f['nparts'], prob_updates=hdr['prob_updates'], cats=f['cats'], sharpness=hdr['sharpness'],
                  level=hdr['level'], segmentation=(hdr['segmentation'], hdr['update_map'], hdr['update_data'], hdr['absolute']),
                  lf_delta=(hdr['lf_delta'], hdr['ref_lf_delta'][0], hdr['mode_lf_delta'][0]), use_skip=hdr['use_skip'],
                  colour_bits=(hdr['colour_space'], hdr['clamp']), qdelta=tuple(hdr['qdelta']), qi=hdr['qi'], version=f['version'],
                  has_b=any(m['is_b'] for row in f['mbs'] for m in row))
    W, H = f['width'], f['height']
    res = {'planes': tuple(P[1:, 1:] for P in planes), 'level': 0, 'inner': inner}
    return E.decoded_rgb(res, H, W), report, f, coefs


def decode(data):
    """a still lossy .webp file -> (B, G, R, A uint8 [H,W,4], report)"""
    vp8, alph = container(data)
    rgb, report, _, _ = decode_vp8(vp8)
    H, W = rgb.shape[:2]
    a = decode_alpha(alph, W, H, report) if alph is not None else np.full((H, W), 255, np.uint8)
    return np.dstack([rgb[..., ::-1], a]), report
