// csm_vp8dec.h -- the VP8 key-frame decoder of the lossy WebP reader (contract DESIGN.md §4.16: the result equals what libwebp decodes
// on every byte): the boolean decoder, the frame-header parser, the per-macroblock mode parser, the coefficient token parser, and the
// per-macroblock arithmetic behind them (prediction, inverse transforms, loop filter, chroma upsampling and colour conversion),
// written so that the same text compiles for the device (csrc/webplossy.hip: one lane walks a file, macroblock wavefronts rebuild
// and filter it) and for the host (tools/vp8_host_check.cpp, where corrupt streams are exercised under the sanitizers).  The format
// is RFC 6386; tests/webplossy_restatement.py restates it independently in Python.
//
// Every read of the input is bounded by the partition's length: bytes behind the end read as zero and raise kErrEnd.  Every store
// is bounded by the macroblock counts the caller sized its buffers with, whatever the data.
#pragma once
#include <stdint.h>

#include "csm_vp8_tables.h"

#if defined(__HIPCC__)
#define CSM_VP8D_FN __host__ __device__ inline
#else
#define CSM_VP8D_FN inline
#endif

namespace csm_vp8d {

constexpr int kMaxParts = 8;
constexpr int kCoefPerMb = 25 * 16;          // int16: 16 luma blocks, 4 U, 4 V, the Y2 block; raster order inside a block

enum : uint32_t {                            // bits of the error word of a file
    kErrEnd = 1,          // a partition ended early
    kErrTag = 2,          // the frame tag, the start code or the size is not what the descriptor says
    kErrPartition = 4,    // the first partition or the table of partition sizes runs past the chunk
    kErrAlpha = 8,        // the ALPH chunk: a bad header byte, or fewer raw bytes than pixels
    kErrAlphaShift = 8,   // from this bit up: the error word of the alpha plane's VP8L stream (csm_vp8l.h)
};

// sub-block modes, numbered as the leaves of the format's mode tree from left to right; a whole-block mode is stored as the
// sub-block mode it stands for in its neighbours' contexts
enum : int { B_DC = 0, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU };
enum : int { DC_PRED = B_DC, TM_PRED = B_TM, V_PRED = B_VE, H_PRED = B_HE };
enum : int { kSkip = 1, kInner = 2, kBPred = 4, kCoded = 8 };      // MbRec::flags
// the key-frame sub-block mode probabilities (vp8::kBModeProbs) are in csm_vp8_tables.h, shared with the writer

// ---- the boolean decoder --------------------------------------------------------------------------------------------------------
struct Bool {
    const uint8_t *in;
    uint32_t len, pos;                   // pos: the next byte to load
    uint64_t value;                      // the bits loaded and not yet decided: 8 + bits of them
    int32_t bits;                        // bits of `value` past the 8 the next decision compares; negative: a load is due
    uint32_t range;                      // the range minus one, 127..254 between calls
    uint32_t past;                       // a load met the end
};

CSM_VP8D_FN void bool_init(Bool &b, const uint8_t *in, uint32_t len) {
    b.in = in; b.len = len; b.pos = 0; b.value = 0; b.bits = -8; b.range = 254; b.past = 0;
}

// seven bytes in one load while eight are left, single bytes behind that, zeros behind the end
CSM_VP8D_FN void bool_load(Bool &b) {
    if (b.len - b.pos >= 8 && b.pos <= b.len) {
        uint64_t v;
        __builtin_memcpy(&v, b.in + b.pos, 8);
        b.value = (b.value << 56) | (__builtin_bswap64(v) >> 8);
        b.pos += 7; b.bits += 56;
    } else if (b.pos < b.len) {
        b.value = (b.value << 8) | b.in[b.pos++];
        b.bits += 8;
    } else {
        b.value <<= 8;
        b.bits += 8;
        b.past = 1;
    }
}

CSM_VP8D_FN int get(Bool &b, int prob) {
    if (b.bits < 0) bool_load(b);
    const uint32_t split = (b.range * (uint32_t)prob) >> 8;
    int bit;
    if ((uint32_t)(b.value >> b.bits) > split) {
        b.range -= split + 1;
        b.value -= (uint64_t)(split + 1) << b.bits;
        bit = 1;
    } else {
        b.range = split;
        bit = 0;
    }
    if (b.range < 127) {
        const int shift = __builtin_clz(b.range + 1) - 24;
        b.range = ((b.range + 1) << shift) - 1;
        b.bits -= shift;
    }
    return bit;
}

CSM_VP8D_FN int literal(Bool &b, int n) {
    int v = 0;
    for (int k = 0; k < n; ++k) v = (v << 1) | get(b, 128);
    return v;
}

CSM_VP8D_FN int optional_signed(Bool &b, int n) {
    if (!get(b, 128)) return 0;
    const int v = literal(b, n);
    return get(b, 128) ? -v : v;
}

// the bytes that hold the bits shifted out so far and the 8 behind them (what the next decision compares), however far the loads ran
CSM_VP8D_FN uint32_t bytes_used(const Bool &b) {
    const int64_t shifted = 8 * (int64_t)b.pos - 8 - b.bits;
    const int64_t bytes = (shifted + 15) >> 3;
    return bytes > (int64_t)b.len ? b.len : (uint32_t)bytes;
}

// ---- the frame header -------------------------------------------------------------------------------------------------------------
struct Header {
    uint8_t colour_space, clamp, segmentation, update_map, update_data, absolute, simple, level, sharpness, lf_delta, lf_delta_update,
        log2parts, qi, refresh_entropy, use_skip, prob_skip;
    uint8_t filter_type;                 // 0 none, 1 simple, 2 normal
    uint8_t seg_probs[3];
    int8_t seg_quant[4], seg_level[4], ref_lf[4], mode_lf[4], qdelta[5];     // qdelta: y1 dc, y2 dc, y2 ac, uv dc, uv ac
    uint16_t quant[4][6];                // per segment: y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac
    uint8_t limit[4][2], ilimit[4][2], hev[4][2];                            // per segment and (whole-block | sub-block) macroblock; limit 0: no filter
    uint32_t prob_updates;
    uint8_t probs[1056];                 // [block type 4][band 8][context 3][node 11]
};

CSM_VP8D_FN int clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

CSM_VP8D_FN void read_header(Bool &d, Header &h) {
    h.colour_space = (uint8_t)literal(d, 1);
    h.clamp = (uint8_t)literal(d, 1);
    h.segmentation = (uint8_t)literal(d, 1);
    h.update_map = h.update_data = 0;
    h.absolute = 1;                      // what libwebp starts from: a map without a data update means quantiser 0 and level 0, absolute
    for (int s = 0; s < 4; ++s) h.seg_quant[s] = h.seg_level[s] = h.ref_lf[s] = h.mode_lf[s] = 0;
    for (int k = 0; k < 3; ++k) h.seg_probs[k] = 255;
    if (h.segmentation) {
        h.update_map = (uint8_t)literal(d, 1);
        h.update_data = (uint8_t)literal(d, 1);
        if (h.update_data) {
            h.absolute = (uint8_t)literal(d, 1);
            for (int s = 0; s < 4; ++s) h.seg_quant[s] = (int8_t)optional_signed(d, 7);
            for (int s = 0; s < 4; ++s) h.seg_level[s] = (int8_t)optional_signed(d, 6);
        }
        if (h.update_map)
            for (int k = 0; k < 3; ++k) h.seg_probs[k] = get(d, 128) ? (uint8_t)literal(d, 8) : (uint8_t)255;
    }
    h.simple = (uint8_t)literal(d, 1);
    h.level = (uint8_t)literal(d, 6);
    h.sharpness = (uint8_t)literal(d, 3);
    h.lf_delta = (uint8_t)literal(d, 1);
    h.lf_delta_update = 0;
    if (h.lf_delta) {
        h.lf_delta_update = (uint8_t)literal(d, 1);
        if (h.lf_delta_update) {
            for (int k = 0; k < 4; ++k) h.ref_lf[k] = (int8_t)optional_signed(d, 6);
            for (int k = 0; k < 4; ++k) h.mode_lf[k] = (int8_t)optional_signed(d, 6);
        }
    }
    h.log2parts = (uint8_t)literal(d, 2);
    h.qi = (uint8_t)literal(d, 7);
    for (int k = 0; k < 5; ++k) h.qdelta[k] = (int8_t)optional_signed(d, 4);
    h.refresh_entropy = (uint8_t)literal(d, 1);
    h.prob_updates = 0;
    for (int i = 0; i < 1056; ++i) {
        uint8_t p = vp8::kCoeffProbs[i];
        if (get(d, vp8::kCoeffUpdateProbs[i])) { p = (uint8_t)literal(d, 8); ++h.prob_updates; }
        h.probs[i] = p;
    }
    h.use_skip = (uint8_t)literal(d, 1);
    h.prob_skip = h.use_skip ? (uint8_t)literal(d, 8) : (uint8_t)0;
    // quantiser steps per segment
    for (int s = 0; s < 4; ++s) {
        int q = h.qi;
        if (h.segmentation) q = h.seg_quant[s] + (h.absolute ? 0 : h.qi);
        const int y2ac = (vp8::kAcTable[clip(q + h.qdelta[2], 0, 127)] * 101581) >> 16;
        h.quant[s][0] = vp8::kDcTable[clip(q + h.qdelta[0], 0, 127)];
        h.quant[s][1] = vp8::kAcTable[clip(q, 0, 127)];
        h.quant[s][2] = (uint16_t)(2 * vp8::kDcTable[clip(q + h.qdelta[1], 0, 127)]);
        h.quant[s][3] = (uint16_t)(y2ac < 8 ? 8 : y2ac);
        h.quant[s][4] = vp8::kDcTable[clip(q + h.qdelta[3], 0, 117)];
        h.quant[s][5] = vp8::kAcTable[clip(q + h.qdelta[4], 0, 127)];
    }
    // loop-filter strengths per segment and macroblock kind; the frame's level 0 switches the filter off whatever the segments say
    h.filter_type = h.level == 0 ? 0 : h.simple ? 1 : 2;
    for (int s = 0; s < 4; ++s)
        for (int b = 0; b < 2; ++b) {
            int level = h.level;
            if (h.segmentation) level = h.seg_level[s] + (h.absolute ? 0 : h.level);
            if (h.lf_delta) level += h.ref_lf[0] + (b ? h.mode_lf[0] : 0);
            level = clip(level, 0, 63);
            int inner = level;
            if (h.sharpness > 0) {
                inner >>= h.sharpness > 4 ? 2 : 1;
                if (inner > 9 - h.sharpness) inner = 9 - h.sharpness;
            }
            if (inner < 1) inner = 1;
            h.limit[s][b] = level ? (uint8_t)(2 * level + inner) : (uint8_t)0;
            h.ilimit[s][b] = (uint8_t)inner;
            h.hev[s][b] = level >= 40 ? 2 : level >= 15 ? 1 : 0;
        }
}

// ---- one macroblock's modes -----------------------------------------------------------------------------------------------------
struct MbRec {
    uint8_t segment, flags, ymode, uvmode;       // ymode: the whole-block mode (sub-block macroblocks: B_DC, unused)
    uint8_t bmodes[16];
    uint8_t limit, ilimit, hev, pad;             // loop filter: limit 0 = not filtered
};

CSM_VP8D_FN int read_bmode(Bool &d, const uint8_t *p) {
    if (!get(d, p[0])) return B_DC;
    if (!get(d, p[1])) return B_TM;
    if (!get(d, p[2])) return B_VE;
    if (!get(d, p[3])) {
        if (!get(d, p[4])) return B_HE;
        return get(d, p[5]) ? B_VR : B_RD;
    }
    if (!get(d, p[6])) return B_LD;
    if (!get(d, p[7])) return B_VL;
    return get(d, p[8]) ? B_HU : B_HD;
}

// top: the 4 sub-block modes above the macroblock, left: the 4 to its left; both are replaced by this macroblock's
CSM_VP8D_FN void read_modes(Bool &d, const Header &h, uint8_t *top, uint8_t *left, MbRec &m) {
    m.segment = 0;
    if (h.update_map) m.segment = (uint8_t)(get(d, h.seg_probs[0]) ? 2 + get(d, h.seg_probs[2]) : get(d, h.seg_probs[1]));
    m.flags = (uint8_t)((h.use_skip && get(d, h.prob_skip)) ? kSkip : 0);
    m.pad = 0;
    if (!get(d, 145)) {
        m.flags |= kBPred;
        m.ymode = B_DC;
        for (int by = 0; by < 4; ++by)
            for (int bx = 0; bx < 4; ++bx) {
                const int mode = read_bmode(d, vp8::kBModeProbs +(top[bx] * 10 + left[by]) * 9);
                top[bx] = left[by] = m.bmodes[4 * by + bx] = (uint8_t)mode;
            }
    } else {
        const int ym = get(d, 156) ? (get(d, 128) ? TM_PRED : H_PRED) : (get(d, 163) ? V_PRED : DC_PRED);
        m.ymode = (uint8_t)ym;
        for (int k = 0; k < 16; ++k) m.bmodes[k] = (uint8_t)ym;
        for (int k = 0; k < 4; ++k) top[k] = left[k] = (uint8_t)ym;
    }
    m.uvmode = (uint8_t)(!get(d, 142) ? DC_PRED : !get(d, 114) ? V_PRED : get(d, 183) ? TM_PRED : H_PRED);
    const int b = (m.flags & kBPred) ? 1 : 0;
    m.limit = h.filter_type ? h.limit[m.segment][b] : (uint8_t)0;
    m.ilimit = h.ilimit[m.segment][b];
    m.hev = h.hev[m.segment][b];
}

// ---- one block's tokens -----------------------------------------------------------------------------------------------------------
CSM_VP8D_FN int large_value(Bool &t, const uint8_t *p) {
    if (!get(t, p[3])) return !get(t, p[4]) ? 2 : 3 + get(t, p[5]);
    if (!get(t, p[6])) {
        if (!get(t, p[7])) return 5 + get(t, 159);
        const int v = 7 + 2 * get(t, 165);
        return v + get(t, 145);
    }
    const int b1 = get(t, p[8]);
    const int cat = 2 * b1 + get(t, p[9 + b1]);
    const int first = cat == 0 ? 0 : cat == 1 ? 3 : cat == 2 ? 7 : 12, n = cat == 0 ? 3 : cat == 1 ? 4 : cat == 2 ? 5 : 11;
    int v = 0;
    for (int k = 0; k < n; ++k) v = 2 * v + get(t, vp8::kCat[first + k]);
    return v + 3 + (8 << cat);
}

// probs: the [band 8][context 3][node 11] table of the block's type; out: 16 zeros, receives the dequantised coefficients in raster
// order, kept in 16 bits as the format's decoders keep them.  Returns the position behind the last token read
CSM_VP8D_FN int read_block(Bool &t, const uint8_t *probs, int ctx, int first, int dcq, int acq, int16_t *out) {
    int n = first;
    const uint8_t *p = probs + (vp8::kBands[n] * 3 + ctx) * 11;
    for (; n < 16; ++n) {
        if (!get(t, p[0])) return n;
        while (!get(t, p[1])) {
            if (++n == 16) return 16;
            p = probs + vp8::kBands[n] * 33;
        }
        const uint8_t *next = probs + vp8::kBands[n + 1] * 33;
        int v;
        if (!get(t, p[2])) { v = 1; p = next + 11; } else { v = large_value(t, p); p = next + 22; }
        if (get(t, 128)) v = -v;
        out[vp8::kZigzag[n]] = (int16_t)(uint16_t)(uint32_t)(v * (n > 0 ? acq : dcq));
    }
    return 16;
}

// ---- the inverse transforms -----------------------------------------------------------------------------------------------------
// 16 Y2 coefficients -> the DC of the 16 luma blocks (out[16 * k])
CSM_VP8D_FN void iwht(const int16_t *in, int16_t *out) {
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[i] + in[12 + i], a1 = in[4 + i] + in[8 + i], a2 = in[4 + i] - in[8 + i], a3 = in[i] - in[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
    for (int i = 0; i < 4; ++i) {
        const int dc = t[4 * i] + 3;
        const int a0 = dc + t[4 * i + 3], a1 = t[4 * i + 1] + t[4 * i + 2], a2 = t[4 * i + 1] - t[4 * i + 2], a3 = dc - t[4 * i + 3];
        out[16 * (4 * i + 0)] = (int16_t)(uint16_t)(uint32_t)((a0 + a1) >> 3);
        out[16 * (4 * i + 1)] = (int16_t)(uint16_t)(uint32_t)((a3 + a2) >> 3);
        out[16 * (4 * i + 2)] = (int16_t)(uint16_t)(uint32_t)((a0 - a1) >> 3);
        out[16 * (4 * i + 3)] = (int16_t)(uint16_t)(uint32_t)((a3 - a2) >> 3);
    }
}

// 64-bit products: coefficients near the 16-bit limits (corrupt streams only) must not overflow
CSM_VP8D_FN int mul1(int a) { return (int)(((int64_t)a * 20091) >> 16) + a; }
CSM_VP8D_FN int mul2(int a) { return (int)(((int64_t)a * 35468) >> 16); }

// 16 coefficients -> 16 residuals, both in raster order
CSM_VP8D_FN void idct(const int16_t *c, int *r) {
    int t[16];
    for (int i = 0; i < 4; ++i) {                                   // vertical pass: t[4 * column + row]
        const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
        const int cc = mul2(c[4 + i]) - mul1(c[12 + i]), d = mul1(c[4 + i]) + mul2(c[12 + i]);
        t[4 * i] = a + d; t[4 * i + 1] = b + cc; t[4 * i + 2] = b - cc; t[4 * i + 3] = a - d;
    }
    for (int y = 0; y < 4; ++y) {                                   // horizontal pass over row y
        const int dc = t[y] + 4;
        const int a = dc + t[8 + y], b = dc - t[8 + y];
        const int cc = mul2(t[4 + y]) - mul1(t[12 + y]), d = mul1(t[4 + y]) + mul2(t[12 + y]);
        r[4 * y] = (a + d) >> 3; r[4 * y + 1] = (b + cc) >> 3; r[4 * y + 2] = (b - cc) >> 3; r[4 * y + 3] = (a - d) >> 3;
    }
}

// ---- one macroblock's tokens ------------------------------------------------------------------------------------------------------
// top, left: the non-zero contexts above and to the left (4 luma, 2 U, 2 V, Y2); coef: kCoefPerMb zeros.  Sets kCoded and kInner
CSM_VP8D_FN void read_residuals(Bool &t, const Header &h, MbRec &m, uint8_t *top, uint8_t *left, int16_t *coef) {
    const bool bpred = (m.flags & kBPred) != 0;
    if (m.flags & kSkip) {
        for (int k = 0; k < 8; ++k) top[k] = left[k] = 0;
        if (!bpred) top[8] = left[8] = 0;                           // a sub-block macroblock leaves the Y2 context as it found it
        if (bpred) m.flags |= kInner;
        return;
    }
    const uint16_t *q = h.quant[m.segment];
    int first = 0;
    const uint8_t *luma = h.probs + 3 * 264;
    if (!bpred) {
        const int end = read_block(t, h.probs + 264, top[8] + left[8], 0, q[2], q[3], coef + 24 * 16);
        top[8] = left[8] = (uint8_t)(end > 0);
        iwht(coef + 24 * 16, coef);
        first = 1;
        luma = h.probs;
    }
    bool coded = false;
    for (int by = 0; by < 4; ++by)
        for (int bx = 0; bx < 4; ++bx) {
            int16_t *c = coef + 16 * (4 * by + bx);
            const int end = read_block(t, luma, top[bx] + left[by], first, q[0], q[1], c);
            top[bx] = left[by] = (uint8_t)(end > first);
            coded = coded || end > 1 || c[0] != 0;
        }
    for (int ch = 0; ch < 2; ++ch)
        for (int by = 0; by < 2; ++by)
            for (int bx = 0; bx < 2; ++bx) {
                int16_t *c = coef + 16 * (16 + 4 * ch + 2 * by + bx);
                const int end = read_block(t, h.probs + 2 * 264, top[4 + 2 * ch + bx] + left[4 + 2 * ch + by], 0, q[4], q[5], c);
                top[4 + 2 * ch + bx] = left[4 + 2 * ch + by] = (uint8_t)(end > 0);
                coded = coded || end > 1 || c[0] != 0;
            }
    if (coded) m.flags |= kCoded;
    if (coded || bpred) m.flags |= kInner;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------
struct Frame {
    uint32_t err;
    int32_t mbw, mbh, filter_type, nparts, colour_space, clamp;
    uint32_t prob_updates;
    uint32_t used[1 + kMaxParts];        // bytes read of the first partition and of every token partition
};

struct WalkBufs {
    uint8_t *top_modes;                  // 4 * mbw
    uint8_t *top_nz;                     // 9 * mbw
    MbRec *recs;                         // mbw * mbh
    int16_t *coef;                       // mbw * mbh * kCoefPerMb, zeros
};

// One VP8 chunk of a W x H image: the plain bytes in front (frame tag, start code, size, partition sizes), then every macroblock
// in raster order: modes from the first partition, tokens from partition row % parts.  parts: kMaxParts decoder states
CSM_VP8D_FN void walk_frame(Header &h, Bool &first, Bool *parts, const uint8_t *in, uint32_t len, uint32_t W, uint32_t H, const WalkBufs &B,
                            Frame &F) {
    const int mbw = (int)((W + 15) >> 4), mbh = (int)((H + 15) >> 4);
    F.err = 0; F.mbw = mbw; F.mbh = mbh; F.filter_type = 0; F.nparts = 0; F.colour_space = 0; F.clamp = 0; F.prob_updates = 0;
    for (int k = 0; k <= kMaxParts; ++k) F.used[k] = 0;
    if (len < 10) { F.err = kErrTag; return; }
    const uint32_t tag = in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16;
    const uint32_t w = in[6] | (uint32_t)in[7] << 8, hh = in[8] | (uint32_t)in[9] << 8;
    if ((tag & 1) || !((tag >> 4) & 1) || ((tag >> 1) & 7) > 3 || in[3] != 0x9d || in[4] != 0x01 || in[5] != 0x2a || w != W || hh != H) {
        F.err = kErrTag;
        return;
    }
    const uint32_t size = tag >> 5;
    if (size > len - 10) { F.err = kErrPartition; return; }
    bool_init(first, in + 10, size);
    read_header(first, h);
    const int nparts = 1 << h.log2parts;
    F.filter_type = h.filter_type; F.nparts = nparts; F.colour_space = h.colour_space; F.clamp = h.clamp; F.prob_updates = h.prob_updates;
    uint32_t p = 10 + size;
    if ((uint32_t)(3 * (nparts - 1)) > len - p) { F.err = kErrPartition; return; }
    uint32_t at = p + 3 * (nparts - 1);
    for (int k = 0; k < nparts; ++k) {
        uint32_t n = len - at;                                     // the last partition takes the rest; a size past the end is cut
        if (k < nparts - 1) {
            const uint32_t s = in[p + 3 * k] | (uint32_t)in[p + 3 * k + 1] << 8 | (uint32_t)in[p + 3 * k + 2] << 16;
            if (s < n) n = s;
        }
        bool_init(parts[k], in + at, n);
        at += n;
    }
    for (int k = 0; k < 4 * mbw; ++k) B.top_modes[k] = B_DC;
    for (int k = 0; k < 9 * mbw; ++k) B.top_nz[k] = 0;
    for (int mby = 0; mby < mbh; ++mby) {
        Bool &t = parts[mby & (nparts - 1)];
        uint8_t left_modes[4] = {B_DC, B_DC, B_DC, B_DC};
        uint8_t left_nz[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int mbx = 0; mbx < mbw; ++mbx) {
            const int at_mb = mby * mbw + mbx;
            MbRec m;
            read_modes(first, h, B.top_modes + 4 * mbx, left_modes, m);
            read_residuals(t, h, m, B.top_nz + 9 * mbx, left_nz, B.coef + (int64_t)at_mb * kCoefPerMb);
            B.recs[at_mb] = m;
        }
        if (first.past) break;                                     // the rest would be decoded from zeros
    }
    F.used[0] = bytes_used(first);
    uint32_t past = first.past;
    for (int k = 0; k < nparts; ++k) { F.used[1 + k] = bytes_used(parts[k]); past |= parts[k].past; }
    if (past) F.err |= kErrEnd;
}

// ---- planes -----------------------------------------------------------------------------------------------------------------------
// p points at pixel (0, 0).  Row -1 holds 127 from column -1 to 4 columns past the last macroblock, column -1 holds 129 from row 0
// down: what the format predicts from outside the frame
struct Plane {
    uint8_t *p;
    int stride;
};

CSM_VP8D_FN int plane_stride(int mbw, int size) { return mbw * size + 32; }
CSM_VP8D_FN int64_t plane_bytes(int mbw, int mbh, int size) { return (int64_t)(mbh * size + 1) * plane_stride(mbw, size); }
CSM_VP8D_FN int64_t plane_origin(int mbw, int size) { return plane_stride(mbw, size) + 16; }

CSM_VP8D_FN uint32_t clip255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// prediction rows (4 pixels packed little-endian) plus the residuals of the coefficients c (nullptr: none) into the 4x4 block at b
CSM_VP8D_FN void put_block(uint8_t *b, int stride, const uint32_t *rows, const int16_t *c) {
    if (c) {
        const uint64_t *z = (const uint64_t *)c;
        if (!(z[0] | z[1] | z[2] | z[3])) c = nullptr;
    }
    if (!c) {
        for (int y = 0; y < 4; ++y) *(uint32_t *)(b + y * stride) = rows[y];
        return;
    }
    int r[16];
    idct(c, r);
    for (int y = 0; y < 4; ++y) {
        uint32_t v = 0;
        for (int x = 0; x < 4; ++x) v |= clip255((int)((rows[y] >> (8 * x)) & 255u) + r[4 * y + x]) << (8 * x);
        *(uint32_t *)(b + y * stride) = v;
    }
}

CSM_VP8D_FN int avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
CSM_VP8D_FN int avg2(int a, int b) { return (a + b + 1) >> 1; }
CSM_VP8D_FN uint32_t pack4(int a, int b, int c, int d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24; }

// the 4x4 prediction of a sub-block mode.  e: the 13 pixels around the block from bottom-left over the corner to top-right:
// e[0..3] the left column from the bottom up, e[4] the corner, e[5..12] the row above and its continuation to the right
CSM_VP8D_FN void predict4(int mode, const int *e, uint32_t *rows) {
    const int L = e[0], K = e[1], J = e[2], I = e[3], X = e[4], A = e[5], B = e[6], C = e[7], D = e[8], E = e[9], F = e[10], G = e[11], H = e[12];
    switch (mode) {
    case B_DC: {
        const int dc = (A + B + C + D + I + J + K + L + 4) >> 3;
        rows[0] = rows[1] = rows[2] = rows[3] = pack4(dc, dc, dc, dc);
        break;
    }
    case B_TM: {
        const int l[4] = {I, J, K, L};
        for (int y = 0; y < 4; ++y)
            rows[y] = clip255(l[y] + A - X) | clip255(l[y] + B - X) << 8 | clip255(l[y] + C - X) << 16 | clip255(l[y] + D - X) << 24;
        break;
    }
    case B_VE:
        rows[0] = rows[1] = rows[2] = rows[3] = pack4(avg3(X, A, B), avg3(A, B, C), avg3(B, C, D), avg3(C, D, E));
        break;
    case B_HE: {
        const int r0 = avg3(X, I, J), r1 = avg3(I, J, K), r2 = avg3(J, K, L), r3 = avg3(K, L, L);
        rows[0] = pack4(r0, r0, r0, r0); rows[1] = pack4(r1, r1, r1, r1); rows[2] = pack4(r2, r2, r2, r2); rows[3] = pack4(r3, r3, r3, r3);
        break;
    }
    case B_LD: {
        const int d0 = avg3(A, B, C), d1 = avg3(B, C, D), d2 = avg3(C, D, E), d3 = avg3(D, E, F), d4 = avg3(E, F, G), d5 = avg3(F, G, H), d6 = avg3(G, H, H);
        rows[0] = pack4(d0, d1, d2, d3); rows[1] = pack4(d1, d2, d3, d4); rows[2] = pack4(d2, d3, d4, d5); rows[3] = pack4(d3, d4, d5, d6);
        break;
    }
    case B_RD: {
        const int d0 = avg3(J, K, L), d1 = avg3(I, J, K), d2 = avg3(X, I, J), d3 = avg3(A, X, I), d4 = avg3(B, A, X), d5 = avg3(C, B, A), d6 = avg3(D, C, B);
        rows[0] = pack4(d3, d4, d5, d6); rows[1] = pack4(d2, d3, d4, d5); rows[2] = pack4(d1, d2, d3, d4); rows[3] = pack4(d0, d1, d2, d3);
        break;
    }
    case B_VR: {
        const int xa = avg2(X, A), ab = avg2(A, B), bc = avg2(B, C), cd = avg2(C, D);
        const int ixa = avg3(I, X, A), xab = avg3(X, A, B), abc = avg3(A, B, C), bcd = avg3(B, C, D), jix = avg3(J, I, X), kji = avg3(K, J, I);
        rows[0] = pack4(xa, ab, bc, cd); rows[1] = pack4(ixa, xab, abc, bcd); rows[2] = pack4(jix, xa, ab, bc); rows[3] = pack4(kji, ixa, xab, abc);
        break;
    }
    case B_VL: {
        const int ab = avg2(A, B), bc = avg2(B, C), cd = avg2(C, D), de = avg2(D, E);
        const int abc = avg3(A, B, C), bcd = avg3(B, C, D), cde = avg3(C, D, E), def = avg3(D, E, F), efg = avg3(E, F, G), fgh = avg3(F, G, H);
        rows[0] = pack4(ab, bc, cd, de); rows[1] = pack4(abc, bcd, cde, def); rows[2] = pack4(bc, cd, de, efg); rows[3] = pack4(bcd, cde, def, fgh);
        break;
    }
    case B_HD: {
        const int ix = avg2(I, X), ji = avg2(J, I), kj = avg2(K, J), lk = avg2(L, K);
        const int abc = avg3(A, B, C), xab = avg3(X, A, B), ixa = avg3(I, X, A), jix = avg3(J, I, X), kji = avg3(K, J, I), lkj = avg3(L, K, J);
        rows[0] = pack4(ix, ixa, xab, abc); rows[1] = pack4(ji, jix, ix, ixa); rows[2] = pack4(kj, kji, ji, jix); rows[3] = pack4(lk, lkj, kj, kji);
        break;
    }
    default: {
        const int ij = avg2(I, J), jk = avg2(J, K), kl = avg2(K, L), ijk = avg3(I, J, K), jkl = avg3(J, K, L), kll = avg3(K, L, L);
        rows[0] = pack4(ij, ijk, jk, jkl); rows[1] = pack4(jk, jkl, kl, kll); rows[2] = pack4(kl, kll, L, L); rows[3] = pack4(L, L, L, L);
        break;
    }
    }
}

// the four whole-block predictions of the size x size block at d (16 luma, 8 chroma), block by block, plus the residuals
// (coded: the macroblock has coefficients; coef: its first block of this plane)
CSM_VP8D_FN void recon_whole(uint8_t *d, int stride, int size, int mbx, int mby, int mode, bool coded, const int16_t *coef) {
    const uint8_t *above = d - stride;
    int dc = 128;
    if (mode == DC_PRED) {
        int top = 0, left = 0;
        for (int k = 0; k < size; ++k) { top += above[k]; left += d[k * stride - 1]; }
        const int sh = size == 8 ? 3 : 4;
        if (mbx > 0 && mby > 0) dc = (top + left + size) >> (sh + 1);
        else if (mby > 0) dc = (top + (size >> 1)) >> sh;
        else if (mbx > 0) dc = (left + (size >> 1)) >> sh;
    }
    const int corner = above[-1], n = size >> 2;
    for (int by = 0; by < n; ++by)
        for (int bx = 0; bx < n; ++bx) {
            uint8_t *b = d + 4 * by * stride + 4 * bx;
            uint32_t rows[4];
            if (mode == DC_PRED) {
                rows[0] = rows[1] = rows[2] = rows[3] = (uint32_t)dc * 0x01010101u;
            } else if (mode == V_PRED) {
                rows[0] = rows[1] = rows[2] = rows[3] = *(const uint32_t *)(above + 4 * bx);
            } else if (mode == H_PRED) {
                for (int y = 0; y < 4; ++y) rows[y] = (uint32_t)d[(4 * by + y) * stride - 1] * 0x01010101u;
            } else {
                for (int y = 0; y < 4; ++y) {
                    const int l = d[(4 * by + y) * stride - 1] - corner;
                    rows[y] = clip255(l + above[4 * bx]) | clip255(l + above[4 * bx + 1]) << 8 | clip255(l + above[4 * bx + 2]) << 16 |
                              clip255(l + above[4 * bx + 3]) << 24;
                }
            }
            put_block(b, stride, rows, coded ? coef + 16 * (n * by + bx) : nullptr);
        }
}

// the luma of macroblock (mbx, mby) into the plane; its neighbours above, above-right and to the left are final (unfiltered)
CSM_VP8D_FN void recon_luma(const Plane &Y, int mbx, int mby, int mbw, const MbRec &m, const int16_t *coef) {
    uint8_t *d = Y.p + (int64_t)16 * mby * Y.stride + 16 * mbx;
    const bool coded = (m.flags & kCoded) != 0;
    if (!(m.flags & kBPred)) { recon_whole(d, Y.stride, 16, mbx, mby, m.ymode, coded, coef); return; }
    // the 4 pixels above and right of the macroblock serve the right-hand sub-blocks of all four rows; at the right border of the
    // frame they repeat the last pixel above, and above the frame row -1 holds them
    int tr[4];
    for (int k = 0; k < 4; ++k) tr[k] = (mby > 0 && mbx == mbw - 1) ? d[-Y.stride + 15] : d[-Y.stride + 16 + k];
    for (int by = 0; by < 4; ++by)
        for (int bx = 0; bx < 4; ++bx) {
            uint8_t *b = d + 4 * by * Y.stride + 4 * bx;
            int e[13];
            for (int k = 0; k < 4; ++k) e[3 - k] = b[k * Y.stride - 1];
            for (int k = 0; k < 5; ++k) e[4 + k] = b[-Y.stride - 1 + k];
            for (int k = 0; k < 4; ++k) e[9 + k] = bx == 3 ? tr[k] : b[-Y.stride + 4 + k];
            uint32_t rows[4];
            predict4(m.bmodes[4 * by + bx], e, rows);
            put_block(b, Y.stride, rows, coded ? coef + 16 * (4 * by + bx) : nullptr);
        }
}

CSM_VP8D_FN void recon_chroma(const Plane &U, const Plane &V, int mbx, int mby, const MbRec &m, const int16_t *coef) {
    const bool coded = (m.flags & kCoded) != 0;
    recon_whole(U.p + (int64_t)8 * mby * U.stride + 8 * mbx, U.stride, 8, mbx, mby, m.uvmode, coded, coef + 16 * 16);
    recon_whole(V.p + (int64_t)8 * mby * V.stride + 8 * mbx, V.stride, 8, mbx, mby, m.uvmode, coded, coef + 20 * 16);
}

// ---- the loop filter ----------------------------------------------------------------------------------------------------------------
CSM_VP8D_FN int abs_i(int v) { return v < 0 ? -v : v; }

// one line of pixels across an edge: q points at the first pixel behind it, step leads across.  kind 0: the simple filter, 1: the
// normal filter at a macroblock edge, 2: at an inner edge.  limit: the edge limit (+4 at macroblock edges)
CSM_VP8D_FN void filter_line(uint8_t *q, int step, int kind, int limit, int ilimit, int hev_thr) {
    const int p1 = q[-2 * step], p0 = q[-step], q0 = q[0], q1 = q[step];
    if (4 * abs_i(p0 - q0) + abs_i(p1 - q1) > 2 * limit + 1) return;
    const int outer = clip(p1 - q1, -128, 127);
    if (kind == 0) {
        const int a = 3 * (q0 - p0) + outer;
        q[-step] = (uint8_t)clip255(p0 + clip((a + 3) >> 3, -16, 15));
        q[0] = (uint8_t)clip255(q0 - clip((a + 4) >> 3, -16, 15));
        return;
    }
    const int p3 = q[-4 * step], p2 = q[-3 * step], q2 = q[2 * step], q3 = q[3 * step];
    if (abs_i(p3 - p2) > ilimit || abs_i(p2 - p1) > ilimit || abs_i(p1 - p0) > ilimit || abs_i(q3 - q2) > ilimit || abs_i(q2 - q1) > ilimit ||
        abs_i(q1 - q0) > ilimit)
        return;
    if (abs_i(p1 - p0) > hev_thr || abs_i(q1 - q0) > hev_thr) {      // high edge variance: only the two pixels at the edge move
        const int a = 3 * (q0 - p0) + outer;
        q[-step] = (uint8_t)clip255(p0 + clip((a + 3) >> 3, -16, 15));
        q[0] = (uint8_t)clip255(q0 - clip((a + 4) >> 3, -16, 15));
    } else if (kind == 1) {
        const int a = clip(3 * (q0 - p0) + outer, -128, 127);
        const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
        q[-3 * step] = (uint8_t)clip255(p2 + a3); q[-2 * step] = (uint8_t)clip255(p1 + a2); q[-step] = (uint8_t)clip255(p0 + a1);
        q[0] = (uint8_t)clip255(q0 - a1); q[step] = (uint8_t)clip255(q1 - a2); q[2 * step] = (uint8_t)clip255(q2 - a3);
    } else {
        const int a = 3 * (q0 - p0);
        const int a1 = clip((a + 4) >> 3, -16, 15), a2 = clip((a + 3) >> 3, -16, 15), a3 = (a1 + 1) >> 1;
        q[-2 * step] = (uint8_t)clip255(p1 + a3); q[-step] = (uint8_t)clip255(p0 + a2);
        q[0] = (uint8_t)clip255(q0 - a1); q[step] = (uint8_t)clip255(q1 - a3);
    }
}

// the edges of macroblock (mbx, mby) in one plane (size 16 luma, 8 chroma), in the format's order: the left edge, the inner vertical
// edges, the top edge, the inner horizontal edges.  Every macroblock before it in raster order is done
CSM_VP8D_FN void filter_mb(const Plane &P, int size, int mbx, int mby, const MbRec &m, bool simple) {
    if (!m.limit) return;
    uint8_t *d = P.p + (int64_t)size * mby * P.stride + size * mbx;
    const bool inner = (m.flags & kInner) != 0;
    for (int k = 0; k < size; k += 4) {
        if (k == 0 ? mbx == 0 : !inner) continue;
        for (int i = 0; i < size; ++i) filter_line(d + i * P.stride + k, 1, simple ? 0 : k ? 2 : 1, m.limit + (k ? 0 : 4), m.ilimit, m.hev);
    }
    for (int k = 0; k < size; k += 4) {
        if (k == 0 ? mby == 0 : !inner) continue;
        for (int i = 0; i < size; ++i) filter_line(d + k * P.stride + i, P.stride, simple ? 0 : k ? 2 : 1, m.limit + (k ? 0 : 4), m.ilimit, m.hev);
    }
}

// ---- the pixels libwebp shows ---------------------------------------------------------------------------------------------------
// pixel (x, y) of a W x H image: chroma upsampled by (9 near + 3 + 3 + far + 8) >> 4 with replicated edges, then the 14-bit
// fixed-point conversion; returns B | G << 8 | R << 16
CSM_VP8D_FN uint32_t pixel_bgr(const Plane &Y, const Plane &U, const Plane &V, int x, int y, int W, int H) {
    const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const int nx = x >> 1, ny = y >> 1;
    const int fx = clip(nx + ((x & 1) ? 1 : -1), 0, cw - 1), fy = clip(ny + ((y & 1) ? 1 : -1), 0, ch - 1);
    const uint8_t *un = U.p + (int64_t)ny * U.stride, *uf = U.p + (int64_t)fy * U.stride;
    const uint8_t *vn = V.p + (int64_t)ny * V.stride, *vf = V.p + (int64_t)fy * V.stride;
    const int u = (9 * un[nx] + 3 * un[fx] + 3 * uf[nx] + uf[fx] + 8) >> 4;
    const int v = (9 * vn[nx] + 3 * vn[fx] + 3 * vf[nx] + vf[fx] + 8) >> 4;
    const int yy = (Y.p[(int64_t)y * Y.stride + x] * 19077) >> 8;
    const int r = yy + ((v * 26149) >> 8) - 14234;
    const int g = yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708;
    const int b = yy + ((u * 33050) >> 8) - 17685;
    return clip255(b >> 6) | clip255(g >> 6) << 8 | clip255(r >> 6) << 16;
}

// ---- the alpha plane ----------------------------------------------------------------------------------------------------------------
// the ALPH chunk's filters 1..3 (horizontal, vertical, gradient) predict a value from its left, top and top-left neighbours
CSM_VP8D_FN int alpha_predict(int filter, int x, int y, int L, int T, int TL) {
    if (x == 0 && y == 0) return 0;
    if (y == 0 || (filter == 1 && x > 0)) return L;
    if (x == 0 || filter == 2) return T;
    return (int)clip255(L + T - TL);
}

}  // namespace csm_vp8d
