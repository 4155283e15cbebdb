// webp.hip -- the device half of the WebP writer, for gfx950: every frame of a clip as one VP8 key frame (16x16 luma and 8x8 chroma
// prediction out of DC / V / H / TM, the format's transforms, one quantiser index, default coefficient probabilities, the boolean
// coder).  The contract is fixed to the byte and restated in numpy in tests/webp_restatement.py; the frame header,
// the partition sizes and the RIFF container are host work (webpcode.py).
//
//   colour:      k_webp_yuv   (one thread per 2x2 cell: BGR -> Y Cb Cr 4:2:0, the edges replicated up to macroblock multiples)
//   macroblocks: k_webp_mb    (ONE workgroup per frame walks the anti-diagonals of the macroblock grid; a wave takes a macroblock:
//                              borders from the reconstruction, the mode by SSE, forward transforms, quantiser, and the decoder's
//                              own reconstruction back to global memory; __syncthreads() between diagonals)
//   code:        k_webp_code  (ONE lane per partition: the first partition of a frame or one of its token partitions; the lane
//                              walks its macroblocks, derives every (probability, bit) pair from the stored levels and the
//                              neighbours' non-zero flags and feeds the boolean coder, bytes into its own segment of scratch;
//                              the probability tables and each lane's current macroblock of levels sit in LDS)
//   sizes:       k_webp_offsets (one workgroup: byte offset of every partition in the blob; sizes and status to `info`)
//   write:       k_webp_pack  (one workgroup per partition copies its bytes into the blob)
//
// A macroblock needs its left, top and top-left neighbours reconstructed, so frames are the parallel axis and a frame is a
// wavefront of diagonals inside one workgroup: no waiting between workgroups, no flags in global memory, no cooperative launch.
// The reconstruction a later diagonal reads was written to global memory by the same workgroup before a __syncthreads().
// The (probability, bit) pairs are not materialised.  A list of them would let every coder lane run one uniform loop, but scratch
// is sized before the one host sync, so from the worst case: 25 * 305 pairs of 2 B, 15 KB per macroblock on top of the 6.7 KB of
// token segment, a third of the frames per chunk.  The lane that range-codes a partition derives the pairs as it goes instead and
// pays with divergence (DESIGN.md §4.12 has the figures).
// No float arithmetic anywhere; the only atomics are integer adds of the skip count and an OR into the status word.
#include "csm_common.h"
#include "csm_vp8_tables.h"
#include "csm_vp8dec.h"
#include "csm_boolenc.h"
#include "csm_bits.h"
//
// Method 1 (restated in tests/webp_m1_restatement.py) adds B_PRED macroblocks and per-frame coefficient-probability
// updates; method 0 is the text above and its kernels are the <0> instances below, unchanged.
//   macroblocks: k_webp_mb<1>   (the diagonals have slope two, mbx + 2 mby, because a B_PRED macroblock reads the macroblock above
//                                and to the right; inside the wave the 16 sub-blocks are a slope-two wavefront of 10 steps too.  Both
//                                luma candidates stay in LDS until the integer rate-distortion rule has chosen)
//   counts:      k_webp_stats   (one lane per 4x4 block walks its tokens and counts every branch decision: LDS, then global adds)
//   tables:      k_webp_probs   (one lane per probability: the update rule; the frame's 1056 probabilities and update flags)
//   code:        k_webp_code<1> (whole frames per workgroup, so that their probability tables and kBModeProbs sit in LDS)

namespace {
namespace dec = csm_vp8d;        // the sub-block mode numbering and predict4, shared with the decoder

constexpr int kBlock = 256;
constexpr int kWaves = 8;                    // waves of the macroblock kernel's workgroup
constexpr int kMaxLevel = 2047;
// a block codes at most 1 + 16 * 19 pairs (per coefficient: six tree nodes, 11 extra bits, the sign, the next "more" flag), a
// macroblock 25 blocks; one pair moves at most 7 bits out of the coder (the range minus one drops to 0 at worst)
constexpr int kPairsPerMb = 25 * 305;
constexpr int kBytesPerMb = (7 * kPairsPerMb + 7) / 8;
constexpr int kHeaderPairs = 1100;           // 30 header bits, 1056 update flags, 9 skip-probability bits
constexpr int kPairsPerMbFirst = 7;          // skip flag, three luma mode nodes, three chroma mode nodes
// method 1: 30 header bits, 1056 update flags with 8 value bits each, 9 skip-probability bits; per macroblock the skip flag, the
// B_PRED branch, 16 sub-block modes of at most 7 tree nodes, three chroma mode nodes.  A token partition's bound does not move: a
// B_PRED macroblock codes 24 blocks of at most 305 pairs, fewer than the 25 of the others
constexpr int kHeaderPairs1 = 30 + 1056 * 9 + 9;
constexpr int kPairsPerMbFirst1 = 1 + 1 + 16 * 7 + 3;
constexpr int kRdShift = 14;                 // J = D + ((3 ac^2 R) >> kRdShift), R in 1/256 bit
constexpr int kStage = 8;                    // frames whose probability tables a workgroup of k_webp_code<1> holds in LDS

struct Geo {
    int n, H, W, Hp, Wp, mbw, mbh, nmb, log2p, parts, units;
    int64_t ypx, cpx;          // samples of a padded luma / chroma plane
    int64_t first_cap, part_cap;
};

bool make_geo(int n, int H, int W, Geo &g, int method = 0) {
    if (n < 0 || H < 1 || H > 16383 || W < 1 || W > 16383) return false;
    g.n = n; g.H = H; g.W = W;
    g.mbw = (W + 15) >> 4; g.mbh = (H + 15) >> 4;
    g.Wp = g.mbw * 16; g.Hp = g.mbh * 16;
    g.nmb = g.mbw * g.mbh;
    g.log2p = 0;
    while (g.log2p < 3 && (2 << g.log2p) <= g.mbh) ++g.log2p;
    g.parts = 1 << g.log2p;
    if ((int64_t)n * (g.parts + 1) >= (1 << 20)) return false;
    g.units = n * (g.parts + 1);
    g.ypx = (int64_t)g.Hp * g.Wp; g.cpx = g.ypx >> 2;
    // the bytes a partition can take: 7 bits per pair, 17 padding bits at the end, the held-back byte
    g.first_cap = (7 * ((int64_t)(method ? kHeaderPairs1 : kHeaderPairs) + (int64_t)(method ? kPairsPerMbFirst1 : kPairsPerMbFirst) * g.nmb) + 7) / 8 + 8;
    g.part_cap = (int64_t)((g.mbh + g.parts - 1) / g.parts) * g.mbw * kBytesPerMb + 8;
    return true;
}

struct Scratch {
    uint8_t *src, *rec;        // [n][ypx + 2 cpx]: Y, U, V of every frame
    int16_t *levels;           // [n][nmb][25][16], zigzag order: Y2, 16 Y, 4 U, 4 V
    uint32_t *nz;              // [n][nmb]: bit b = block b has a non-zero level
    uint8_t *modes;            // [n][nmb]: luma mode | chroma mode << 2
    uint32_t *nskip;           // [n]: macroblocks without a non-zero level
    uint32_t *status;          // bit 0: a partition met the end of its segment
    int64_t *sizes, *offs;     // [units]
    uint8_t *first, *part;     // [n][first_cap], [n][parts][part_cap]
    // method 1 only
    uint8_t *bmodes;           // [n][nmb][16]: the sub-block modes; in a 16x16 macroblock the mode it stands for in contexts
    uint8_t *y2c;              // [n][nmb]: the Y2 non-zero context this macroblock hands on, bit 0 to the right, bit 1 downwards
    uint32_t *counts;          // [n][1056][2]: the frame's branch decisions
    uint8_t *probs, *upd;      // [n][1056]: the frame's coefficient probabilities and their update flags
    int64_t total;
};

Scratch make_scratch(const Geo &g, void *base, int method = 0) {
    Scratch s;
    char *p = (char *)base;
    int64_t o = 0;
    const int64_t frame = g.ypx + 2 * g.cpx, n = g.n;
    s.src = (uint8_t *)(p + o);      o += csm::align16(n * frame);
    s.rec = (uint8_t *)(p + o);      o += csm::align16(n * frame);
    s.levels = (int16_t *)(p + o);   o += csm::align16(n * g.nmb * 800);
    s.nz = (uint32_t *)(p + o);      o += csm::align16(n * g.nmb * 4);
    s.modes = (uint8_t *)(p + o);    o += csm::align16(n * g.nmb);
    s.nskip = (uint32_t *)(p + o);   o += csm::align16(n * 4 + 4);
    s.status = s.nskip + n;
    s.sizes = (int64_t *)(p + o);    o += csm::align16((int64_t)g.units * 8);
    s.offs = (int64_t *)(p + o);     o += csm::align16((int64_t)g.units * 8);
    s.first = (uint8_t *)(p + o);    o += csm::align16(n * g.first_cap);
    s.part = (uint8_t *)(p + o);     o += csm::align16(n * g.parts * g.part_cap);
    s.bmodes = s.y2c = s.probs = s.upd = nullptr; s.counts = nullptr;
    if (method) {
        s.bmodes = (uint8_t *)(p + o);   o += csm::align16(n * g.nmb * 16);
        s.y2c = (uint8_t *)(p + o);      o += csm::align16(n * g.nmb);
        s.counts = (uint32_t *)(p + o);  o += csm::align16(n * 2112 * 4);
        s.probs = (uint8_t *)(p + o);    o += csm::align16(n * 1056);
        s.upd = (uint8_t *)(p + o);      o += csm::align16(n * 1056);
    }
    s.total = o;
    return s;
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// quality 100..1 onto the quantiser index 0..127
__host__ __device__ inline int quality_to_qi(int quality) { return ((100 - quality) * 127 + 49) / 99; }

// ---- colour -------------------------------------------------------------------------------------------------------------------
// BT.601 studio range in 16 / 18 fraction bits, round half up; chroma from the sums over a 2x2 cell
__global__ __launch_bounds__(kBlock) void k_webp_yuv(const uint8_t *__restrict__ frames, Geo g, uint8_t *__restrict__ src) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.n * g.cpx) return;
    const int f = (int)(i / g.cpx);
    const int64_t r = i - (int64_t)f * g.cpx;
    const int cw = g.Wp >> 1, cy = (int)(r / cw), cx = (int)(r - (int64_t)cy * cw);
    const uint8_t *F = frames + (int64_t)f * g.H * g.W * 3;
    uint8_t *Y = src + (int64_t)f * (g.ypx + 2 * g.cpx), *U = Y + g.ypx, *V = U + g.cpx;
    int sb = 0, sg = 0, sr = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * cy + (k >> 1), x = 2 * cx + (k & 1);
        const uint8_t *q = F + ((int64_t)min(y, g.H - 1) * g.W + min(x, g.W - 1)) * 3;
        const int b = q[0], gg = q[1], rr = q[2];
        Y[(int64_t)y * g.Wp + x] = (uint8_t)clip8((16839 * rr + 33059 * gg + 6420 * b + 1081344) >> 16);
        sb += b; sg += gg; sr += rr;
    }
    U[r] = (uint8_t)clip8((-9719 * sr - 19081 * sg + 28800 * sb + 33685504) >> 18);
    V[r] = (uint8_t)clip8((28800 * sr - 24116 * sg - 4684 * sb + 33685504) >> 18);
}

// ---- transforms ---------------------------------------------------------------------------------------------------------------
// forward 4x4 transform (ours): d residuals 4 * row + column -> c coefficients 4 * vertical + horizontal frequency
__device__ __forceinline__ void fdct(const int *d, int *c) {
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2];
        const int a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
        t[4 * i] = (a0 + a1) * 8;
        t[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
        t[4 * i + 2] = (a0 - a1) * 8;
        t[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a0 = t[i] + t[12 + i], a1 = t[4 + i] + t[8 + i], a2 = t[4 + i] - t[8 + i], a3 = t[i] - t[12 + i];
        c[i] = (a0 + a1 + 7) >> 4;
        c[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0);
        c[8 + i] = (a0 - a1 + 7) >> 4;
        c[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
    }
}

__device__ __forceinline__ int mul1(int a) { return ((a * 20091) >> 16) + a; }
__device__ __forceinline__ int mul2(int a) { return (a * 35468) >> 16; }

// the format's inverse 4x4 transform: c -> residuals r (4 * row + column), before the add to the prediction
__device__ __forceinline__ void idct(const int *c, int *r) {
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                              // column i
        const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
        const int cc = mul2(c[4 + i]) - mul1(c[12 + i]), d = mul1(c[4 + i]) + mul2(c[12 + i]);
        t[4 * i] = a + d; t[4 * i + 1] = b + cc; t[4 * i + 2] = b - cc; t[4 * i + 3] = a - d;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                              // row i
        const int dc = t[i] + 4, a = dc + t[8 + i], b = dc - t[8 + i];
        const int cc = mul2(t[4 + i]) - mul1(t[12 + i]), d = mul1(t[4 + i]) + mul2(t[12 + i]);
        r[4 * i] = (a + d) >> 3; r[4 * i + 1] = (b + cc) >> 3; r[4 * i + 2] = (b - cc) >> 3; r[4 * i + 3] = (a - d) >> 3;
    }
}

// forward Walsh-Hadamard transform (ours) of the 16 luma DCs, 4 * block row + block column
__device__ __forceinline__ void fwht(const int *v, int *o) {
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a0 = v[4 * i] + v[4 * i + 2], a1 = v[4 * i + 1] + v[4 * i + 3];
        const int a2 = v[4 * i + 1] - v[4 * i + 3], a3 = v[4 * i] - v[4 * i + 2];
        t[4 * i] = a0 + a1; t[4 * i + 1] = a3 + a2; t[4 * i + 2] = a3 - a2; t[4 * i + 3] = a0 - a1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a0 = t[i] + t[8 + i], a1 = t[4 + i] + t[12 + i], a2 = t[4 + i] - t[12 + i], a3 = t[i] - t[8 + i];
        o[i] = (a0 + a1) >> 1; o[4 + i] = (a3 + a2) >> 1; o[8 + i] = (a3 - a2) >> 1; o[12 + i] = (a0 - a1) >> 1;
    }
}

// the format's inverse Walsh-Hadamard transform: 16 Y2 coefficients -> the DC of the 16 luma blocks
__device__ __forceinline__ void iwht(const int *v, int *o) {
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a0 = v[i] + v[12 + i], a1 = v[4 + i] + v[8 + i], a2 = v[4 + i] - v[8 + i], a3 = v[i] - v[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int dc = t[4 * i] + 3, a0 = dc + t[4 * i + 3], a1 = t[4 * i + 1] + t[4 * i + 2];
        const int a2 = t[4 * i + 1] - t[4 * i + 2], a3 = dc - t[4 * i + 3];
        o[4 * i] = (a0 + a1) >> 3; o[4 * i + 1] = (a3 + a2) >> 3; o[4 * i + 2] = (a0 - a1) >> 3; o[4 * i + 3] = (a3 - a2) >> 3;
    }
}

// level of coefficient c at step q: (|c| + bias) / q with the sign of c, clamped to the token alphabet
__device__ __forceinline__ int quant(int c, int q, int bias) {
    const int l = min((abs(c) + bias) / q, kMaxLevel);
    return c < 0 ? -l : l;
}

// ---- macroblocks --------------------------------------------------------------------------------------------------------------
struct MbLds {
    uint8_t src[384], pred[384];      // Y 16x16, U 8x8, V 8x8
    int top[3][16], left[3][16], tl[3];
    int dcin[16], dcs[16];
    int y2nz;
};

// method 1: both luma candidates of a wave's macroblock, kept until the rule has chosen
struct MbLdsB {
    alignas(16) int16_t lev16[17 * 16];   // the 16x16 candidate's levels: Y2 and the 16 Y blocks, zigzag order
    int16_t levb[16 * 16];                // the B_PRED candidate's
    uint8_t rec16[256];                   // the 16x16 candidate's reconstruction
    uint8_t nb[17 * 24];                  // the B_PRED candidate's with its border: row 0 is the row above the macroblock from column -1
                                          // to column 19, column 0 the column to its left; rows 4, 8, 12 repeat columns 16..19 of row 0
    uint8_t bm[16], anyb[16];             // the sub-block modes; whether a sub-block has a non-zero level
};

__device__ __forceinline__ int bit_cost(int prob, int bit) { return vp8::kProbCost[(bit ? 256 - prob : prob) - 1]; }

// the coefficient-cost proxy of one block's 16 zigzag-ordered levels in 1/256 bit: nothing for an empty block, else one bit for the
// block, one for every zero before the last level and 1 + 2 * bit_length(|v|) for every level v
__device__ __forceinline__ int level_cost(const int16_t *lv) {
    int last = 15;
    while (last >= 0 && lv[last] == 0) --last;
    if (last < 0) return 0;
    int bits = 1;
    for (int i = 0; i <= last; ++i) {
        const int v = abs((int)lv[i]);
        bits += v ? 1 + 2 * (32 - __clz(v)) : 1;
    }
    return 256 * bits;
}

// the decisions of sub-block mode `mode` in the format's sub-block mode tree, each with its probability out of p[9]
template <class Put>
__device__ __forceinline__ void walk_bmode(int mode, const uint8_t *p, Put put) {
    put(p[0], mode != dec::B_DC);
    if (mode == dec::B_DC) return;
    put(p[1], mode != dec::B_TM);
    if (mode == dec::B_TM) return;
    put(p[2], mode != dec::B_VE);
    if (mode == dec::B_VE) return;
    const bool right = mode >= dec::B_LD;
    put(p[3], right);
    if (!right) {
        put(p[4], mode != dec::B_HE);
        if (mode != dec::B_HE) put(p[5], mode == dec::B_VR);
        return;
    }
    put(p[6], mode != dec::B_LD);
    if (mode == dec::B_LD) return;
    put(p[7], mode != dec::B_VL);
    if (mode == dec::B_VL) return;
    put(p[8], mode == dec::B_HU);
}

// One workgroup per frame, kWaves waves.  Diagonal d holds the macroblocks with mbx + mby = d; wave w takes those of index w,
// w + kWaves, ... along it.  Every wave runs the same number of rounds so that all of them meet every __syncthreads().
template <int M>
__global__ __launch_bounds__(kWaves * 64) void k_webp_mb(Geo g, int qi, const uint8_t *__restrict__ src, uint8_t *rec,
                                                        int16_t *__restrict__ levels, uint32_t *__restrict__ nz,
                                                        uint8_t *__restrict__ modes, uint32_t *__restrict__ nskip, uint8_t *bmodes,
                                                        uint8_t *y2c) {
    __shared__ MbLds sMb[kWaves];
    __shared__ MbLdsB sMbB[M ? kWaves : 1];                    // touched by method 1 alone
    const int f = blockIdx.x, wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    MbLds &S = sMb[wave];
    // method 1 walks diagonals of slope two: the macroblocks with mbx + 2 mby = d, whose neighbours to the left, above, above left
    // and above right all lie on earlier diagonals
    const int64_t frame = g.ypx + 2 * g.cpx;
    const uint8_t *sY = src + (int64_t)f * frame;
    uint8_t *rY = rec + (int64_t)f * frame;
    const int cw = g.Wp >> 1;
    const int dcq = vp8::kDcTable[qi], acq = vp8::kAcTable[qi];
    const int y2dc = 2 * dcq, y2ac = max(8, acq * 155 / 100), uvdc = min(dcq, 132);
    // this lane's samples: 4 luma in one row, 2 chroma in one row of U (lanes 0..31) or V
    const int ly = l >> 2, lx = (l & 3) * 4;
    const int cp = l >> 5, cy = (l & 31) >> 2, cx = (l & 3) * 2;

    for (int d = 0; d < (M ? g.mbw + 2 * (g.mbh - 1) : g.mbw + g.mbh - 1); ++d) {
        const int ylo = M ? max(0, (d - (g.mbw - 1) + 1) / 2) : max(0, d - (g.mbw - 1)), yhi = M ? min(d / 2, g.mbh - 1) : min(d, g.mbh - 1);
        const int len = yhi - ylo + 1;
        for (int it = 0; it * kWaves < len; ++it) {
            const int idx = it * kWaves + wave;
            const bool active = idx < len;                     // the same for all lanes of a wave
            const int mby = ylo + idx, mbx = M ? d - 2 * mby : d - mby;
            unsigned long long bal = 0;                        // lanes 0..23: the block has a non-zero level
            const int x0 = mbx * 16, y0 = mby * 16, ux0 = mbx * 8, uy0 = mby * 8;
            const int64_t m = (int64_t)f * g.nmb + (int64_t)mby * g.mbw + mbx;
            int ymode = 0, uvmode = 0;
            // A: the source samples and the borders of the three planes
            if (active) {
                *(uint32_t *)&S.src[16 * ly + lx] = *(const uint32_t *)&sY[(int64_t)(y0 + ly) * g.Wp + x0 + lx];
                const uint8_t *sC = sY + g.ypx + cp * g.cpx;
                *(uint16_t *)&S.src[256 + 64 * cp + 8 * cy + cx] = *(const uint16_t *)&sC[(int64_t)(uy0 + cy) * cw + ux0 + cx];
                if (l < 16) S.top[0][l] = mby ? rY[(int64_t)(y0 - 1) * g.Wp + x0 + l] : 127;
                else if (l < 32) S.left[0][l - 16] = mbx ? rY[(int64_t)(y0 + l - 16) * g.Wp + x0 - 1] : 129;
                else {
                    const int p = 1 + ((l - 32) >> 4), k = l & 7;
                    const uint8_t *rC = rY + g.ypx + (p - 1) * g.cpx;
                    if ((l & 8) == 0) S.top[p][k] = mby ? rC[(int64_t)(uy0 - 1) * cw + ux0 + k] : 127;
                    else S.left[p][k] = mbx ? rC[(int64_t)(uy0 + k) * cw + ux0 - 1] : 129;
                }
                if (l < 3) {
                    int v = mby ? 129 : 127;
                    if (mbx && mby) v = l == 0 ? rY[(int64_t)(y0 - 1) * g.Wp + x0 - 1]
                                               : rY[g.ypx + (l - 1) * g.cpx + (int64_t)(uy0 - 1) * cw + ux0 - 1];
                    S.tl[l] = v;
                }
                if constexpr (M) {
                    // the B_PRED candidate's border.  Above right (csm_vp8dec.h's rule): 127 above the frame, the last pixel above
                    // repeated in the last macroblock column, else the macroblock above and to the right, which is done
                    MbLdsB &B = sMbB[wave];
                    if (l < 21) {
                        int v = 127;
                        if (mby) {
                            const uint8_t *above = rY + (int64_t)(y0 - 1) * g.Wp + x0;
                            if (l == 0) v = mbx ? above[-1] : 129;
                            else if (l < 17) v = above[l - 1];
                            else v = mbx == g.mbw - 1 ? above[15] : above[l - 1];
                        }
                        B.nb[l] = (uint8_t)v;
                        if (l >= 17) B.nb[4 * 24 + l] = B.nb[8 * 24 + l] = B.nb[12 * 24 + l] = (uint8_t)v;
                    } else if (l >= 32 && l < 48) {
                        B.nb[(l - 31) * 24] = (uint8_t)(mbx ? rY[(int64_t)(y0 + l - 32) * g.Wp + x0 - 1] : 129);
                    }
                }
            }
            __syncthreads();
            // B: the four predictions of this lane's samples, their squared errors summed over the wave, the modes
            if (active) {
                int sse[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                int py[4][4], pc[4][2];
                {
                    int st = 0, sl = 0;
                    for (int k = 0; k < 16; ++k) { st += S.top[0][k]; sl += S.left[0][k]; }
                    const int dc = mbx && mby ? (st + sl + 16) >> 5 : mby ? (st + 8) >> 4 : mbx ? (sl + 8) >> 4 : 128;
                    const int lf = S.left[0][ly], t0 = S.tl[0];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int tp = S.top[0][lx + k], s = S.src[16 * ly + lx + k];
                        py[0][k] = dc; py[1][k] = tp; py[2][k] = lf; py[3][k] = clip8(lf + tp - t0);
#pragma unroll
                        for (int mo = 0; mo < 4; ++mo) sse[mo] += (py[mo][k] - s) * (py[mo][k] - s);
                    }
                }
                {
                    const int p = 1 + cp;
                    int st = 0, sl = 0;
                    for (int k = 0; k < 8; ++k) { st += S.top[p][k]; sl += S.left[p][k]; }
                    const int dc = mbx && mby ? (st + sl + 8) >> 4 : mby ? (st + 4) >> 3 : mbx ? (sl + 4) >> 3 : 128;
                    const int lf = S.left[p][cy], t0 = S.tl[p];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int tp = S.top[p][cx + k], s = S.src[256 + 64 * cp + 8 * cy + cx + k];
                        pc[0][k] = dc; pc[1][k] = tp; pc[2][k] = lf; pc[3][k] = clip8(lf + tp - t0);
#pragma unroll
                        for (int mo = 0; mo < 4; ++mo) sse[4 + mo] += (pc[mo][k] - s) * (pc[mo][k] - s);
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    for (int sh = 32; sh >= 1; sh >>= 1) sse[k] += __shfl_xor(sse[k], sh, 64);
#pragma unroll
                for (int mo = 1; mo < 4; ++mo) {               // strict: ties go to the lower mode number
                    if (sse[mo] < sse[ymode]) ymode = mo;
                    if (sse[4 + mo] < sse[4 + uvmode]) uvmode = mo;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    S.pred[16 * ly + lx + k] = (uint8_t)(ymode == 0 ? py[0][k] : ymode == 1 ? py[1][k] : ymode == 2 ? py[2][k] : py[3][k]);
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    S.pred[256 + 64 * cp + 8 * cy + cx + k] =
                        (uint8_t)(uvmode == 0 ? pc[0][k] : uvmode == 1 ? pc[1][k] : uvmode == 2 ? pc[2][k] : pc[3][k]);
            }
            __syncthreads();
            // C: lanes 0..23 take one 4x4 block each: 16 of Y, 4 of U, 4 of V
            int c[16];
            int boff = 0, bstride = 16;                        // the block's first sample in S.src / S.pred, its row stride
            if (l < 16) { boff = 64 * (l >> 2) + 4 * (l & 3); }
            else if (l < 24) { boff = 256 + 64 * ((l - 16) >> 2) + 32 * ((l >> 1) & 1) + 4 * (l & 1); bstride = 8; }
            if (active && l < 24) {
                int dd[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int o = boff + bstride * (k >> 2) + (k & 3);
                    dd[k] = (int)S.src[o] - (int)S.pred[o];
                }
                fdct(dd, c);
                if (l < 16) S.dcin[l] = c[0];
            }
            __syncthreads();
            // D: lane 0 takes the Y2 block: the luma DCs through the WHT, quantised, and back
            if (active && l == 0) {
                int v[16], w[16], lev[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = S.dcin[k];
                fwht(v, w);
                int any = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int q = k ? y2ac : y2dc;
                    lev[k] = quant(w[k], q, k ? (3 * q) >> 3 : q >> 1);
                    any |= lev[k];
                    w[k] = lev[k] * q;
                }
                int16_t *L = levels + m * 400;
                if constexpr (M) L = sMbB[wave].lev16;         // method 1: the luma candidate stays in LDS until the rule has chosen
#pragma unroll
                for (int k = 0; k < 16; ++k) L[k] = (int16_t)lev[vp8::kZigzag[k]];
                iwht(w, v);
#pragma unroll
                for (int k = 0; k < 16; ++k) S.dcs[k] = v[k];
                S.y2nz = any != 0;
            }
            __syncthreads();
            // E: quantise, store the levels, reconstruct as a decoder does
            if (active) {
                int any = 0;
                if (l < 24) {
                    const int q0 = l < 16 ? acq : uvdc;
                    int lev[16], r[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int q = k ? acq : q0;
                        lev[k] = (k == 0 && l < 16) ? 0 : quant(c[k], q, k ? (3 * q) >> 3 : q >> 1);
                        any |= lev[k];
                        c[k] = lev[k] * q;
                    }
                    if (l < 16) c[0] = S.dcs[l];
                    int16_t *L = levels + m * 400 + 16 * (1 + l);
                    if constexpr (M) { if (l < 16) L = sMbB[wave].lev16 + 16 * (1 + l); }
#pragma unroll
                    for (int k = 0; k < 16; ++k) L[k] = (int16_t)lev[vp8::kZigzag[k]];
                    idct(c, r);
                    uint8_t *R;
                    int rs;
                    if (l < 16) { R = rY + (int64_t)(y0 + 4 * (l >> 2)) * g.Wp + x0 + 4 * (l & 3); rs = g.Wp; }
                    else {
                        R = rY + g.ypx + ((l - 16) >> 2) * g.cpx + (int64_t)(uy0 + 4 * ((l >> 1) & 1)) * cw + ux0 + 4 * (l & 1);
                        rs = cw;
                    }
                    if constexpr (M) { if (l < 16) { R = sMbB[wave].rec16 + boff; rs = 16; } }
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        R[(int64_t)rs * (k >> 2) + (k & 3)] = (uint8_t)clip8((int)S.pred[boff + bstride * (k >> 2) + (k & 3)] + r[k]);
                }
                bal = __ballot(any != 0);
                if constexpr (M == 0) {
                    if (l == 0) {
                        const uint32_t flags = (uint32_t)(bal & 0xFFFFFFu) << 1 | (uint32_t)S.y2nz;
                        nz[m] = flags;
                        modes[m] = (uint8_t)(ymode | uvmode << 2);
                        if (flags == 0) atomicAdd(nskip + f, 1u);
                    }
                }
            }
            __syncthreads();
            if constexpr (M) {
                MbLdsB &B = sMbB[wave];
                // F: the B_PRED candidate.  Sub-block (bx, by) predicts from the sub-blocks to its left, above and above right, so the
                // 16 of them are a wavefront bx + 2 by = t of 10 steps with at most two sub-blocks each; half a wave takes one:
                // 16 lanes per pixel and 5 of the ten modes, the squared errors summed over the 16, the smallest error with the
                // lower mode number on ties; the half's first lane then transforms, quantises and reconstructs into B.nb
                for (int t = 0; t < 10; ++t) {
                    const int by = max(0, (t - 2) >> 1) + (l >> 5), bx = t - 2 * by;
                    if (active && by <= min(3, t >> 1)) {
                        const int k = l & 31, py = (k >> 2) & 3, px = k & 3, half = k >> 4;
                        const uint8_t *N = B.nb + 4 * by * 24 + 4 * bx;        // the corner pixel above and to the left of the sub-block
                        int e[13];
#pragma unroll
                        for (int i = 0; i < 4; ++i) e[i] = N[(4 - i) * 24];
#pragma unroll
                        for (int i = 0; i < 9; ++i) e[4 + i] = N[i];
                        const int s = S.src[16 * (4 * by + py) + 4 * bx + px];
                        uint32_t rows[4];
                        int best = 0x7FFFFFFF;
                        for (int i = 0; i < 5; ++i) {
                            const int mode = 5 * half + i;
                            dec::predict4(mode, e, rows);
                            const int p = (int)((rows[py] >> (8 * px)) & 255u);
                            int err = (p - s) * (p - s);
                            for (int sh = 8; sh >= 1; sh >>= 1) err += __shfl_xor(err, sh, 64);
                            best = min(best, err * 16 + mode);                 // at most 16 * 255^2 * 16
                        }
                        best = min(best, __shfl_xor(best, 16, 64));
                        if (k == 0) {
                            const int mode = best & 15, b = 4 * by + bx;
                            dec::predict4(mode, e, rows);
                            int dd[16], cc[16], lev[16], r[16];
#pragma unroll
                            for (int i = 0; i < 16; ++i)
                                dd[i] = (int)S.src[16 * (4 * by + (i >> 2)) + 4 * bx + (i & 3)] - (int)((rows[i >> 2] >> (8 * (i & 3))) & 255u);
                            fdct(dd, cc);
                            int any = 0;
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int q = i ? acq : dcq;
                                lev[i] = quant(cc[i], q, i ? (3 * q) >> 3 : q >> 1);
                                any |= lev[i];
                                cc[i] = lev[i] * q;
                            }
#pragma unroll
                            for (int i = 0; i < 16; ++i) B.levb[16 * b + i] = (int16_t)lev[vp8::kZigzag[i]];
                            idct(cc, r);
#pragma unroll
                            for (int i = 0; i < 16; ++i)
                                B.nb[(4 * by + 1 + (i >> 2)) * 24 + 4 * bx + 1 + (i & 3)] =
                                    (uint8_t)clip8((int)((rows[i >> 2] >> (8 * (i & 3))) & 255u) + r[i]);
                            B.bm[b] = (uint8_t)mode;
                            B.anyb[b] = (uint8_t)(any != 0);
                        }
                    }
                    __syncthreads();
                }
                // G: the rule.  J = D + ((3 ac^2 R) >> kRdShift) for both candidates: D the squared error of the reconstruction, R the
                // mode bits (kProbCost) plus the level proxy; B_PRED wins only when its J is smaller
                if (active) {
                    int d16 = 0, db = 0, r16 = 0, rb = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int s = S.src[16 * ly + lx + k];
                        const int a = B.rec16[16 * ly + lx + k], c2 = B.nb[(1 + ly) * 24 + 1 + lx + k];
                        d16 += (s - a) * (s - a);
                        db += (s - c2) * (s - c2);
                    }
                    if (l < 17) r16 = level_cost(B.lev16 + 16 * l);
                    if (l < 16) {
                        const int bx = l & 3, by = l >> 2;
                        const int above = by ? B.bm[l - 4] : mby ? bmodes[(m - g.mbw) * 16 + 12 + bx] : dec::B_DC;
                        const int left = bx ? B.bm[l - 1] : mbx ? bmodes[(m - 1) * 16 + 4 * by + 3] : dec::B_DC;
                        rb = level_cost(B.levb + 16 * l);
                        walk_bmode(B.bm[l], vp8::kBModeProbs + (above * 10 + left) * 9, [&](int p, int bit) { rb += bit_cost(p, bit); });
                    }
                    for (int sh = 32; sh >= 1; sh >>= 1) {
                        d16 += __shfl_xor(d16, sh, 64); db += __shfl_xor(db, sh, 64);
                        r16 += __shfl_xor(r16, sh, 64); rb += __shfl_xor(rb, sh, 64);
                    }
                    r16 += bit_cost(vp8::kYModeProbs[0], 1) + bit_cost(vp8::kYModeProbs[1], ymode >> 1) +
                           bit_cost(ymode >> 1 ? vp8::kYModeProbs[3] : vp8::kYModeProbs[2], ymode & 1);
                    rb += bit_cost(vp8::kYModeProbs[0], 0);
                    const int64_t lam = 3 * (int64_t)acq * acq;
                    const bool isb = db + ((lam * rb) >> kRdShift) < d16 + ((lam * r16) >> kRdShift);
                    // the chosen candidate's levels, reconstruction and sub-block modes to global memory
                    const int implied = ymode == 0 ? dec::B_DC : ymode == 1 ? dec::B_VE : ymode == 2 ? dec::B_HE : dec::B_TM;
                    if (l < 17 && (isb ? l >= 1 : true)) {
                        const uint4 *from = (const uint4 *)(isb ? B.levb + 16 * (l - 1) : B.lev16 + 16 * l);
                        uint4 *to = (uint4 *)(levels + m * 400 + 16 * l);
                        to[0] = from[0]; to[1] = from[1];
                    }
                    if (l < 16) bmodes[m * 16 + l] = (uint8_t)(isb ? B.bm[l] : implied);
                    *(uint32_t *)&rY[(int64_t)(y0 + ly) * g.Wp + x0 + lx] =
                        isb ? (uint32_t)B.nb[(1 + ly) * 24 + 1 + lx] | (uint32_t)B.nb[(1 + ly) * 24 + 2 + lx] << 8 |
                                  (uint32_t)B.nb[(1 + ly) * 24 + 3 + lx] << 16 | (uint32_t)B.nb[(1 + ly) * 24 + 4 + lx] << 24
                            : *(const uint32_t *)&B.rec16[16 * ly + lx];
                    const unsigned long long balb = __ballot(l < 16 && B.anyb[l & 15] != 0);
                    if (l == 0) {
                        // a B_PRED macroblock has no Y2 block: it neither reads nor writes that context and hands on what it was given
                        const uint32_t flags = isb ? (uint32_t)(balb & 0xFFFFu) << 1 | (uint32_t)(bal & 0xFF0000u) << 1
                                                   : (uint32_t)(bal & 0xFFFFFFu) << 1 | (uint32_t)S.y2nz;
                        const int in_l = mbx ? y2c[m - 1] & 1 : 0, in_t = mby ? (y2c[m - g.mbw] >> 1) & 1 : 0;
                        nz[m] = flags;
                        modes[m] = (uint8_t)(ymode | uvmode << 2 | (isb ? 16 : 0));
                        y2c[m] = (uint8_t)(isb ? in_l | in_t << 1 : (flags & 1) * 3);
                        if (flags == 0) atomicAdd(nskip + f, 1u);
                    }
                }
                __syncthreads();
            }
        }
    }
}

// the tables the coder walks, copied to LDS once per workgroup: a probability is then an LDS read, not a dependent global load
struct CodeTables {
    uint8_t probs[1056], update[1056], bands[20], cat[24];
};
constexpr int kLevStride = 201;              // dwords of a lane's 25 * 16 levels in LDS, odd so that the lanes spread over the banks

// one block's tokens: 16 zigzag-ordered levels coded from position `first` with the probabilities of block type `kind`
// (`probs`: the frame's 1056 coefficient probabilities; method 0 passes the defaults in T)
__device__ __forceinline__ void code_block(csm::BoolEnc &e, const CodeTables &T, const uint8_t *probs, const int16_t *lv, int first, int kind,
                                           int ctx, bool has) {
    const uint8_t *P = probs + kind * 264;
    const uint8_t *p = P + T.bands[first] * 33 + ctx * 11;
    e.put(p[0], has);
    if (!has) return;
    int last = 15;
    while (last > first && lv[last] == 0) --last;
    int n = first;
    while (n < 16) {
        const int cf = lv[n++];
        int v = abs(cf);
        e.put(p[1], v != 0);
        if (v == 0) { p = P + T.bands[n] * 33; continue; }
        e.put(p[2], v > 1);
        if (v == 1) {
            p = P + T.bands[n] * 33 + 11;
        } else {
            e.put(p[3], v > 4);
            if (v <= 4) {
                e.put(p[4], v != 2);
                if (v != 2) e.put(p[5], v == 4);
            } else {
                e.put(p[6], v > 10);
                if (v <= 10) {
                    e.put(p[7], v > 6);
                    if (v <= 6) e.put(159, v == 6);
                    else { e.put(165, v >= 9); e.put(145, !(v & 1)); }
                } else {
                    int nb, toff;
                    if (v < 3 + (8 << 1))      { e.put(p[8], 0); e.put(p[9], 0);  v -= 3 + (8 << 0); nb = 3;  toff = 0; }
                    else if (v < 3 + (8 << 2)) { e.put(p[8], 0); e.put(p[9], 1);  v -= 3 + (8 << 1); nb = 4;  toff = 3; }
                    else if (v < 3 + (8 << 3)) { e.put(p[8], 1); e.put(p[10], 0); v -= 3 + (8 << 2); nb = 5;  toff = 7; }
                    else                       { e.put(p[8], 1); e.put(p[10], 1); v -= 3 + (8 << 3); nb = 11; toff = 12; }
                    for (int k = 0; k < nb; ++k) e.put(T.cat[toff + k], (v >> (nb - 1 - k)) & 1);
                }
            }
            p = P + T.bands[n] * 33 + 22;
        }
        e.put(128, cf < 0);
        if (n == 16) return;
        e.put(p[0], n <= last);
        if (n > last) return;
    }
}

// the frames a workgroup of k_webp_code<1> takes: whole frames, as many as fit its 64 lanes, at most kStage
__host__ __device__ inline int code_frames_per_block(int parts) { return 64 / (parts + 1) < kStage ? 64 / (parts + 1) : kStage; }

// the sub-block mode above and to the left of sub-block b of macroblock m (mbx, mby): inside the macroblock from bm, else the
// neighbour's stored modes, B_DC outside the frame
__device__ __forceinline__ const uint8_t *bmode_probs(const uint8_t *table, const uint8_t *bmodes, int64_t m, int mbx, int mby, int mbw, int b) {
    const int bx = b & 3, by = b >> 2;
    const int above = by ? bmodes[m * 16 + b - 4] : mby ? bmodes[(m - mbw) * 16 + 12 + bx] : dec::B_DC;
    const int left = bx ? bmodes[m * 16 + b - 1] : mbx ? bmodes[(m - 1) * 16 + 4 * by + 3] : dec::B_DC;
    return table + (above * 10 + left) * 9;
}

// One lane per unit: unit f * (parts + 1) is frame f's first partition, the units behind it its token partitions.  Method 1: a
// workgroup takes whole frames (code_frames_per_block), so that every lane's probabilities are one of the tables staged in LDS.
template <int M>
__global__ __launch_bounds__(64) void k_webp_code(Geo g, int qi, const int16_t *__restrict__ levels, const uint32_t *__restrict__ nz,
                                                   const uint8_t *__restrict__ modes, const uint32_t *__restrict__ nskip,
                                                   uint8_t *__restrict__ first, uint8_t *__restrict__ part,
                                                   int64_t *__restrict__ sizes, uint32_t *__restrict__ status,
                                                   const uint8_t *__restrict__ bmodes, const uint8_t *__restrict__ y2c,
                                                   const uint8_t *__restrict__ fprobs, const uint8_t *__restrict__ fupd) {
    __shared__ CodeTables T;
    __shared__ uint32_t sLev[64 * kLevStride];
    __shared__ uint8_t sProbs[M ? kStage * 1056 : 1], sBm[M ? 900 : 1];      // method 1: the frames' tables and kBModeProbs
    for (int i = threadIdx.x; i < 1056; i += 64) { T.probs[i] = vp8::kCoeffProbs[i]; T.update[i] = vp8::kCoeffUpdateProbs[i]; }
    if (threadIdx.x < 17) T.bands[threadIdx.x] = vp8::kBands[threadIdx.x];
    if (threadIdx.x < 23) T.cat[threadIdx.x] = vp8::kCat[threadIdx.x];
    int u = blockIdx.x * 64 + threadIdx.x;
    const uint8_t *probs = T.probs;
    if constexpr (M) {
        const int fpb = code_frames_per_block(g.parts), f0 = blockIdx.x * fpb, fl = threadIdx.x / (g.parts + 1);
        for (int i = threadIdx.x; i < fpb * 1056; i += 64) {
            const int fr = f0 + i / 1056;
            if (fr < g.n) sProbs[i] = fprobs[(int64_t)fr * 1056 + i % 1056];
        }
        for (int i = threadIdx.x; i < 900; i += 64) sBm[i] = vp8::kBModeProbs[i];
        u = fl < fpb && f0 + fl < g.n ? f0 * (g.parts + 1) + threadIdx.x : g.units;
        probs = sProbs + min(fl, fpb - 1) * 1056;
    }
    __syncthreads();
    if (u >= g.units) return;
    const int f = u / (g.parts + 1), k = u - f * (g.parts + 1);
    uint32_t *myLev = sLev + threadIdx.x * kLevStride;
    const int64_t mb0 = (int64_t)f * g.nmb;
    csm::BoolEnc e;
    if (k == 0) {
        e.open(first + (int64_t)f * g.first_cap, g.first_cap);
        const int prob_skip = max(1, (int)(((int64_t)(g.nmb - (int)nskip[f]) * 255) / g.nmb));
        e.put_bits(0, 3);                      // colour space 0, clamping needed, no segmentation
        e.put_bits(1, 1);                      // simple loop filter
        e.put_bits(qi >> 2, 6);                // its level
        e.put_bits(0, 4);                      // sharpness 0, no filter deltas
        e.put_bits(g.log2p, 2);
        e.put_bits(qi, 7);
        e.put_bits(0, 6);                      // no quantiser deltas; refresh_entropy_probs 0
        if constexpr (M) {
            const uint8_t *U = fupd + (int64_t)f * 1056;
            for (int i = 0; i < 1056; ++i) {
                const int flag = U[i];
                e.put(T.update[i], flag);
                if (flag) e.put_bits(probs[i], 8);
            }
        } else {
            for (int i = 0; i < 1056; ++i) e.put(T.update[i], 0);
        }
        e.put_bits(1, 1);                      // mb_no_coeff_skip
        e.put_bits(prob_skip, 8);
        for (int i = 0; i < g.nmb; ++i) {
            const int mo = modes[mb0 + i], ym = mo & 3, uv = M ? (mo >> 2) & 3 : mo >> 2;
            e.put(prob_skip, nz[mb0 + i] == 0);
            if (M && (mo & 16)) {
                e.put(vp8::kYModeProbs[0], 0); // B_PRED: the 16 sub-block modes, each in the context of its neighbours above and to the left
                const int mby = i / g.mbw, mbx = i - mby * g.mbw;
                for (int b = 0; b < 16; ++b)
                    walk_bmode(bmodes[(mb0 + i) * 16 + b], bmode_probs(sBm, bmodes, mb0 + i, mbx, mby, g.mbw, b),
                               [&](int p, int bit) { e.put(p, bit); });
            } else {
                e.put(vp8::kYModeProbs[0], 1);     // not B_PRED
                e.put(vp8::kYModeProbs[1], ym >> 1);
                e.put(ym >> 1 ? vp8::kYModeProbs[3] : vp8::kYModeProbs[2], ym & 1);
            }
            e.put(vp8::kUvModeProbs[0], uv != 0);
            if (uv != 0) {
                e.put(vp8::kUvModeProbs[1], uv != 1);
                if (uv != 1) e.put(vp8::kUvModeProbs[2], uv == 3);
            }
        }
    } else {
        const int p = k - 1;
        e.open(part + ((int64_t)f * g.parts + p) * g.part_cap, g.part_cap);
        for (int mby = p; mby < g.mbh; mby += g.parts) {
            for (int mbx = 0; mbx < g.mbw; ++mbx) {
                const int64_t m = mb0 + (int64_t)mby * g.mbw + mbx;
                const uint32_t cur = nz[m];
                if (cur == 0) continue;                        // skipped: no tokens
                const uint32_t lf = mbx ? nz[m - 1] : 0, tf = mby ? nz[m - g.mbw] : 0;
                // the levels of the blocks that have any, from global memory to this lane's LDS in one round of independent loads
                const uint4 *G = (const uint4 *)(levels + m * 400);
                for (int b = 0; b < 25; ++b) {
                    if (!((cur >> b) & 1)) continue;
                    const uint4 lo = G[2 * b], hi = G[2 * b + 1];
                    uint32_t *d = myLev + 8 * b;
                    d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w; d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
                }
                const int16_t *L = (const int16_t *)myLev;
                // method 1: a B_PRED macroblock has no Y2 block and codes its luma blocks whole, as type 3; the Y2 context of the
                // others is the one carried past B_PRED macroblocks (y2c), not the neighbour's own flag
                bool bpred = false;
                if constexpr (M) {
                    bpred = (modes[m] & 16) != 0;
                    if (!bpred) code_block(e, T, probs, L, 0, 1, (mbx ? y2c[m - 1] & 1 : 0) + (mby ? (y2c[m - g.mbw] >> 1) & 1 : 0), cur & 1);
                } else {
                    code_block(e, T, probs, L, 0, 1, (int)(lf & 1) + (int)(tf & 1), cur & 1);
                }
                for (int b = 0; b < 16; ++b) {
                    const int bx = b & 3, by = b >> 2;
                    const int cl = bx ? (cur >> b) & 1 : (lf >> (4 * by + 4)) & 1;          // bit 1 + b - 1; bit 1 + 4 by + 3
                    const int ct = by ? (cur >> (b - 3)) & 1 : (tf >> (13 + bx)) & 1;       // bit 1 + b - 4; bit 1 + 12 + bx
                    code_block(e, T, probs, L + 16 * (1 + b), M && bpred ? 0 : 1, M && bpred ? 3 : 0, cl + ct, (cur >> (1 + b)) & 1);
                }
                for (int b = 0; b < 8; ++b) {
                    const int base = 17 + (b & 4), bx = b & 1, by = (b >> 1) & 1, bit = base + 2 * by + bx;
                    const int cl = bx ? (cur >> (bit - 1)) & 1 : (lf >> (bit + 1)) & 1;
                    const int ct = by ? (cur >> (bit - 2)) & 1 : (tf >> (bit + 2)) & 1;
                    code_block(e, T, probs, L + 16 * bit, 0, 2, cl + ct, (cur >> bit) & 1);
                }
            }
        }
    }
    sizes[u] = e.finish();
    if (e.over) atomicOr(status, 1u);
}

// ---- method 1: the frame's branch counts and its probabilities ----------------------------------------------------------------------
// code_block's walk with a counter in place of the coder: cnt[2 * entry + bit] for every decision that reads one of the 1056
// probabilities (the fixed ones -- extra bits, signs -- are not counted)
__device__ __forceinline__ void count_block(uint32_t *cnt, const uint8_t *bands, const int16_t *lv, int first, int kind, int ctx, bool has) {
    const int P = kind * 264;
    int p = P + bands[first] * 33 + ctx * 11;
    atomicAdd(&cnt[2 * p + has], 1u);
    if (!has) return;
    int last = 15;
    while (last > first && lv[last] == 0) --last;
    int n = first;
    while (n < 16) {
        const int v = abs((int)lv[n++]);
        atomicAdd(&cnt[2 * (p + 1) + (v != 0)], 1u);
        if (v == 0) { p = P + bands[n] * 33; continue; }
        atomicAdd(&cnt[2 * (p + 2) + (v > 1)], 1u);
        if (v == 1) {
            p = P + bands[n] * 33 + 11;
        } else {
            atomicAdd(&cnt[2 * (p + 3) + (v > 4)], 1u);
            if (v <= 4) {
                atomicAdd(&cnt[2 * (p + 4) + (v != 2)], 1u);
                if (v != 2) atomicAdd(&cnt[2 * (p + 5) + (v == 4)], 1u);
            } else {
                atomicAdd(&cnt[2 * (p + 6) + (v > 10)], 1u);
                if (v <= 10) {
                    atomicAdd(&cnt[2 * (p + 7) + (v > 6)], 1u);
                } else {
                    const int hi = v >= 3 + (8 << 2);
                    atomicAdd(&cnt[2 * (p + 8) + hi], 1u);
                    atomicAdd(&cnt[2 * (p + 9 + hi) + (hi ? v >= 3 + (8 << 3) : v >= 3 + (8 << 1))], 1u);
                }
            }
            p = P + bands[n] * 33 + 22;
        }
        if (n == 16) return;
        atomicAdd(&cnt[2 * p + (n <= last)], 1u);
        if (n > last) return;
    }
}

// One lane per 4x4 block slot (25 per macroblock) of a frame.  A block's kind, first position and context follow from the
// masks, the B_PRED marks and the carried Y2 contexts, exactly as k_webp_code<1> derives them, so blocks are independent.  The
// counts go to LDS first and from there, where not zero, to the frame's counters: integer sums, the same whatever the order.
__global__ __launch_bounds__(kBlock) void k_webp_stats(Geo g, const int16_t *__restrict__ levels, const uint32_t *__restrict__ nz,
                                                        const uint8_t *__restrict__ modes, const uint8_t *__restrict__ y2c,
                                                        uint32_t *__restrict__ counts) {
    __shared__ uint32_t sCnt[2112];
    __shared__ uint32_t sLv[kBlock * 9];                       // a lane's 16 levels; 9 dwords apart, so that the lanes spread over the banks
    __shared__ uint8_t sBands[20];
    const int per = (g.nmb * 25 + kBlock - 1) / kBlock, f = blockIdx.x / per, t = threadIdx.x;      // `per` workgroups per frame
    for (int i = t; i < 2112; i += kBlock) sCnt[i] = 0;
    if (t < 17) sBands[t] = vp8::kBands[t];
    __syncthreads();
    const int i = (blockIdx.x - f * per) * kBlock + t;
    if (i < g.nmb * 25) {
        const int mb = i / 25, slot = i - mb * 25, mby = mb / g.mbw, mbx = mb - mby * g.mbw;
        const int64_t m = (int64_t)f * g.nmb + mb;
        const uint32_t cur = nz[m];
        const bool bpred = (modes[m] & 16) != 0;
        if (cur != 0 && !(bpred && slot == 0)) {               // a skipped macroblock codes no token, a B_PRED one no Y2 block
            const uint32_t lf = mbx ? nz[m - 1] : 0, tf = mby ? nz[m - g.mbw] : 0;
            const bool has = (cur >> slot) & 1;
            uint32_t *my = sLv + t * 9;
            if (has) {
                const uint4 *G = (const uint4 *)(levels + m * 400 + 16 * slot);
                const uint4 lo = G[0], hi = G[1];
                my[0] = lo.x; my[1] = lo.y; my[2] = lo.z; my[3] = lo.w; my[4] = hi.x; my[5] = hi.y; my[6] = hi.z; my[7] = hi.w;
            }
            int first = 0, kind, ctx;
            if (slot == 0) {
                kind = 1;
                ctx = (mbx ? y2c[m - 1] & 1 : 0) + (mby ? (y2c[m - g.mbw] >> 1) & 1 : 0);
            } else if (slot < 17) {
                const int b = slot - 1, bx = b & 3, by = b >> 2;
                kind = bpred ? 3 : 0;
                first = bpred ? 0 : 1;
                ctx = (int)(bx ? (cur >> b) & 1 : (lf >> (4 * by + 4)) & 1) + (int)(by ? (cur >> (b - 3)) & 1 : (tf >> (13 + bx)) & 1);
            } else {
                const int b = slot - 17, bx = b & 1, by = (b >> 1) & 1;
                kind = 2;
                ctx = (int)(bx ? (cur >> (slot - 1)) & 1 : (lf >> (slot + 1)) & 1) + (int)(by ? (cur >> (slot - 2)) & 1 : (tf >> (slot + 2)) & 1);
            }
            count_block(sCnt, sBands, (const int16_t *)my, first, kind, ctx, has);
        }
    }
    __syncthreads();
    for (int k = t; k < 2112; k += kBlock)
        if (sCnt[k]) atomicAdd(&counts[(int64_t)f * 2112 + k], sCnt[k]);
}

// One lane per probability of a frame: p_new = clamp(1, 255, (255 c0 + (c0 + c1) / 2) / (c0 + c1)); the entry is updated
// exactly when the saving c0 (C[old] - C[new]) + c1 (C[256 - old] - C[256 - new]) exceeds 8 * 256 + C[256 - u] - C[u], the price of
// a set flag with its 8 bits over a clear one (C = kProbCost, u the flag's probability)
__global__ __launch_bounds__(kBlock) void k_webp_probs(const uint32_t *__restrict__ counts, uint8_t *__restrict__ probs, uint8_t *__restrict__ upd) {
    const int per = (1056 + kBlock - 1) / kBlock, f = blockIdx.x / per, i = (blockIdx.x - f * per) * kBlock + threadIdx.x;
    if (i >= 1056) return;
    const int64_t c0 = counts[(int64_t)f * 2112 + 2 * i], c1 = counts[(int64_t)f * 2112 + 2 * i + 1];
    const int old = vp8::kCoeffProbs[i], u = vp8::kCoeffUpdateProbs[i];
    int p = old, flag = 0;
    if (c0 + c1 > 0) {
        const int cand = (int)min((int64_t)255, max((int64_t)1, (255 * c0 + (c0 + c1) / 2) / (c0 + c1)));
        const int64_t saving = c0 * ((int)vp8::kProbCost[old - 1] - (int)vp8::kProbCost[cand - 1]) +
                               c1 * ((int)vp8::kProbCost[255 - old] - (int)vp8::kProbCost[255 - cand]);
        if (saving > 8 * 256 + (int)vp8::kProbCost[255 - u] - (int)vp8::kProbCost[u - 1]) { p = cand; flag = 1; }
    }
    probs[(int64_t)f * 1056 + i] = (uint8_t)p;
    upd[(int64_t)f * 1056 + i] = (uint8_t)flag;
}

// one workgroup: offs[u] = the bytes of the units before u; info[u] = (offset, bytes), info[units] = (status, total)
__global__ __launch_bounds__(kBlock) void k_webp_offsets(int units, const int64_t *__restrict__ sizes, const uint32_t *__restrict__ status,
                                                          int64_t *__restrict__ offs, int64_t *__restrict__ info) {
    __shared__ int64_t sScan[kBlock];
    const int t = threadIdx.x;
    const int per = (units + kBlock - 1) / kBlock, u0 = min(units, t * per), u1 = min(units, u0 + per);
    int64_t sum = 0, total;
    for (int u = u0; u < u1; ++u) sum += sizes[u];
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int u = u0; u < u1; ++u) { offs[u] = ex; info[2 * u] = ex; info[2 * u + 1] = sizes[u]; ex += sizes[u]; }
    if (t == 0) { info[2 * units] = *status; info[2 * units + 1] = total; }
}

// one workgroup per unit copies its bytes; nothing is read past the unit's segment or written past out_bytes
__global__ __launch_bounds__(kBlock) void k_webp_pack(Geo g, const uint8_t *__restrict__ first, const uint8_t *__restrict__ part,
                                                       const int64_t *__restrict__ sizes, const int64_t *__restrict__ offs,
                                                       uint8_t *__restrict__ out, int64_t out_bytes) {
    const int u = blockIdx.x, f = u / (g.parts + 1), k = u - f * (g.parts + 1);
    const uint8_t *seg = k ? part + ((int64_t)f * g.parts + (k - 1)) * g.part_cap : first + (int64_t)f * g.first_cap;
    const int64_t off = offs[u], bytes = min(min(sizes[u], k ? g.part_cap : g.first_cap), max(out_bytes - off, (int64_t)0));
    for (int64_t i = threadIdx.x; i < bytes; i += kBlock) out[off + i] = seg[i];
}

int webp_stage(int stage, const uint8_t *frames, int n, int H, int W, int quality, int method, int64_t *info, void *scratch, void *stream) {
    Geo g;
    CSM_REQUIRE(method == 0 || method == 1);
    CSM_REQUIRE(make_geo(n, H, W, g, method));
    CSM_REQUIRE(quality >= 1 && quality <= 100 && stage >= 1 && stage <= 4);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(frames && info && scratch);
    const Scratch sc = make_scratch(g, scratch, method);
    hipStream_t st = (hipStream_t)stream;
    const int qi = quality_to_qi(quality);
    switch (stage) {
    case 1:
        k_webp_yuv<<<csm::cdiv(n * g.cpx, kBlock), kBlock, 0, st>>>(frames, g, sc.src);
        return csm::check_launch("k_webp_yuv");
    case 2:
        CSM_HIP(hipMemsetAsync(sc.nskip, 0, (size_t)(n + 1) * 4, st));       // the skip counts and the status word behind them
        if (method) k_webp_mb<1><<<n, kWaves * 64, 0, st>>>(g, qi, sc.src, sc.rec, sc.levels, sc.nz, sc.modes, sc.nskip, sc.bmodes, sc.y2c);
        else k_webp_mb<0><<<n, kWaves * 64, 0, st>>>(g, qi, sc.src, sc.rec, sc.levels, sc.nz, sc.modes, sc.nskip, nullptr, nullptr);
        return csm::check_launch("k_webp_mb");
    case 3:
        if (method) {                          // the frame's branch counts, its probabilities, then the coder that reads them
            CSM_HIP(hipMemsetAsync(sc.counts, 0, (size_t)n * 2112 * 4, st));
            k_webp_stats<<<n * csm::cdiv(g.nmb * 25, kBlock), kBlock, 0, st>>>(g, sc.levels, sc.nz, sc.modes, sc.y2c, sc.counts);
            if (const int rc = csm::check_launch("k_webp_stats")) return rc;
            k_webp_probs<<<n * csm::cdiv(1056, kBlock), kBlock, 0, st>>>(sc.counts, sc.probs, sc.upd);
            if (const int rc = csm::check_launch("k_webp_probs")) return rc;
            k_webp_code<1><<<csm::cdiv(n, code_frames_per_block(g.parts)), 64, 0, st>>>(g, qi, sc.levels, sc.nz, sc.modes, sc.nskip, sc.first,
                                                                                        sc.part, sc.sizes, sc.status, sc.bmodes, sc.y2c,
                                                                                        sc.probs, sc.upd);
        } else {
            k_webp_code<0><<<csm::cdiv(g.units, 64), 64, 0, st>>>(g, qi, sc.levels, sc.nz, sc.modes, sc.nskip, sc.first, sc.part, sc.sizes,
                                                                  sc.status, nullptr, nullptr, nullptr, nullptr);
        }
        return csm::check_launch("k_webp_code");
    default:
        k_webp_offsets<<<1, kBlock, 0, st>>>(g.units, sc.sizes, sc.status, sc.offs, info);
        return csm::check_launch("k_webp_offsets");
    }
}

int webp_write(int n, int H, int W, int method, uint8_t *out, int64_t out_bytes, void *scratch, void *stream) {
    Geo g;
    CSM_REQUIRE(method == 0 || method == 1);
    CSM_REQUIRE(make_geo(n, H, W, g, method));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(out && scratch && out_bytes > 0);
    const Scratch sc = make_scratch(g, scratch, method);
    k_webp_pack<<<g.units, kBlock, 0, (hipStream_t)stream>>>(g, sc.first, sc.part, sc.sizes, sc.offs, out, out_bytes);
    return csm::check_launch("k_webp_pack");
}

}  // namespace

extern "C" size_t csm_webp_scratch_bytes(int n, int H, int W) { return csm_webp_scratch_bytes_m(n, H, W, 0); }

extern "C" size_t csm_webp_scratch_bytes_m(int n, int H, int W, int method) {
    Geo g;
    if ((method != 0 && method != 1) || !make_geo(n, H, W, g, method)) return 0;
    return (size_t)make_scratch(g, nullptr, method).total;
}

extern "C" int csm_webp_stage(int stage, const uint8_t *frames, int n, int H, int W, int quality, int64_t *info, void *scratch,
                              void *stream) {
    return webp_stage(stage, frames, n, H, W, quality, 0, info, scratch, stream);
}

extern "C" int csm_webp_stage_m(int stage, const uint8_t *frames, int n, int H, int W, int quality, int method, int64_t *info,
                                void *scratch, void *stream) {
    return webp_stage(stage, frames, n, H, W, quality, method, info, scratch, stream);
}

extern "C" int csm_webp_measure(const uint8_t *frames, int n, int H, int W, int quality, int64_t *info, void *scratch, void *stream) {
    return csm_webp_measure_m(frames, n, H, W, quality, 0, info, scratch, stream);
}

extern "C" int csm_webp_measure_m(const uint8_t *frames, int n, int H, int W, int quality, int method, int64_t *info, void *scratch,
                                  void *stream) {
    for (int stage = 1; stage <= 4; ++stage) {
        const int rc = webp_stage(stage, frames, n, H, W, quality, method, info, scratch, stream);
        if (rc) return rc;
    }
    return CSM_OK;
}

extern "C" int csm_webp_write(int n, int H, int W, uint8_t *out, int64_t out_bytes, void *scratch, void *stream) {
    return webp_write(n, H, W, 0, out, out_bytes, scratch, stream);
}

extern "C" int csm_webp_write_m(int n, int H, int W, int method, uint8_t *out, int64_t out_bytes, void *scratch, void *stream) {
    return webp_write(n, H, W, method, out, out_bytes, scratch, stream);
}
