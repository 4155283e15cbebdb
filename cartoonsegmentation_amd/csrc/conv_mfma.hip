// conv_mfma.hip -- k_conv_mfma: the register-staged implicit-GEMM convolution on the exact-fp32 matrix pipe.  It runs every layer the
// LDS-DMA kernels (conv_dma.hip, conv_patch.hip) cannot: channel counts that are no multiple of 32, unaligned views, > 2 GiB views.
// Design and numerical contract: see nets.hip and include/csm355.h.
#include "csm_convcfg.h"

using namespace csmconv;

namespace {

// Implicit-GEMM convolution on the exact-fp32 matrix pipe.
//   MT = 32: v_mfma_f32_32x32x2_f32, wave tile 32 x (32*TN); LDS rows hold 32 channels in natural order, a lane
//            (i, h) reads float4 at channel 4h of each 8-block: MFMA t multiplies channels (t, 4+t).
//   MT = 16: v_mfma_f32_16x16x4_f32, wave tile 16 x (16*TN) -- 4x more tiles for small feature maps, so that all
//            1024 SIMDs get work.  LDS 8-blocks are stored permuted [0,2,4,6,1,3,5,7]; lane (i, g) reads float2 at
//            position 2g: MFMA 1 multiplies channels (0,4,1,5), MFMA 2 (2,6,3,7).
// Both give the contract's chain order 0,4,1,5,2,6,3,7 per 8-block, so they are bit-identical to each other.
// FULLK: cin_g % 32 == 0, every chunk is 4 full 8-channel blocks -> the MFMA phase is straight-line code (no branch
// around it: a branch makes hipcc copy the 16 accumulator registers out and back every chunk behind a full MFMA drain).
// SER (split-K executed serially): csm_op.ksplit = S cuts K into S runs of chunks, each its own fmaf chain, summed ((p0+p1)+p2)...
// -- that is part of the NUMERICAL contract and follows the per-sample shape only.  How the runs are EXECUTED is a speed decision:
// S blocks along grid z writing raw partials + k_splitk_reduce (small grids: batch 1), or -- SER -- one block that walks all S
// runs and combines them in registers at the run boundaries (`tot = tot + acc; acc = 0`: the same fp32 additions in the same
// order), so a batched program produces the bits of the single-frame program without the partial-sum traffic.
template <int MT, int WM, int WN, int TN, bool FULLK, bool SER = false>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN >= 8 ? 4 : 2)) void k_conv_mfma(ConvArgs a) {
    constexpr int NT = 64 * WM * WN;
    constexpr int BM = MT * WM, BN = MT * WN * TN;
    constexpr int A_IT = (BM * 8 + NT - 1) / NT, B_IT = (BN * 8 + NT - 1) / NT;
    constexpr bool A_FULL = A_IT * NT == BM * 8, B_FULL = B_IT * NT == BN * 8;
    constexpr int NACC = MT == 32 ? 16 : 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kStage = (BM + BN) * kLdsLd;   // floats per pipeline stage: A rows then B rows

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = MT == 32 ? (lane & 31) : (lane & 15);
    const int lh = MT == 32 ? (lane >> 5) : (lane >> 4);

    int mt, ntile, zz;
    block_to_tile(mt, ntile, zz);
    const int m0 = mt * BM, n0 = ntile * BN;
    const int g = SER ? zz : zz / a.ksplit, ks = SER ? 0 : zz - g * a.ksplit;
    const int ho = a.out.h, wo = a.out.w;
    const int cin_off = g * a.cin_g, cout_off = g * a.cout_g;

    // Per-thread A rows (output pixels): base pointer of the receptive-field origin and a per-tap validity mask,
    // computed once; the K loop then only adds block-uniform offsets (no integer divisions, ~2 VALU per load).
    const float *rowp[A_IT]; unsigned long long vmask[A_IT];
    const int c4 = (tid & 7) * 4;
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        int row = (tid + NT * it) >> 3;
        int m = m0 + row;
        bool rv = m < a.M && (A_FULL || row < BM);
        int mm = rv ? m : 0;
        int n = mm / (ho * wo), rem = mm - n * ho * wo;
        int oy = rem / wo, ox = rem - oy * wo;
        int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
        rowp[it] = a.in.p + ((int64_t)(n * a.in.h + iy0) * a.in.w + ix0) * a.in.ld + cin_off + c4;
        unsigned long long vm = 0ull;
        if (rv)
            for (int kh = 0; kh < a.kh; ++kh)
                for (int kw = 0; kw < a.kw; ++kw) {
                    int iy = iy0 + kh * a.dil, ix = ix0 + kw * a.dil;
                    if (iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w) vm |= 1ull << (kh * a.kw + kw);
                }
        vmask[it] = vm;
    }
    const int Tall = a.kh * a.kw * a.ncb;
    const int c_begin = SER ? 0 : (int)(((int64_t)ks * Tall) / a.ksplit), T = SER ? Tall : (int)(((int64_t)(ks + 1) * Tall) / a.ksplit);
    // loader state = the NEXT chunk to fetch (block-uniform -> SGPRs).  Chunk order = the chain order: 32-channel block outer,
    // taps row-major inner (so that a 3x3 kernel can keep one block's input patch in LDS for all its taps, k_conv_patch).
    const int ntaps = a.kh * a.kw;
    int l_cb = c_begin / ntaps, l_tap = c_begin - l_cb * ntaps;
    int l_kh = l_tap / a.kw, l_kw = l_tap - l_kh * a.kw;
    const float *wp[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it)
        wp[it] = a.w + ((int64_t)g * Tall + c_begin) * a.npad * 32 + (int64_t)(n0 + ((tid + NT * it) >> 3)) * 32 + c4;

    // two register sets: loads run TWO chunks ahead of the MFMAs (set = parity of the chunk), so a chunk's HBM/L2 latency
    // is covered by two full compute phases; hipcc emits the counted vmcnt that leaves the younger set in flight.
    float4 ra[2][A_IT] = {}, rb[2][B_IT] = {};
    unsigned vbits[2] = {0u, 0u};           // validity of each load of a set (A: bit it, B: bit 8+it); zeros are applied at the LDS store
    auto gload = [&](const int set, const bool live) {   // always issues the same number of loads (see below)
        const int64_t toff = ((int64_t)l_kh * a.dil * a.in.w + l_kw * a.dil) * a.in.ld + l_cb * 32;
        const bool cv = live && !(CSM_DBG(a) & 1) && (FULLK || l_cb * 32 + c4 < a.cin_g);
        unsigned vb = 0u;
        // Loads are UNCONDITIONAL and their count per step is fixed (dead lanes / dead steps read a safe address): a branch
        // around a load makes hipcc fall back to vmcnt(0..3) at the next use, which would serialise the two-deep prefetch.
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            bool v = cv && ((vmask[it] >> l_tap) & 1ull);
            const float *p = v ? rowp[it] + toff : a.in.p;
            ra[set][it] = *reinterpret_cast<const float4 *>(p);
            vb |= v ? (1u << it) : 0u;
        }
#pragma unroll
        for (int it = 0; it < B_IT; ++it) {
            int row = (tid + NT * it) >> 3;
            bool v = live && !(CSM_DBG(a) & 1) && n0 + row < a.npad && (B_FULL || row < BN);
            const float *p = v ? wp[it] : a.w;
            rb[set][it] = *reinterpret_cast<const float4 *>(p);
            vb |= v ? (1u << (8 + it)) : 0u;
            wp[it] += (int64_t)a.npad * 32;
        }
        vbits[set] = vb;
        ++l_tap;
        if (++l_kw == a.kw) { l_kw = 0; if (++l_kh == a.kh) { l_kh = 0; l_tap = 0; ++l_cb; } }
    };
    auto put = [&](float *dst, float4 v) {
        if (MT == 32) *reinterpret_cast<float4 *>(dst + c4) = v;
        else {  // permuted 8-block [0,2,4,6,1,3,5,7]
            float *b8 = dst + (c4 & ~7) + 2 * ((c4 >> 2) & 1);
            *reinterpret_cast<float2 *>(b8) = make_float2(v.x, v.z);
            *reinterpret_cast<float2 *>(b8 + 4) = make_float2(v.y, v.w);
        }
    };
    auto lstore = [&](const int set, int buf) {
        if (CSM_DBG(a) & 4) return;
#pragma unroll
        for (int it = 0; it < A_IT; ++it)
            if (A_FULL || ((tid + NT * it) >> 3) < BM)
                put(lds + buf * kStage + ((tid + NT * it) >> 3) * kLdsLd, (vbits[set] >> it) & 1u ? ra[set][it] : make_float4(0.f, 0.f, 0.f, 0.f));
#pragma unroll
        for (int it = 0; it < B_IT; ++it)
            if (B_FULL || ((tid + NT * it) >> 3) < BN)
                put(lds + buf * kStage + (BM + ((tid + NT * it) >> 3)) * kLdsLd, (vbits[set] >> (8 + it)) & 1u ? rb[set][it] : make_float4(0.f, 0.f, 0.f, 0.f));
    };

    // accumulators start at the (folded-BN) bias
    float acc[TN][NACC];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        int n = n0 + MT * (TN * wn + tn) + li;
        float b = (a.bias && ks == 0 && n < a.cout_g) ? a.bias[cout_off + n] : 0.0f;
#pragma unroll
        for (int r = 0; r < NACC; ++r) acc[tn][r] = b;
    }

    auto kblock = [&](const float *A, const float *B, int kb) {
        if (MT == 32) {
            float4 af = *reinterpret_cast<const float4 *>(A + kb * 8);
            float4 bf[TN];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bf[tn] = *reinterpret_cast<const float4 *>(B + tn * 32 * kLdsLd + kb * 8);
            const float av[4] = {af.x, af.y, af.z, af.w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const float bv = t == 0 ? bf[tn].x : (t == 1 ? bf[tn].y : (t == 2 ? bf[tn].z : bf[tn].w));
                    f32x16 c;
#pragma unroll
                    for (int r = 0; r < 16; ++r) c[r] = acc[tn][r];
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv, c, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tn][r] = c[r];
                }
        } else {
            float2 af = *reinterpret_cast<const float2 *>(A + kb * 8);
            float2 bf[TN];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bf[tn] = *reinterpret_cast<const float2 *>(B + tn * 16 * kLdsLd + kb * 8);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    f32x4v c;
#pragma unroll
                    for (int r = 0; r < 4; ++r) c[r] = acc[tn][r];
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(t == 0 ? af.x : af.y, t == 0 ? bf[tn].x : bf[tn].y, c, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[tn][r] = c[r];
                }
        }
    };

    int cb = c_begin / ntaps, ctap = c_begin - cb * ntaps;      // position of the chunk being multiplied
    float tot[SER ? TN : 1][SER ? NACC : 1];
    int run = 0, next_b = SER ? (int)((int64_t)Tall / a.ksplit) : 0;          // SER: first chunk of the next run
    auto compute = [&](int chunk) {
        if constexpr (SER) {
            if (chunk == next_b) {                                             // block-uniform: S - 1 times per block
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int r = 0; r < NACC; ++r) { tot[tn][r] = run == 0 ? acc[tn][r] : tot[tn][r] + acc[tn][r]; acc[tn][r] = 0.0f; }
                ++run; next_b = (int)(((int64_t)(run + 1) * Tall) / a.ksplit);
            }
        }
        const int buf = chunk & 1;
        const float *A = lds + buf * kStage + (MT * wm + li) * kLdsLd + (MT == 32 ? 4 : 2) * lh;
        const float *B = lds + buf * kStage + (BM + MT * TN * wn + li) * kLdsLd + (MT == 32 ? 4 : 2) * lh;
        if (CSM_DBG(a) & 2) return;
        if (FULLK) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) kblock(A, B, kb);
        } else {
            int rem = a.cin_g - cb * 32;
            if (++ctap == ntaps) { ctap = 0; ++cb; }
            int nkb = rem >= 32 ? 4 : (rem + 7) >> 3;
#pragma unroll 1
            for (int kb = 0; kb < nkb; ++kb) kblock(A, B, kb);
        }
    };
    gload(0, true);                             // chunk c_begin     -> set 0
    lstore(0, c_begin & 1);
    gload(1, c_begin + 1 < T);                  // chunk c_begin + 1 -> set 1, stays in flight
    __syncthreads();
    int chunk = c_begin;
    for (; chunk + 1 < T; chunk += 2) {
        gload(0, chunk + 2 < T);                // two ahead
        compute(chunk);
        lstore(1, (chunk + 1) & 1);             // needs only the older set: counted vmcnt keeps set 0 in flight
        __syncthreads();
        gload(1, chunk + 3 < T);
        compute(chunk + 1);
        lstore(0, (chunk + 2) & 1);             // (a dead step stores zeros into the idle buffer)
        __syncthreads();
    }
    if (chunk < T) compute(chunk);

    // epilogue.  MT=32: lane holds column li, rows (r&3)+8*(r>>2)+4*lh.  MT=16: column li, rows 4*lh + r.
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        int n = n0 + MT * (TN * wn + tn) + li;
        if (n >= a.cout_g) continue;
        float slope = a.slope ? a.slope[cout_off + n] : 0.0f;
        const int mb = m0 + MT * wm + 4 * lh;
        auto val = [&](int r) { if constexpr (SER) return tot[tn][r] + acc[tn][r]; else return acc[tn][r]; };
        auto eo = [](int r) { return (int64_t)(MT == 32 ? (r & 3) + 8 * (r >> 2) : r); };
        auto ok = [&](int r) { return mb + (MT == 32 ? (r & 3) + 8 * (r >> 2) : r) < a.M; };
        if (CSM_DBG(a) & 8) {
#pragma unroll
            for (int r = 0; r < NACC; ++r)
                if (ok(r) && val(r) == 123.456f) a.out.p[0] = val(r);
        } else if (!SER && a.ksplit > 1)
            conv_tail_partial<NACC>(a.partial + ((int64_t)mb * a.ksplit + ks) * a.cout_g + n, (int64_t)a.ksplit * a.cout_g, val, ok, eo);
        else
            conv_tail<NACC>(a, slope, a.out.p + (int64_t)mb * a.out.ld + cout_off + n, a.out.ld,
                            a.res_mode ? a.res.p + (int64_t)mb * a.res.ld + cout_off + n : nullptr, a.res.ld, val, ok, eo);
    }
}

template <int MT, int WM, int WN, int TN, bool FULLK, bool SER>
int launch_conv_k(const ConvArgs &a0, hipStream_t st) {
    constexpr int BM = MT * WM, BN = MT * WN * TN;
    ConvArgs a = a0;
    a.m_tiles = (a.M + BM - 1) / BM;
    size_t lds = (size_t)2 * (BM + BN) * kLdsLd * sizeof(float);
    static KernelPrep prep;
    (void)prep.ensure([&] { return prepare_kernel(&k_conv_mfma<MT, WM, WN, TN, FULLK, SER>, 64 * WM * WN, lds); });
    dim3 grid(a.m_tiles, (a.cout_g + BN - 1) / BN, a.groups * (SER ? 1 : a.ksplit));
    k_conv_mfma<MT, WM, WN, TN, FULLK, SER><<<grid, 64 * WM * WN, lds, st>>>(a);
    int rc = csm::check_launch("k_conv_mfma");
    if (rc || SER || a.ksplit <= 1) return rc;
    return launch_reduce(a, st);
}

template <int MT, int WM, int WN, int TN>
int launch_conv(const ConvArgs &a, hipStream_t st) {
    const bool full = (a.cin_g & 31) == 0;
    if (a.ksplit > 1 && a.serial) return full ? launch_conv_k<MT, WM, WN, TN, true, true>(a, st) : launch_conv_k<MT, WM, WN, TN, false, true>(a, st);
    return full ? launch_conv_k<MT, WM, WN, TN, true, false>(a, st) : launch_conv_k<MT, WM, WN, TN, false, false>(a, st);
}

// ---- table rows: BN = MT * WN * TN
template <int MT, int WM, int WN, int TN>
constexpr ConvCfg mfma_cfg(int id, const char *name) { return {id, name, FAM_MFMA, MT * WN * TN, &launch_conv<MT, WM, WN, TN>}; }
#define ROW(NAME, ...) mfma_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
constexpr ConvCfg kRows[] = {
    ROW(128x128_4w, 32, 4, 1, 4), ROW(128x64, 32, 4, 1, 2), ROW(64x64, 32, 2, 2, 1), ROW(128x128_8w, 32, 4, 2, 2), ROW(128x32, 32, 4, 1, 1),
    ROW(64x16, 16, 4, 1, 1),
};
#undef ROW

}  // namespace

std::span<const ConvCfg> csmconv::conv_cfgs_mfma() { return kRows; }
