// conv_patch.hip -- the 3x3 (stride 1, dilation 1) convolutions that keep the input patch of a tile in LDS for all nine taps:
// k_conv_patch, its persistent form k_conv_patch_p and the weights-stationary k_conv_ws, with their launchers.
#include "csm_convcfg.h"
#include "csm_convtile.h"

using namespace csmconv;

namespace {

// Swizzle key of patch pixel pp = py * PW + px (k_conv_patch / k_conv_patch_p): the 16-B slot s of a pixel's 128-B row lives at physical slot
// s ^ key.  A ds_read_b128 is serviced in groups of 16 lanes, conflict-free when they hit 16 distinct 16-B bank slots, i.e. distinct
// (px & 1, key) -- the row pitch of 128 B makes the pixel's parity the upper half of the bank slot, and PW is even.  The 16 lanes of a group
// read 16 tile pixels: with a 16-wide tile they have 16 consecutive px (key = px >> 1 suffices, whatever their rows); with an 8-wide tile 8
// consecutive px on rows of either parity (+ 4 for odd rows).  Round 3 used the key of the LINEAR index ((pp >> 1) & 7), which the 18-pixel
// row pitch of the patch misaligns: two of every sixteen lanes collided and every A-fragment read took 8 LDS cycles instead of 4
// (SQ_LDS_BANK_CONFLICT = 40 % of SQ_LDS_IDX_ACTIVE, profiles/r04_conv_pmc.txt).
template <int PW, int TW> __device__ __forceinline__ int patch_key(int pp) {
    const int py = pp / PW, px = pp - py * PW;
    return ((px >> 1) + (TW == 8 ? 4 * (py & 1) : 0)) & 7;
}

// ---- 3x3 (stride 1, dilation 1) convolution with input-patch re-use -------------------------------------------------------
// k_conv_dma moves the A tile (BM pixels x 32 channels) once per (32-channel block, tap): nine times per block for a 3x3.
// The micro-benchmark (tools/ubench/glds_loop.hip, "A/5") shows that LDS-DMA volume is what costs MFMA rate (64x64 tile:
// 74 % -> 81 %, 128x128: 83 % -> 87 % when the A moves drop five-fold), so here the output tile is a TH x TW pixel rectangle
// and the block keeps the (TH+2) x (TW+2) x 32-channel input PATCH of the current channel block in LDS for all nine taps
// (the chain order is block-major for exactly this reason): the A fragment of output pixel (y, x) under tap (kh, kw) is patch
// pixel (y+kh, x+kw).  Patch: 2 stages (the next block's patch is fetched during the first tap of the current one); weights:
// 2 stages, one tile per tap.  Same 128-B rows / XOR swizzle / buffer-range-check zero fill / raw barrier as k_conv_dma.
template <int WM, int WN, int TM, int TN, int TW, bool SER = false>
__global__ __launch_bounds__(64 * WM * WN, 2) void k_conv_patch(ConvArgs a, int tiles_x, int tiles_y) {
    constexpr int NW = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, TH = BM / TW;
    constexpr int PH = TH + 2, PW = TW + 2, NPIX = PH * PW;
    constexpr int NPP = (NPIX + 7) / 8;                         // patch DMA pieces (8 pixels each)
    constexpr int QP = (NPP + NW - 1) / NW;                     // per wave
    constexpr int GB = BN / 8 / NW;
    static_assert(GB * 8 * NW == BN && TH * TW == BM && (TW == 16 || TW == 8), "tile shape");
    constexpr int kPatchF = QP * NW * 8 * 32, kBF = BN * 32;    // floats per patch stage (every wave's QP pieces have a home) / weight stage
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [patch 0][patch 1][B 0][B 1]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    int mt, ntile, zz;
    block_to_tile(mt, ntile, zz, a.ngroup);
    const int tx = mt % tiles_x, ty = (mt / tiles_x) % tiles_y, n = mt / (tiles_x * tiles_y);
    const int n0 = ntile * BN;
    const int g = SER ? zz : zz / a.ksplit, ks = SER ? 0 : zz - g * a.ksplit;
    const int ho = a.out.h, wo = a.out.w;
    const int cin_off = g * a.cin_g, cout_off = g * a.cout_g;
    const int Tall = 9 * a.ncb;
    const int c_begin = SER ? 0 : (int)(((int64_t)ks * Tall) / a.ksplit), T = SER ? Tall : (int)(((int64_t)(ks + 1) * Tall) / a.ksplit);

    i32x4 ra, rb;
    {
        uint64_t pa = (uint64_t)a.in.p, pb = (uint64_t)a.w;
        unsigned na = (unsigned)((((int64_t)a.in.n * a.in.h * a.in.w - 1) * a.in.ld + a.in.c) * 4);
        unsigned nb = (unsigned)((int64_t)a.groups * Tall * a.npad * 128);
        ra = i32x4{(int)(unsigned)pa, (int)(unsigned)(pa >> 32), (int)na, 0x00020000};
        rb = i32x4{(int)(unsigned)pb, (int)(unsigned)(pb >> 32), (int)nb, 0x00020000};
    }
    // patch loader: wave w owns pieces w, w+NW, ...; lane -> patch pixel 8*piece + lane/8, physical slot lane%8
    unsigned offP[QP], offB[GB];
    const int iy0 = ty * TH - a.pad, ix0 = tx * TW - a.pad;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        int pp = 8 * (wave + q * NW) + (lane >> 3);
        int slot = (lane & 7) ^ patch_key<PW, TW>(pp);
        int py = pp / PW, px = pp - py * PW;
        int iy = iy0 + py, ix = ix0 + px;
        bool v = pp < NPIX && iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w;
        offP[q] = v ? (unsigned)(((n * a.in.h + iy) * a.in.w + ix) * a.in.ld + cin_off + slot * 4) * 4u : kOob;
    }
#pragma unroll
    for (int p = 0; p < GB; ++p) {
        int row = 8 * (wave * GB + p) + (lane >> 3);
        int slot = (lane & 7) ^ ((row >> 1) & 7);
        offB[p] = n0 + row < a.npad ? (unsigned)((n0 + row) * 32 + slot * 4) * 4u : kOob;
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const unsigned ldsB = lds0 + (unsigned)(2 * kPatchF * 4) + (unsigned)(wave * GB * 8) * 128u;

    // all 32-channel rows of block cb -> patch stage cb & 1.  Branch-free (a branch around the asm makes hipcc shuffle the
    // accumulators): `live` false turns every lane out of range, the DMA then writes zeros into a stage nobody reads any more.
    auto issue_patch = [&](int cb, bool live) {
        const unsigned sb = lds0 + (unsigned)(cb & 1) * (unsigned)(kPatchF * 4);
#pragma unroll
        for (int q = 0; q < QP; ++q)
            dma16((offP[q] == kOob || !live) ? kOob : offP[q] + (unsigned)cb * 128u, ra, sb + (unsigned)(wave + q * NW) * 1024u);
    };
    unsigned l_w = (unsigned)(((int64_t)g * Tall + c_begin) * a.npad * 128);
    auto issue_b = [&](int stage) {
#pragma unroll
        for (int p = 0; p < GB; ++p)
            dma16(offB[p] == kOob ? kOob : offB[p] + l_w, rb, ldsB + (unsigned)stage * (unsigned)(kBF * 4) + (unsigned)p * 1024u);
        l_w += (unsigned)a.npad * 128u;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        int nn = n0 + 32 * (TN * wn + j) + li;
        float b = (a.bias && ks == 0 && nn < a.cout_g) ? a.bias[cout_off + nn] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = b;
    }
    // MFMA row li of sub-tile t = TM*wm + i is tile pixel 32 t + li = (py, px); its patch pixel under tap (kh, kw) is
    // ppb[i] + kh*PW + kw
    int ppb[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int rr = 32 * (TM * wm + i) + li;
        ppb[i] = (rr / TW) * PW + (rr % TW);
    }
    int swb[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) swb[kb] = frag_slot(kb, li, lh);
    const int rowB = (32 * TN * wn + li) * 32;
    f32x16 tot[SER ? TM : 1][SER ? TN : 1];
    int run = 0, next_b = SER ? (int)((int64_t)Tall / a.ksplit) : 0;          // SER: first chunk of the next run
    auto compute = [&](int cb, int tap, int bstage) {
        if constexpr (SER) {
            if (9 * cb + tap == next_b) {                                      // block-uniform: S - 1 times per block
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) { tot[i][j][r] = run == 0 ? acc[i][j][r] : tot[i][j][r] + acc[i][j][r]; acc[i][j][r] = 0.0f; }
                ++run; next_b = (int)(((int64_t)(run + 1) * Tall) / a.ksplit);
            }
        }
        const float *SP = lds + (cb & 1) * kPatchF;
        const float *SB = lds + 2 * kPatchF + bstage * kBF;
        const int kh = tap / 3, toff = kh * PW + (tap - 3 * kh);
        int arow[TM], asw[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) { int pp = ppb[i] + toff; arow[i] = pp * 32; asw[i] = patch_key<PW, TW>(pp); }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4 *>(SP + arow[i] + (((2 * kb + lh) ^ asw[i]) << 2));
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4 *>(SB + rowB + j * 1024 + swb[kb]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float av = t == 0 ? af[i].x : (t == 1 ? af[i].y : (t == 2 ? af[i].z : af[i].w));
                        const float bv = t == 0 ? bf[j].x : (t == 1 ? bf[j].y : (t == 2 ? bf[j].z : bf[j].w));
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
                    }
        }
    };

    int cb = c_begin / 9, tap = c_begin - 9 * cb;
    issue_patch(cb, true);
    issue_b(0);
    for (int chunk = c_begin, st = 0; chunk < T;) {
        const int tap_end = min(9, tap + (T - chunk));
        // first chunk of this channel block: the weights of the next chunk AND the next block's patch go out behind the barrier
        // (the weight fetch is unconditional: past the end of this K run it lands in a stage nobody reads)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // (lgkmcnt: see k_conv_dma_p)
        __builtin_amdgcn_s_barrier();
        issue_b(st ^ 1);
        issue_patch(cb + 1, (cb + 1) * 9 < T);
        compute(cb, tap, st);
        ++chunk; st ^= 1;
        for (++tap; tap < tap_end; ++tap, ++chunk, st ^= 1) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            issue_b(st ^ 1);
            compute(cb, tap, st);
        }
        tap = 0; ++cb;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (dead) fetches must land before the block's LDS is released

    // epilogue: the pixel index is computed once per accumulator row and shared by the TN column tiles
    float slope[TN]; int ncol[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        ncol[j] = n0 + 32 * (TN * wn + j) + li;
        slope[j] = (a.slope && ncol[j] < a.cout_g) ? a.slope[cout_off + ncol[j]] : 0.0f;
    }
    // (one row pointer per accumulator: a lane's 16 pixels sit at compile-time (dy, dx) from its first one -- 4 lh + (r & 3) never carries
    // into the next tile row -- so an element's address is pointer + a UNIFORM offset, no per-element 64-bit multiply)
    const int64_t ldo = a.out.ld, ldr = a.res.ld;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int oyb = ty * TH + (32 / TW) * (TM * wm + i), oxb = tx * TW + 4 * lh;
        const int64_t mb = ((int64_t)n * ho + oyb) * wo + oxb;
        float *ob = a.out.p + mb * ldo + cout_off;
        const float *rb = a.res_mode ? a.res.p + mb * ldr + cout_off : nullptr;
        auto ok = [&](int r) { const int rl = (r & 3) + 8 * (r >> 2); return oyb + rl / TW < ho && oxb + rl % TW < wo; };
        auto eo = [&](int r) { const int rl = (r & 3) + 8 * (r >> 2); return (int64_t)(rl / TW) * wo + rl % TW; };
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nn = ncol[j];
            if (nn >= a.cout_g) continue;
            auto val = [&](int r) { if constexpr (SER) return tot[i][j][r] + acc[i][j][r]; else return acc[i][j][r]; };
            if (!SER && a.ksplit > 1) conv_tail_partial<16>(a.partial + (mb * a.ksplit + ks) * a.cout_g + nn, (int64_t)a.ksplit * a.cout_g, val, ok, eo);
            else conv_tail<16>(a, slope[j], ob + nn, ldo, rb + nn, ldr, val, ok, eo);
        }
    }
}

// ---- persistent form of k_conv_patch: the NEXT tile's input patch is fetched during the current tile's taps -------------------------
// With 32 or 64 input channels a tile has one or two channel blocks: k_conv_patch fetches the tile's only (first) patch in its
// prologue, the one DMA round trip of the tile that nothing hides (all blocks of a CU run in lock-step), and the plain DMA kernel has
// one chunk of MFMAs (1.7 us at four 128x32 blocks per CU) to hide every HBM miss behind.  Here a block walks several tiles and the
// sequence of (tile, channel block) patches is double-buffered ACROSS tiles: at the first tap of a tile's last channel block the
// loader switches to the next tile and sends its first patch -- nine taps of MFMAs ahead of its use; the weights of the next tile's
// first tap go out behind the barrier of the last tap.  Same chunks, same chain per output.  SER: the serial split-K walk of k_conv_patch
// (runs combined in registers at the run boundaries); parallel split-K layers keep the one-tile-per-block kernel.
// MINW = waves per SIMD the register allocation must allow (launch bound): 4 caps the 8-wave 128 x 128 tile at 128 VGPRs, so that TWO
// blocks (2 x 80 KB of LDS) share a CU instead of one
template <int WM, int WN, int TM, int TN, int TW, bool SER = false, int MINW = 2, bool ILV = (CSM_ILV != 0)>
__global__ __launch_bounds__(64 * WM * WN, MINW) void k_conv_patch_p(ConvArgs a, int tiles_x, int tiles_y, int n_n, int total) {
    constexpr int NW = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, TH = BM / TW;
    constexpr int PH = TH + 2, PW = TW + 2, NPIX = PH * PW;
    constexpr int NPP = (NPIX + 7) / 8;
    constexpr int QP = (NPP + NW - 1) / NW;
    constexpr int GB = BN / 8 / NW;
    static_assert(GB * 8 * NW == BN && TH * TW == BM && (TW == 16 || TW == 8), "tile shape");
    constexpr int kPPT = (QP + 7) / 8, kPT = (QP + kPPT - 1) / kPPT;      // patch pieces per tap / taps that carry a slice (<= 8)
    // the counted wait `vmcnt(kPPT)` at the tap after a slice assumes that the slice had exactly kPPT pieces behind the weights: a shorter
    // last slice would let a weight DMA be in flight at the barrier
    static_assert(QP % kPPT == 0, "every patch slice must carry kPPT pieces (counted vmcnt)");
    constexpr int kPatchF = QP * NW * 8 * 32, kBF = BN * 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [patch 0][patch 1][B 0][B 1]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const int ho = a.out.h, wo = a.out.w;
    const int ncb = a.ncb, Tall = 9 * ncb;
    const int per = (int)(gridDim.x >> 3), x = (int)(blockIdx.x & 7u), i0 = (int)(blockIdx.x >> 3);
    const int q = total >> 3, r = total & 7;
    const int start = x * q + (x < r ? x : r), len = q + (x < r ? 1 : 0);
    if (i0 >= len) return;
    const int per_z = a.m_tiles * n_n, per_img = tiles_x * tiles_y;

    i32x4 ra, rb;
    {
        uint64_t pa = (uint64_t)a.in.p, pb = (uint64_t)a.w;
        unsigned na = (unsigned)((((int64_t)a.in.n * a.in.h * a.in.w - 1) * a.in.ld + a.in.c) * 4);
        unsigned nb = (unsigned)((int64_t)a.groups * Tall * a.npad * 128);
        ra = i32x4{(int)(unsigned)pa, (int)(unsigned)(pa >> 32), (int)na, 0x00020000};
        rb = i32x4{(int)(unsigned)pb, (int)(unsigned)(pb >> 32), (int)nb, 0x00020000};
    }
    auto tile_of = [&](int k, int &mt, int &nt, int &g) {
        const int j = start + k; g = j / per_z;
        rem_to_tile((unsigned)(j - g * per_z), (unsigned)a.m_tiles, (unsigned)n_n, a.ngroup, mt, nt);
    };
    // patch loader (tile being fetched): wave w owns pieces w, w+NW, ...; lane -> patch pixel 8*piece + lane/8, physical slot lane%8
    unsigned offP[QP], offB[GB];
    auto patch_setup = [&](int k, bool live) {
        int mt, nt, g; tile_of(k, mt, nt, g);
        const int tx = mt % tiles_x, ty = (mt / tiles_x) % tiles_y, n = mt / per_img;
        const int iy0 = ty * TH - a.pad, ix0 = tx * TW - a.pad, cin_off = g * a.cin_g;
#pragma unroll
        for (int qq = 0; qq < QP; ++qq) {
            int pp = 8 * (wave + qq * NW) + (lane >> 3);
            int slot = (lane & 7) ^ patch_key<PW, TW>(pp);
            int py = pp / PW, px = pp - py * PW;
            int iy = iy0 + py, ix = ix0 + px;
            bool v = live && pp < NPIX && iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w;
            offP[qq] = v ? (unsigned)(((n * a.in.h + iy) * a.in.w + ix) * a.in.ld + cin_off + slot * 4) * 4u : kOob;
        }
    };
    unsigned l_w = 0u;
    auto b_setup = [&](int k, bool live) {
        int mt, nt, g; tile_of(k, mt, nt, g);
        const int n0 = nt * BN;
#pragma unroll
        for (int p = 0; p < GB; ++p) {
            int row = 8 * (wave * GB + p) + (lane >> 3);
            int slot = (lane & 7) ^ ((row >> 1) & 7);
            offB[p] = (live && n0 + row < a.npad) ? (unsigned)((n0 + row) * 32 + slot * 4) * 4u : kOob;
        }
        l_w = (unsigned)((int64_t)g * Tall * a.npad * 128);
    };
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const unsigned ldsB = lds0 + (unsigned)(2 * kPatchF * 4) + (unsigned)(wave * GB * 8) * 128u;
    auto issue_patch = [&](int cb, int pstage) {               // all 32-channel rows of block cb of the tile offP describes
        const unsigned sb = lds0 + (unsigned)pstage * (unsigned)(kPatchF * 4);
#pragma unroll
        for (int qq = 0; qq < QP; ++qq)
            dma16(offP[qq] == kOob ? kOob : offP[qq] + (unsigned)cb * 128u, ra, sb + (unsigned)(wave + qq * NW) * 1024u);
    };
    auto issue_b = [&](int stage) {
#pragma unroll
        for (int p = 0; p < GB; ++p)
            dma16(offB[p] == kOob ? kOob : offB[p] + l_w, rb, ldsB + (unsigned)stage * (unsigned)(kBF * 4) + (unsigned)p * 1024u);
        l_w += (unsigned)a.npad * 128u;
    };

    int ppb[TM];
    int abase[TM][3][4];                                        // (patch pixel of MFMA row li) * 32 + swizzled 16-B slot, per tap column kw and k-block
    static_assert(TW == 16, "abase: the swizzle key of a 16-wide tile depends on the patch column only");
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int rr = 32 * (TM * wm + i) + li;
        ppb[i] = (rr / TW) * PW + (rr % TW);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) abase[i][kw][kb] = ppb[i] * 32 + (((2 * kb + lh) ^ ((((rr % TW) + kw) >> 1) & 7)) << 2);
    }
    int swb[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) swb[kb] = frag_slot(kb, li, lh);
    const int rowB = (32 * TN * wn + li) * 32;
    SerialRuns<SER, TM, TN> runs;                               // (reset per tile)
    f32x16 acc[TM][TN];
    auto compute = [&](int pstage, int tap, int bstage) {
        const float *SP = lds + pstage * kPatchF;
        const float *SB = lds + 2 * kPatchF + bstage * kBF;
        const int kh = tap / 3, toff = kh * PW + (tap - 3 * kh);
        int arow[TM], asw[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) { int pp = ppb[i] + toff; arow[i] = pp * 32; asw[i] = patch_key<PW, TW>(pp); }
        mfma_chunk(acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(SP + arow[i] + (((2 * kb + lh) ^ asw[i]) << 2)); },
                   [&](int kb, int j) { return *reinterpret_cast<const float4 *>(SB + rowB + j * 1024 + swb[kb]); });
    };

    patch_setup(i0, true);
    b_setup(i0, true);
    issue_patch(0, 0);
    issue_b(0);
    int ps = 0, st = 0;                                         // stage of the patch / of the weights about to be consumed
    for (int k = i0; k < len; k += per) {
        int mt, nt, g; tile_of(k, mt, nt, g);
        const int tx = mt % tiles_x, ty = (mt / tiles_x) % tiles_y, n = mt / per_img;
        const int n0 = nt * BN, cout_off = g * a.cout_g;
        const int kn = k + per;
        const bool more = kn < len;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int nn = n0 + 32 * (TN * wn + j) + li;
            float b = (a.bias && nn < a.cout_g) ? a.bias[cout_off + nn] : 0.0f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[i][j][rr] = b;
        }
        runs.begin(Tall, a.ksplit);
        for (int cb = 0; cb < ncb; ++cb, ps ^= 1) {
            const bool last_cb = cb + 1 == ncb;
            // The next patch of the sequence -- block cb + 1 of this tile or (last block) block 0 of the NEXT tile, for which the loader
            // state is switched at tap 0 -- goes out in SLICES of kPPT pieces behind the weights of taps 0 .. kPT - 1.  vmcnt retires in
            // order, so "at most kPPT outstanding" at the next barrier means the weights have landed and the slice may still fly:
            // every slice has two taps of MFMAs to arrive in (HBM misses included) instead of one.  Branch-free: past the end every
            // lane is out of range and the DMA writes zeros into a stage nobody reads.
            auto chunk = [&](auto TAPC) {
                constexpr int tap = decltype(TAPC)::value;
                // The nine taps are straight-line code: hipcc moves the barrier of tap t + 1 up between the last LDS reads of tap t and
                // the MFMAs that consume them, so a wave could pass the barrier with fragment reads still in flight while the next
                // DMA into that stage is issued behind it (a few wrong values in 10^7, seen once in the 8-wide 64 x 64 tile).  The
                // fragment reads of the previous tap must have COMPLETED before this wave arrives at the barrier:
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if constexpr (tap >= 1 && tap <= kPT) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kPPT) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if constexpr (tap == 0) { if (last_cb) patch_setup(more ? kn : k, more); }
                if constexpr (tap == 8) { if (last_cb) b_setup(more ? kn : k, more); }      // the weights of the next tile's first tap
                const unsigned psb = lds0 + (unsigned)(ps ^ 1) * (unsigned)(kPatchF * 4);
                const unsigned cbo = (unsigned)(last_cb ? 0 : cb + 1) * 128u;
                if constexpr (!ILV) {
                    issue_b(st ^ 1);
                    if constexpr (tap < kPT) {
#pragma unroll
                        for (int qq = tap * kPPT; qq < (tap + 1) * kPPT && qq < QP; ++qq)
                            dma16(offP[qq] == kOob ? kOob : offP[qq] + cbo, ra, psb + (unsigned)(wave + qq * NW) * 1024u);
                    }
                }
                runs.boundary(9 * cb + tap, acc, Tall, a.ksplit);
                if constexpr (!ILV) compute(ps, tap, st);
                else {
                    // the tap's MFMAs with this tap's DMA pieces between the groups (same order as the burst: the weights of the next tap
                    // first, then the patch slice -- the counted vmcnt at the next barrier relies on it); see k_conv_dma_p
                    constexpr int NSL = tap < kPT ? ((tap + 1) * kPPT <= QP ? kPPT : QP - tap * kPPT) : 0;
                    // fragment addresses = per-lane bases that do not depend on the tile (abase: 12 per accumulator row) + a tap constant + the
                    // stage: the nine unrolled taps used to keep 72 precomputed addresses per accumulator row alive (187 - 233 VGPRs)
                    constexpr int kh = tap / 3, kw = tap - 3 * kh, toff = kh * PW + kw;
                    const float *SP = lds + ps * kPatchF + toff * 32;
                    const float *SB = lds + 2 * kPatchF + st * kBF;
                    mfma_chunk_ilv<TM, TN, GB + NSL>(
                        acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(SP + abase[i][kw][kb]); },
                        [&](int kb, int j) { return *reinterpret_cast<const float4 *>(SB + rowB + j * 1024 + swb[kb]); },
                        [&](auto GC) {
                            constexpr int G = decltype(GC)::value;
                            if constexpr (G < GB)
                                dma16(offB[G] == kOob ? kOob : offB[G] + l_w, rb, ldsB + (unsigned)(st ^ 1) * (unsigned)(kBF * 4) + (unsigned)G * 1024u);
                            else {
                                constexpr int qq = tap * kPPT + (G - GB);
                                dma16(offP[qq] == kOob ? kOob : offP[qq] + cbo, ra, psb + (unsigned)(wave + qq * NW) * 1024u);
                            }
                        });
                    l_w += (unsigned)a.npad * 128u;
                }
                st ^= 1;
            };
            chunk(std::integral_constant<int, 0>{}); chunk(std::integral_constant<int, 1>{}); chunk(std::integral_constant<int, 2>{});
            chunk(std::integral_constant<int, 3>{}); chunk(std::integral_constant<int, 4>{}); chunk(std::integral_constant<int, 5>{});
            chunk(std::integral_constant<int, 6>{}); chunk(std::integral_constant<int, 7>{}); chunk(std::integral_constant<int, 8>{});
        }
        // epilogue
        float slope[TN]; int ncol[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            ncol[j] = n0 + 32 * (TN * wn + j) + li;
            slope[j] = (a.slope && ncol[j] < a.cout_g) ? a.slope[cout_off + ncol[j]] : 0.0f;
        }
        const int64_t ldo = a.out.ld, ldr = a.res.ld;              // (row pointers once per accumulator, as in k_conv_patch)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int oyb = ty * TH + (32 / TW) * (TM * wm + i), oxb = tx * TW + 4 * lh;
            const int64_t mb = ((int64_t)n * ho + oyb) * wo + oxb;
            float *ob = a.out.p + mb * ldo + cout_off;
            const float *rb = a.res_mode ? a.res.p + mb * ldr + cout_off : nullptr;
            auto ok = [&](int rr) { const int rl = (rr & 3) + 8 * (rr >> 2); return oyb + rl / TW < ho && oxb + rl % TW < wo; };
            auto eo = [&](int rr) { const int rl = (rr & 3) + 8 * (rr >> 2); return (int64_t)(rl / TW) * wo + rl % TW; };
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nn = ncol[j];
                if (nn >= a.cout_g) continue;
                conv_tail<16>(a, slope[j], ob + nn, ldo, rb + nn, ldr,
                              [&](int rr) { return runs.value(i, j, rr, acc); }, ok, eo);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (dead) fetches must land before the block's LDS is released
}

// ---- weights-stationary 3x3 convolution (stride 1, dilation 1, one K run): the block's WEIGHT PANEL stays in LDS --------------------------
// k_conv_patch(_p) stream a weight tile per tap: one barrier and GB DMA pieces every tap, although a layer with few input channels has
// very little weight data -- all nine taps x all channel blocks of a 32-wide column tile are 36.9 KB at 32 input channels and 73.7 KB at 64
// (ISNet / RTMDet 32- and 64-channel stages, the 32-channel groups of ResNeXt, the Ken Burns GridNets).  Here a persistent block of eight
// waves loads its column tile's panel ONCE, then walks 16 x 16 output tiles: only the (18 x 18 x 32-channel) input patch of the next
// (tile, channel block) streams, double-buffered, its DMA pieces interleaved with the MFMAs of taps 0 .. 2, and the only barrier left is the
// one per (tile, channel block) that publishes a patch -- 144 MFMAs per wave between barriers instead of 16, a quarter of the DMA volume.
// Wave w owns output rows 2w, 2w + 1 of the tile (32 pixels) x all 32 TN columns.  Same chunks, same chain per output as every other
// configuration (block-major: channel block outer, taps row-major inner).  Column tile = (group, N tile): grouped convolutions with
// 32-channel groups are the case "one channel block, one N tile per group".  Blocks of one XCD with consecutive ids work on the same M tiles
// for different column tiles, so the second reader of a patch finds it in that XCD's L2.
template <int TN>
__global__ __launch_bounds__(512, 2) void k_conv_ws(ConvArgs a, int tiles_x, int tiles_y, int n_n, int n_ct) {
    constexpr int NW = 8, TW = 16, TH = 16, BN = 32 * TN;
    constexpr int PH = TH + 2, PW = TW + 2, NPIX = PH * PW, NPP = (NPIX + 7) / 8, QP = (NPP + NW - 1) / NW;
    constexpr int kPatchF = (NPP + 1) * 8 * 32;                 // floats per patch stage: NPP pieces + one dump slot for the surplus pieces of the last round
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [patch 0][patch 1][weight panel: chunk][BN rows][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int ho = a.out.h, wo = a.out.w, ncb = a.ncb, Tall = 9 * ncb;
    // block -> (XCD x, column tile ct, position i0 among the `per` blocks of that column tile on this XCD)
    const int x = (int)(blockIdx.x & 7u), slot = (int)(blockIdx.x >> 3);
    const int ct = slot % n_ct, i0 = slot / n_ct, per = (int)(gridDim.x >> 3) / n_ct;
    const int total = a.m_tiles, q = total >> 3, r = total & 7;
    const int start = x * q + (x < r ? x : r), len = q + (x < r ? 1 : 0);
    const int g = ct / n_n, n0 = (ct - g * n_n) * BN, cin_off = g * a.cin_g, cout_off = g * a.cout_g, per_img = tiles_x * tiles_y;
    if (i0 >= len) return;

    i32x4 ra, rb;
    {
        uint64_t pa = (uint64_t)a.in.p, pb = (uint64_t)a.w;
        unsigned na = (unsigned)((((int64_t)a.in.n * a.in.h * a.in.w - 1) * a.in.ld + a.in.c) * 4);
        unsigned nb = (unsigned)((int64_t)a.groups * Tall * a.npad * 128);
        ra = i32x4{(int)(unsigned)pa, (int)(unsigned)(pa >> 32), (int)na, 0x00020000};
        rb = i32x4{(int)(unsigned)pb, (int)(unsigned)(pb >> 32), (int)nb, 0x00020000};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const unsigned ldsW = lds0 + (unsigned)(2 * kPatchF * 4);
    // ---- the weight panel, once: piece p = 8 rows of chunk p / (BN / 8); rows beyond the layer's padded width come in as zeros
    {
        const int npieces = Tall * (BN / 8);
        const unsigned wbase = (unsigned)((int64_t)g * Tall * a.npad * 128);
        for (int p = wave; p < npieces; p += NW) {
            const int c = p / (BN / 8), row = 8 * (p - c * (BN / 8)) + (lane >> 3);
            const int sl = (lane & 7) ^ ((row >> 1) & 7);
            const unsigned off = n0 + row < a.npad ? wbase + (unsigned)(((c * a.npad + n0 + row) * 32 + sl * 4) * 4) : kOob;
            dma16(off, rb, ldsW + (unsigned)p * 1024u);
        }
    }
    // ---- patch loader (tile being fetched): wave w owns pieces w, w + NW, ...; lane -> patch pixel 8 * piece + lane / 8, physical slot lane % 8
    unsigned offP[QP];
    auto patch_setup = [&](int k, bool live) {
        const int mt = start + k;
        const int tx = mt % tiles_x, ty = (mt / tiles_x) % tiles_y, n = mt / per_img;
        const int iy0 = ty * TH - a.pad, ix0 = tx * TW - a.pad;
#pragma unroll
        for (int qq = 0; qq < QP; ++qq) {
            int pp = 8 * (wave + qq * NW) + (lane >> 3);
            int sl = (lane & 7) ^ patch_key<PW, TW>(pp);
            int py = pp / PW, px = pp - py * PW;
            int iy = iy0 + py, ix = ix0 + px;
            bool v = live && pp < NPIX && iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w;
            offP[qq] = v ? (unsigned)(((n * a.in.h + iy) * a.in.w + ix) * a.in.ld + cin_off + sl * 4) * 4u : kOob;
        }
    };
    auto patch_piece = [&](auto QC, int cb, int pstage) {
        constexpr int qq = decltype(QC)::value;
        const int piece = wave + qq * NW;
        dma16(offP[qq] == kOob ? kOob : offP[qq] + (unsigned)cb * 128u, ra,
              lds0 + (unsigned)pstage * (unsigned)(kPatchF * 4) + (unsigned)(piece < NPP ? piece : NPP) * 1024u);
    };
    int abase[3][4];                                            // (patch pixel of MFMA row li) * 32 + swizzled 16-B slot, per tap column and k-block
    {
        const int rr = 32 * wave + li;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) abase[kw][kb] = ((rr / TW) * PW + (rr % TW)) * 32 + (((2 * kb + lh) ^ ((((rr % TW) + kw) >> 1) & 7)) << 2);
    }
    int swb[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) swb[kb] = li * 32 + frag_slot(kb, li, lh);
    f32x16 acc[TN];

    patch_setup(i0, true);
    [&]<int... Q>(std::integer_sequence<int, Q...>) { (patch_piece(std::integral_constant<int, Q>{}, 0, 0), ...); }(std::make_integer_sequence<int, QP>{});
    int ps = 0;
    for (int k = i0; k < len; k += per) {
        const int mt = start + k;
        const int tx = mt % tiles_x, ty = (mt / tiles_x) % tiles_y, n = mt / per_img;
        const int kn = k + per;
        const bool more = kn < len;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nn = n0 + 32 * j + li;
            const float b = (a.bias && nn < a.cout_g) ? a.bias[cout_off + nn] : 0.0f;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[j][rr] = b;
        }
        for (int cb = 0; cb < ncb; ++cb, ps ^= 1) {
            const bool last_cb = cb + 1 == ncb;
            // this (tile, channel block)'s patch has landed (every wave waits for its own pieces, then the barrier), and everybody has finished
            // reading the other stage (its fragment reads have completed: lgkmcnt) -- it is refilled below
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (last_cb) patch_setup(more ? kn : k, more);
            const int ncbo = last_cb ? 0 : cb + 1;
            const float *SW = lds + 2 * kPatchF + (cb * 9) * (BN * 32);
            auto tapf = [&](auto TAPC) {
                constexpr int tap = decltype(TAPC)::value, kh = tap / 3, kw = tap - 3 * kh;
                const float *SP = lds + ps * kPatchF + (kh * PW + kw) * 32;
                const float *SB = SW + tap * (BN * 32);
                float4 af[2], bf[2][TN];
                auto rd = [&](int kb, int buf) {
                    af[buf] = *reinterpret_cast<const float4 *>(SP + abase[kw][kb]);
#pragma unroll
                    for (int j = 0; j < TN; ++j) bf[buf][j] = *reinterpret_cast<const float4 *>(SB + j * 1024 + swb[kb]);
                };
                rd(0, 0);
                [&]<int... G>(std::integer_sequence<int, G...>) {
                    ([&] {
                        constexpr int kb = G / 4, t = G % 4, buf = kb & 1;
                        // the next patch goes out four pieces per tap (behind MFMA groups 0, 4, 8, 12 of taps 0, 1, ...)
                        if constexpr (t == 0 && 4 * tap + kb < QP) { patch_piece(std::integral_constant<int, 4 * tap + kb>{}, ncbo, ps ^ 1); __builtin_amdgcn_sched_barrier(0); }
                        if constexpr (t == 1 && kb < 3) { rd(kb + 1, buf ^ 1); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const float av = t == 0 ? af[buf].x : (t == 1 ? af[buf].y : (t == 2 ? af[buf].z : af[buf].w));
                            const float bv = t == 0 ? bf[buf][j].x : (t == 1 ? bf[buf][j].y : (t == 2 ? bf[buf][j].z : bf[buf][j].w));
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }(), ...);
                }(std::make_integer_sequence<int, 16>{});
            };
            static_assert(QP <= 36, "the patch pieces must fit the nine taps");
            tapf(std::integral_constant<int, 0>{}); tapf(std::integral_constant<int, 1>{}); tapf(std::integral_constant<int, 2>{});
            tapf(std::integral_constant<int, 3>{}); tapf(std::integral_constant<int, 4>{}); tapf(std::integral_constant<int, 5>{});
            tapf(std::integral_constant<int, 6>{}); tapf(std::integral_constant<int, 7>{}); tapf(std::integral_constant<int, 8>{});
        }
        // epilogue: lane holds column li of each 32-wide column tile, tile pixels 32 wave + (r & 3) + 8 (r >> 2) + 4 lh
        float slope[TN]; int ncol[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            ncol[j] = n0 + 32 * j + li;
            slope[j] = (a.slope && ncol[j] < a.cout_g) ? a.slope[cout_off + ncol[j]] : 0.0f;
        }
        const int64_t ldo = a.out.ld, ldr = a.res.ld;              // (row pointer once per tile, as in k_conv_patch)
        const int oyb = ty * TH + (32 / TW) * wave, oxb = tx * TW + 4 * lh;
        const int64_t mb = ((int64_t)n * ho + oyb) * wo + oxb;
        float *ob = a.out.p + mb * ldo + cout_off;
        const float *rb = a.res_mode ? a.res.p + mb * ldr + cout_off : nullptr;
        auto ok = [&](int rr) { const int rl = (rr & 3) + 8 * (rr >> 2); return oyb + rl / TW < ho && oxb + rl % TW < wo; };
        auto eo = [&](int rr) { const int rl = (rr & 3) + 8 * (rr >> 2); return (int64_t)(rl / TW) * wo + rl % TW; };
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nn = ncol[j];
            if (nn >= a.cout_g) continue;
            conv_tail<16>(a, slope[j], ob + nn, ldo, rb + nn, ldr, [&](int rr) { return acc[j][rr]; }, ok, eo);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (dead) fetches must land before the block's LDS is released
}

template <int WM, int WN, int TM, int TN, int TW, bool SER>
int launch_conv_patch_t(const ConvArgs &a0, hipStream_t st) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, TH = BM / TW;
    constexpr int NW = WM * WN, NPP = ((((TH + 2) * (TW + 2) + 7) / 8 + NW - 1) / NW) * NW;   // pieces, padded to the wave count
    ConvArgs a = a0;
    const int tiles_x = (a.out.w + TW - 1) / TW, tiles_y = (a.out.h + TH - 1) / TH;
    a.m_tiles = tiles_x * tiles_y * a.out.n;
    a.ngroup = choose_ngroup(a, BN);
    size_t lds = ((size_t)2 * NPP * 8 * 32 + (size_t)2 * BN * 32) * 4;
    static KernelPrep prep;
    (void)prep.ensure([&] { return prepare_kernel(&k_conv_patch<WM, WN, TM, TN, TW, SER>, 64 * WM * WN, lds); });
    dim3 grid(a.m_tiles, (a.cout_g + BN - 1) / BN, a.groups * (SER ? 1 : a.ksplit));
    k_conv_patch<WM, WN, TM, TN, TW, SER><<<grid, 64 * WM * WN, lds, st>>>(a, tiles_x, tiles_y);
    int rc = csm::check_launch("k_conv_patch");
    if (rc || SER || a.ksplit <= 1) return rc;
    return launch_reduce(a, st);
}

template <int WM, int WN, int TM, int TN, int TW>
int launch_conv_patch(const ConvArgs &a, hipStream_t st) {
    if (a.ksplit > 1 && a.serial) return launch_conv_patch_t<WM, WN, TM, TN, TW, true>(a, st);
    return launch_conv_patch_t<WM, WN, TM, TN, TW, false>(a, st);
}

template <int WM, int WN, int TM, int TN, int TW, bool SER, int MINW = 2>
int launch_conv_patch_p_t(const ConvArgs &a0, hipStream_t st) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, TH = BM / TW;
    constexpr int NW = WM * WN, NPP = ((((TH + 2) * (TW + 2) + 7) / 8 + NW - 1) / NW) * NW;
    ConvArgs a = a0;
    const int tiles_x = (a.out.w + TW - 1) / TW, tiles_y = (a.out.h + TH - 1) / TH;
    a.m_tiles = tiles_x * tiles_y * a.out.n;
    a.ngroup = choose_ngroup(a, BN);
    const size_t lds = ((size_t)2 * NPP * 8 * 32 + (size_t)2 * BN * 32) * 4;
    static KernelPrep prep;
    const int blocks_per_cu = prep.ensure([&] { return prepare_kernel(&k_conv_patch_p<WM, WN, TM, TN, TW, SER, MINW>, 64 * WM * WN, lds); });
    const int n_n = (a.cout_g + BN - 1) / BN;
    const int64_t total = (int64_t)a.m_tiles * n_n * a.groups;
    if (total >= (1ll << 30)) return launch_conv_patch<WM, WN, TM, TN, TW>(a0, st);
    int64_t grid = 256ll * blocks_per_cu;
    if (grid > ((total + 7) & ~7ll)) grid = (total + 7) & ~7ll;
    k_conv_patch_p<WM, WN, TM, TN, TW, SER, MINW><<<(unsigned)grid, 64 * WM * WN, lds, st>>>(a, tiles_x, tiles_y, n_n, (int)total);
    return csm::check_launch("k_conv_patch_p");
}
template <int WM, int WN, int TM, int TN, int TW, int MINW = 2>
int launch_conv_patch_p(const ConvArgs &a, hipStream_t st) {
    if (a.ksplit > 1) {
        if (a.serial && a.groups == 1) return launch_conv_patch_p_t<WM, WN, TM, TN, TW, true, MINW>(a, st);
        return launch_conv_patch<WM, WN, TM, TN, TW>(a, st);                   // parallel split-K: one tile per block + reduce
    }
    return launch_conv_patch_p_t<WM, WN, TM, TN, TW, false, MINW>(a, st);
}

// weights-stationary launch: one round of blocks, 8 XCDs x (column tiles x `per` blocks), every block keeps ITS column tile's weight panel
template <int TN>
int launch_conv_ws(const ConvArgs &a0, hipStream_t st) {
    constexpr int BN = 32 * TN;
    ConvArgs a = a0;
    const int tiles_x = (a.out.w + 15) / 16, tiles_y = (a.out.h + 15) / 16;
    a.m_tiles = tiles_x * tiles_y * a.out.n;
    const int n_n = (a.cout_g + BN - 1) / BN, n_ct = a.groups * n_n;
    const size_t lds = (size_t)kWsPatchBytes + (size_t)9 * a.ncb * BN * 128;
    static KernelPrep prep;
    (void)prep.ensure([&] { return prepare_kernel(&k_conv_ws<TN>, 512, (size_t)160 * 1024); });
    // 32 CUs per XCD, one block per CU: `per` blocks share a column tile's M range on an XCD (at least one; never more than it has tiles)
    int per = 32 / n_ct;
    if (per < 1) per = 1;
    const int len_max = (a.m_tiles + 7) / 8;
    if (per > len_max) per = len_max;
    k_conv_ws<TN><<<(unsigned)(8 * n_ct * per), 512, lds, st>>>(a, tiles_x, tiles_y, n_n, n_ct);
    return csm::check_launch("k_conv_ws");
}

// ---- table rows: BN = 32 * TN * WN (k_conv_ws: 32 * TN)
template <int WM, int WN, int TM, int TN, int TW>
constexpr ConvCfg patch_cfg(int id, const char *name) { return {id, name, FAM_PATCH, 32 * TN * WN, &launch_conv_patch<WM, WN, TM, TN, TW>}; }
template <int WM, int WN, int TM, int TN, int TW, int MINW = 2>
constexpr ConvCfg patch_p_cfg(int id, const char *name) { return {id, name, FAM_PATCH_P, 32 * TN * WN, &launch_conv_patch_p<WM, WN, TM, TN, TW, MINW>}; }
template <int TN>
constexpr ConvCfg ws_cfg(int id, const char *name) { return {id, name, FAM_WS, 32 * TN, &launch_conv_ws<TN>}; }
#define ROW(NAME, ...) patch_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
#define ROW_P(NAME, ...) patch_p_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
#define ROW_W(NAME, ...) ws_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
constexpr ConvCfg kRows[] = {
    ROW(P64x64, 2, 2, 1, 1, 16), ROW(P128x64, 2, 2, 2, 1, 16), ROW(P64x128, 2, 2, 1, 2, 16), ROW(P128x128, 2, 2, 2, 2, 16),
    ROW(P256x128, 4, 2, 2, 2, 16), ROW(P128x32, 4, 1, 1, 1, 16), ROW(P64x64_w8, 2, 2, 1, 1, 8), ROW(P128x128_w8, 2, 2, 2, 2, 8),
    ROW(P128x32_w8, 4, 1, 1, 1, 8), ROW(P128x128_8w, 2, 4, 2, 1, 16), ROW(P256x64, 4, 1, 2, 2, 16),
    ROW_P(R128x32, 4, 1, 1, 1, 16), ROW_P(R64x64, 2, 2, 1, 1, 16), ROW_P(R128x64, 2, 2, 2, 1, 16), ROW_P(R128x128_8w, 2, 4, 2, 1, 16),
    ROW_P(R64x128, 2, 2, 1, 2, 16), ROW_P(R128x128_8w_o4, 2, 4, 2, 1, 16, 4),
    // (the 8-wide persistent tiles: where the LDS-read / barrier hazard of the unrolled taps showed; found by tools/check_persistent.py,
    // fixed in k_conv_patch_p, the variants themselves were dropped -- their ids stay defined and launch what R128x32 / R64x64 launch)
    ROW_P(R128x32_w8, 4, 1, 1, 1, 16), ROW_P(R64x64_w8, 2, 2, 1, 1, 16),
    ROW_W(W256x32, 1), ROW_W(W256x64, 2),
};
#undef ROW
#undef ROW_P
#undef ROW_W

}  // namespace

std::span<const ConvCfg> csmconv::conv_cfgs_patch() { return kRows; }

bool csmconv::patch_eligible(const ConvArgs &a) {
    return a.kh == 3 && a.kw == 3 && a.stride == 1 && a.dil == 1 && dma_eligible(a);
}

bool csmconv::ws_fits(const ConvArgs &a, int BN) {
    return a.kh == 3 && a.kw == 3 && a.stride == 1 && a.dil == 1 && a.ksplit <= 1 && a.m_begin == 0 && (a.cin_g & 31) == 0 &&
           (size_t)kWsPatchBytes + (size_t)9 * a.ncb * BN * 128 <= (size_t)160 * 1024;
}
