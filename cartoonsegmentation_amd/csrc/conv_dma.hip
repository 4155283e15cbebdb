// conv_dma.hip -- k_conv_dma and its persistent form k_conv_dma_p: the implicit-GEMM convolution whose operand tiles go global -> LDS by
// buffer_load ... lds (the main kernel of the dense nets), with their launchers and the mixed-tile launch.
#include "csm_convcfg.h"
#include "csm_convtile.h"

using namespace csmconv;

namespace {

// ---- LDS-DMA implicit-GEMM convolution (the main kernel) ------------------------------------------------------------
// Same arithmetic as k_conv_mfma (one fmaf chain per output, chunk = (32-channel block, tap) block-major, 8-block order
// 0,4,1,5,2,6,3,7) --
// what changes is how operands reach the matrix pipe:
//  * tiles go global -> LDS by `buffer_load_dwordx4 ... lds` (no staging VGPRs, no ds_write, no per-element zero select):
//    one wave-instruction moves 8 rows x 128 B.  Out-of-image taps, M / N tails use the buffer range check: their lanes
//    carry offset 0x80000000, the load is out of range and the DMA writes zeros.
//  * LDS rows are exactly 128 B (the DMA writes lane-linear), 16-B slots XOR-swizzled by (row>>1)&7: applied to the SOURCE
//    address of the DMA and to the ds_read_b128 address, conflict-free for the 4x16 lane groups of ds_read_b128.
//  * each wave owns TM x TN accumulators of 32x32 (independent MFMA chains interleave, A/B fragments reused TN/TM times);
//    block tile (32 TM WM) x (32 TN WN), two LDS stages, ONE raw s_barrier per chunk, vmcnt counted by hand (the loads are
//    asm: with the builtin hipcc puts vmcnt(0) in front of every ds_read and the prefetch serialises).
// Requirements (host-checked, else k_conv_mfma): cin_g % 32 == 0, kh*kw <= 32, views < 2 GiB.

template <int WM, int WN, int TM, int TN, int NS, bool SER = false, bool ILV = (CSM_ILV != 0)>
__global__ __launch_bounds__(64 * WM * WN) void k_conv_dma(ConvArgs a) {
    constexpr int NW = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int GA = BM / 8 / NW, GB = BN / 8 / NW;          // DMA pieces (8 rows) per wave per chunk
    static_assert(GA * 8 * NW == BM && GB * 8 * NW == BN, "tile rows must split evenly over the waves");
    constexpr int kStageF = (BM + BN) * 32;                     // floats per stage
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    int mt, ntile, zz;
    block_to_tile(mt, ntile, zz, a.ngroup);
    const int m0 = a.m_begin + mt * BM, n0 = ntile * BN;
    const int g = SER ? zz : zz / a.ksplit, ks = SER ? 0 : zz - g * a.ksplit;
    const int cin_off = g * a.cin_g, cout_off = g * a.cout_g;
    const int Tall = a.kh * a.kw * a.ncb;
    const int c_begin = SER ? 0 : (int)(((int64_t)ks * Tall) / a.ksplit), T = SER ? Tall : (int)(((int64_t)(ks + 1) * Tall) / a.ksplit);

    // buffer descriptors (raw, range-checked): activations view and this op's packed weights
    i32x4 ra, rb;
    conv_rsrc(a, Tall, ra, rb);
    // per-lane loader state.  A piece g: rows 8*(wave*GA+g)+lane/8 of the tile; physical slot lane%8 holds logical slot
    // (lane%8) ^ ((row>>1)&7).  offA = byte offset of (pixel's receptive-field origin, channel) -- may be "negative" (wraps)
    // for border pixels; a VALID tap always brings it back inside the view.
    unsigned offA[GA], vmA[GA], offB[GB];
#pragma unroll
    for (int p = 0; p < GA; ++p) {
        int row = 8 * (wave * GA + p) + (lane >> 3);
        int slot = (lane & 7) ^ ((row >> 1) & 7);
        int m = m0 + row;
        bool rv = m < a.M;
        const RowSetup rs = row_setup(a, rv ? m : 0, rv);
        offA[p] = (unsigned)(((rs.n * a.in.h + rs.iy0) * a.in.w + rs.ix0) * a.in.ld + cin_off + slot * 4) * 4u;
        vmA[p] = rs.vm;
    }
#pragma unroll
    for (int p = 0; p < GB; ++p) {
        int row = 8 * (wave * GB + p) + (lane >> 3);
        int slot = (lane & 7) ^ ((row >> 1) & 7);
        offB[p] = n0 + row < a.npad ? (unsigned)((n0 + row) * 32 + slot * 4) * 4u : kOob;
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const unsigned ldsA = lds0 + (unsigned)(wave * GA * 8) * 128u, ldsB = lds0 + (unsigned)(BM + wave * GB * 8) * 128u;

    // loader position = the NEXT chunk to fetch (block-uniform); chunk order = 32-channel block outer, taps row-major inner
    const int ntaps = a.kh * a.kw;
    int l_cb = c_begin / ntaps, l_tap = c_begin - l_cb * ntaps;
    int l_kh = l_tap / a.kw, l_kw = l_tap - l_kh * a.kw;
    unsigned l_w = (unsigned)(((int64_t)g * Tall + c_begin) * a.npad * 128);     // byte offset of the chunk's weight tile
    // one DMA piece of the loader's current chunk (pieces 0 .. GA-1: activations, GA .. GA+GB-1: weights); !live: every lane out of range
    auto piece = [&](auto PC, int stage, bool live) {
        constexpr int p = decltype(PC)::value;
        const unsigned sb = (unsigned)stage * (unsigned)(kStageF * 4);
        if constexpr (p < GA) {
            const unsigned coff = (unsigned)(((l_kh * a.dil * a.in.w + l_kw * a.dil) * a.in.ld + l_cb * 32) * 4);
            dma16((live && ((vmA[p] >> l_tap) & 1u)) ? offA[p] + coff : kOob, ra, ldsA + sb + (unsigned)p * 1024u);
        } else
            dma16((!live || offB[p - GA] == kOob) ? kOob : offB[p - GA] + l_w, rb, ldsB + sb + (unsigned)(p - GA) * 1024u);
    };
    auto advance = [&]() {
        l_w += (unsigned)a.npad * 128u;
        ++l_tap;
        if (++l_kw == a.kw) { l_kw = 0; if (++l_kh == a.kh) { l_kh = 0; l_tap = 0; ++l_cb; } }
    };
    auto issue = [&](int stage) {
        [&]<int... P>(std::integer_sequence<int, P...>) { (piece(std::integral_constant<int, P>{}, stage, true), ...); }(std::make_integer_sequence<int, GA + GB>{});
        advance();
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        int n = n0 + 32 * (TN * wn + j) + li;
        float b = (a.bias && ks == 0 && n < a.cout_g) ? a.bias[cout_off + n] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = b;
    }
    // MFMA-side fragment addresses: row (32*tile + li), logical slot 2*kb + lh -> physical ^ ((li>>1)&7)
    int sw[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) sw[kb] = frag_slot(kb, li, lh);
    const int rowA = (32 * TM * wm + li) * 32, rowB = (BM + 32 * TN * wn + li) * 32;
    SerialRuns<SER, TM, TN> runs;
    runs.begin(Tall, a.ksplit);
    auto compute = [&](int stage, int chunk) {
        runs.boundary(chunk, acc, Tall, a.ksplit);
        const float *S = lds + stage * kStageF;
        mfma_chunk(acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(S + rowA + i * 1024 + sw[kb]); },
                   [&](int kb, int j) { return *reinterpret_cast<const float4 *>(S + rowB + j * 1024 + sw[kb]); });
    };

    // ILV (two-stage pipeline): the DMA pieces of the next chunk go out BETWEEN the MFMA groups of this one instead of in a burst behind
    // the barrier (see k_conv_dma_p); branch-free -- behind the last chunk the lanes are out of range and the DMA writes zeros into the
    // stage nobody reads any more
    auto compute_ilv = [&](int stage, int fill, int chunk, bool live) {
        runs.boundary(chunk, acc, Tall, a.ksplit);
        const float *S = lds + stage * kStageF;
        mfma_chunk_ilv<TM, TN, GA + GB>(acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(S + rowA + i * 1024 + sw[kb]); },
                                        [&](int kb, int j) { return *reinterpret_cast<const float4 *>(S + rowB + j * 1024 + sw[kb]); },
                                        [&](auto G) { piece(G, fill, live); });
        advance();
    };

    if constexpr (ILV && GA + GB <= 16) {
        // NS stages: while chunk c is multiplied, the pieces of chunk c + NS - 1 go out between its MFMA groups (into the stage chunk c - 1
        // was read from), so a piece has NS - 2 further chunks to land in before it is waited for -- HBM / Infinity-Cache misses
        // included.  Every step issues exactly GA + GB pieces (dead ones past the end), so the counted wait "at most (NS - 2)(GA + GB)
        // outstanding" always means "the pieces of this chunk have landed" (loads retire in order).
        for (int s0 = 0; s0 < NS - 1; ++s0) {
            const bool live = c_begin + s0 < T;
            [&]<int... P>(std::integer_sequence<int, P...>) { (piece(std::integral_constant<int, P>{}, s0, live), ...); }(std::make_integer_sequence<int, GA + GB>{});
            advance();
        }
        for (int chunk = c_begin, st = 0; chunk < T; ++chunk, st = (st + 1 == NS ? 0 : st + 1)) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"((NS - 2) * (GA + GB)) : "memory");
            __builtin_amdgcn_s_barrier();
            compute_ilv(st, st == 0 ? NS - 1 : st - 1, chunk, chunk + NS - 1 < T);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (dead) fetches must land before the block's LDS is released
    } else if constexpr (NS == 2) {
        issue(0);
        for (int chunk = c_begin, st = 0; chunk < T; ++chunk, st ^= 1) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // this wave's pieces of `chunk` have landed, its fragment reads of stage st^1 have completed ...
            __builtin_amdgcn_s_barrier();                          // ... everybody's have, and everybody is done reading stage st^1
            if (chunk + 1 < T) issue(st ^ 1);
            compute(st, chunk);
        }
    } else {
        // NS stages: the loads of chunk + NS - 1 are issued while chunk is consumed, so a load may take NS - 1 chunk times
        // (L2 misses of the short-K-chunk 1x1 layers) before it stalls the pipe.  vmcnt retires in order: "at most
        // (NS - 2) * (GA + GB) outstanding" == the pieces of `chunk` have landed.
        for (int s0 = 0; s0 < NS - 1; ++s0)
            if (c_begin + s0 < T) issue(s0);
        for (int chunk = c_begin, st = 0; chunk < T; ++chunk, st = (st + 1 == NS ? 0 : st + 1)) {
            if (chunk + NS - 2 < T) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NS - 2) * (GA + GB)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (in the barrier's own block: tools/check_isa_barriers.py)
            __builtin_amdgcn_s_barrier();                          // everybody is done reading the stage refilled next
            if (chunk + NS - 1 < T) issue(st == 0 ? NS - 1 : st - 1);
            compute(st, chunk);
        }
    }

    // epilogue: lane holds column li of each 32x32 tile, rows (r&3) + 8*(r>>2) + 4*lh
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        int n = n0 + 32 * (TN * wn + j) + li;
        if (n >= a.cout_g) continue;
        float slope = a.slope ? a.slope[cout_off + n] : 0.0f;
        // (row pointers once per accumulator: the 16 rows of a lane are at compile-time row offsets x the uniform pitch -- no per-element
        // 64-bit multiply; the quarter-rate integer multiplies were ~500 cycles of a tile's epilogue)
        const int64_t ldo = a.out.ld, ldr = a.res.ld;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + 32 * (TM * wm + i) + 4 * lh;
            float *ob = a.out.p + (int64_t)mb * ldo + cout_off + n;
            const float *rb = a.res_mode ? a.res.p + (int64_t)mb * ldr + cout_off + n : nullptr;
            auto val = [&](int r) { return runs.value(i, j, r, acc); };
            auto ok = [&](int r) { return mb + (r & 3) + 8 * (r >> 2) < a.M; };
            auto eo = [](int r) { return (int64_t)((r & 3) + 8 * (r >> 2)); };
            if (!SER && a.ksplit > 1) conv_tail_partial<16>(a.partial + ((int64_t)mb * a.ksplit + ks) * a.cout_g + n, (int64_t)a.ksplit * a.cout_g, val, ok, eo);
            else conv_tail<16>(a, slope, ob, ldo, rb, ldr, val, ok, eo);
        }
    }
}


// ---- persistent form of k_conv_dma: a block walks SEVERAL tiles and the loader runs one chunk ahead ACROSS tile boundaries ----------
// In k_conv_dma every tile pays its prologue (address set-up, the first chunk's DMA round trip: ~3 us) and its epilogue with the matrix
// pipe idle, and because all tiles of a launch take the same time the blocks of a CU stay in lock-step: their prologues never run under
// another block's MFMA phase.  For short-K layers (K = 288: nine chunks, ~15 us of MFMA per tile) that is a fifth of the kernel.  Here
// the grid is one round of resident blocks; a block takes tiles i, i + stride, ... of its XCD's run (the same XCD-aware order), and
// behind the barrier of a tile's LAST chunk it sets the loader up for the NEXT tile and sends that tile's chunk 0 into the free stage:
// the round trip runs under the last chunk's MFMAs and the epilogue's stores.  Same chunks, same chain per output: the bits of every
// other tile configuration.  SER: the serial split-K walk of k_conv_dma (runs combined in registers at the run boundaries).
template <int WM, int WN, int TM, int TN, bool SER = false, bool ILV = (CSM_ILV != 0)>
__global__ __launch_bounds__(64 * WM * WN) void k_conv_dma_p(ConvArgs a, int n_n /* N tiles per group */, int total /* tiles */) {
    constexpr int NW = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int GA = BM / 8 / NW, GB = BN / 8 / NW;
    static_assert(GA * 8 * NW == BM && GB * 8 * NW == BN, "tile rows must split evenly over the waves");
    constexpr int kStageF = (BM + BN) * 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const int Tall = a.kh * a.kw * a.ncb;
    // this block's tiles: XCD x = blockIdx & 7 owns the run [start, start + len) of the (z, m-tile, n-tile) order, n fastest
    const int per = (int)(gridDim.x >> 3), x = (int)(blockIdx.x & 7u), i0 = (int)(blockIdx.x >> 3);
    const int q = total >> 3, r = total & 7;
    const int start = x * q + (x < r ? x : r), len = q + (x < r ? 1 : 0);
    if (i0 >= len) return;
    const int per_z = a.m_tiles * n_n;

    i32x4 ra, rb;
    conv_rsrc(a, Tall, ra, rb);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const unsigned ldsA = lds0 + (unsigned)(wave * GA * 8) * 128u, ldsB = lds0 + (unsigned)(BM + wave * GB * 8) * 128u;

    // loader state of the tile being FETCHED (one chunk ahead of the tile being computed)
    unsigned offA[GA], vmA[GA], offB[GB];
    int l_cb = 0, l_tap = 0, l_kh = 0, l_kw = 0;
    unsigned l_w = 0u;
    auto loader_setup = [&](int k, bool live) {                 // tile k of the run (clamped by the caller); !live: every lane out of range
        const int j = start + k;
        const int g = j / per_z, rem = j - g * per_z;
        int mt, nt;
        rem_to_tile((unsigned)rem, (unsigned)a.m_tiles, (unsigned)n_n, a.ngroup, mt, nt);
        const int m0 = mt * BM, n0 = nt * BN, cin_off = g * a.cin_g;
#pragma unroll
        for (int p = 0; p < GA; ++p) {
            int row = 8 * (wave * GA + p) + (lane >> 3);
            int slot = (lane & 7) ^ ((row >> 1) & 7);
            int m = m0 + row;
            bool rv = live && m < a.M;
            const RowSetup rs = row_setup(a, rv ? m : 0, rv);
            offA[p] = (unsigned)(((rs.n * a.in.h + rs.iy0) * a.in.w + rs.ix0) * a.in.ld + cin_off + slot * 4) * 4u;
            vmA[p] = rs.vm;
        }
#pragma unroll
        for (int p = 0; p < GB; ++p) {
            int row = 8 * (wave * GB + p) + (lane >> 3);
            int slot = (lane & 7) ^ ((row >> 1) & 7);
            offB[p] = (live && n0 + row < a.npad) ? (unsigned)((n0 + row) * 32 + slot * 4) * 4u : kOob;
        }
        l_cb = 0; l_tap = 0; l_kh = 0; l_kw = 0;
        l_w = (unsigned)((int64_t)g * Tall * a.npad * 128);
    };
    // one DMA piece of the loader's current chunk (pieces 0 .. GA-1: activations, GA .. GA+GB-1: weights), then the step to the next chunk
    auto piece = [&](auto PC, int stage) {
        constexpr int p = decltype(PC)::value;
        const unsigned sb = (unsigned)stage * (unsigned)(kStageF * 4);
        if constexpr (p < GA) {
            const unsigned coff = (unsigned)(((l_kh * a.dil * a.in.w + l_kw * a.dil) * a.in.ld + l_cb * 32) * 4);
            dma16(((vmA[p] >> l_tap) & 1u) ? offA[p] + coff : kOob, ra, ldsA + sb + (unsigned)p * 1024u);
        } else
            dma16(offB[p - GA] == kOob ? kOob : offB[p - GA] + l_w, rb, ldsB + sb + (unsigned)(p - GA) * 1024u);
    };
    auto advance = [&]() {
        l_w += (unsigned)a.npad * 128u;
        ++l_tap;
        if (++l_kw == a.kw) { l_kw = 0; if (++l_kh == a.kh) { l_kh = 0; l_tap = 0; ++l_cb; } }
    };
    auto issue = [&](int stage) {
        [&]<int... P>(std::integer_sequence<int, P...>) { (piece(std::integral_constant<int, P>{}, stage), ...); }(std::make_integer_sequence<int, GA + GB>{});
        advance();
    };

    int sw[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) sw[kb] = frag_slot(kb, li, lh);
    const int rowA = (32 * TM * wm + li) * 32, rowB = (BM + 32 * TN * wn + li) * 32;
    SerialRuns<SER, TM, TN> runs;                               // (reset per tile)
    f32x16 acc[TM][TN];
    // ILV: the chunk's MFMAs with the DMA pieces of the NEXT chunk spread between them -- piece g goes out behind MFMA group g (a group =
    // one k step of all TM x TN accumulators), so the pieces leave in the first half of the chunk and the matrix pipe never waits for a
    // burst of GA + GB address computations and DMA issues behind the barrier (each costs the wave 60-180 cycles of issue time, which an
    // MFMA in flight covers).  The fragments of k-block kb + 1 are requested behind the second group of kb.  The order is pinned with
    // sched_barrier: hipcc otherwise regroups the asm statements in front of the MFMAs.
    auto compute_ilv = [&](int stage, int fill) {
        const float *S = lds + stage * kStageF;
        mfma_chunk_ilv<TM, TN, GA + GB>(acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(S + rowA + i * 1024 + sw[kb]); },
                                        [&](int kb, int j) { return *reinterpret_cast<const float4 *>(S + rowB + j * 1024 + sw[kb]); },
                                        [&](auto G) { piece(G, fill); });
        advance();
    };
    auto compute = [&](int stage) {
        const float *S = lds + stage * kStageF;
        mfma_chunk(acc, [&](int kb, int i) { return *reinterpret_cast<const float4 *>(S + rowA + i * 1024 + sw[kb]); },
                   [&](int kb, int j) { return *reinterpret_cast<const float4 *>(S + rowB + j * 1024 + sw[kb]); });
    };

    loader_setup(i0, true);
    issue(0);
    int st = 0;
    for (int k = i0; k < len; k += per) {
        const int j = start + k;
        const int g = j / per_z, rem = j - g * per_z;
        int mt, nt;
        rem_to_tile((unsigned)rem, (unsigned)a.m_tiles, (unsigned)n_n, a.ngroup, mt, nt);
        const int m0 = mt * BM, n0 = nt * BN, cout_off = g * a.cout_g;
#pragma unroll
        for (int jj = 0; jj < TN; ++jj) {
            int n = n0 + 32 * (TN * wn + jj) + li;
            float b = (a.bias && n < a.cout_g) ? a.bias[cout_off + n] : 0.0f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[i][jj][rr] = b;
        }
        runs.begin(Tall, a.ksplit);
        for (int chunk = 0; chunk + 1 < Tall; ++chunk, st ^= 1) {
            // (lgkmcnt: this wave's fragment reads of the stage refilled next must have COMPLETED before it arrives -- hipcc may sink
            // the last MFMAs of the previous chunk, and with them the wait for their operands, below the barrier)
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if constexpr (ILV) { runs.boundary(chunk, acc, Tall, a.ksplit); compute_ilv(st, st ^ 1); }
            else { issue(st ^ 1); runs.boundary(chunk, acc, Tall, a.ksplit); compute(st); }
        }
        // the tile's last chunk: the NEXT tile's chunk 0 goes out behind the barrier (branch-free: past the end every lane is out
        // of range and the DMA writes zeros into a stage nobody reads)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const int kn = k + per;
            const bool more = kn < len;
            loader_setup(more ? kn : k, more);
            if constexpr (!ILV) issue(st ^ 1);
        }
        runs.boundary(Tall - 1, acc, Tall, a.ksplit);
        if constexpr (ILV) compute_ilv(st, st ^ 1); else compute(st);
        st ^= 1;
        // epilogue: lane holds column li of each 32x32 tile, rows (r&3) + 8*(r>>2) + 4*lh
#pragma unroll
        for (int jj = 0; jj < TN; ++jj) {
            int n = n0 + 32 * (TN * wn + jj) + li;
            if (n >= a.cout_g) continue;
            float slope = a.slope ? a.slope[cout_off + n] : 0.0f;
            const int64_t ldo = a.out.ld, ldr = a.res.ld;          // (row pointers once per accumulator, as in k_conv_dma)
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + 32 * (TM * wm + i) + 4 * lh;
                float *ob = a.out.p + (int64_t)mb * ldo + cout_off + n;
                const float *rb = a.res_mode ? a.res.p + (int64_t)mb * ldr + cout_off + n : nullptr;
                conv_tail<16>(a, slope, ob, ldo, rb, ldr,
                              [&](int rr) { return runs.value(i, jj, rr, acc); },
                              [&](int rr) { return mb + (rr & 3) + 8 * (rr >> 2) < a.M; }, [](int rr) { return (int64_t)((rr & 3) + 8 * (rr >> 2)); });
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (dead) fetch must land before the block's LDS is released
}

// Grid quantisation: a launch of `total` equal tiles on S = 256 x (blocks per CU) slots takes ceil(total / S) rounds; with 3.1 rounds
// (the 40 x 40 x 1024 layers of ResNeXt at batch 8: 800 tiles of 128 x 128) a quarter of the machine time is an almost empty fourth
// round.  Every tile configuration produces the same bits, so a launch may MIX them: when `split` is set the big tiles cover whole
// rounds only and the remaining rows (less than ~0.6 of a round) are covered by a second launch of 64 x 64 tiles, which spreads
// them over all CUs.  Speed only; chosen per layer by the autotuner (csm_op.tile bit 7).
static int conv_split_rows(const ConvArgs &a, int BM, int BN, int blocks_per_cu) {
    const int64_t n_n = (int64_t)((a.cout_g + BN - 1) / BN) * a.groups * ((a.ksplit > 1 && !a.serial) ? a.ksplit : 1);
    const int64_t m_tiles = (a.M + BM - 1) / BM, slots = 256ll * (blocks_per_cu > 0 ? blocks_per_cu : 1);
    const double rounds = (double)(m_tiles * n_n) / (double)slots;
    const int64_t full = (int64_t)rounds;
    const double frac = rounds - (double)full;
    if (full < 1 || frac < 0.02 || frac > 0.6) return 0;
    const int64_t mt_main = full * slots / n_n;
    if (mt_main <= 0 || mt_main >= m_tiles) return 0;
    return (int)(mt_main * BM);
}

template <int WM, int WN, int TM, int TN, int NS, bool SER>
int launch_conv_dma_t(const ConvArgs &a0, hipStream_t st) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    ConvArgs a = a0;
    size_t lds = (size_t)NS * (BM + BN) * 128;
    static KernelPrep prep;
    const int blocks_per_cu = prep.ensure([&] { return prepare_kernel(&k_conv_dma<WM, WN, TM, TN, NS, SER>, 64 * WM * WN, lds); });
    if (a.split && (BM > 64 || BN > 64) && (a.ksplit <= 1 || SER)) {
        const int rows = conv_split_rows(a, BM, BN, blocks_per_cu);
        if (rows > 0) {
            ConvArgs tail = a;
            tail.m_begin = a.m_begin + rows; tail.split = 0;
            a.M = a.m_begin + rows; a.split = 0;
            int rc = launch_conv_dma_t<WM, WN, TM, TN, NS, SER>(a, st);
            if (rc) return rc;
            return launch_conv_dma_t<2, 2, 1, 1, 2, SER>(tail, st);
        }
    }
    a.m_tiles = (a.M - a.m_begin + BM - 1) / BM;
    a.ngroup = choose_ngroup(a, BN);
    dim3 grid(a.m_tiles, (a.cout_g + BN - 1) / BN, a.groups * (SER ? 1 : a.ksplit));
    k_conv_dma<WM, WN, TM, TN, NS, SER><<<grid, 64 * WM * WN, lds, st>>>(a);
    int rc = csm::check_launch("k_conv_dma");
    if (rc || SER || a.ksplit <= 1) return rc;
    return launch_reduce(a, st);
}

template <int WM, int WN, int TM, int TN, int NS = 2>
int launch_conv_dma(const ConvArgs &a, hipStream_t st) {
    if constexpr (NS == 2)        // (three- / four-stage tiles measured slower than two stages on every layer, also with interleaved issue: r04g)
        if (a.ksplit > 1 && a.serial) return launch_conv_dma_t<WM, WN, TM, TN, 2, true>(a, st);
    return launch_conv_dma_t<WM, WN, TM, TN, NS, false>(a, st);
}

// persistent launch: one round of resident blocks (a multiple of 8, at most one block per tile); layers that split K take the
// one-tile-per-block kernel of the same shape
template <int WM, int WN, int TM, int TN, bool SER>
int launch_conv_dma_p_t(const ConvArgs &a0, hipStream_t st) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    ConvArgs a = a0;
    const size_t lds = (size_t)2 * (BM + BN) * 128;
    static KernelPrep prep;
    const int blocks_per_cu = prep.ensure([&] { return prepare_kernel(&k_conv_dma_p<WM, WN, TM, TN, SER>, 64 * WM * WN, lds); });
    a.m_tiles = (a.M + BM - 1) / BM;
    a.ngroup = choose_ngroup(a, BN);
    const int n_n = (a.cout_g + BN - 1) / BN;
    const int64_t total = (int64_t)a.m_tiles * n_n * a.groups;
    if (total >= (1ll << 30)) return launch_conv_dma<WM, WN, TM, TN>(a0, st);
    int64_t grid = 256ll * blocks_per_cu;
    if (grid > ((total + 7) & ~7ll)) grid = (total + 7) & ~7ll;
    k_conv_dma_p<WM, WN, TM, TN, SER><<<(unsigned)grid, 64 * WM * WN, lds, st>>>(a, n_n, (int)total);
    return csm::check_launch("k_conv_dma_p");
}
template <int WM, int WN, int TM, int TN>
int launch_conv_dma_p(const ConvArgs &a, hipStream_t st) {
    if (a.m_begin != 0) return launch_conv_dma<WM, WN, TM, TN>(a, st);
    if (a.ksplit > 1) {
        if (a.serial && a.groups == 1) return launch_conv_dma_p_t<WM, WN, TM, TN, true>(a, st);
        return launch_conv_dma<WM, WN, TM, TN>(a, st);                          // parallel split-K: one tile per block + reduce
    }
    return launch_conv_dma_p_t<WM, WN, TM, TN, false>(a, st);
}

// ---- table rows: BN = 32 * TN * WN
template <int WM, int WN, int TM, int TN, int NS = 2>
constexpr ConvCfg dma_cfg(int id, const char *name) { return {id, name, FAM_DMA, 32 * TN * WN, &launch_conv_dma<WM, WN, TM, TN, NS>}; }
template <int WM, int WN, int TM, int TN>
constexpr ConvCfg dma_p_cfg(int id, const char *name) { return {id, name, FAM_DMA_P, 32 * TN * WN, &launch_conv_dma_p<WM, WN, TM, TN>}; }
#define ROW(NAME, ...) dma_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
#define ROW_P(NAME, ...) dma_p_cfg<__VA_ARGS__>(CFG_##NAME, #NAME)
constexpr ConvCfg kRows[] = {
    ROW(D64x64, 2, 2, 1, 1), ROW(D128x64, 2, 2, 2, 1), ROW(D64x128, 2, 2, 1, 2), ROW(D128x128, 2, 2, 2, 2), ROW(D128x128_8w, 2, 4, 2, 1),
    ROW(D256x128_8w, 4, 2, 2, 2), ROW(D128x32, 4, 1, 1, 1),
    ROW(D96x128, 1, 4, 3, 1), ROW(D160x128, 1, 4, 5, 1), ROW(D224x128, 1, 4, 7, 1), ROW(D192x128, 1, 4, 6, 1),
    ROW(D64x64_s3, 2, 2, 1, 1, 3), ROW(D128x64_s3, 2, 2, 2, 1, 3), ROW(D64x128_s3, 2, 2, 1, 2, 3), ROW(D128x128_s3, 2, 2, 2, 2, 3),
    ROW(D128x128_8w_s3, 2, 4, 2, 1, 3), ROW(D256x128_8w_s3, 4, 2, 2, 2, 3), ROW(D256x64, 4, 1, 2, 2), ROW(D256x64_s3, 4, 1, 2, 2, 3),
    ROW(D64x64_s4, 2, 2, 1, 1, 4),
    ROW_P(Q64x64, 2, 2, 1, 1), ROW_P(Q128x64, 2, 2, 2, 1), ROW_P(Q64x128, 2, 2, 1, 2), ROW_P(Q128x128_8w, 2, 4, 2, 1), ROW_P(Q128x32, 4, 1, 1, 1),
};
#undef ROW
#undef ROW_P

}  // namespace

std::span<const ConvCfg> csmconv::conv_cfgs_dma() { return kRows; }

bool csmconv::dma_eligible(const ConvArgs &a) {
    int64_t bytes_in = (((int64_t)a.in.n * a.in.h * a.in.w - 1) * a.in.ld + a.in.c) * 4;
    int64_t bytes_w = (int64_t)a.groups * a.kh * a.kw * a.ncb * a.npad * 128;
    return (a.cin_g & 31) == 0 && a.kh * a.kw <= 32 && bytes_in < (1ll << 31) && bytes_w < (1ll << 31) && !(a.in.ld & 3) &&
           !(((uintptr_t)a.in.p | (uintptr_t)a.w) & 15);
}

// N tiles per group of the tile order (rem_to_tile): grouping pays when the layer's weights do not fit an XCD's 4 MB L2 next to the
// activation tiles in flight; the group's weight slices should take about half of it.  Speed only.
int csmconv::choose_ngroup(const ConvArgs &a, int BN) {
    if (!g_ngroup_enable || a.groups != 1) return 0;
    const int nn = (a.cout_g + BN - 1) / BN;
    int64_t kbytes = (int64_t)a.kh * a.kw * a.ncb * 128;                 // packed weight bytes of one output channel
    if (a.ksplit > 1 && !a.serial) kbytes /= a.ksplit;                   // (parallel split-K: a z slice reads its K run only)
    if (nn < 2 || kbytes * a.npad <= (3ll << 20)) return 0;
    int best = 0;
    for (int d = 1; d < nn; ++d)
        if (nn % d == 0 && (int64_t)d * BN * kbytes <= (2ll << 20)) best = d;
    if (!best && (int64_t)BN * kbytes <= (7ll << 19)) best = 1;
    return best;
}
