// csm_convtile.h -- device pieces shared by the direct (non-Winograd) convolution kernels: k_conv_dma / k_conv_dma_p (conv_dma.hip) and
// k_conv_patch_p / k_conv_ws / k_conv_patch (conv_patch.hip); wino.hip takes the buffer descriptor.  Everything here is __forceinline__
// and takes its operands by reference.  A piece lives here only if the kernels built from it compile to the instructions of the kernels
// written out in full (tools/compare_kernel_isa.py, profiles/convtile_isa.txt): hipcc simplifies every function once BEFORE it inlines,
// so where a helper starts and ends decides which instructions are sunk below a loop or re-associated, and with it the register
// allocation of the whole kernel.  The comments say where that fixed a signature or an order.
// Conventions: a wave owns TM x TN accumulators of 32 x 32; lane = (li, lh) = (lane & 31, lane >> 5) holds column li of each, rows
// (r & 3) + 8 (r >> 2) + 4 lh; LDS rows are 128 B, their 16-B slots XOR-swizzled.
#pragma once
#include "csm_conv.h"
#include <utility>

namespace csmconv {

template <int N> using ic = std::integral_constant<int, N>;

constexpr unsigned kOob = 0x80000000u;          // byte offset of a DMA lane that must read nothing: out of range, the DMA writes zeros

// ---- raw, range-checked buffer descriptor over [address, address + bytes) ----------------------------------------------------------------
__device__ __forceinline__ i32x4 buffer_rsrc(uint64_t address, unsigned bytes) {
    return i32x4{(int)(unsigned)address, (int)(unsigned)(address >> 32), (int)bytes, 0x00020000};
}
__device__ __forceinline__ i32x4 buffer_rsrc(const void *p, unsigned bytes) { return buffer_rsrc((uint64_t)p, bytes); }
// bytes of an NHWC view up to the last channel of its last pixel / of an op's packed weights (Tall chunks of npad rows x 128 B per group)
__device__ __forceinline__ unsigned view_bytes(const View &v) { return (unsigned)((((int64_t)v.n * v.h * v.w - 1) * v.ld + v.c) * 4); }
__device__ __forceinline__ unsigned packed_weight_bytes(const ConvArgs &a, int Tall) { return (unsigned)((int64_t)a.groups * Tall * a.npad * 128); }
// the two descriptors of a direct conv kernel: the activations view and this op's packed weights (both addresses first, then both sizes:
// the order of the kernels this came from)
__device__ __forceinline__ void conv_rsrc(const ConvArgs &a, int Tall, i32x4 &ra, i32x4 &rb) {
    const uint64_t pa = (uint64_t)a.in.p, pb = (uint64_t)a.w;
    const unsigned na = view_bytes(a.in), nb = packed_weight_bytes(a, Tall);
    ra = buffer_rsrc(pa, na);
    rb = buffer_rsrc(pb, nb);
}

// MFMA-side fragment offset (floats) of k-block kb inside row (32 tile + li): logical slot 2 kb + lh -> physical ^ ((li >> 1) & 7).
// (per k-block: the loop over kb stays in the kernel)
__device__ __forceinline__ int frag_slot(int kb, int li, int lh) { return ((2 * kb + lh) ^ ((li >> 1) & 7)) * 4; }

// ---- split K executed serially: one block walks all `ksplit` runs of chunks and combines them in registers at the run boundaries
// (`tot = tot + acc; acc = 0`: the additions of k_splitk_reduce in the same order).  SER == false: no state, no code.
// Declare it in front of the accumulators in a persistent kernel and behind them in a one-tile kernel.
template <bool SER, int TM, int TN> struct SerialRuns;
template <int TM, int TN> struct SerialRuns<false, TM, TN> {
    __device__ __forceinline__ void begin(int, int) {}
    __device__ __forceinline__ void boundary(int, f32x16 (&)[TM][TN], int, int) {}
    __device__ __forceinline__ float value(int i, int j, int r, const f32x16 (&acc)[TM][TN]) const { return acc[i][j][r]; }
};
template <int TM, int TN> struct SerialRuns<true, TM, TN> {
    f32x16 tot[TM][TN];
    int next_b, run;                             // first chunk of the next run / runs folded so far
    // a tile of Tall chunks starts
    __device__ __forceinline__ void begin(int Tall, int ksplit) { run = 0; next_b = (int)((int64_t)Tall / ksplit); }
    // in front of the MFMAs of `chunk` (block-uniform: the fold runs ksplit - 1 times per tile)
    __device__ __forceinline__ void boundary(int chunk, f32x16 (&acc)[TM][TN], int Tall, int ksplit) {
        if (chunk == next_b) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { tot[i][j][r] = run == 0 ? acc[i][j][r] : tot[i][j][r] + acc[i][j][r]; acc[i][j][r] = 0.0f; }
            ++run; next_b = (int)(((int64_t)(run + 1) * Tall) / ksplit);
        }
    }
    // the finished sum of element r of accumulator (i, j): what the epilogue's val(r) returns
    __device__ __forceinline__ float value(int i, int j, int r, const f32x16 (&acc)[TM][TN]) const { return tot[i][j][r] + acc[i][j][r]; }
};

// ---- the MFMAs of one chunk (32 channels): 4 k-blocks x 4 k-steps x TM x TN.  read_a(kb, i) / read_b(kb, j) -> the float4 fragment of
// k-block kb for accumulator row i / column j; k-step t multiplies component t of both.
template <int T> __device__ __forceinline__ float frag_elem(const float4 &f) { return T == 0 ? f.x : (T == 1 ? f.y : (T == 2 ? f.z : f.w)); }
__device__ __forceinline__ float frag_elem(const float4 &f, int t) { return t == 0 ? f.x : (t == 1 ? f.y : (t == 2 ? f.z : f.w)); }

template <int TM, int TN, class ReadA, class ReadB>
__device__ __forceinline__ void mfma_chunk(f32x16 (&acc)[TM][TN], ReadA &&read_a, ReadB &&read_b) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        float4 af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = read_a(kb, i);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = read_b(kb, j);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(frag_elem(af[i], t), frag_elem(bf[j], t), acc[i][j], 0, 0, 0);
    }
}
// The same MFMAs as 16 groups (a group = one k-step of all TM x TN accumulators) with the chunk's DMA spread between them: piece(ic<G>)
// goes out in front of group G (G < NPIECES), so the pieces leave in the first half of the chunk and the matrix pipe never waits for a
// burst of address computations and DMA issues behind the barrier (each costs the wave 60-180 cycles of issue time, which an MFMA in
// flight covers).  The fragments of k-block kb + 1 are requested behind the second group of kb.  The order is pinned with sched_barrier:
// hipcc otherwise regroups the asm statements in front of the MFMAs.
template <int TM, int TN, int NPIECES, class ReadA, class ReadB, class Piece>
__device__ __forceinline__ void mfma_chunk_ilv(f32x16 (&acc)[TM][TN], ReadA &&read_a, ReadB &&read_b, Piece &&piece) {
    static_assert(NPIECES <= 16, "one DMA piece per MFMA group");
    float4 af[2][TM], bf[2][TN];
    auto rd = [&](int kb, int buf) {
#pragma unroll
        for (int i = 0; i < TM; ++i) af[buf][i] = read_a(kb, i);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[buf][j] = read_b(kb, j);
    };
    rd(0, 0);
    [&]<int... G>(std::integer_sequence<int, G...>) {
        ([&] {
            constexpr int kb = G / 4, t = G % 4, buf = kb & 1;
            if constexpr (G < NPIECES) { piece(ic<G>{}); __builtin_amdgcn_sched_barrier(0); }
            if constexpr (t == 1 && kb < 3) { rd(kb + 1, buf ^ 1); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(frag_elem<t>(af[buf][i]), frag_elem<t>(bf[buf][j]), acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }(), ...);
    }(std::make_integer_sequence<int, 16>{});
}

}  // namespace csmconv
