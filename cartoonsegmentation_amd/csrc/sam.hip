// sam.hip -- what Segment Anything needs next to the convolution engine and tokens.hip (CSM_OP_ATTENTION_RELPOS / CROSS_ATTENTION /
// CHANNEL_DOT, CSM_OP_TOKENS modes 3..6, and the pre- / post-processing calls csm_sam_*; include/csm355.h):
//   * k_attention_rp: self-attention of the ViT image encoder with the DECOMPOSED relative position bias
//         bias(i, j) = q_i . Rh[yi - yj + gh - 1] + q_i . Rw[xi - xj + gw - 1]
//     on a gh x gw token grid (a 14 x 14 window or the whole 64 x 64 map) -- k_attention's streaming structure, see below;
//   * k_window: window partition with zero padding / un-partition with crop and the residual add;
//   * k_bcast_add: batch-1 tensors and constants added to batch-n ones (position embeddings, the image embedding shared by all boxes);
//   * k_xattn_*: cross-attention between two token sets of different length (the mask decoder's two-way transformer);
//   * k_channel_dot: the hypernetwork product mask[b, p] = sum_c upscaled[b, p, c] hyper[b, c];
//   * image -> model input, low-res logits -> full-size masks, boxes -> prompt tokens.
#include "csm_common.h"
#include "csm_tokens.h"
#include <mutex>
#include <utility>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- self-attention with the decomposed relative position bias ---------------------------------------------------------------------------
// Same machine as tokens.hip::k_attention (read its header first): a block = 4 waves = (2 tiles of 32 queries) x (2 halves of the key
// range), one query per lane, s^T = K q^T and o^T += V^T p^T on v_mfma_f32_32x32x2_f32 with P straight from the score registers, running
// max / sum, split-softmax merge of the two halves.  N = gh * gw tokens, token y * gw + x = grid position (y, x); no class token.
//
// The bias of a query needs only its products with the (2 gh - 1) + (2 gw - 1) table rows: G[t][query] = q . R[t], R = (Rh ; Rw) stacked.
// That is the SAME product shape as a score tile (A = 32 table rows, B = the query registers), so the prologue runs it on the matrix
// pipe with the table rows read straight from global memory (once per block: no staging) and leaves G in LDS as [t][32 queries]; the two
// waves of a query tile split the row tiles.  Per score the loop then adds  G[yi - yj + gh - 1] + G[2 gh - 1 + xi - xj + gw - 1]:  two LDS
// reads at (row of the lane's own query, key term staged per tile).  q carries the 1/sqrt(d) scale (folded into the packed qkv weights),
// so the host packs the tables as R * sqrt(d): q_scaled . R' = q . R up to rounding.  Cost of the prologue: TT / 32 row tiles x D / 2
// MFMAs per query tile against N / 32 x (D / 2 + 16 NCT) in the loop -- 6 % at 64 x 64 tokens, 12 % in a 14 x 14 window.
//
// D = head dimension, D % 16 == 0: 32, 64, 80 (ViT-H: 1280 / 16) or 128.  D = 80 is NATIVE, not padded to 96: q k^T runs exactly D / 2 = 40
// MFMAs; the output takes NCT = 3 column tiles of which the last is half used (its upper 16 columns re-read column D - 1 and are never
// stored), 48 MFMAs -- 88 per key tile against 96 for zero-padded heads, and the qkv GEMM, its output and the K / V traffic stay at 80
// columns per head instead of 96.
template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_attention_rp(const float *__restrict__ qkv, int ld, float *__restrict__ out, int out_ld, int N,
                                                                                                 int heads, const float *__restrict__ table /* [TT][D] */, int gh, int gw) {
    constexpr int NCT = (D + 31) / 32, PITCH = D + 4, TILE = 32 * PITCH;
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [half][K tile | V tile], [64] key terms, [query tile][TTP][32] bias products
    int2 *kterm = reinterpret_cast<int2 *>(lds + 4 * TILE);             // [2][32]: (32 ky, 32 kx) of the staged keys
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int qt = wave & 1, kh = wave >> 1;
    const int head = blockIdx.y, b = blockIdx.z, C = heads * D;
    const int q0 = (blockIdx.x * 2 + qt) * 32, qi = q0 + li;
    const float *base = qkv + (int64_t)b * N * ld;
    const float *Q = base + head * D, *K = base + C + head * D, *V = base + 2 * C + head * D;
    const int TT = 2 * gh - 1 + 2 * gw - 1, TTP = (TT + 31) & ~31;
    float *G = lds + 4 * TILE + 128 + qt * TTP * 32;
    const int qc = min(qi, N - 1), qy = qc / gw, qx = qc - qy * gw;      // (padded queries compute the last one's values and store nothing)
    const int hb = (qy + gh - 1) * 32 + li, wb = (2 * gh - 1 + qx + gw - 1) * 32 + li;

    float4 qf[D / 8];
    {
        const float *qrow = Q + (int64_t)qc * ld;
#pragma unroll
        for (int kb = 0; kb < D / 8; ++kb) qf[kb] = *reinterpret_cast<const float4 *>(qrow + 8 * kb + 4 * lh);
    }
    // ---- prologue: G[t][query] = q . R[t] for this wave's share of the table row tiles
    for (int tt = kh; tt * 32 < TTP; tt += 2) {
        const float *rrow = table + (int64_t)min(tt * 32 + li, TT - 1) * D;
        f32x16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < D / 8; ++kb) {
            const float4 rf = *reinterpret_cast<const float4 *>(rrow + 8 * kb + 4 * lh);
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(rf.x, qf[kb].x, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(rf.y, qf[kb].y, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(rf.z, qf[kb].z, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(rf.w, qf[kb].w, g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) G[(tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = g[r];
    }

    f32x16 o[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[ct][r] = 0.0f;
    float m_run = -3.0e38f, l_run = 0.0f;
    int vcol[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) vcol[ct] = min(32 * ct + li, D - 1);

    const int NT = (N + 31) >> 5, half = (NT + 1) >> 1;
    constexpr int NPF = 2 * 32 * (D / 4) / 256;                          // float4 per thread and tensor for the two halves' tiles
    static_assert(2 * 32 * (D / 4) % 256 == 0, "head dimension must be a multiple of 16");
    f32x4 pk[NPF], pv[NPF];
    auto prefetch = [&](int itn) __attribute__((always_inline)) {
        [&]<int... U>(std::integer_sequence<int, U...>) {
            ([&] {
                const int e = tid + U * 256;
                const int hs = e / (32 * (D / 4)), rem = e - hs * (32 * (D / 4)), row = rem / (D / 4), c4 = rem - row * (D / 4);
                const int key = min((hs * half + itn) * 32 + row, N - 1);
                pk[U] = *reinterpret_cast<const f32x4 *>(K + (int64_t)key * ld + 4 * c4);
                pv[U] = *reinterpret_cast<const f32x4 *>(V + (int64_t)key * ld + 4 * c4);
            }(), ...);
        }(std::make_integer_sequence<int, NPF>{});
    };
    prefetch(0);
    for (int it = 0; it < half; ++it) {
        __syncthreads();                                                // everybody is done with the previous tiles (first pass: G is complete)
        [&]<int... U>(std::integer_sequence<int, U...>) {
            ([&] {
                const int e = tid + U * 256;
                const int hsel = e / (32 * (D / 4)), rem = e - hsel * (32 * (D / 4)), row = rem / (D / 4), c4 = rem - row * (D / 4);
                *reinterpret_cast<f32x4 *>(lds + 2 * hsel * TILE + row * PITCH + 4 * c4) = pk[U];
                *reinterpret_cast<f32x4 *>(lds + (2 * hsel + 1) * TILE + row * PITCH + 4 * c4) = pv[U];
            }(), ...);
        }(std::make_integer_sequence<int, NPF>{});
        if (tid < 64) {
            const int j = min(((tid >> 5) * half + it) * 32 + (tid & 31), N - 1);
            const int yj = j / gw;
            kterm[tid] = make_int2(32 * yj, 32 * (j - yj * gw));
        }
        __syncthreads();
        prefetch(min(it + 1, half - 1));
        const int tile = kh * half + it;
        if (tile >= NT) continue;                                       // (odd tile counts: the second half has one tile fewer)
        const float *Kt = lds + 2 * kh * TILE, *Vt = Kt + TILE;
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < D / 8; ++kb) {
            const float4 kf = *reinterpret_cast<const float4 *>(Kt + li * PITCH + 8 * kb + 4 * lh);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[kb].x, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[kb].y, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[kb].z, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[kb].w, sacc, 0, 0, 0);
        }
        // ---- bias, padded keys, running max
        float mt = -3.0e38f;
        {
            int2 kt[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) kt[r] = kterm[kh * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] += G[hb - kt[r].x] + G[wb - kt[r].y];
        }
        if (tile * 32 + 32 > N) {                                       // (wave-uniform: the last tile only)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh >= N) sacc[r] = -3.0e38f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sacc[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        float lt = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f((sacc[r] - m_new) * 1.44269504088896341f);
            sacc[r] = p;
            lt += p;
        }
        lt += __shfl_xor(lt, 32, 64);
        if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * 1.44269504088896341f);
            l_run *= alpha;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
        }
        l_run += lt;
        m_run = m_new;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int krow = (r & 3) + 8 * (r >> 2) + 4 * lh;
                o[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[krow * PITCH + vcol[ct]], sacc[r], o[ct], 0, 0, 0);
            }
        }
    }
    // ---- merge the two key halves of each query tile, normalise, store
    __syncthreads();
    float *X = lds + qt * (64 * (16 * NCT + 2));                        // per query tile: [lane][16 NCT + 2] (inside the K / V tiles' region)
    static_assert(2 * 64 * (16 * NCT + 2) <= 4 * TILE, "exchange region");
    if (kh == 1) {
        float *x = X + lane * (16 * NCT + 2);
        x[0] = m_run; x[1] = l_run;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) x[2 + 16 * ct + r] = o[ct][r];
    }
    __syncthreads();
    if (kh == 0) {
        const float *x = X + lane * (16 * NCT + 2);
        const float m1 = x[0], l1 = x[1];
        const float m = fmaxf(m_run, m1);
        const float a0 = exp2f((m_run - m) * 1.44269504088896341f), a1 = exp2f((m1 - m) * 1.44269504088896341f);
        const float inv = 1.0f / (l_run * a0 + l1 * a1);
        if (qi < N) {
            float *orow = out + ((int64_t)b * N + qi) * out_ld + head * D;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (32 * ct + 8 * g >= D) continue;                 // (compile time: the unused half of the last column tile at D = 80)
                    float4 v;
                    v.x = (o[ct][4 * g + 0] * a0 + x[2 + 16 * ct + 4 * g + 0] * a1) * inv;
                    v.y = (o[ct][4 * g + 1] * a0 + x[2 + 16 * ct + 4 * g + 1] * a1) * inv;
                    v.z = (o[ct][4 * g + 2] * a0 + x[2 + 16 * ct + 4 * g + 2] * a1) * inv;
                    v.w = (o[ct][4 * g + 3] * a0 + x[2 + 16 * ct + 4 * g + 3] * a1) * inv;
                    *reinterpret_cast<float4 *>(orow + 32 * ct + 8 * g + 4 * lh) = v;
                }
        }
    }
}

// ---- window partition / un-partition ---------------------------------------------------------------------------------------------------------
// part: in [n, gh, gw, c] -> out [n * wy * wx, ws * ws, 1, c], window (b, iy, ix) = batch (b * wy + iy) * wx + ix, token ty * ws + tx = pixel
// (iy ws + ty, ix ws + tx), zeros beyond the map.  unpart: out [n, gh, gw, c] = res + in[window layout] (the padding is dropped).
__global__ __launch_bounds__(256) void k_window(int unpart, const float *__restrict__ in, int in_ld, const float *__restrict__ res, int res_ld,
                                                float *__restrict__ out, int out_ld, int n, int gh, int gw, int ws, int c) {
    const int c4 = c >> 2, wy = (gh + ws - 1) / ws, wx = (gw + ws - 1) / ws;
    const int64_t rows = unpart ? (int64_t)n * gh * gw : (int64_t)n * wy * wx * ws * ws;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * c4) return;
    const int64_t row = idx / c4;
    const int q = (int)(idx - row * c4);
    if (unpart) {
        const int x = (int)(row % gw), y = (int)((row / gw) % gh);
        const int64_t b = row / ((int64_t)gw * gh);
        const int iy = y / ws, ix = x / ws;
        const int64_t src = ((b * wy + iy) * wx + ix) * (int64_t)(ws * ws) + (y - iy * ws) * ws + (x - ix * ws);
        float4 v = *reinterpret_cast<const float4 *>(in + src * in_ld + 4 * q);
        if (res) {
            const float4 r = *reinterpret_cast<const float4 *>(res + row * res_ld + 4 * q);
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        *reinterpret_cast<float4 *>(out + row * out_ld + 4 * q) = v;
    } else {
        const int t = (int)(row % (ws * ws));
        const int64_t win = row / (ws * ws);
        const int ix = (int)(win % wx), iy = (int)((win / wx) % wy);
        const int64_t b = win / ((int64_t)wx * wy);
        const int y = iy * ws + t / ws, x = ix * ws + t % ws;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (y < gh && x < gw) v = *reinterpret_cast<const float4 *>(in + ((b * gh + y) * gw + x) * (int64_t)in_ld + 4 * q);
        *reinterpret_cast<float4 *>(out + row * out_ld + 4 * q) = v;
    }
}

// out[b, p, :] = in0[b % n0, p, :] (+ in1[b % n1, p, :]) (+ aux: per channel [c], or per position and channel [np][c])
__global__ __launch_bounds__(256) void k_bcast_add(const float *__restrict__ a, int a_ld, int n0, const float *__restrict__ bb, int b_ld, int n1,
                                                   float *__restrict__ out, int out_ld, int n, int64_t np, int c, const float *__restrict__ aux, int aux_map) {
    const int c4 = c >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * np * c4) return;
    const int64_t row = idx / c4;
    const int q = (int)(idx - row * c4);
    const int64_t b = row / np, p = row - b * np;
    float4 v = *reinterpret_cast<const float4 *>(a + ((b % n0) * np + p) * a_ld + 4 * q);
    if (bb) {
        const float4 w = *reinterpret_cast<const float4 *>(bb + ((b % n1) * np + p) * b_ld + 4 * q);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    if (aux) {
        const float4 w = *reinterpret_cast<const float4 *>(aux + (aux_map ? p * c : 0) + 4 * q);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    *reinterpret_cast<float4 *>(out + row * out_ld + 4 * q) = v;
}

// out[b, p, 0] = sum_c in[b, p, c] * h[b, c]   (in ascending channel order, fp32)
__global__ __launch_bounds__(256) void k_channel_dot(const float *__restrict__ in, int in_ld, const float *__restrict__ h, int h_ld, float *__restrict__ out,
                                                     int out_ld, int n, int64_t np, int c) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * np) return;
    const int64_t b = idx / np;
    const float *x = in + idx * in_ld, *hv = h + b * h_ld;
    float s = 0.0f;
    for (int i = 0; i < c; i += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(x + i), w = *reinterpret_cast<const float4 *>(hv + i);
        s = fmaf(v.x, w.x, s); s = fmaf(v.y, w.y, s); s = fmaf(v.z, w.z, s); s = fmaf(v.w, w.w, s);
    }
    out[idx * out_ld] = s;
}

// ---- cross-attention: q [n, Nq, heads D] (pre-scaled), kv [n, Nk, (k: heads D | v: heads D)] -> out [n, Nq, heads D] ---------------------------
// Small problems (7 tokens against the image's pixels and the reverse): plain fp32 sums, no matrix pipe.
// k_xattn_wave: a wave per (sample, head, query); the lanes stride over the keys with a running max / sum each and are merged at the end.
template <int D>
__global__ __launch_bounds__(256) void k_xattn_wave(const float *__restrict__ q, int q_ld, const float *__restrict__ kv, int kv_ld, float *__restrict__ out,
                                                    int out_ld, int64_t total, int Nq, int Nk, int heads) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= total) return;
    const int qi = (int)(wid % Nq), head = (int)((wid / Nq) % heads);
    const int64_t b = wid / ((int64_t)Nq * heads);
    const float *qp = q + (b * Nq + qi) * q_ld + head * D;
    float qv[D], o[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { qv[i] = qp[i]; o[i] = 0.0f; }
    float m = -3.0e38f, l = 0.0f;
    for (int j = lane; j < Nk; j += 64) {
        const float *kp = kv + (b * Nk + j) * kv_ld + head * D, *vp = kp + heads * D;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < D; ++i) s = fmaf(qv[i], kp[i], s);
        const float mn = fmaxf(m, s), alpha = expf(m - mn), p = expf(s - mn);
        l = l * alpha + p;
#pragma unroll
        for (int i = 0; i < D; ++i) o[i] = fmaf(p, vp[i], o[i] * alpha);
        m = mn;
    }
    const float M = wave_max(m), f = expf(m - M);                       // (a lane without keys: l = 0, o = 0)
    const float L = wave_sum(l * f);
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float t = wave_sum(o[i] * f);
        if (lane == i) mine = t;
    }
    if (lane < D) out[(b * Nq + qi) * out_ld + head * D + lane] = mine / L;
}

// k_xattn_lane: a lane per (sample, head, query) for SHORT key sets (every pixel attending to the 7 tokens): the keys are the same
// addresses across the lanes of a wave
template <int D>
__global__ __launch_bounds__(256) void k_xattn_lane(const float *__restrict__ q, int q_ld, const float *__restrict__ kv, int kv_ld, float *__restrict__ out,
                                                    int out_ld, int64_t total, int Nq, int Nk, int heads) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int qi = (int)(id % Nq), head = (int)((id / Nq) % heads);
    const int64_t b = id / ((int64_t)Nq * heads);
    const float *qp = q + (b * Nq + qi) * q_ld + head * D;
    float qv[D], o[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { qv[i] = qp[i]; o[i] = 0.0f; }
    float m = -3.0e38f, l = 0.0f;
    for (int j = 0; j < Nk; ++j) {
        const float *kp = kv + (b * Nk + j) * kv_ld + head * D, *vp = kp + heads * D;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < D; ++i) s = fmaf(qv[i], kp[i], s);
        const float mn = fmaxf(m, s), alpha = expf(m - mn), p = expf(s - mn);
        l = l * alpha + p;
#pragma unroll
        for (int i = 0; i < D; ++i) o[i] = fmaf(p, vp[i], o[i] * alpha);
        m = mn;
    }
    float *op = out + (b * Nq + qi) * out_ld + head * D;
    const float inv = 1.0f / l;
#pragma unroll
    for (int i = 0; i < D; ++i) op[i] = o[i] * inv;
}

// ---- image -> model input ----------------------------------------------------------------------------------------------------------------------
// BGR uint8 [H, W, 3] -> RGB float NCHW [3, S, S]: bilinear (align_corners = False, no antialiasing) to nh x nw, (v - mean) / std, zeros beyond
__device__ __forceinline__ void src_index(int dst, float scale, int in_size, int &i0, int &i1, float &l1) {
    const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)s, in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    l1 = s - (float)i0;
}

__global__ __launch_bounds__(256) void k_sam_preprocess(const uint8_t *__restrict__ img, int H, int W, int S, int nh, int nw, float *__restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    float r[3] = {0.0f, 0.0f, 0.0f};
    if (y < nh && x < nw) {
        int y0, y1, x0, x1;
        float ly, lx;
        src_index(y, (float)H / (float)nh, H, y0, y1, ly);
        src_index(x, (float)W / (float)nw, W, x0, x1, lx);
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int ch = 2 - c;                                       // RGB plane c <- BGR byte 2 - c
            const float p00 = img[((int64_t)y0 * W + x0) * 3 + ch], p01 = img[((int64_t)y0 * W + x1) * 3 + ch];
            const float p10 = img[((int64_t)y1 * W + x0) * 3 + ch], p11 = img[((int64_t)y1 * W + x1) * 3 + ch];
            const float v = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
            r[c] = (v - mean[c]) / sd[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(int64_t)c * S * S + idx] = r[c];
}

// low-res logits [n, L, L] -> bilinear to S x S -> crop [nh, nw] -> bilinear to H x W -> > 0, fused: an output pixel reads its four
// neighbours in the cropped S-space map, each of them four logits
__global__ __launch_bounds__(256) void k_sam_postprocess(const float *__restrict__ lg, int n, int L, int S, int nh, int nw, int H, int W, uint8_t *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * H * W) return;
    const int x = (int)(idx % W), y = (int)((idx / W) % H);
    const float *src = lg + (idx / ((int64_t)W * H)) * L * L;
    int Y[2], X[2];
    float ly, lx;
    src_index(y, (float)nh / (float)H, nh, Y[0], Y[1], ly);
    src_index(x, (float)nw / (float)W, nw, X[0], X[1], lx);
    const float up = (float)L / (float)S;
    float v[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        int y0, y1;
        float my;
        src_index(Y[a], up, L, y0, y1, my);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int x0, x1;
            float mx;
            src_index(X[c], up, L, x0, x1, mx);
            v[a][c] = (1.0f - my) * ((1.0f - mx) * src[y0 * L + x0] + mx * src[y0 * L + x1]) + my * ((1.0f - mx) * src[y1 * L + x0] + mx * src[y1 * L + x1]);
        }
    }
    const float r = (1.0f - ly) * ((1.0f - lx) * v[0][0] + lx * v[0][1]) + ly * ((1.0f - lx) * v[1][0] + lx * v[1][1]);
    out[idx] = r > 0.0f ? 1 : 0;
}

// boxes [n, 4] (x0, y0, x1, y1; scaled by (sx, sy) into the model's input frame) -> decoder tokens NCHW [n, C, T, 1], T = n_static + 2:
// rows < n_static = the constant output tokens, then the two corners: sin | cos of 2 pi ((2 (p + 0.5) / S - 1) . gauss) + point embedding.
// consts: [n_static][C] tokens, [2][C] corner embeddings, [2][C / 2] the Gaussian matrix.  Trigonometry in double (a few hundred values).
__global__ __launch_bounds__(256) void k_sam_box_tokens(const float *__restrict__ boxes, int n, double sx, double sy, int S, const float *__restrict__ consts, int C,
                                                        int n_static, float *__restrict__ out) {
    const int T = n_static + 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * C * T) return;
    const int t = idx % T, c = (idx / T) % C, b = idx / (T * C);
    float v;
    if (t < n_static) v = consts[t * C + c];
    else {
        const int k = t - n_static, hf = C / 2, f = c < hf ? c : c - hf;
        const float *gauss = consts + (n_static + 2) * C;
        const double px = 2.0 * (((double)boxes[b * 4 + 2 * k] * sx + 0.5) / (double)S) - 1.0;
        const double py = 2.0 * (((double)boxes[b * 4 + 2 * k + 1] * sy + 0.5) / (double)S) - 1.0;
        const double arg = 6.283185307179586476925 * (px * (double)gauss[f] + py * (double)gauss[hf + f]);
        v = (float)((c < hf ? sin(arg) : cos(arg)) + (double)consts[(n_static + k) * C + c]);
    }
    out[idx] = v;
}

}  // namespace

namespace csm {

template <int D> static int launch_attention_rp_t(const float *qkv, int ld, float *out, int out_ld, int n, int N, int heads, const float *table, int gh, int gw,
                                                  hipStream_t st) {
    const int TT = 2 * gh - 1 + 2 * gw - 1, TTP = (TT + 31) & ~31;
    const size_t lds = sizeof(float) * ((size_t)4 * 32 * (D + 4) + 128 + (size_t)2 * TTP * 32);
    if (lds > 160 * 1024) { set_error("attention_relpos: a %d x %d token grid needs %zu bytes of LDS (160 KB available)", gh, gw, lds); return CSM_ERR_ARG; }
    static std::mutex prep_mutex;
    static size_t have[32] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 31;
    {
        std::lock_guard<std::mutex> lk(prep_mutex);
        if (lds > have[dev]) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_attention_rp<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) { set_error("attention_relpos: %zu bytes of LDS requested: %s", lds, hipGetErrorString(e)); return CSM_ERR_HIP; }
            have[dev] = lds;
        }
    }
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)heads, (unsigned)n);
    k_attention_rp<D><<<grid, 256, lds, st>>>(qkv, ld, out, out_ld, N, heads, table, gh, gw);
    return check_launch("k_attention_rp");
}

int launch_attention_relpos(const float *qkv, int ld, float *out, int out_ld, int n, int N, int heads, int d, const float *table, int gh, int gw,
                            hipStream_t st) {
    if (N < 1 || gh < 1 || gw < 1 || gh * gw != N || !table) { set_error("attention_relpos: N == gh * gw tokens and the (Rh ; Rw) table required (%d x %d vs %d)", gh, gw, N); return CSM_ERR_ARG; }
    if (n < 1 || n > 65535 || heads < 1 || heads > 65535) { set_error("attention_relpos: batch / heads out of range (%d, %d)", n, heads); return CSM_ERR_ARG; }
    if ((ld & 3) || (out_ld & 3) || (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)table) & 15)) { set_error("attention_relpos: qkv / out / table must be 16-byte aligned"); return CSM_ERR_ARG; }
    switch (d) {
        case 32: return launch_attention_rp_t<32>(qkv, ld, out, out_ld, n, N, heads, table, gh, gw, st);
        case 64: return launch_attention_rp_t<64>(qkv, ld, out, out_ld, n, N, heads, table, gh, gw, st);
        case 80: return launch_attention_rp_t<80>(qkv, ld, out, out_ld, n, N, heads, table, gh, gw, st);
        case 128: return launch_attention_rp_t<128>(qkv, ld, out, out_ld, n, N, heads, table, gh, gw, st);
        default: set_error("attention_relpos: head dimension %d not built (32, 64, 80, 128)", d); return CSM_ERR_ARG;
    }
}

int launch_window(int unpart, const float *in, int in_ld, const float *res, int res_ld, float *out, int out_ld, int n, int gh, int gw, int ws, int c,
                  hipStream_t st) {
    if ((c & 3) || (in_ld & 3) || (out_ld & 3) || (res_ld & 3) || ws < 1 || gh < 1 || gw < 1) { set_error("window: channels %% 4 == 0 and a window size required"); return CSM_ERR_ARG; }
    const int wy = (gh + ws - 1) / ws, wx = (gw + ws - 1) / ws;
    const int64_t total = (unpart ? (int64_t)n * gh * gw : (int64_t)n * wy * wx * ws * ws) * (c >> 2);
    k_window<<<cdiv(total, 256), 256, 0, st>>>(unpart, in, in_ld, res, res_ld, out, out_ld, n, gh, gw, ws, c);
    return check_launch("k_window");
}

int launch_bcast_add(const float *a, int a_ld, int n0, const float *b, int b_ld, int n1, float *out, int out_ld, int n, int64_t np, int c, const float *aux,
                     int aux_map, hipStream_t st) {
    if ((c & 3) || (a_ld & 3) || (out_ld & 3) || (b && (b_ld & 3)) || (n0 != 1 && n0 != n) || (b && n1 != 1 && n1 != n)) { set_error("broadcast add: channels %% 4 == 0, operand batch 1 or the output's"); return CSM_ERR_ARG; }
    k_bcast_add<<<cdiv((int64_t)n * np * (c >> 2), 256), 256, 0, st>>>(a, a_ld, n0, b, b_ld, b ? n1 : 1, out, out_ld, n, np, c, aux, aux_map);
    return check_launch("k_bcast_add");
}

int launch_channel_dot(const float *in, int in_ld, const float *h, int h_ld, float *out, int out_ld, int n, int64_t np, int c, hipStream_t st) {
    if ((c & 3) || (in_ld & 3) || (h_ld & 3)) { set_error("channel_dot: channels %% 4 == 0"); return CSM_ERR_ARG; }
    k_channel_dot<<<cdiv((int64_t)n * np, 256), 256, 0, st>>>(in, in_ld, h, h_ld, out, out_ld, n, np, c);
    return check_launch("k_channel_dot");
}

template <int D> static int launch_xattn_t(const float *q, int q_ld, const float *kv, int kv_ld, float *out, int out_ld, int n, int Nq, int Nk, int heads,
                                           hipStream_t st) {
    const int64_t total = (int64_t)n * heads * Nq;
    if (Nk <= 16) k_xattn_lane<D><<<cdiv(total, 256), 256, 0, st>>>(q, q_ld, kv, kv_ld, out, out_ld, total, Nq, Nk, heads);
    else k_xattn_wave<D><<<cdiv(total, 4), 256, 0, st>>>(q, q_ld, kv, kv_ld, out, out_ld, total, Nq, Nk, heads);
    return check_launch("k_xattn");
}

int launch_cross_attention(const float *q, int q_ld, const float *kv, int kv_ld, float *out, int out_ld, int n, int Nq, int Nk, int heads, int d,
                           hipStream_t st) {
    if (n < 1 || Nq < 1 || Nk < 1 || heads < 1) { set_error("cross_attention: empty operand"); return CSM_ERR_ARG; }
    if ((int64_t)n * heads * Nq / 4 >= 0x7fffffff) { set_error("cross_attention: too many queries for one launch"); return CSM_ERR_ARG; }
    switch (d) {
        case 2: return launch_xattn_t<2>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        case 4: return launch_xattn_t<4>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        case 8: return launch_xattn_t<8>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        case 16: return launch_xattn_t<16>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        case 32: return launch_xattn_t<32>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        case 64: return launch_xattn_t<64>(q, q_ld, kv, kv_ld, out, out_ld, n, Nq, Nk, heads, st);
        default: set_error("cross_attention: head dimension %d not built (2, 4, 8, 16, 32, 64)", d); return CSM_ERR_ARG;
    }
}

}  // namespace csm

extern "C" int csm_sam_preprocess(const uint8_t *bgr, int H, int W, int S, int nh, int nw, float *out, void *stream) {
    CSM_REQUIRE(bgr && out && H > 0 && W > 0 && S > 0 && nh > 0 && nw > 0 && nh <= S && nw <= S && S <= 32768);
    k_sam_preprocess<<<csm::cdiv((int64_t)S * S, 256), 256, 0, (hipStream_t)stream>>>(bgr, H, W, S, nh, nw, out);
    return csm::check_launch("k_sam_preprocess");
}

extern "C" int csm_sam_postprocess(const float *logits, int n, int L, int S, int nh, int nw, int H, int W, uint8_t *masks, void *stream) {
    CSM_REQUIRE(n >= 0 && L > 0 && S > 0 && nh > 0 && nw > 0 && nh <= S && nw <= S && H > 0 && W > 0 && L <= 32768);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(logits && masks);
    k_sam_postprocess<<<csm::cdiv((int64_t)n * H * W, 256), 256, 0, (hipStream_t)stream>>>(logits, n, L, S, nh, nw, H, W, masks);
    return csm::check_launch("k_sam_postprocess");
}

extern "C" int csm_sam_box_tokens(const float *boxes, int n, double sx, double sy, int S, const float *consts, int C, int n_static, float *tokens,
                                  void *stream) {
    CSM_REQUIRE(n >= 0 && S > 0 && C > 0 && (C & 1) == 0 && n_static >= 0 && (int64_t)n * C * (n_static + 2) < 0x7fffffff);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(boxes && consts && tokens);
    k_sam_box_tokens<<<csm::cdiv((int64_t)n * C * (n_static + 2), 256), 256, 0, (hipStream_t)stream>>>(boxes, n, sx, sy, S, consts, C, n_static, tokens);
    return csm::check_launch("k_sam_box_tokens");
}
