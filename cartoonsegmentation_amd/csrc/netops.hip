// netops.hip -- the layer kernels of the program executor (nets.hip) that are not tiled implicit GEMMs: the stem and narrow-output
// convolutions, the split-K reduction, depthwise conv, pooling, resampling, element-wise ops, the ZoeDepth head ops and the layout
// transposes, each with its launch code.
#include "csm_convcfg.h"

using namespace csmconv;

namespace {

// ---- stem convolution (cin padded to 4: RTMDet / ISNet / LeReS first layers) -----------------------------------------------
// The generic kernels spend one 32-channel chunk per tap with 4 channels in use.  Here K is packed (tap, channel): a chunk holds
// 8 taps x 4 channels (weights packed to match on the host, program.py::pack_stem_weights), 7 chunks instead of 49 for the
// 7x7.  Each loader thread fetches one pixel's 4 channels for one tap (one float4) and scatters them into the 8-block positions
// that make the MFMA lane order 0,4,1,5,2,6,3,7 walk tap 2j's channels 0..3 and then tap 2j+1's -- the contract's chain.
// 64x64 tile, 2x2 waves, register-staged (the permutation rules out LDS-DMA), one LDS buffer; HBM-bound for the 3x3 stems.
__global__ __launch_bounds__(256) void k_conv_stem(ConvArgs a) {
    constexpr int BM = 64, BN = 64;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * kLdsLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    int mt, ntile, zz;
    block_to_tile(mt, ntile, zz);
    const int m0 = mt * BM, n0 = ntile * BN;
    const int ho = a.out.h, wo = a.out.w, ntaps = a.kh * a.kw, nck = (ntaps + 7) >> 3;
    // A loader: thread -> rows (tid>>3) and (tid>>3)+32, tap slot j = tid&7 of the chunk
    const int j = tid & 7;
    const float *rowp[2]; int iy0[2], ix0[2]; bool rv[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        int m = m0 + (tid >> 3) + 32 * it;
        rv[it] = m < a.M;
        int mm = rv[it] ? m : 0;
        int n = mm / (ho * wo), rem = mm - n * ho * wo;
        int oy = rem / wo, ox = rem - oy * wo;
        iy0[it] = oy * a.stride - a.pad; ix0[it] = ox * a.stride - a.pad;
        rowp[it] = a.in.p + (int64_t)n * a.in.h * a.in.w * a.in.ld;
    }
    const float *wp[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) wp[it] = a.w + (int64_t)(n0 + (tid >> 3) + 32 * it) * 32 + j * 4;
    float4 ra[2], rb[2];
    auto gload = [&](int c) {
        const int t = 8 * c + j, kh = t / a.kw, kw = t - kh * a.kw;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            int iy = iy0[it] + kh * a.dil, ix = ix0[it] + kw * a.dil;
            bool v = rv[it] && t < ntaps && iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w;
            ra[it] = v ? *reinterpret_cast<const float4 *>(rowp[it] + ((int64_t)iy * a.in.w + ix) * a.in.ld) : make_float4(0.f, 0.f, 0.f, 0.f);
            bool vb = n0 + (tid >> 3) + 32 * it < a.npad;
            rb[it] = vb ? *reinterpret_cast<const float4 *>(wp[it] + (int64_t)c * a.npad * 32) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            float *row = lds + ((tid >> 3) + 32 * it) * kLdsLd + 8 * (j >> 1) + 2 * (j & 1);
            *reinterpret_cast<float2 *>(row) = make_float2(ra[it].x, ra[it].z);          // (c0, c2) of this tap
            *reinterpret_cast<float2 *>(row + 4) = make_float2(ra[it].y, ra[it].w);      // (c1, c3)
            *reinterpret_cast<float4 *>(lds + (BM + (tid >> 3) + 32 * it) * kLdsLd + j * 4) = rb[it];
        }
    };
    f32x16 acc;
    {
        int n = n0 + 32 * wn + li;
        float b = (a.bias && n < a.cout_g) ? a.bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = b;
    }
    const float *A = lds + (32 * wm + li) * kLdsLd + 4 * lh;
    const float *B = lds + (BM + 32 * wn + li) * kLdsLd + 4 * lh;
    gload(0);
    for (int c = 0; c < nck; ++c) {
        lstore();
        __syncthreads();
        if (c + 1 < nck) gload(c + 1);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const float4 af = *reinterpret_cast<const float4 *>(A + kb * 8);
            const float4 bf = *reinterpret_cast<const float4 *>(B + kb * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int n = n0 + 32 * wn + li;
    if (n >= a.cout_g) return;
    const float slope = a.slope ? a.slope[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int m = m0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= a.M) continue;
        float v = acc[r];
        if (a.res_mode == 1) v += a.res.p[(int64_t)m * a.res.ld + n];
        v = apply_act(v, a.act, slope);
        if (a.res_mode == 2) v += a.res.p[(int64_t)m * a.res.ld + n];
        a.out.p[(int64_t)m * a.out.ld + n] = v;
    }
}

// ---- narrow-output convolution (cout <= 4, groups == 1, no split-K): ISNet side outputs / LeReS last conv -------------------
// An N = 1 output wastes 31/32 of an MFMA tile; this is the same fmaf chain (32-channel blocks, taps row-major, 8-channel
// sub-blocks in the order 0,4,1,5,2,6,3,7; out-of-image taps contribute exact zeros) evaluated one output pixel per lane on the VALU.  A lane's chain
// cannot be shared between lanes, so a lane reads whole pixels: straight from global that is 64 scattered 16-B pieces per
// load instruction (TA-bound, measured no faster than the MFMA path); instead the block stages its input region
// (TH x 32 outputs + halo, all channels) into LDS with coalesced loads -- pixel pitch cin+4 floats makes the per-lane
// ds_read_b128 conflict-free -- and the weights too.  HBM-bound: the input is read once.
template <int NOUT, int TH>
__global__ __launch_bounds__(32 * TH) void k_conv_narrow(ConvArgs a, int tiles_x, int tiles_y, int rh, int rw) {
    constexpr int TW = 32, NT = 32 * TH;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int T = a.kh * a.kw * a.ncb, pitch = a.cin_g + 4;
    float *wl = sm;                                   // [cb][tap][NOUT][32] (= chunk order of the packed weights)
    float *xl = sm + ((T * NOUT * 32 + 3) & ~3);      // [rh][rw][pitch]
    const int tid = threadIdx.x;
    for (int i = tid; i < T * NOUT * 32; i += NT) {
        int c = i & 31, n = (i >> 5) % NOUT, ch = i / (32 * NOUT);
        wl[i] = n < a.cout_g ? a.w[((int64_t)ch * a.npad + n) * 32 + c] : 0.0f;
    }
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
    const int c4n = a.cin_g >> 2, total = rh * rw * c4n;
    for (int i0 = tid; i0 < total; i0 += NT * 8) {               // 8 loads in flight per lane before the first LDS store
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int i = i0 + u * NT;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < total) {
                int c4 = i % c4n, pix = i / c4n;
                int ry = pix / rw, rx = pix - ry * rw;
                int iy = iy0 + ry, ix = ix0 + rx;
                if (iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w)
                    v[u] = *reinterpret_cast<const float4 *>(a.in.p + ((int64_t)(n * a.in.h + iy) * a.in.w + ix) * a.in.ld + c4 * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int i = i0 + u * NT;
            if (i < total) *reinterpret_cast<float4 *>(xl + (i / c4n) * pitch + (i % c4n) * 4) = v[u];
        }
    }
    __syncthreads();
    const int ly = tid >> 5, lx = tid & 31;
    const int oy = oy0 + ly, ox = ox0 + lx;
    if (oy >= a.out.h || ox >= a.out.w) return;
    float acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = (a.bias && j < a.cout_g) ? a.bias[j] : 0.0f;
    for (int cb = 0; cb < a.ncb; ++cb)
        for (int kh = 0; kh < a.kh; ++kh)
            for (int kw = 0; kw < a.kw; ++kw) {
                const float *P = xl + ((ly * a.stride + kh * a.dil) * rw + lx * a.stride + kw * a.dil) * pitch;
                const float *W = wl + (cb * a.kh * a.kw + kh * a.kw + kw) * NOUT * 32;
#pragma unroll 4
                for (int c8 = cb * 32; c8 < cb * 32 + 32 && c8 < a.cin_g; c8 += 8) {   // cin_g % 4 == 0; a trailing half block is 4 channels
                    const float4 lo = *reinterpret_cast<const float4 *>(P + c8);
                    const float4 hi = c8 + 4 < a.cin_g ? *reinterpret_cast<const float4 *>(P + c8 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float *w8 = W + (c8 & 31);
#pragma unroll
                    for (int j = 0; j < NOUT; ++j) {
                        const float *w = w8 + j * 32;
                        float v = acc[j];
                        v = fmaf(lo.x, w[0], v); v = fmaf(hi.x, w[4], v);
                        v = fmaf(lo.y, w[1], v); v = fmaf(hi.y, w[5], v);
                        v = fmaf(lo.z, w[2], v); v = fmaf(hi.z, w[6], v);
                        v = fmaf(lo.w, w[3], v); v = fmaf(hi.w, w[7], v);
                        acc[j] = v;
                    }
                }
            }
    const int64_t m = ((int64_t)n * a.out.h + oy) * a.out.w + ox;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        if (j >= a.cout_g) break;
        float v = acc[j];
        float slope = a.slope ? a.slope[j] : 0.0f;
        if (a.res_mode == 1) v += a.res.p[m * a.res.ld + j];
        v = apply_act(v, a.act, slope);
        if (a.res_mode == 2) v += a.res.p[m * a.res.ld + j];
        a.out.p[m * a.out.ld + j] = v;
    }
}

// The same kernel with the input staged ONE 32-channel block at a time (the chain order is block-major anyway): the region of an 8 x 32
// output tile then takes 49 KB instead of 92 KB at 64 channels, three 256-thread blocks share a CU, and each block has 43 KB of loads in
// flight per staging step instead of 16 KB -- the whole-region form ran the 64 -> 1 side output of ISNet at 1.0 TB/s (0.52 ms at batch 16:
// 531 MB of input), bound by bytes in flight, not by arithmetic (576 fmaf per pixel = 15 us of VALU) or LDS.
template <int NOUT>
__global__ __launch_bounds__(256) void k_conv_narrow_cb(ConvArgs a, int tiles_x, int tiles_y, int rh, int rw) {
    constexpr int TH = 8, TW = 32, NT = 256, PITCH = 36;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int taps = a.kh * a.kw, T = taps * a.ncb;
    float *wl = sm;                                   // [cb][tap][NOUT][32] (= chunk order of the packed weights)
    float *xl = sm + ((T * NOUT * 32 + 3) & ~3);      // [rh][rw][PITCH]: the current channel block of the input region
    const int tid = threadIdx.x;
    for (int i = tid; i < T * NOUT * 32; i += NT) {
        int c = i & 31, n = (i >> 5) % NOUT, ch = i / (32 * NOUT);
        wl[i] = n < a.cout_g ? a.w[((int64_t)ch * a.npad + n) * 32 + c] : 0.0f;
    }
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
    const int ly = tid >> 5, lx = tid & 31;
    const int oy = oy0 + ly, ox = ox0 + lx;
    const bool live = oy < a.out.h && ox < a.out.w;
    float acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = (a.bias && j < a.cout_g) ? a.bias[j] : 0.0f;
    for (int cb = 0; cb < a.ncb; ++cb) {
        const int cw = min(32, a.cin_g - 32 * cb), c4n = cw >> 2, total = rh * rw * c4n;
        __syncthreads();                                         // the previous block's reads are done (first pass: nothing)
        for (int i0 = tid; i0 < total; i0 += NT * 8) {           // 8 loads in flight per lane before the first LDS store
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int i = i0 + u * NT;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < total) {
                    int c4 = i % c4n, pix = i / c4n;
                    int ry = pix / rw, rx = pix - ry * rw;
                    int iy = iy0 + ry, ix = ix0 + rx;
                    if (iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w)
                        v[u] = *reinterpret_cast<const float4 *>(a.in.p + ((int64_t)(n * a.in.h + iy) * a.in.w + ix) * a.in.ld + 32 * cb + c4 * 4);
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int i = i0 + u * NT;
                if (i < total) *reinterpret_cast<float4 *>(xl + (i / c4n) * PITCH + (i % c4n) * 4) = v[u];
            }
        }
        __syncthreads();
        if (!live) continue;
        for (int kh = 0; kh < a.kh; ++kh)
            for (int kw = 0; kw < a.kw; ++kw) {
                const float *P = xl + ((ly * a.stride + kh * a.dil) * rw + lx * a.stride + kw * a.dil) * PITCH;
                const float *W = wl + (cb * taps + kh * a.kw + kw) * NOUT * 32;
#pragma unroll 4
                for (int c8 = 0; c8 < cw; c8 += 8) {             // cin_g % 4 == 0; a trailing half block is 4 channels
                    const float4 lo = *reinterpret_cast<const float4 *>(P + c8);
                    const float4 hi = c8 + 4 < cw ? *reinterpret_cast<const float4 *>(P + c8 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float *w8 = W + c8;
#pragma unroll
                    for (int j = 0; j < NOUT; ++j) {
                        const float *w = w8 + j * 32;
                        float v = acc[j];
                        v = fmaf(lo.x, w[0], v); v = fmaf(hi.x, w[4], v);
                        v = fmaf(lo.y, w[1], v); v = fmaf(hi.y, w[5], v);
                        v = fmaf(lo.z, w[2], v); v = fmaf(hi.z, w[6], v);
                        v = fmaf(lo.w, w[3], v); v = fmaf(hi.w, w[7], v);
                        acc[j] = v;
                    }
                }
            }
    }
    if (!live) return;
    const int64_t m = ((int64_t)n * a.out.h + oy) * a.out.w + ox;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        if (j >= a.cout_g) break;
        float v = acc[j];
        float slope = a.slope ? a.slope[j] : 0.0f;
        if (a.res_mode == 1) v += a.res.p[m * a.res.ld + j];
        v = apply_act(v, a.act, slope);
        if (a.res_mode == 2) v += a.res.p[m * a.res.ld + j];
        a.out.p[m * a.out.ld + j] = v;
    }
}

// LDS bytes of k_conv_narrow for a TH-row tile; 0 = does not fit
static size_t narrow_lds(const ConvArgs &a, int TH, int *rh_out, int *rw_out) {
    int nout = a.cout_g == 1 ? 1 : 4;
    int rh = (TH - 1) * a.stride + (a.kh - 1) * a.dil + 1, rw = 31 * a.stride + (a.kw - 1) * a.dil + 1;
    size_t fl = (((size_t)a.kh * a.kw * a.ncb * nout * 32 + 3) & ~(size_t)3) + (size_t)rh * rw * (a.cin_g + 4);
    if (rh_out) { *rh_out = rh; *rw_out = rw; }
    return fl * 4 <= 150 * 1024 ? fl * 4 : 0;
}

template <int NOUT, int TH>
static int launch_narrow_t(const ConvArgs &a, size_t lds, int rh, int rw, hipStream_t st) {
    static KernelPrep prep;
    (void)prep.ensure([&] { return prepare_kernel(&k_conv_narrow<NOUT, TH>, 32 * TH, (size_t)150 * 1024); });
    int tiles_x = (a.out.w + 31) / 32, tiles_y = (a.out.h + TH - 1) / TH;
    k_conv_narrow<NOUT, TH><<<(unsigned)(tiles_x * tiles_y * a.out.n), 32 * TH, lds, st>>>(a, tiles_x, tiles_y, rh, rw);
    return csm::check_launch("k_conv_narrow");
}

template <int NOUT>
static int launch_narrow_cb_t(const ConvArgs &a, size_t lds, int rh, int rw, hipStream_t st) {
    static KernelPrep prep;
    (void)prep.ensure([&] { return prepare_kernel(&k_conv_narrow_cb<NOUT>, 256, (size_t)64 * 1024); });
    int tiles_x = (a.out.w + 31) / 32, tiles_y = (a.out.h + 7) / 8;
    k_conv_narrow_cb<NOUT><<<(unsigned)(tiles_x * tiles_y * a.out.n), 256, lds, st>>>(a, tiles_x, tiles_y, rh, rw);
    return csm::check_launch("k_conv_narrow_cb");
}

static int launch_narrow(const ConvArgs &a, hipStream_t st) {
    int rh, rw;
    if (a.ncb > 1) {                                  // more than one channel block: stage them one at a time (three blocks per CU)
        const int nout = a.cout_g == 1 ? 1 : 4;
        rh = 7 * a.stride + (a.kh - 1) * a.dil + 1; rw = 31 * a.stride + (a.kw - 1) * a.dil + 1;
        const size_t fl = (((size_t)a.kh * a.kw * a.ncb * nout * 32 + 3) & ~(size_t)3) + (size_t)rh * rw * 36;
        if (fl * 4 <= 54400) return a.cout_g == 1 ? launch_narrow_cb_t<1>(a, fl * 4, rh, rw, st) : launch_narrow_cb_t<4>(a, fl * 4, rh, rw, st);
    }
    size_t lds = narrow_lds(a, 8, &rh, &rw);
    if (lds && lds <= 50 * 1024) return a.cout_g == 1 ? launch_narrow_t<1, 8>(a, lds, rh, rw, st) : launch_narrow_t<4, 8>(a, lds, rh, rw, st);
    lds = narrow_lds(a, 4, &rh, &rw);
    return a.cout_g == 1 ? launch_narrow_t<1, 4>(a, lds, rh, rw, st) : launch_narrow_t<4, 4>(a, lds, rh, rw, st);
}

// split-K tail: v = ((p0 + p1) + p2) + ... in run order, then the usual epilogue
__global__ __launch_bounds__(256) void k_splitk_reduce(ConvArgs a) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.M * a.cout_g) return;
    int n = (int)(idx % a.cout_g); int64_t m = idx / a.cout_g;
    const float *P = a.partial + m * a.ksplit * a.cout_g + n;
    float v = P[0];
    for (int s = 1; s < a.ksplit; ++s) v += P[(int64_t)s * a.cout_g];
    float slope = a.slope ? a.slope[n] : 0.0f;
    if (a.res_mode == 1) v += a.res.p[m * a.res.ld + n];
    v = apply_act(v, a.act, slope);
    if (a.res_mode == 2) v += a.res.p[m * a.res.ld + n];
    a.out.p[m * a.out.ld + n] = v;
}

// depthwise conv (RTMDet CSPNeXt 5x5): lane = (pixel, 4 channels); weights [tap][C]; fmaf chain over taps
struct DwArgs { View in, out; const float *w, *bias, *slope; int kh, kw, stride, pad, dil, act; };
__global__ __launch_bounds__(256) void k_dwconv(DwArgs a) {
    const int c4n = a.out.c >> 2;
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)a.out.n * a.out.h * a.out.w * c4n;
    if (idx >= total) return;
    int c = (int)(idx % c4n) * 4; int64_t pix = idx / c4n;
    int ox = (int)(pix % a.out.w); int64_t t = pix / a.out.w; int oy = (int)(t % a.out.h); int n = (int)(t / a.out.h);
    float4 acc = a.bias ? *reinterpret_cast<const float4 *>(a.bias + c) : make_float4(0, 0, 0, 0);
    for (int kh = 0; kh < a.kh; ++kh) {
        int iy = oy * a.stride - a.pad + kh * a.dil;
        if (iy < 0 || iy >= a.in.h) continue;
        for (int kw = 0; kw < a.kw; ++kw) {
            int ix = ox * a.stride - a.pad + kw * a.dil;
            if (ix < 0 || ix >= a.in.w) continue;
            float4 x = *reinterpret_cast<const float4 *>(a.in.p + ((int64_t)(n * a.in.h + iy) * a.in.w + ix) * a.in.ld + c);
            float4 w = *reinterpret_cast<const float4 *>(a.w + (int64_t)(kh * a.kw + kw) * a.out.c + c);
            acc.x = fmaf(x.x, w.x, acc.x); acc.y = fmaf(x.y, w.y, acc.y);
            acc.z = fmaf(x.z, w.z, acc.z); acc.w = fmaf(x.w, w.w, acc.w);
        }
    }
    float4 s = a.slope ? *reinterpret_cast<const float4 *>(a.slope + c) : make_float4(0, 0, 0, 0);
    acc.x = apply_act(acc.x, a.act, s.x); acc.y = apply_act(acc.y, a.act, s.y);
    acc.z = apply_act(acc.z, a.act, s.z); acc.w = apply_act(acc.w, a.act, s.w);
    *reinterpret_cast<float4 *>(a.out.p + pix * a.out.ld + c) = acc;
}


// depthwise conv, stride 1 / dilation 1 (CSPNeXt 5x5): same chain as k_dwconv, but the block first stages its input region
// (8x16 outputs + halo, 32 channels) in LDS -- every input element is used by kh*kw outputs, and from global that re-use
// came out of L2 (measured ~12 TB/s of L2 traffic, L2-bound); from LDS the kernel is HBM-bound.  Out-of-image taps add
// exact zeros.  Thread = (channel quad, 4 output pixels).
__global__ __launch_bounds__(256) void k_dwconv_lds(DwArgs a, int tiles_x, int tiles_y) {
    constexpr int TH = 8, TW = 16;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int rh = TH + a.kh - 1, rw = TW + a.kw - 1, taps = a.kh * a.kw;
    float *wl = sm;                       // [tap][32]
    float *xl = sm + taps * 32;           // [rh*rw][32]
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int c0 = blockIdx.y * 32;
    const int oy0 = ty * TH, ox0 = tx * TW, iy0 = oy0 - a.pad, ix0 = ox0 - a.pad;
    for (int i = tid; i < taps * 32; i += 256) wl[i] = a.w[(int64_t)(i >> 5) * a.out.c + c0 + (i & 31)];
    const int total = rh * rw * 8;
    for (int i0 = tid; i0 < total; i0 += 256 * 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int i = i0 + u * 256;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < total) {
                int c4 = i & 7, pix = i >> 3;
                int ry = pix / rw, rx = pix - ry * rw;
                int iy = iy0 + ry, ix = ix0 + rx;
                if (iy >= 0 && iy < a.in.h && ix >= 0 && ix < a.in.w)
                    v[u] = *reinterpret_cast<const float4 *>(a.in.p + ((int64_t)(n * a.in.h + iy) * a.in.w + ix) * a.in.ld + c0 + c4 * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int i = i0 + u * 256;
            if (i < total) *reinterpret_cast<float4 *>(xl + (i >> 3) * 32 + (i & 7) * 4) = v[u];
        }
    }
    __syncthreads();
    const int c4 = tid & 7, p0 = tid >> 3;              // pixels p0 + 32*j of the 8x16 tile
    const float4 bias = a.bias ? *reinterpret_cast<const float4 *>(a.bias + c0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 sl = a.slope ? *reinterpret_cast<const float4 *>(a.slope + c0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bias;
    for (int kh = 0; kh < a.kh; ++kh)
        for (int kw = 0; kw < a.kw; ++kw) {
            const float4 w = *reinterpret_cast<const float4 *>(wl + (kh * a.kw + kw) * 32 + c4 * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pix = p0 + 32 * j, py = pix >> 4, px = pix & 15;
                const float4 x = *reinterpret_cast<const float4 *>(xl + ((py + kh) * rw + px + kw) * 32 + c4 * 4);
                acc[j].x = fmaf(x.x, w.x, acc[j].x); acc[j].y = fmaf(x.y, w.y, acc[j].y);
                acc[j].z = fmaf(x.z, w.z, acc[j].z); acc[j].w = fmaf(x.w, w.w, acc[j].w);
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = p0 + 32 * j, oy = oy0 + (pix >> 4), ox = ox0 + (pix & 15);
        if (oy >= a.out.h || ox >= a.out.w) continue;
        float4 v = acc[j];
        v.x = apply_act(v.x, a.act, sl.x); v.y = apply_act(v.y, a.act, sl.y);
        v.z = apply_act(v.z, a.act, sl.z); v.w = apply_act(v.w, a.act, sl.w);
        *reinterpret_cast<float4 *>(a.out.p + ((int64_t)(n * a.out.h + oy) * a.out.w + ox) * a.out.ld + c0 + c4 * 4) = v;
    }
}

// max pooling (window clipped to the input; ceil_mode handled by the host-computed output size)
__global__ __launch_bounds__(256) void k_maxpool(View in, View out, int k, int stride, int pad) {
    const int c4n = out.c >> 2;
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * c4n;
    if (idx >= total) return;
    int c = (int)(idx % c4n) * 4; int64_t pix = idx / c4n;
    int ox = (int)(pix % out.w); int64_t t = pix / out.w; int oy = (int)(t % out.h); int n = (int)(t / out.h);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int ky = 0; ky < k; ++ky) {
        int iy = oy * stride - pad + ky;
        if (iy < 0 || iy >= in.h) continue;
        for (int kx = 0; kx < k; ++kx) {
            int ix = ox * stride - pad + kx;
            if (ix < 0 || ix >= in.w) continue;
            float4 x = *reinterpret_cast<const float4 *>(in.p + ((int64_t)(n * in.h + iy) * in.w + ix) * in.ld + c);
            m.x = fmaxf(m.x, x.x); m.y = fmaxf(m.y, x.y); m.z = fmaxf(m.z, x.z); m.w = fmaxf(m.w, x.w);
        }
    }
    *reinterpret_cast<float4 *>(out.p + pix * out.ld + c) = m;
}

// torch upsample_bilinear2d index/lambda (aten UpSample.h: area_pixel_compute_source_index + guard)
__device__ __forceinline__ void src_index(int dst, int in_size, int out_size, float scale, bool align, int &i0, int &i1,
                                          float &l0, float &l1) {
    if (in_size == out_size) { i0 = i1 = dst; l0 = 1.0f; l1 = 0.0f; return; }
    float real;
    if (align) real = scale * (float)dst;
    else { real = scale * ((float)dst + 0.5f) - 0.5f; if (real < 0.0f) real = 0.0f; }
    i0 = min((int)real, in_size - 1);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = fminf(fmaxf(real - (float)i0, 0.0f), 1.0f);
    l0 = 1.0f - l1;
}

// bilinear resize: VEC = 4 handles 4 channels per lane with 16-byte accesses (c, pitches and bases 16-byte aligned),
// VEC = 1 is the generic path (single-channel side outputs).  Same expression per element in both.
template <int VEC>
__global__ __launch_bounds__(256) void k_bilinear(View in, View out, int align, float sh, float sw, int act, const float *__restrict__ slope) {
    const int cv = out.c / VEC;
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * cv;
    if (idx >= total) return;
    int c = (int)(idx % cv) * VEC; int64_t pix = idx / cv;
    int ox = (int)(pix % out.w); int64_t t = pix / out.w; int oy = (int)(t % out.h); int n = (int)(t / out.h);
    int y0, y1, x0, x1; float hl0, hl1, wl0, wl1;
    src_index(oy, in.h, out.h, sh, align != 0, y0, y1, hl0, hl1);
    src_index(ox, in.w, out.w, sw, align != 0, x0, x1, wl0, wl1);
    const float *P = in.p + (int64_t)n * in.h * in.w * in.ld + c;
    const float *a00 = P + ((int64_t)y0 * in.w + x0) * in.ld, *a01 = P + ((int64_t)y0 * in.w + x1) * in.ld;
    const float *a10 = P + ((int64_t)y1 * in.w + x0) * in.ld, *a11 = P + ((int64_t)y1 * in.w + x1) * in.ld;
    float *O = out.p + pix * out.ld + c;
    if (VEC == 4) {
        float4 p00 = *reinterpret_cast<const float4 *>(a00), p01 = *reinterpret_cast<const float4 *>(a01);
        float4 p10 = *reinterpret_cast<const float4 *>(a10), p11 = *reinterpret_cast<const float4 *>(a11);
        float4 r;
        r.x = hl0 * (wl0 * p00.x + wl1 * p01.x) + hl1 * (wl0 * p10.x + wl1 * p11.x);
        r.y = hl0 * (wl0 * p00.y + wl1 * p01.y) + hl1 * (wl0 * p10.y + wl1 * p11.y);
        r.z = hl0 * (wl0 * p00.z + wl1 * p01.z) + hl1 * (wl0 * p10.z + wl1 * p11.z);
        r.w = hl0 * (wl0 * p00.w + wl1 * p01.w) + hl1 * (wl0 * p10.w + wl1 * p11.w);
        if (act) {
            r.x = apply_act(r.x, act, slope ? slope[c] : 0.0f); r.y = apply_act(r.y, act, slope ? slope[c + 1] : 0.0f);
            r.z = apply_act(r.z, act, slope ? slope[c + 2] : 0.0f); r.w = apply_act(r.w, act, slope ? slope[c + 3] : 0.0f);
        }
        *reinterpret_cast<float4 *>(O) = r;
    } else {
        const float r = hl0 * (wl0 * a00[0] + wl1 * a01[0]) + hl1 * (wl0 * a10[0] + wl1 * a11[0]);
        O[0] = act ? apply_act(r, act, slope ? slope[c] : 0.0f) : r;
    }
}

// The same resize with the output ROW as the block coordinate (grid = (runs of 256 (pixel, 4-channel) pairs, out.h, out.n)): the sample
// and the row's source rows / weights are wave-uniform, the column index needs one magic-number division -- k_bilinear<4> spends most of
// its instructions in three 64-bit divisions per output word (3.5 TB/s in + out on the 2x decoder upsamplings; this form: see
// profiles/r06_elementwise.txt).  Same expressions per element, same bits.
__global__ __launch_bounds__(256) void k_bilinear_rows(View in, View out, int align, float sh, float sw, int act, const float *__restrict__ slope,
                                                       unsigned cv_mul, unsigned cv_shr) {
    const int cv = out.c >> 2, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= out.w * cv) return;
    const int oy = blockIdx.y, n = blockIdx.z;
    const int ox = (int)fast_div((unsigned)j, cv_mul, cv_shr), c = (j - ox * cv) * 4;
    int y0, y1, x0, x1; float hl0, hl1, wl0, wl1;
    src_index(oy, in.h, out.h, sh, align != 0, y0, y1, hl0, hl1);
    src_index(ox, in.w, out.w, sw, align != 0, x0, x1, wl0, wl1);
    const float *P = in.p + (int64_t)n * in.h * in.w * in.ld + c;
    const float *r0 = P + (int64_t)y0 * in.w * in.ld, *r1 = P + (int64_t)y1 * in.w * in.ld;
    const float4 p00 = *reinterpret_cast<const float4 *>(r0 + x0 * in.ld), p01 = *reinterpret_cast<const float4 *>(r0 + x1 * in.ld);
    const float4 p10 = *reinterpret_cast<const float4 *>(r1 + x0 * in.ld), p11 = *reinterpret_cast<const float4 *>(r1 + x1 * in.ld);
    float4 r;
    r.x = hl0 * (wl0 * p00.x + wl1 * p01.x) + hl1 * (wl0 * p10.x + wl1 * p11.x);
    r.y = hl0 * (wl0 * p00.y + wl1 * p01.y) + hl1 * (wl0 * p10.y + wl1 * p11.y);
    r.z = hl0 * (wl0 * p00.z + wl1 * p01.z) + hl1 * (wl0 * p10.z + wl1 * p11.z);
    r.w = hl0 * (wl0 * p00.w + wl1 * p01.w) + hl1 * (wl0 * p10.w + wl1 * p11.w);
    if (act) {
        r.x = apply_act(r.x, act, slope ? slope[c] : 0.0f); r.y = apply_act(r.y, act, slope ? slope[c + 1] : 0.0f);
        r.z = apply_act(r.z, act, slope ? slope[c + 2] : 0.0f); r.w = apply_act(r.w, act, slope ? slope[c + 3] : 0.0f);
    }
    *reinterpret_cast<float4 *>(out.p + (((int64_t)n * out.h + oy) * out.w + ox) * out.ld + c) = r;
}

__global__ __launch_bounds__(256) void k_nearest(View in, View out) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * (out.c >> 2);
    if (idx >= total) return;
    int c4n = out.c >> 2;
    int c = (int)(idx % c4n) * 4; int64_t pix = idx / c4n;
    int ox = (int)(pix % out.w); int64_t t = pix / out.w; int oy = (int)(t % out.h); int n = (int)(t / out.h);
    int fy = out.h / in.h, fx = out.w / in.w;
    int iy = oy / fy, ix = ox / fx;
    *reinterpret_cast<float4 *>(out.p + pix * out.ld + c) =
        *reinterpret_cast<const float4 *>(in.p + ((int64_t)(n * in.h + iy) * in.w + ix) * in.ld + c);
}

// out = act(a + b), or unary act / copy when b.p == nullptr
// float4 form of k_eltwise for modes 0 (act / copy) and 1 (add): channel counts and strides that are multiples of 4, 16-B aligned
// views (everything the layer programs produce).  Same arithmetic per element; 1 thread = 4 channels of one pixel.
__global__ __launch_bounds__(256) void k_eltwise4(View a, View b, View out, int act, int mode, const float *__restrict__ slope) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c4n = out.c >> 2;
    const int64_t total = (int64_t)out.n * out.h * out.w * c4n;
    if (idx >= total) return;
    const int c = (int)(idx % c4n) * 4; const int64_t pix = idx / c4n;
    float4 v = *reinterpret_cast<const float4 *>(a.p + pix * a.ld + c);
    if (mode == 1) {
        const float4 w = *reinterpret_cast<const float4 *>(b.p + pix * b.ld + c);
        v.x = v.x + w.x; v.y = v.y + w.y; v.z = v.z + w.z; v.w = v.w + w.w;
    }
    float4 sl = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if (slope) sl = *reinterpret_cast<const float4 *>(slope + c);
    v.x = apply_act(v.x, act, sl.x); v.y = apply_act(v.y, act, sl.y); v.z = apply_act(v.z, act, sl.z); v.w = apply_act(v.w, act, sl.w);
    *reinterpret_cast<float4 *>(out.p + pix * out.ld + c) = v;
}
static bool eltwise4_ok(const View &a, const View *b, const View &out, const float *slope) {
    uintptr_t bits = (uintptr_t)a.p | (uintptr_t)out.p | (uintptr_t)slope;
    int lds = a.ld | out.ld | out.c;
    if (b) { bits |= (uintptr_t)b->p; lds |= b->ld; }
    return !(bits & 15) && !(lds & 3);
}

__global__ __launch_bounds__(256) void k_eltwise(View a, View b, View out, int act, int mode, const float *__restrict__ slope) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * out.c;
    if (idx >= total) return;
    int c = (int)(idx % out.c); int64_t pix = idx / out.c;
    float v;
    if (mode == 3) {        // add with a CROPPED first operand: a is up to one row / column larger than out (torch's negative pad)
        const int64_t hw = (int64_t)out.h * out.w; const int64_t n = pix / hw, r = pix - n * hw;
        const int y = (int)(r / out.w), x = (int)(r - (int64_t)y * out.w);
        v = a.p[((n * a.h + y) * a.w + x) * a.ld + c] + b.p[pix * b.ld + c];
    } else {
        v = a.p[pix * a.ld + c];
        if (mode == 1) v = v + b.p[pix * b.ld + c];
        else if (mode == 2) { int64_t n = pix / ((int64_t)out.h * out.w); v = v * b.p[n * b.ld + c]; }
    }
    out.p[pix * out.ld + c] = apply_act(v, act, slope ? slope[c] : 0.0f);
}

// ZoeDepth attractor update (attractor.py:117-208, memory_efficient loop): out_k = b_k + agg_i dist(A_i - b_k)
__global__ __launch_bounds__(256) void k_attractor(View A, View b, View out, const float *__restrict__ par, int flags) {
    const float alpha = par[0];
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * out.c;
    if (idx >= total) return;
    int k = (int)(idx % out.c); int64_t pix = idx / out.c;
    const float c = b.p[pix * b.ld + k];
    const float *a = A.p + pix * A.ld;
    float delta = 0.0f;
    for (int i = 0; i < A.c; ++i) {
        const float dx = a[i] - c;
        float d;
        if (flags & 1) d = csm_expf(-alpha * (fabsf(dx) * fabsf(dx))) * dx;      // exp_attractor, gamma = 2
        else d = dx / (1.0f + alpha * (dx * dx));                                // inv_attractor, gamma = 2
        delta += d;
    }
    if (flags & 2) delta = delta / (float)A.c;
    out.p[pix * out.ld + k] = c + delta;
}

// ConditionalLogBinomial tail + expectation over the bins (dist_layers.py:46-121, zoedepth_v1.py:196-199); NB <= 256
__global__ __launch_bounds__(256) void k_logbinom(View pt, View cen, View out, const float *__restrict__ par) {
    int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w;
    if (pix >= total) return;
    const float p_eps = par[0], min_temp = par[1], max_temp = par[2];
    const float *lb = par + 3;
    const float *q = pt.p + pix * pt.ld;
    const float p0 = q[0] + p_eps, p1 = q[1] + p_eps, t0 = q[2] + p_eps, t1 = q[3] + p_eps;
    const float p = p0 / (p0 + p1);
    float t = t0 / (t0 + t1);
    t = (max_temp - min_temp) * t + min_temp;
    const float eps = 1e-4f;                                           // LogBinomial.forward eps
    const float omx = fminf(fmaxf(1.0f - p, eps), 1.0f), x = fminf(fmaxf(p, eps), 1.0f);
    const float lx = csm_logf(x), lo = csm_logf(omx);
    const int K = cen.c;
    const float *c = cen.p + pix * cen.ld;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const float y = (lb[k] + (float)k * lx + (float)(K - 1 - k) * lo) / t;
        mx = fmaxf(mx, y);
    }
    float den = 0.0f, num = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float y = (lb[k] + (float)k * lx + (float)(K - 1 - k) * lo) / t;
        const float e = csm_expf(y - mx);
        den += e; num += e * c[k];
    }
    out.p[pix * out.ld] = num / den;
}

// global average pool with a fixed, oracle-reproducible reduction tree:
// 256 strided partial sums (sequential), then a binary tree 128,64,...,1, then / (h*w).
__global__ __launch_bounds__(256) void k_gavgpool(View in, View out) {
    __shared__ float part[256];
    int c = blockIdx.x, n = blockIdx.y;
    int hw = in.h * in.w;
    const float *P = in.p + (int64_t)n * hw * in.ld + c;
    float s = 0.0f;
    for (int i = threadIdx.x; i < hw; i += 256) s += P[(int64_t)i * in.ld];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out.p[(int64_t)n * out.ld + c] = part[0] / (float)hw;
}

// same reduction order as k_gavgpool (256 strided sequential partials per channel, then the tree 128,...,1), but a block owns
// 32 channels and lane t reads the 32 consecutive channels of pixels t, t+256, ...: 128-B pieces instead of one float per
// 1-KB stride (the per-channel kernel fetched 195 MB for a 26 MB tensor).
__global__ __launch_bounds__(256) void k_gavgpool32(View in, View out) {
    __shared__ float part[256][33];
    const int c0 = blockIdx.x * 32, n = blockIdx.y, t = threadIdx.x;
    const int hw = in.h * in.w;
    const float *P = in.p + (int64_t)n * hw * in.ld + c0;
    float s[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) s[c] = 0.0f;
    for (int i = t; i < hw; i += 256) {
        const float4 *q = reinterpret_cast<const float4 *>(P + (int64_t)i * in.ld);
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
            float4 v = q[c4];
            s[4 * c4] += v.x; s[4 * c4 + 1] += v.y; s[4 * c4 + 2] += v.z; s[4 * c4 + 3] += v.w;
        }
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) part[t][c] = s[c];
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        for (int i = t; i < st * 32; i += 256) {
            int r = i >> 5, c = i & 31;
            part[r][c] += part[r + st][c];
        }
        __syncthreads();
    }
    if (t < 32) out.p[(int64_t)n * out.ld + c0 + t] = part[0][t] / (float)hw;
}

__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const float *__restrict__ src, int csrc, View out) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)out.n * out.h * out.w * out.c;
    if (idx >= total) return;
    int c = (int)(idx % out.c); int64_t pix = idx / out.c;
    int64_t hw = (int64_t)out.h * out.w; int64_t n = pix / hw, p = pix - n * hw;
    out.p[pix * out.ld + c] = c < csrc ? src[(n * csrc + c) * hw + p] : 0.0f;
}

__global__ __launch_bounds__(256) void k_nhwc_to_nchw(View in, float *__restrict__ dst) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t hw = (int64_t)in.h * in.w;
    int64_t total = (int64_t)in.n * in.c * hw;
    if (idx >= total) return;
    int64_t p = idx % hw; int64_t t = idx / hw; int c = (int)(t % in.c); int64_t n = t / in.c;
    dst[idx] = in.p[(n * hw + p) * in.ld + c];
}

// LDS-tiled forms for wide tensors (the 64 / 69-channel planes around the inpainting splat: 270-290 MB each).  The one-element-
// per-lane kernels above read (resp. write) 64 different cache lines per wave and ran at 1.25 TB/s (read + write); here a block
// moves 64 pixels x C channels through LDS, global accesses on both sides are contiguous runs (pixels of one channel plane /
// channels of consecutive pixels), the [c][65] pitch keeps both LDS phases conflict-free.
constexpr int kTrPix = 64;
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_tile(const float *__restrict__ src, int csrc, View out) {
    extern __shared__ float tr[];                      // [out.c][kTrPix + 1]
    const int64_t hw = (int64_t)out.h * out.w;
    const int64_t tiles = (hw + kTrPix - 1) / kTrPix;
    const int64_t n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * kTrPix;
    const int C = out.c;
    for (int i = threadIdx.x; i < C * kTrPix; i += 256) {
        const int c = i >> 6, p = i & 63;
        tr[c * (kTrPix + 1) + p] = (c < csrc && p0 + p < hw) ? src[(n * csrc + c) * hw + p0 + p] : 0.0f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * kTrPix; i += 256) {
        const int p = i / C, c = i - p * C;
        if (p0 + p < hw) out.p[(n * hw + p0 + p) * out.ld + c] = tr[c * (kTrPix + 1) + p];
    }
}
__global__ __launch_bounds__(256) void k_nhwc_to_nchw_tile(View in, float *__restrict__ dst) {
    extern __shared__ float tr[];                      // [in.c][kTrPix + 1]
    const int64_t hw = (int64_t)in.h * in.w;
    const int64_t tiles = (hw + kTrPix - 1) / kTrPix;
    const int64_t n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * kTrPix;
    const int C = in.c;
    for (int i = threadIdx.x; i < C * kTrPix; i += 256) {
        const int p = i / C, c = i - p * C;
        tr[c * (kTrPix + 1) + p] = p0 + p < hw ? in.p[(n * hw + p0 + p) * in.ld + c] : 0.0f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * kTrPix; i += 256) {
        const int c = i >> 6, p = i & 63;
        if (p0 + p < hw) dst[(n * C + c) * hw + p0 + p] = tr[c * (kTrPix + 1) + p];
    }
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + 255) / 256); }

constexpr ConvCfg kRows[] = {{CFG_NARROW, "NARROW", FAM_NARROW, 4, &launch_narrow}};

}  // namespace

std::span<const ConvCfg> csmconv::conv_cfgs_narrow() { return kRows; }

bool csmconv::narrow_eligible(const ConvArgs &a) {
    return a.cout_g <= 4 && a.groups == 1 && a.ksplit == 1 && !(a.cin_g & 3) && !(a.in.ld & 3) && narrow_lds(a, 4, nullptr, nullptr) != 0;
}

int csmconv::launch_reduce(const ConvArgs &a, hipStream_t st) {
    k_splitk_reduce<<<(unsigned)(((int64_t)a.M * a.cout_g + 255) / 256), 256, 0, st>>>(a);
    return csm::check_launch("k_splitk_reduce");
}

int csmconv::launch_conv_stem(const ConvArgs &a, hipStream_t st) {
    dim3 grid((a.M + 63) / 64, (a.cout_g + 63) / 64, 1);
    k_conv_stem<<<grid, 256, 0, st>>>(a);
    return csm::check_launch("k_conv_stem");
}

int csmconv::launch_netop(const csm_op &op, int i, const View &in, const View &in1, const View &out, const float *weights, hipStream_t st) {
    switch (op.kind) {
        case CSM_OP_DWCONV: {
            if ((in.ld & 3) || (out.ld & 3) || (out.c & 3)) { csm::set_error("op %d: dwconv needs c%%4==0", i); return CSM_ERR_ARG; }
            DwArgs a{in, out, weights + op.w_off, op.b_off >= 0 ? weights + op.b_off : nullptr,
                     op.aux_off >= 0 ? weights + op.aux_off : nullptr, op.kh, op.kw, op.stride, op.pad, op.dil, op.act};
            size_t lds = ((size_t)op.kh * op.kw * 32 + (size_t)(8 + op.kh - 1) * (16 + op.kw - 1) * 32) * 4;
            if (op.stride == 1 && op.dil == 1 && !(out.c & 31) && lds <= 64 * 1024 && out.h == in.h + 2 * op.pad - op.kh + 1) {
                int tiles_x = (out.w + 15) / 16, tiles_y = (out.h + 7) / 8;
                k_dwconv_lds<<<dim3((unsigned)(tiles_x * tiles_y * out.n), (unsigned)(out.c / 32)), 256, lds, st>>>(a, tiles_x, tiles_y);
            } else
                k_dwconv<<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(a);
            break;
        }
        case CSM_OP_MAXPOOL:
            if ((in.ld & 3) || (out.ld & 3) || (out.c & 3)) { csm::set_error("op %d: maxpool needs c%%4==0", i); return CSM_ERR_ARG; }
            k_maxpool<<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(in, out, op.kh, op.stride, op.pad);
            break;
        case CSM_OP_BILINEAR: {
            bool align = op.flags & 1;
            float sh, sw;
            if (align) { sh = out.h > 1 ? (float)(in.h - 1) / (float)(out.h - 1) : 0.0f; sw = out.w > 1 ? (float)(in.w - 1) / (float)(out.w - 1) : 0.0f; }
            else { sh = (float)in.h / (float)out.h; sw = (float)in.w / (float)out.w; }
            bool vec = !(out.c & 3) && !(in.ld & 3) && !(out.ld & 3) && !(((uintptr_t)in.p | (uintptr_t)out.p) & 15);
            const float *bsl = op.aux_off >= 0 ? weights + op.aux_off : nullptr;
            if (vec && out.h <= 65535 && out.n <= 65535 && (int64_t)out.w * (out.c >> 2) < (1ll << 30)) {
                unsigned mul, shr;
                set_fast_div((unsigned)(out.c >> 2), mul, shr);
                k_bilinear_rows<<<dim3(blocks_for((int64_t)out.w * (out.c >> 2)), (unsigned)out.h, (unsigned)out.n), 256, 0, st>>>(in, out, align ? 1 : 0, sh, sw, op.act, bsl, mul, shr);
            } else if (vec) k_bilinear<4><<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(in, out, align ? 1 : 0, sh, sw, op.act, bsl);
            else k_bilinear<1><<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in, out, align ? 1 : 0, sh, sw, op.act, bsl);
            break;
        }
        case CSM_OP_NEAREST:
            if ((in.ld & 3) || (out.ld & 3) || (out.c & 3)) { csm::set_error("op %d: nearest needs c%%4==0", i); return CSM_ERR_ARG; }
            k_nearest<<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(in, out);
            break;
        case CSM_OP_ADD:
            if (in.h < out.h || in.w < out.w || in.h > out.h + 1 || in.w > out.w + 1 || in1.h != out.h || in1.w != out.w) {
                csm::set_error("op %d: add: the first operand may exceed the output by at most one row / column", i); return CSM_ERR_ARG;
            }
            if (in.h == out.h && in.w == out.w && eltwise4_ok(in, &in1, out, nullptr))
                k_eltwise4<<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(in, in1, out, op.act, 1, nullptr);
            else
                k_eltwise<<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in, in1, out, op.act,
                                                                                            (in.h != out.h || in.w != out.w) ? 3 : 1, nullptr);
            break;
        case CSM_OP_SCALE:
            k_eltwise<<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in, in1, out, op.act, 2, nullptr);
            break;
        case CSM_OP_ACT:
        case CSM_OP_COPY:
            if (eltwise4_ok(in, nullptr, out, op.aux_off >= 0 ? weights + op.aux_off : nullptr))
                k_eltwise4<<<blocks_for((int64_t)out.n * out.h * out.w * (out.c >> 2)), 256, 0, st>>>(in, in1, out, op.kind == CSM_OP_ACT ? op.act : 0, 0,
                                                                                                    op.aux_off >= 0 ? weights + op.aux_off : nullptr);
            else
                k_eltwise<<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in, in1, out, op.kind == CSM_OP_ACT ? op.act : 0, 0,
                                                                                              op.aux_off >= 0 ? weights + op.aux_off : nullptr);
            break;
        case CSM_OP_GAVGPOOL:
            if (!(in.c & 31) && !(in.ld & 3) && !(((uintptr_t)in.p) & 15)) k_gavgpool32<<<dim3(in.c / 32, in.n), 256, 0, st>>>(in, out);
            else k_gavgpool<<<dim3(in.c, in.n), 256, 0, st>>>(in, out);
            break;
        case CSM_OP_ATTRACTOR:
            if (op.aux_off < 0 || in.n != in1.n || in.h != in1.h || in.w != in1.w) { csm::set_error("op %d: attractor operands", i); return CSM_ERR_ARG; }
            k_attractor<<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in, in1, out, weights + op.aux_off, op.flags);
            break;
        case CSM_OP_LOGBINOM:
            if (op.aux_off < 0 || in.c < 4 || in1.c > 256) { csm::set_error("op %d: logbinom operands", i); return CSM_ERR_ARG; }
            k_logbinom<<<blocks_for((int64_t)out.n * out.h * out.w), 256, 0, st>>>(in, in1, out, weights + op.aux_off);
            break;
        case CSM_OP_NCHW_TO_NHWC:
            if (out.c >= 8 && out.c <= 240)
                k_nchw_to_nhwc_tile<<<(unsigned)(out.n * (((int64_t)out.h * out.w + kTrPix - 1) / kTrPix)), 256,
                                      sizeof(float) * (size_t)out.c * (kTrPix + 1), st>>>(in.p, in.c, out);
            else
                k_nchw_to_nhwc<<<blocks_for((int64_t)out.n * out.h * out.w * out.c), 256, 0, st>>>(in.p, in.c, out);
            break;
        case CSM_OP_NHWC_TO_NCHW:
            if (in.c >= 8 && in.c <= 240)
                k_nhwc_to_nchw_tile<<<(unsigned)(in.n * (((int64_t)in.h * in.w + kTrPix - 1) / kTrPix)), 256,
                                      sizeof(float) * (size_t)in.c * (kTrPix + 1), st>>>(in, out.p);
            else
                k_nhwc_to_nchw<<<blocks_for((int64_t)in.n * in.h * in.w * in.c), 256, 0, st>>>(in, out.p);
            break;
        default:
            csm::set_error("op %d: unknown kind %d", i, op.kind);
            return CSM_ERR_ARG;
    }
    return CSM_OK;
}
