// csm_glue.h -- the device expressions of the per-frame depth glue (image tensor, LeReS post-processing, depth adjustment, raw
// min/max, normalisation, disparity -> points, crop minMaxLoc), shared by the single-frame entry points (imageops.hip, warp.hip) and
// the batched ones (frameglue.hip): both compile THIS code, so a batched call returns the bits of the per-frame calls.
// Block functions (`*_block`) are called by all 256 threads of a block; `bid` / `nblk` are the block's index and the number of
// blocks that share the reduction (the single-frame kernels pass blockIdx.x / gridDim.x).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "csm_resample.h"

namespace csmglue {

using csmimg::cv_lin_u8;

__device__ __forceinline__ unsigned f2ord(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// ---- uint8 HWC -> float32 CHW * (1/255) ----------------------------------------------------------------------------------------
__device__ __forceinline__ void u8_hwc_to_f32_chw_px(const uint8_t *__restrict__ src, int64_t plane, int64_t i, float *__restrict__ out) {
    const float s = (float)(1.0 / 255.0);
    out[i] = (float)src[i * 3] * s; out[plane + i] = (float)src[i * 3 + 1] * s; out[2 * plane + i] = (float)src[i * 3 + 2] * s;
}

// ---- LeReS output: quantise, resize back, zero fix ----------------------------------------------------------------------------
// depth fp32 -> u8: 65535*(d-min)/(max-min) -> uint16 (trunc) -> cvRound(x*255/65535) -> 255 - v
__device__ __forceinline__ uint8_t leres_quantize_px(float d, float mn, float mx) {
    float o = 0.0f;
    if ((double)(mx - mn) > 2.220446049250313e-16) o = 65535.0f * (d - mn) / (mx - mn);
    uint16_t u16 = (uint16_t)o;
    float s = (float)u16 * (float)(255.0 / 65535.0);
    int v = (int)rintf(fabsf(s));
    v = v > 255 ? 255 : v;
    return (uint8_t)(255 - v);
}

// INTER_AREA when up-sampling: linear taps with "area" fractions (resize.cpp, area_mode branch)
__device__ __forceinline__ void cv_src_area(int d, int in_size, double scale, int &i0, int &i1, float &f) {
    int sx = (int)floor(d * scale);
    float fx = (float)((d + 1) - (sx + 1) * (1.0 / scale));
    fx = fx <= 0.0f ? 0.0f : fx - floorf(fx);
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= in_size - 1) { fx = 0.0f; sx = in_size - 1; }
    i0 = sx; i1 = min(sx + 1, in_size - 1); f = fx;
}

// u8 [h,w] -> fp32 value at (y, x) of [H,W] with cv2.resize: INTER_AREA when enlarging, identity if same size
__device__ __forceinline__ float resize_u8_to_f32_px(const uint8_t *__restrict__ src, int h, int w, int H, int W, int y, int x) {
    int q;
    if (h == H && w == W) q = src[(int64_t)y * w + x];
    else {
        int y0, y1, x0, x1; float fy, fx;
        cv_src_area(y, h, (double)h / H, y0, y1, fy); cv_src_area(x, w, (double)w / W, x0, x1, fx);
        q = cv_lin_u8(src[(int64_t)y0 * w + x0], src[(int64_t)y0 * w + x1], src[(int64_t)y1 * w + x0], src[(int64_t)y1 * w + x1], fx, fy);
    }
    return (float)q;
}

// interpolateLanczos4 coefficients in float -> short Q11 (cvRound)
__device__ __forceinline__ void lanczos4_q11(float x, int c[8]) {
    const double s45 = 0.70710678118654752440084436210485;
    const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    float coeffs[8], sum = 0.0f;
    const double y0 = -(x + 3) * 3.14159265358979323846 * 0.25, s0 = sin(y0), c0 = cos(y0);
    for (int i = 0; i < 8; ++i) {
        const float y0_ = (x + 3 - i);
        if (fabsf(y0_) >= 1e-6f) {
            const double y = -y0_ * 3.14159265358979323846 * 0.25;
            coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        } else coeffs[i] = 1e30f;
        sum += coeffs[i];
    }
    sum = 1.0f / sum;
    for (int i = 0; i < 8; ++i) {
        const float v = coeffs[i] * sum * 2048.0f;
        int q = (int)rintf(v);
        c[i] = q > 32767 ? 32767 : (q < -32768 ? -32768 : q);
    }
}

// cv2.resize(u8 [h,w], (W,H), INTER_LANCZOS4) value at (y, x), as float32
__device__ __forceinline__ float resize_u8_lanczos4_px(const uint8_t *__restrict__ src, int h, int w, int H, int W, int y, int x) {
    float fx = (float)((x + 0.5) * ((double)w / W) - 0.5), fy = (float)((y + 0.5) * ((double)h / H) - 0.5);
    int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= (float)sx; fy -= (float)sy;
    int cx[8], cy[8];
    lanczos4_q11(fx, cx); lanczos4_q11(fy, cy);
    int acc = 0;
    for (int j = 0; j < 8; ++j) {
        int yy = sy - 3 + j; yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
        int row = 0;
        for (int i = 0; i < 8; ++i) {
            int xx = sx - 3 + i; xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
            row += (int)src[(int64_t)yy * w + xx] * cx[i];
        }
        acc += row * cy[j];
    }
    int v = (acc + (1 << 21)) >> 22;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    return (float)v;
}

// `depth[depth == 0] = depth[depth > 0].min()`: a thread folds its values with minpos_acc, the block folds the threads with
// minpos_fold_block; thread 0 then holds the block's smallest positive value (as bits: positive floats order like their bit
// patterns; 0xffffffff = none) and whether a zero was seen.
__device__ __forceinline__ void minpos_acc(float v, unsigned &mn, int &z) {
    if (v > 0.0f) mn = min(mn, __float_as_uint(v));
    z |= v == 0.0f;
}
__device__ __forceinline__ void minpos_fold_block(unsigned &mn, int &z) {
    __shared__ unsigned smn[256]; __shared__ int sz[256];
    smn[threadIdx.x] = mn; sz[threadIdx.x] = z;
    __syncthreads();
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
        if ((int)threadIdx.x < s2) { smn[threadIdx.x] = min(smn[threadIdx.x], smn[threadIdx.x + s2]); sz[threadIdx.x] |= sz[threadIdx.x + s2]; }
        __syncthreads();
    }
    mn = smn[0]; z = sz[0];
}
// rewrite only when a zero exists and something is positive
__device__ __forceinline__ void minpos_apply_px(float *__restrict__ x, int64_t i, unsigned min_pos_bits, bool zero_seen) {
    if (!zero_seen || min_pos_bits == 0xffffffffu) return;
    if (x[i] == 0.0f) x[i] = __uint_as_float(min_pos_bits);
}

// ---- {min, max} of x[0..n): partial pairs per block, one block folds them (min / max are order-free) --------------------------
// float4 loads over the 16-byte aligned body; the (at most 3) elements in front of it and the tail go to block 0 one by one
__device__ __forceinline__ void minmax_partial_block(const float *__restrict__ x, int64_t n, int bid, int nblk, float *__restrict__ part) {
    __shared__ float smn[256], smx[256];
    float mn = INFINITY, mx = -INFINITY;
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    const int64_t n4 = (n - head) >> 2;
    const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < n4; i += (int64_t)nblk * 256) {
        float4 v = x4[i];
        mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    if (bid == 0) {
        for (int64_t i = head + (n4 << 2) + threadIdx.x; i < n; i += 256) { float v = x[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
        if ((int64_t)threadIdx.x < head) { float v = x[threadIdx.x]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    }
    smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) {
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + st]);
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * bid] = smn[0]; part[2 * bid + 1] = smx[0]; }
}
__device__ __forceinline__ void minmax_final_block(const float *__restrict__ part, int nparts, float *__restrict__ out) {
    __shared__ float smn[256], smx[256];
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += 256) { mn = fminf(mn, part[2 * i]); mx = fmaxf(mx, part[2 * i + 1]); }
    smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) {
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + st]);
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = smn[0]; out[1] = smx[0]; }
}
// number of partial blocks csm_minmax uses for n elements (<= 256: the scratch holds 512 floats)
inline int minmax_nparts(int64_t n) { return (int)(n >= (1 << 18) ? 256 : (n + 1023) / 1024 > 0 ? (n + 1023) / 1024 : 1); }

// ---- depth_adjustment_animesseg, one instance (kenburns_effect.py:68-78) -------------------------------------------------------
// plane = disp * mask.  Rows of the instance = rows whose plane has a positive entry (the reference tests `plane.sum(3) > 0`;
// disparities are non-negative, so "sum > 0" == "any > 0"); r0 = round_half_even(top + 0.97 (bottom - top)) in float64;
// val = max of the plane over rows >= r0 (zeros outside the mask included, like the reference's slice); pixels of the mask
// become val.  Skipped when the plane is empty (`plane.sum() == 0`).
// row r: maximum of the plane and flags (bit 0: a positive entry, bit 1: a non-zero entry)
__device__ __forceinline__ void adjust_rows_block(const float *__restrict__ disp, const uint8_t *__restrict__ mask, int W, int r,
                                                  float *__restrict__ rowmax, float *__restrict__ rowflag) {
    __shared__ float smax[256];
    __shared__ int sflag[256];
    float mx = -INFINITY; int fl = 0;
    for (int x = threadIdx.x; x < W; x += 256) {
        float p = disp[(int64_t)r * W + x] * (mask[(int64_t)r * W + x] ? 1.0f : 0.0f);
        mx = fmaxf(mx, p);
        fl |= (p > 0.0f ? 1 : 0) | (p != 0.0f ? 2 : 0);
    }
    smax[threadIdx.x] = mx; sflag[threadIdx.x] = fl;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) {
            smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + st]);
            sflag[threadIdx.x] |= sflag[threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { rowmax[r] = smax[0]; rowflag[r] = (float)sflag[0]; }
}
// out2 = {val, apply ? 1 : 0}
__device__ __forceinline__ void adjust_pick_block(const float *__restrict__ rowmax, const float *__restrict__ rowflag, int H,
                                                  float *__restrict__ out2) {
    __shared__ int stop[256], sbot[256], snz[256];
    __shared__ float smax[256];
    int top = H, bot = -1, nz = 0;
    for (int r = threadIdx.x; r < H; r += 256) {
        int f = (int)rowflag[r];
        if (f & 1) { top = min(top, r); bot = max(bot, r); }
        nz |= f & 2;
    }
    stop[threadIdx.x] = top; sbot[threadIdx.x] = bot; snz[threadIdx.x] = nz;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) {
            stop[threadIdx.x] = min(stop[threadIdx.x], stop[threadIdx.x + st]);
            sbot[threadIdx.x] = max(sbot[threadIdx.x], sbot[threadIdx.x + st]);
            snz[threadIdx.x] |= snz[threadIdx.x + st];
        }
        __syncthreads();
    }
    top = stop[0]; bot = sbot[0]; nz = snz[0];
    const bool apply = bot >= 0 && nz != 0;
    const int r0 = apply ? (int)rint((double)top + (0.97 * (double)(bot - top))) : H;
    float mx = -INFINITY;
    for (int r = threadIdx.x; r < H; r += 256)
        if (r >= r0) mx = fmaxf(mx, rowmax[r]);
    smax[threadIdx.x] = mx;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = smax[0]; out2[1] = apply ? 1.0f : 0.0f; }
}
// kenburns_effect.py:78, literally
__device__ __forceinline__ float adjust_apply_px(float d, uint8_t mk, float val) {
    const float m = mk ? 1.0f : 0.0f;
    return ((1.0f - m) * d) + (m * val);
}

// ---- kenburns_effect.py:928 `disparity / disparity.max() * baseline` (two roundings, like torch) ------------------------------
__device__ __forceinline__ float normalise_px(float x, float mx, float scale) { return (x / mx) * scale; }

// ---- kenburns_effect.py:929-933: Laplacian of the (scaled) disparity, depth, valid, points, unaltered -------------------------
// `at(index)` returns the disparity at a row-major index: a stored map, or the normalisation of the raw map evaluated in place
template <class At>
__device__ __forceinline__ float laplacian_f(At at, int x, int y, int H, int W, float scale_div) {
    int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
    int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    float acc = 0.0f;
    if (scale_div != 0.0f) {
        acc += -1.0f * (at((int64_t)ym * W + x) / scale_div);
        acc += -1.0f * (at((int64_t)ym * W + xp) / scale_div);
        acc += -1.0f * (at((int64_t)y * W + xm) / scale_div);
        acc += 4.0f * (at((int64_t)y * W + x) / scale_div);
        acc += -1.0f * (at((int64_t)yp * W + xm) / scale_div);
    } else {
        acc += -1.0f * at((int64_t)ym * W + x);
        acc += -1.0f * at((int64_t)ym * W + xp);
        acc += -1.0f * at((int64_t)y * W + xm);
        acc += 4.0f * at((int64_t)y * W + x);
        acc += -1.0f * at((int64_t)yp * W + xm);
    }
    return acc;
}
__device__ __forceinline__ float laplacian_at(const float *__restrict__ I, int x, int y, int H, int W, float scale_div) {
    return laplacian_f([I](int64_t i) { return I[i]; }, x, y, H, W, scale_div);
}

// one pixel of disparity -> {depth, valid, points, unaltered}; `at` as in laplacian_f, dn = at(o), dmax = the map's maximum.
// Returns the depth.
template <class At>
__device__ __forceinline__ float disparity_to_points_px(At at, float dn, float dmax, int x, int y, int H, int W, float fb, float eps,
                                                         float invf, float x_start, float y_start, float *__restrict__ depth,
                                                         float *__restrict__ valid, float *__restrict__ pts,
                                                         float *__restrict__ unaltered) {
    const int64_t plane = (int64_t)H * W, o = (int64_t)y * W + x;
    float d = (1.0f / (dn + eps)) * fb;  // float / Tensor == reciprocal()*float in torch
    float lap = laplacian_f(at, x, y, H, W, dmax);
    float v = fabsf(lap) < 0.03f ? 1.0f : 0.0f;
    float hx = (x_start + (float)x) * invf, vy = (y_start + (float)y) * invf;
    depth[o] = d; valid[o] = v;
    float dv = d * v;
    pts[o] = dv * hx; pts[plane + o] = dv * vy; pts[2 * plane + o] = dv;
    unaltered[o] = d * hx; unaltered[plane + o] = d * vy; unaltered[2 * plane + o] = d;
    return d;
}

// ---- cv2.minMaxLoc of a crop: value and FIRST row-major position of the minimum and of the maximum -----------------------------
// Keys = (ordered value << 32) | index (smallest wins) and (ordered value << 32) | ~index (largest wins); i = index in the crop
__device__ __forceinline__ void crop_keys_acc(float d, unsigned i, unsigned long long &mn, unsigned long long &mx) {
    unsigned o = f2ord(d);
    unsigned long long a = ((unsigned long long)o << 32) | i, b = ((unsigned long long)o << 32) | (unsigned)(~i);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
}
// after the call thread 0 holds the block's keys
__device__ __forceinline__ void crop_keys_fold_block(unsigned long long &mn, unsigned long long &mx) {
    __shared__ unsigned long long kmn[256], kmx[256];
    kmn[threadIdx.x] = mn; kmx[threadIdx.x] = mx;
    __syncthreads();
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
        if ((int)threadIdx.x < s2) {
            kmn[threadIdx.x] = kmn[threadIdx.x + s2] < kmn[threadIdx.x] ? kmn[threadIdx.x + s2] : kmn[threadIdx.x];
            kmx[threadIdx.x] = kmx[threadIdx.x + s2] > kmx[threadIdx.x] ? kmx[threadIdx.x + s2] : kmx[threadIdx.x];
        }
        __syncthreads();
    }
    mn = kmn[0]; mx = kmx[0];
}
// out[0..5] (float64) = {raw_min_normalised, raw_max_normalised, crop min, crop max, crop argmin, crop argmax}
__device__ __forceinline__ void stats_pack(const float *__restrict__ minmax_raw, float scale, unsigned long long kmin, unsigned long long kmax,
                                           double *__restrict__ out) {
    out[0] = (double)normalise_px(minmax_raw[0], minmax_raw[1], scale);     // min / max of the normalised map: x -> (x/m)*s is monotonic
    out[1] = (double)normalise_px(minmax_raw[1], minmax_raw[1], scale);
    out[2] = (double)ord2f((unsigned)(kmin >> 32)); out[3] = (double)ord2f((unsigned)(kmax >> 32));
    out[4] = (double)(unsigned)(kmin & 0xffffffffull); out[5] = (double)(unsigned)(~(unsigned)(kmax & 0xffffffffull));
}

}  // namespace csmglue
