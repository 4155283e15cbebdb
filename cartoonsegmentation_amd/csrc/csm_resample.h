// csm_resample.h -- device helpers shared by the image / mask glue kernels (imageops.hip, maskhead.hip, animeseg.hip), so the
// resamplers and the sigmoid cannot drift apart between translation units.  Restated in oracle/post_oracle.c.
//   * cv2.resize(INTER_LINEAR) source coordinate, the uint8 11-bit fixed-point blend and the float32 blend
//     [EXT: OpenCV 4.10 resize.cpp; cv2 is not vendored by the reference => parity unpinned],
//   * the exp / sigmoid polynomial of the numerical contract (same as csm_conv.h).
#pragma once
#include <hip/hip_runtime.h>

namespace csmimg {

// cv2.resize(INTER_LINEAR) source coordinate (half-pixel centres, clamped); scale = in_size / out_size
__device__ __forceinline__ void cv_src(int d, int in_size, double scale, int &i0, int &i1, float &f) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= in_size - 1) { fx = 0.0f; sx = in_size - 1; }
    i0 = sx; i1 = min(sx + 1, in_size - 1); f = fx;
}

// uint8 path: coefficients in Q11, horizontal pass to int, vertical pass with the >>4 / >>16 / +2 >>2 rounding, saturated
__device__ __forceinline__ int cv_lin_u8(int p00, int p01, int p10, int p11, float fx, float fy) {
    const int a0 = (int)rintf((1.0f - fx) * 2048.0f), a1 = (int)rintf(fx * 2048.0f);
    const int b0 = (int)rintf((1.0f - fy) * 2048.0f), b1 = (int)rintf(fy * 2048.0f);
    int r0 = p00 * a0 + p01 * a1, r1 = p10 * a0 + p11 * a1;
    int q = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

// float32 path: HResizeLinear (row: s0 * (1 - fx) + s1 * fx) then VResizeLinear (r0 * (1 - fy) + r1 * fy), all in fp32
__device__ __forceinline__ float cv_lin_f32(float p00, float p01, float p10, float p11, float fx, float fy) {
    const float a0 = 1.0f - fx, a1 = fx, b0 = 1.0f - fy, b1 = fy;
    const float r0 = p00 * a0 + p01 * a1;
    const float r1 = p10 * a0 + p11 * a1;
    return r0 * b0 + r1 * b1;
}

__device__ __forceinline__ float csm_expf(float x) {   // same polynomial as nets.hip / DESIGN.md
    x = fminf(fmaxf(x, -87.0f), 88.0f);
    float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);
    r = fmaf(n, -1.42860682030941723212e-6f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    float e = fmaf(p, r * r, r) + 1.0f;
    return e * __int_as_float(((int)n + 127) << 23);
}
__device__ __forceinline__ float csm_sigmoid(float v) { return 1.0f / (1.0f + csm_expf(-v)); }

}  // namespace csmimg
