// animeseg.hip -- glue of refine_method='animeseg' (animeinsseg/__init__.py:78-115, :623-630) around the anime-seg ISNet-IS
// network (ISNetDIS(in_ch=3), a layer program like every other net here), for gfx950:
//   * letterbox input of get_mask (animeinsseg/models/animeseg_refine/__init__.py:169-178): cv2 INTER_LINEAR u8 resize into the
//     centre of a zero s x s canvas, /255, NCHW,
//   * its output tail (:180-188): sigmoid of the d1 logits -> crop -> cv2 float INTER_LINEAR back to the frame -> > 0.5,
//   * the per-instance select of animeseg_refine (:96-105): areas of mask and mask & fg, refined iff area ratio > 0.3.
// All memory-bound, one pass each, no host round trip (the select decides on the device).
#include "csm_common.h"
#include "csm_resample.h"

namespace {

using csmimg::csm_sigmoid;
using csmimg::cv_lin_f32;
using csmimg::cv_lin_u8;
using csmimg::cv_src;

// one thread per canvas pixel of a row (blockIdx.y = canvas row): the three plane stores of a wave are each 256 B contiguous.
// (h, w) = letterboxed extent, placed at (ph / 2, pw / 2).  `v / 255.0f` is the correctly rounded fp32 quotient, which equals
// np.float32(v / 255) (float64 quotient, then stored as float32) for all 256 values (tests/test_animeseg_host.py checks them all).
__global__ __launch_bounds__(256) void k_animeseg_prepare(const uint8_t *__restrict__ img, int H, int W, int h, int w, int s,
                                                           int bgr_to_rgb, float *__restrict__ out) {
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= s) return;
    const int64_t plane = (int64_t)s * s;
    float *O = out + (int64_t)y * s + x;
    const int oy = y - (s - h) / 2, ox = x - (s - w) / 2;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (oy >= 0 && oy < h && ox >= 0 && ox < w) {
        int q[3];
        if (h == H && w == W) {                                      // cv2.resize to the same size is a copy
            for (int c = 0; c < 3; ++c) q[c] = img[((int64_t)oy * W + ox) * 3 + c];
        } else {
            int y0, y1, x0, x1; float fy, fx;
            cv_src(oy, H, (double)H / h, y0, y1, fy); cv_src(ox, W, (double)W / w, x0, x1, fx);
            for (int c = 0; c < 3; ++c)
                q[c] = cv_lin_u8(img[((int64_t)y0 * W + x0) * 3 + c], img[((int64_t)y0 * W + x1) * 3 + c],
                                 img[((int64_t)y1 * W + x0) * 3 + c], img[((int64_t)y1 * W + x1) * 3 + c], fx, fy);
        }
        for (int c = 0; c < 3; ++c) v[bgr_to_rgb ? 2 - c : c] = (float)q[c] / 255.0f;
    }
    for (int c = 0; c < 3; ++c) O[c * plane] = v[c];
}

// prob / fg at frame pixel (y, x): cv2 float INTER_LINEAR from the (h, w) crop of the sigmoid plane to (H0, W0).  The sigmoid is
// taken per tap, before the blend, as the reference takes it on the whole plane before cv2.resize.
__global__ __launch_bounds__(256) void k_animeseg_mask(const float *__restrict__ logits, int s, int h, int w, int H0, int W0,
                                                        float thr, float *__restrict__ prob, uint8_t *__restrict__ fg) {
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W0) return;
    const float *L = logits + (int64_t)((s - h) / 2) * s + (s - w) / 2;
    int y0, y1, x0, x1; float fy, fx;
    cv_src(y, h, (double)h / H0, y0, y1, fy); cv_src(x, w, (double)w / W0, x0, x1, fx);
    const float p = cv_lin_f32(csm_sigmoid(L[(int64_t)y0 * s + x0]), csm_sigmoid(L[(int64_t)y0 * s + x1]),
                               csm_sigmoid(L[(int64_t)y1 * s + x0]), csm_sigmoid(L[(int64_t)y1 * s + x1]), fx, fy);
    const int64_t o = (int64_t)y * W0 + x;
    if (prob) prob[o] = p;
    if (fg) fg[o] = p > thr ? 1 : 0;
}

constexpr int kSelRows = 16;   // mask rows per block of the count pass (bounds the atomics to k * ceil(Hm / 16) * ceil(Wm / 256))

// counts[2 * inst] = sum(mask), counts[2 * inst + 1] = sum(mask & fg[:Hm, :Wm]).  Integer sums: the atomic order cannot change them.
__global__ __launch_bounds__(256) void k_animeseg_count(const uint8_t *__restrict__ masks, int Hm, int Wm,
                                                         const uint8_t *__restrict__ fg, int W0, unsigned *__restrict__ counts) {
    const int inst = blockIdx.z, x = blockIdx.x * 256 + threadIdx.x;
    unsigned ao = 0u, ar = 0u;
    if (x < Wm) {
        const uint8_t *M = masks + (int64_t)inst * Hm * Wm;
        const int yend = min(Hm, (int)(blockIdx.y + 1) * kSelRows);
        for (int y = blockIdx.y * kSelRows; y < yend; ++y) {
            const unsigned m = M[(int64_t)y * Wm + x] ? 1u : 0u;
            ao += m;
            ar += m & (fg[(int64_t)y * W0 + x] ? 1u : 0u);
        }
    }
    for (int off = 32; off > 0; off >>= 1) { ao += __shfl_down(ao, off, 64); ar += __shfl_down(ar, off, 64); }
    __shared__ unsigned part[2][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[0][wave] = ao; part[1][wave] = ar; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned sao = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const unsigned sar = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (sao) atomicAdd(&counts[2 * inst], sao);
        if (sar) atomicAdd(&counts[2 * inst + 1], sar);
    }
}

// reference :103-105: `if area_refined / area_original > 0.3: ins_masks[ii] = masks_refined[ii]`, with int64 numpy sums divided
// in float64.  Decided here as 10 * ar > 3 * ao in 64-bit integers, which is the same predicate for 0 <= ar <= ao < 2^32:
//   * ao == 0: 0/0 is nan and nan > 0.3 is false; 0 > 0 is false.
//   * ar/ao == 3/10 exactly: the quotient rounds to double(0.3), which is not greater than itself; 10ar > 3ao is false.
//   * otherwise |ar/ao - 3/10| = |10ar - 3ao| / (10ao) >= 1 / (10ao) > 2.3e-11, while double(0.3) lies within 2^-55 (< 2.8e-17)
//     below 3/10 and one ulp near 0.3 is 2^-54.  So the true quotient is on the same side of double(0.3) as of 3/10 by many
//     ulps, and rounding (monotone) keeps it there: fl(ar/ao) > double(0.3) exactly when ar/ao > 3/10.
__global__ __launch_bounds__(256) void k_animeseg_apply(uint8_t *__restrict__ masks, int Hm, int Wm, const uint8_t *__restrict__ fg,
                                                         int W0, const unsigned *__restrict__ counts) {
    const int inst = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    const int64_t ao = counts[2 * inst], ar = counts[2 * inst + 1];
    if (x >= Wm || !(10 * ar > 3 * ao)) return;                      // kept: the mask stays as it is
    uint8_t *m = masks + ((int64_t)inst * Hm + y) * Wm + x;
    *m = (*m && fg[(int64_t)y * W0 + x]) ? 1 : 0;
}

}  // namespace

extern "C" int csm_animeseg_prepare(const uint8_t *img_hwc, int H, int W, int h, int w, int s, int bgr_to_rgb, float *out_nchw,
                                    void *stream) {
    CSM_REQUIRE(img_hwc && out_nchw && H > 0 && W > 0 && s > 0 && h > 0 && w > 0 && h <= s && w <= s);
    k_animeseg_prepare<<<dim3(csm::cdiv(s, 256), s), 256, 0, (hipStream_t)stream>>>(img_hwc, H, W, h, w, s, bgr_to_rgb ? 1 : 0,
                                                                                      out_nchw);
    return csm::check_launch("k_animeseg_prepare");
}

extern "C" int csm_animeseg_mask(const float *logits, int s, int h, int w, int H0, int W0, float thr, float *prob_out,
                                 uint8_t *fg_out, void *stream) {
    CSM_REQUIRE(logits && s > 0 && h > 0 && w > 0 && h <= s && w <= s && H0 > 0 && W0 > 0);
    if (!prob_out && !fg_out) return CSM_OK;
    k_animeseg_mask<<<dim3(csm::cdiv(W0, 256), H0), 256, 0, (hipStream_t)stream>>>(logits, s, h, w, H0, W0, thr, prob_out, fg_out);
    return csm::check_launch("k_animeseg_mask");
}

extern "C" int csm_animeseg_select(uint8_t *masks_u8, int k, int Hm, int Wm, const uint8_t *fg, int W0, unsigned *counts_scratch,
                                   void *stream) {
    CSM_REQUIRE(k >= 0 && Hm > 0 && Wm > 0 && Wm <= W0 && (int64_t)Hm * Wm < ((int64_t)1 << 32));
    if (k == 0) return CSM_OK;
    CSM_REQUIRE(masks_u8 && fg && counts_scratch);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(counts_scratch, 0, (size_t)2 * k * sizeof(unsigned), st));
    k_animeseg_count<<<dim3(csm::cdiv(Wm, 256), csm::cdiv(Hm, kSelRows), k), 256, 0, st>>>(masks_u8, Hm, Wm, fg, W0, counts_scratch);
    int rc = csm::check_launch("k_animeseg_count"); if (rc) return rc;
    k_animeseg_apply<<<dim3(csm::cdiv(Wm, 256), Hm, k), 256, 0, st>>>(masks_u8, Hm, Wm, fg, W0, counts_scratch);
    return csm::check_launch("k_animeseg_apply");
}
