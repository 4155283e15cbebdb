// cutout.hip -- instance cut-outs with transparency, composed on the device, for gfx950.
//
//   csm_mask_bbox     the tight box of every mask: k_bbox_init -> k_bbox (one workgroup per mask and band of 32 rows, integer
//                     min / max atomics) -> k_bbox_finish (an empty mask gives 0, 0, 0, 0)
//   csm_cutout_bgra   every instance's [h, w, 4] B, G, R, A image into one packed buffer, one launch over the pixels of all
//                     instances; the host sizes the buffer from the box table and hands over one job per instance
//
// Alpha is 255 where the mask is set, or (uint8)(clamp(p, 0, 1) * 255) of a float plane (an exact fp32 product, truncated) where
// the mask is set, and 0 elsewhere; colour is zero wherever alpha is zero.  Integer atomics only; the output is deterministic.
#include "csm_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBand = 32;                // rows of a mask per workgroup of k_bbox
constexpr int kJobWords = 8;             // int64 per instance: mask index, x0, y0, x1, y1, byte offset in out, first pixel, 0
enum { jMask = 0, jX0 = 1, jY0 = 2, jX1 = 3, jY1 = 4, jOff = 5, jFirst = 6 };

__global__ __launch_bounds__(kBlock) void k_bbox_init(int32_t *__restrict__ boxes, int n, int H, int W) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { boxes[4 * i] = W; boxes[4 * i + 1] = H; boxes[4 * i + 2] = 0; boxes[4 * i + 3] = 0; }
}

__global__ __launch_bounds__(kBlock) void k_bbox(const uint8_t *__restrict__ masks, int H, int W, int bands, int32_t *__restrict__ boxes) {
    __shared__ int sBox[4];
    const int t = threadIdx.x;
    const int f = blockIdx.x / bands, band = blockIdx.x - f * bands;
    const int y0 = band * kBand, y1 = min(H, y0 + kBand);
    const uint8_t *M = masks + (int64_t)f * H * W;
    if (t == 0) { sBox[0] = W; sBox[1] = H; sBox[2] = 0; sBox[3] = 0; }
    __syncthreads();
    int bx0 = W, by0 = H, bx1 = 0, by1 = 0;
    const int count = (y1 - y0) * W;
    for (int i = t; i < count; i += kBlock) {
        const int y = y0 + i / W, x = i - (i / W) * W;
        if (M[(int64_t)y * W + x]) { bx0 = min(bx0, x); by0 = min(by0, y); bx1 = max(bx1, x + 1); by1 = max(by1, y + 1); }
    }
    if (bx1) { atomicMin(sBox, bx0); atomicMin(sBox + 1, by0); atomicMax(sBox + 2, bx1); atomicMax(sBox + 3, by1); }
    __syncthreads();
    if (t == 0 && sBox[2]) {
        int32_t *B = boxes + 4 * (int64_t)f;
        atomicMin(B, sBox[0]); atomicMin(B + 1, sBox[1]); atomicMax(B + 2, sBox[2]); atomicMax(B + 3, sBox[3]);
    }
}

__global__ __launch_bounds__(kBlock) void k_bbox_finish(int32_t *__restrict__ boxes, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && boxes[4 * i + 2] == 0) { boxes[4 * i] = 0; boxes[4 * i + 1] = 0; }
}

// one thread per output pixel of all instances
__global__ __launch_bounds__(kBlock) void k_cutout(const uint8_t *__restrict__ img, int H, int W, const uint8_t *__restrict__ masks,
                                                    int Hm, int Wm, const float *__restrict__ alpha, const int64_t *__restrict__ jobs,
                                                    int k, int64_t pixels, uint8_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= pixels) return;
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[(int64_t)mid * kJobWords + jFirst] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t *J = jobs + (int64_t)lo * kJobWords;
    const int w = (int)(J[jX1] - J[jX0]);
    const int64_t q = p - J[jFirst];
    const int y = (int)J[jY0] + (int)(q / w), x = (int)J[jX0] + (int)(q - (q / w) * w);
    int a = 0;
    if (y < Hm && x < Wm && masks[(J[jMask] * Hm + y) * Wm + x]) {
        a = 255;
        if (alpha) a = (int)(fminf(fmaxf(alpha[(int64_t)y * W + x], 0.0f), 1.0f) * 255.0f);
    }
    uchar4 v = make_uchar4(0, 0, 0, 0);
    if (a) {
        const uint8_t *s = img + ((int64_t)y * W + x) * 3;
        v = make_uchar4(s[0], s[1], s[2], (uint8_t)a);
    }
    *(uchar4 *)(out + J[jOff] + q * 4) = v;
}

}  // namespace

extern "C" int csm_mask_bbox(const uint8_t *masks, int n, int H, int W, int32_t *boxes, void *stream) {
    CSM_REQUIRE(n >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < INT32_MAX);
    if (n == 0) return CSM_OK;
    const int bands = (H + kBand - 1) / kBand;
    CSM_REQUIRE(masks && boxes && (int64_t)n * bands < INT32_MAX);
    hipStream_t st = (hipStream_t)stream;
    k_bbox_init<<<csm::cdiv(n, kBlock), kBlock, 0, st>>>(boxes, n, H, W);
    int rc = csm::check_launch("k_bbox_init"); if (rc) return rc;
    k_bbox<<<(unsigned)(n * bands), kBlock, 0, st>>>(masks, H, W, bands, boxes);
    rc = csm::check_launch("k_bbox"); if (rc) return rc;
    k_bbox_finish<<<csm::cdiv(n, kBlock), kBlock, 0, st>>>(boxes, n);
    return csm::check_launch("k_bbox_finish");
}

extern "C" int csm_cutout_job_words(void) { return kJobWords; }

extern "C" int csm_cutout_bgra(const uint8_t *img, int H, int W, const uint8_t *masks, int n_masks, int Hm, int Wm, const float *alpha,
                               const int64_t *jobs_host, const int64_t *jobs_dev, int k, uint8_t *out, int64_t out_bytes, void *stream) {
    CSM_REQUIRE(k >= 0 && H >= 1 && W >= 1 && n_masks >= 0);
    CSM_REQUIRE(Hm >= 1 && Wm >= 1 && Hm <= H && Wm <= W && H - Hm <= 2 && W - Wm <= 2);
    if (k == 0) return CSM_OK;
    CSM_REQUIRE(img && masks && jobs_host && jobs_dev && out && ((uintptr_t)out & 3) == 0);
    int64_t pixels = 0;
    for (int i = 0; i < k; ++i) {                            // every job stays inside the frame, the masks and the buffer
        const int64_t *J = jobs_host + (int64_t)i * kJobWords;
        CSM_REQUIRE(J[jMask] >= 0 && J[jMask] < n_masks);
        CSM_REQUIRE(0 <= J[jX0] && J[jX0] < J[jX1] && J[jX1] <= W && 0 <= J[jY0] && J[jY0] < J[jY1] && J[jY1] <= H);
        const int64_t count = (J[jX1] - J[jX0]) * (J[jY1] - J[jY0]);
        CSM_REQUIRE(J[jFirst] == pixels && J[jOff] >= 0 && J[jOff] % 4 == 0 && J[jOff] + count * 4 <= out_bytes);
        pixels += count;
    }
    CSM_REQUIRE((pixels + kBlock - 1) / kBlock < INT32_MAX);
    k_cutout<<<csm::cdiv(pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(img, H, W, masks, Hm, Wm, alpha, jobs_dev, k, pixels, out);
    return csm::check_launch("k_cutout");
}
