// frameglue.hip -- the per-frame depth glue of a step for B equally sized frames in ONE asynchronous call each:
//   * csm_frame_glue_batch : image tensor, depth adjustment per instance, raw min/max, normalise + disparity -> points, crop
//                            minMaxLoc, six stats per frame (kenburns_effect.py:68-78, :878-880, :928-935)
//   * csm_leres_post_batch : LeReS output min/max, uint8 quantisation, resize back, zero fix
//                            (depth_modules/leres/__init__.py:121-145, kenburns_effect.py:572-578)
// The frame index is a grid dimension; per-frame pointers travel by value in the kernel arguments (at most kChunk frames per
// launch, larger B goes in chunks).  No allocation, no synchronisation, no block waits for another block: reductions are two
// launches (partial, final) or 64-bit / 32-bit atomic min on keys.  Every expression comes from csm_glue.h, the header the
// single-frame entry points (imageops.hip, warp.hip) compile too: same expressions, same bits.
#include "csm_common.h"
#include "csm_glue.h"

namespace {

constexpr int kChunk = 16;

struct GlueFrames {                       // kernel argument, by value
    const uint8_t *img[kChunk];           // uint8 HWC frame
    const float *coarse[kChunk];          // coarse disparity [H,W]
    const uint8_t *masks[kChunk];         // instance masks [n,H,W] (null when n == 0)
    int n_inst[kChunk];
};

// scratch of csm_frame_glue_batch, carved by glue_scratch(): all of it per frame
struct GlueScratch {
    unsigned long long *keys;             // [B][2]: crop min key, ~(crop max key) -- both folded with atomicMin, cleared by ONE memset 0xff
    float *adj;                           // [B][P4]: private copy of the coarse disparity (frames with instances)
    float *rows;                          // [B][2H + 2]: row maxima, row flags, {val, apply}
    float *part;                          // [B][512]: min/max partials
    float *mm;                            // [B][2]: raw {min, max}
    int64_t P4;
    size_t bytes;
};
inline int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }
GlueScratch glue_scratch(void *base, int B, int H, int W) {
    GlueScratch s;
    char *p = (char *)base;
    s.P4 = round4((int64_t)H * W);
    s.keys = (unsigned long long *)p; p += (size_t)B * 16;
    s.adj = (float *)p; p += (size_t)B * s.P4 * 4;
    s.part = (float *)p; p += (size_t)B * 512 * 4;
    s.mm = (float *)p; p += (size_t)B * 2 * 4;
    s.rows = (float *)p; p += (size_t)B * (2 * H + 2) * 4;
    s.bytes = (size_t)(p - (char *)base);
    return s;
}

// the raw (adjusted) disparity of frame f: its private copy when it has instances, else the caller's coarse map itself
__device__ __forceinline__ const float *raw_of(const GlueFrames &F, int f, const float *adj, int64_t P4) {
    return F.n_inst[f] > 0 ? adj + (int64_t)f * P4 : F.coarse[f];
}

__global__ __launch_bounds__(256) void k_glue_image(GlueFrames F, int64_t plane, float *__restrict__ out, int64_t stride3) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    csmglue::u8_hwc_to_f32_chw_px(F.img[f], plane, i, out + (int64_t)f * stride3);
}

// pass j of the depth adjustment: instance j of every frame that has one.  Pass 0 reads the coarse map and writes the private
// copy (the copy folded into the pass); later passes work on the copy in place.
__global__ __launch_bounds__(256) void k_glue_adjust_rows(GlueFrames F, int j, int H, int W, const float *__restrict__ adj, int64_t P4,
                                                           float *__restrict__ rows) {
    const int f = blockIdx.y;
    if (F.n_inst[f] <= j) return;
    const float *src = j == 0 ? F.coarse[f] : adj + (int64_t)f * P4;
    float *r = rows + (int64_t)f * (2 * H + 2);
    csmglue::adjust_rows_block(src, F.masks[f] + (int64_t)j * H * W, W, blockIdx.x, r, r + H);
}
__global__ __launch_bounds__(256) void k_glue_adjust_pick(GlueFrames F, int j, int H, float *__restrict__ rows) {
    const int f = blockIdx.x;
    if (F.n_inst[f] <= j) return;
    float *r = rows + (int64_t)f * (2 * H + 2);
    csmglue::adjust_pick_block(r, r + H, H, r + 2 * H);
}
__global__ __launch_bounds__(256) void k_glue_adjust_apply(GlueFrames F, int j, int H, int W, float *__restrict__ adj, int64_t P4,
                                                            const float *__restrict__ rows) {
    const int f = blockIdx.y;
    if (F.n_inst[f] <= j) return;
    const int64_t n = (int64_t)H * W, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *out2 = rows + (int64_t)f * (2 * H + 2) + 2 * H;
    const bool apply = out2[1] != 0.0f;
    float *dst = adj + (int64_t)f * P4;
    if (j == 0) {
        const float d = F.coarse[f][i];
        dst[i] = apply ? csmglue::adjust_apply_px(d, F.masks[f][i], out2[0]) : d;
    } else if (apply) {
        dst[i] = csmglue::adjust_apply_px(dst[i], F.masks[f][(int64_t)j * n + i], out2[0]);
    }
}

__global__ __launch_bounds__(256) void k_glue_minmax_partial(GlueFrames F, int64_t n, const float *__restrict__ adj, int64_t P4,
                                                              float *__restrict__ part) {
    const int f = blockIdx.y;
    csmglue::minmax_partial_block(raw_of(F, f, adj, P4), n, blockIdx.x, gridDim.x, part + (int64_t)f * 512);
}
__global__ __launch_bounds__(256) void k_glue_minmax_final(const float *__restrict__ part, int nparts, float *__restrict__ mm) {
    const int f = blockIdx.x;
    csmglue::minmax_final_block(part + (int64_t)f * 512, nparts, mm + 2 * f);
}

// normalise + disparity -> depth / valid / points / unaltered in one pass over the raw map: the normalised value of a pixel and
// of its Laplacian neighbours is the single expression normalise_px(raw, max, scale), so the normalised map is written but never
// read back
__global__ __launch_bounds__(256) void k_glue_points(GlueFrames F, int H, int W, const float *__restrict__ adj, int64_t P4,
                                                      const float *__restrict__ mm, float scale, float fb, float eps, float invf,
                                                      float x_start, float y_start, float *__restrict__ disp, float *__restrict__ depth,
                                                      float *__restrict__ valid, float *__restrict__ pts, float *__restrict__ unaltered,
                                                      int64_t stride1, int64_t stride3, float *__restrict__ nmax) {
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float *raw = raw_of(F, f, adj, P4);
    const float mx = mm[2 * f + 1];
    const float dmax = csmglue::normalise_px(mx, mx, scale);       // = max of the normalised map (the map is monotonic)
    const int64_t o = (int64_t)y * W + x;
    auto at = [raw, mx, scale](int64_t i) { return csmglue::normalise_px(raw[i], mx, scale); };
    const float dn = at(o);
    disp[(int64_t)f * stride1 + o] = dn;
    if (o == 0) nmax[f] = dmax;
    csmglue::disparity_to_points_px(at, dn, dmax, x, y, H, W, fb, eps, invf, x_start, y_start, depth + (int64_t)f * stride1,
                                    valid + (int64_t)f * stride1, pts + (int64_t)f * stride3, unaltered + (int64_t)f * stride3);
}

// minMaxLoc keys of the depth crop: 256 grid-stride blocks per frame, two atomics per block (DESIGN.md 4.1c records why the keys
// are not folded into the points kernel)
__global__ __launch_bounds__(256) void k_glue_crop(const float *__restrict__ depth, int64_t stride1, int W, int cy0, int cx0, int ch, int cw,
                                                    unsigned long long *__restrict__ keys) {
    const int f = blockIdx.y;
    const float *d = depth + (int64_t)f * stride1;
    unsigned long long mn = ~0ull, mx = 0ull;
    const int64_t n = (int64_t)ch * cw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int y = (int)(i / cw), x = (int)(i - (int64_t)y * cw);
        csmglue::crop_keys_acc(d[(int64_t)(cy0 + y) * W + cx0 + x], (unsigned)i, mn, mx);
    }
    csmglue::crop_keys_fold_block(mn, mx);
    if (threadIdx.x == 0) { atomicMin(&keys[2 * f], mn); atomicMin(&keys[2 * f + 1], ~mx); }
}

__global__ void k_glue_stats(const float *__restrict__ mm, float scale, const unsigned long long *__restrict__ keys, int nf,
                             double *__restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    csmglue::stats_pack(mm + 2 * f, scale, keys[2 * f], ~keys[2 * f + 1], out + 6 * f);
}

// ---- LeReS post-processing ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lpost_minmax_partial(const float *__restrict__ y, int64_t n, float *__restrict__ part) {
    const int f = blockIdx.y;
    csmglue::minmax_partial_block(y + (int64_t)f * n, n, blockIdx.x, gridDim.x, part + (int64_t)f * 512);
}
__global__ __launch_bounds__(256) void k_lpost_minmax_final(const float *__restrict__ part, int nparts, float *__restrict__ mm) {
    const int f = blockIdx.x;
    csmglue::minmax_final_block(part + (int64_t)f * 512, nparts, mm + 2 * f);
}
__global__ __launch_bounds__(256) void k_lpost_quantize(const float *__restrict__ y, int64_t n, const float *__restrict__ mm,
                                                         uint8_t *__restrict__ q) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    q[(int64_t)f * n + i] = csmglue::leres_quantize_px(y[(int64_t)f * n + i], mm[2 * f], mm[2 * f + 1]);
}
// resize back + the scan of the zero fix (smallest positive value, zero seen) over the values just written.
// st[2f] = smallest positive value as bits (atomicMin), st[2f + 1] = 0 once a zero was seen (atomicAnd); both start as 0xffffffff
template <bool LANCZOS>
__global__ __launch_bounds__(256) void k_lpost_resize(const uint8_t *__restrict__ q, int h, int w, int H, int W, float *__restrict__ out,
                                                       int64_t out_stride, unsigned *__restrict__ st) {
    const int f = blockIdx.z;
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    unsigned mn = 0xffffffffu; int z = 0;
    if (x < W) {
        const uint8_t *src = q + (int64_t)f * h * w;
        const float v = LANCZOS ? csmglue::resize_u8_lanczos4_px(src, h, w, H, W, y, x) : csmglue::resize_u8_to_f32_px(src, h, w, H, W, y, x);
        out[(int64_t)f * out_stride + (int64_t)y * W + x] = v;
        csmglue::minpos_acc(v, mn, z);
    }
    csmglue::minpos_fold_block(mn, z);
    if (threadIdx.x == 0) {
        if (mn != 0xffffffffu) atomicMin(&st[2 * f], mn);
        if (z) atomicAnd(&st[2 * f + 1], 0u);
    }
}
__global__ __launch_bounds__(256) void k_lpost_fill(float *__restrict__ out, int64_t n, int64_t out_stride, const unsigned *__restrict__ st) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    csmglue::minpos_apply_px(out + (int64_t)f * out_stride, i, st[2 * f], st[2 * f + 1] == 0u);
}

struct LpostScratch { unsigned *st; float *mm, *part; uint8_t *q; size_t bytes; };
LpostScratch lpost_scratch(void *base, int B, int h, int w) {
    LpostScratch s;
    char *p = (char *)base;
    s.st = (unsigned *)p; p += (size_t)B * 8;
    s.mm = (float *)p; p += (size_t)B * 8;
    s.part = (float *)p; p += (size_t)B * 512 * 4;
    s.q = (uint8_t *)p; p += (size_t)B * h * w;
    s.bytes = (size_t)(p - (char *)base);
    return s;
}

}  // namespace

extern "C" size_t csm_frame_glue_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return glue_scratch(nullptr, B, H, W).bytes;
}

extern "C" int csm_frame_glue_batch(int B, int H, int W, const uint8_t *const *frames_hwc, const float *const *coarse,
                                    const uint8_t *const *masks, const int *n_inst, double focal, double baseline, float eps,
                                    float *img_out, float *disp_out, float *depth_out, float *valid_out, float *pts_out,
                                    float *unaltered_out, int64_t stride1, int64_t stride3, float *nmax_out, double *stats_out,
                                    void *scratch, void *stream) {
    CSM_REQUIRE(B > 0 && H > 256 && W > 256 && frames_hwc && coarse && masks && n_inst && focal != 0.0);
    CSM_REQUIRE(img_out && disp_out && depth_out && valid_out && pts_out && unaltered_out && nmax_out && stats_out && scratch);
    CSM_REQUIRE(stride1 >= (int64_t)H * W && stride3 >= 3 * (int64_t)H * W && (int64_t)(H - 256) * (W - 256) < (1ll << 32));
    CSM_REQUIRE(!(((uintptr_t)scratch) & 15));
    for (int k = 0; k < B; ++k)
        CSM_REQUIRE(frames_hwc[k] && coarse[k] && n_inst[k] >= 0 && (n_inst[k] == 0 || masks[k]));
    hipStream_t st = (hipStream_t)stream;
    const GlueScratch S = glue_scratch(scratch, B, H, W);
    const int64_t n = (int64_t)H * W;
    const float scale = (float)baseline, fb = (float)(focal * baseline), invf = (float)(1.0 / focal);
    const float x_start = (float)(-0.5 * W + 0.5), y_start = (float)(-0.5 * H + 0.5);
    const int nparts = csmglue::minmax_nparts(n);
    CSM_HIP(hipMemsetAsync(S.keys, 0xff, (size_t)B * 16, st));              // every frame's two keys in one memset
    for (int f0 = 0; f0 < B; f0 += kChunk) {
        const int nf = B - f0 < kChunk ? B - f0 : kChunk;
        GlueFrames F{};
        int jmax = 0;
        for (int k = 0; k < nf; ++k) {
            F.img[k] = frames_hwc[f0 + k]; F.coarse[k] = coarse[f0 + k]; F.masks[k] = masks[f0 + k]; F.n_inst[k] = n_inst[f0 + k];
            jmax = n_inst[f0 + k] > jmax ? n_inst[f0 + k] : jmax;
        }
        float *adj = S.adj + (int64_t)f0 * S.P4, *rows = S.rows + (int64_t)f0 * (2 * H + 2);
        float *part = S.part + (int64_t)f0 * 512, *mm = S.mm + 2 * f0;
        k_glue_image<<<dim3(csm::cdiv(n, 256), nf), 256, 0, st>>>(F, n, img_out + (int64_t)f0 * stride3, stride3);
        for (int j = 0; j < jmax; ++j) {                                     // instance order: pass j sees pass j - 1's result
            k_glue_adjust_rows<<<dim3(H, nf), 256, 0, st>>>(F, j, H, W, adj, S.P4, rows);
            k_glue_adjust_pick<<<nf, 256, 0, st>>>(F, j, H, rows);
            k_glue_adjust_apply<<<dim3(csm::cdiv(n, 256), nf), 256, 0, st>>>(F, j, H, W, adj, S.P4, rows);
        }
        k_glue_minmax_partial<<<dim3(nparts, nf), 256, 0, st>>>(F, n, adj, S.P4, part);
        k_glue_minmax_final<<<nf, 256, 0, st>>>(part, nparts, mm);
        k_glue_points<<<dim3(csm::cdiv(W, 64), csm::cdiv(H, 4), nf), 256, 0, st>>>(
            F, H, W, adj, S.P4, mm, scale, fb, eps, invf, x_start, y_start, disp_out + (int64_t)f0 * stride1,
            depth_out + (int64_t)f0 * stride1, valid_out + (int64_t)f0 * stride1, pts_out + (int64_t)f0 * stride3,
            unaltered_out + (int64_t)f0 * stride3, stride1, stride3, nmax_out + f0);
        k_glue_crop<<<dim3(256, nf), 256, 0, st>>>(depth_out + (int64_t)f0 * stride1, stride1, W, 128, 128, H - 256, W - 256, S.keys + 2 * f0);
        k_glue_stats<<<1, 64, 0, st>>>(mm, scale, S.keys + 2 * f0, nf, stats_out + 6 * f0);
    }
    return csm::check_launch("k_glue_*");
}

extern "C" size_t csm_leres_post_scratch_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return lpost_scratch(nullptr, B, h, w).bytes;
}

extern "C" int csm_leres_post_batch(const float *y, int B, int h, int w, int H, int W, float *depth_out, int64_t out_stride,
                                    void *scratch, void *stream) {
    CSM_REQUIRE(y && depth_out && scratch && B > 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 && out_stride >= (int64_t)H * W);
    CSM_REQUIRE(!(((uintptr_t)scratch) & 7));
    const bool lanczos = (double)h / H > 1.0;                    // kenburns_effect.py:571-573: k = depth.shape[0] / ori_h
    CSM_REQUIRE(lanczos || (H >= h && W >= w));                  // the area route enlarges only (csm_resize_u8_to_f32)
    hipStream_t st = (hipStream_t)stream;
    const LpostScratch S = lpost_scratch(scratch, B, h, w);
    const int64_t n = (int64_t)h * w, N = (int64_t)H * W;
    const int nparts = csmglue::minmax_nparts(n);
    CSM_HIP(hipMemsetAsync(S.st, 0xff, (size_t)B * 8, st));
    k_lpost_minmax_partial<<<dim3(nparts, B), 256, 0, st>>>(y, n, S.part);
    k_lpost_minmax_final<<<B, 256, 0, st>>>(S.part, nparts, S.mm);
    k_lpost_quantize<<<dim3(csm::cdiv(n, 256), B), 256, 0, st>>>(y, n, S.mm, S.q);
    if (lanczos) k_lpost_resize<true><<<dim3(csm::cdiv(W, 256), H, B), 256, 0, st>>>(S.q, h, w, H, W, depth_out, out_stride, S.st);
    else k_lpost_resize<false><<<dim3(csm::cdiv(W, 256), H, B), 256, 0, st>>>(S.q, h, w, H, W, depth_out, out_stride, S.st);
    k_lpost_fill<<<dim3(csm::cdiv(N, 256), B), 256, 0, st>>>(depth_out, N, out_stride, S.st);
    return csm::check_launch("k_lpost_*");
}
