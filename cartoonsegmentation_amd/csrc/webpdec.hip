// webpdec.hip -- lossless WebP files (VP8L payloads) to uint8 B, G, R (, A) on the device, for gfx950.  The contract is fixed to the
// byte (the result equals what libwebp decodes) and restated in numpy in tests/webpdec_restatement.py; the host side
// (container parser) is cartoonsegmentation_amd/webpread.py; the bit reader, the code builder and the symbol walker are
// csm_vp8l.h, which also compiles for the host.
//
// The entropy stream is serial per file, and the colour cache makes even the copies order-dependent; everything behind it is not.
//
//   k_wd_walk      one wave per file, one lane of it at work: the 5-byte header, the transforms' sub-images, the entropy image, the
//                  prefix-code groups (tables in the file's scratch), the pixels in front of the inverse transforms.  The colour
//                  cache and the code-length work area are in LDS
//   k_wd_pixel     step k = 0..3: the k-th inverse transform of each file, if it is subtract-green, cross-colour or colour indexing
//                  (per pixel, from one ARGB buffer into the other)
//   k_wd_predict   step k: the same if it is the predictor transform.  One workgroup per file: lane r owns row r of a band of
//                  kBandRows rows and takes pixel x = step - 2 r (the stagger of two is for the top-right pixel); the row above
//                  comes through LDS, left and top-left stay in registers, one barrier per step
//   k_wd_store     ARGB to B, G, R or B, G, R, A bytes; A = 255 when the header says the file has no alpha
//
// No kernel waits on another workgroup and there is no spin loop on memory.  Every read and store is bounded by sizes from the
// descriptor, whatever the data: a corrupt stream raises bits of the file's error word and leaves the file's pixels undefined.
//
// The same kernels decode the alpha planes of lossy files (webplossy.hip through csm_webpdec.h): such a "file" is
// a stream without the 5-byte header, and its store writes the green channel as one byte per pixel.
#include "csm_common.h"
#include "csm_vp8l.h"
#include "csm_webpdec.h"
#include <algorithm>
#include <vector>

namespace {

namespace vp = csm_vp8l;

constexpr int kDescWords = 12;
constexpr int kLanes = 256;
constexpr int kBandRows = 256;               // rows of one band of k_wd_predict (tests/webpdec_cases.py has a taller image)
constexpr int kMaxSide = 16384;

struct WFile {
    // from the caller's descriptor
    int H, W, alpha, channels;
    int plane;                               // the lossy decoder's alpha plane: a stream without the 5-byte header, stored as its green bytes
    int in_off, in_len;
    int64_t out_off;
    // derived
    uint32_t sub_cap, group_cap;
    int64_t res_off, argb_off[2], pred_off, colour_off, meta_off, pal_off, group_off;       // byte offsets in scratch
};

struct Plan {
    std::vector<WFile> files;
    int64_t max_pixels = 0;
    int64_t o_files, o_res, total;
};

// false: the descriptors are invalid (the error is set)
bool make_plan(const int32_t *desc, int n, int64_t blob_bytes, int64_t out_bytes, bool check_ranges, bool planes, Plan &p) {
    if (!desc || n < 1 || n > 65535) { csm::set_error("invalid argument: 1 <= n <= 65535 descriptors"); return false; }
    p.files.resize(n);
    int64_t o = 0;
    p.o_files = o;  o += csm::align16((int64_t)n * sizeof(WFile));
    p.o_res = o;    o += csm::align16((int64_t)n * sizeof(vp::Result));
    for (int i = 0; i < n; ++i) {
        const int32_t *d = desc + (int64_t)i * kDescWords;
        WFile &f = p.files[i];
        f.H = d[0]; f.W = d[1]; f.alpha = d[2]; f.channels = d[3]; f.in_off = d[4]; f.in_len = d[5]; f.plane = d[6];
        f.out_off = (int64_t)d[7] | ((int64_t)d[8] << 31);
        bool ok = f.H >= 1 && f.W >= 1 && f.H <= kMaxSide && f.W <= kMaxSide && (f.alpha == 0 || f.alpha == 1);
        ok = ok && (planes ? f.plane == 1 && f.channels == 1 : f.plane == 0 && (f.channels == 3 || f.channels == 4));
        ok = ok && f.in_off >= 0 && (f.in_off & 15) == 0 && f.in_len >= (planes ? 1 : 5) && d[7] >= 0 && d[8] >= 0 && (f.out_off & 3) == 0;
        if (ok && check_ranges)
            ok = (int64_t)f.in_off + f.in_len <= blob_bytes && f.out_off + (int64_t)f.H * f.W * f.channels <= out_bytes;
        if (!ok) { csm::set_error("invalid argument: descriptor %d of the WebP decode", i); return false; }
        const int64_t pixels = (int64_t)f.H * f.W;
        f.sub_cap = vp::subsample((uint32_t)f.W, 2) * vp::subsample((uint32_t)f.H, 2);
        f.group_cap = std::min(vp::kGroupCap, f.sub_cap);
        f.res_off = p.o_res + (int64_t)i * sizeof(vp::Result);
        f.argb_off[0] = o;  o += csm::align16(pixels * 4);
        f.argb_off[1] = o;  o += csm::align16(pixels * 4);
        f.pred_off = o;     o += csm::align16((int64_t)f.sub_cap * 4);
        f.colour_off = o;   o += csm::align16((int64_t)f.sub_cap * 4);
        f.meta_off = o;     o += csm::align16((int64_t)f.sub_cap * 4);
        f.pal_off = o;      o += 1024;
        f.group_off = o;    o += csm::align16((int64_t)f.group_cap * sizeof(vp::Group));
        p.max_pixels = std::max(p.max_pixels, pixels);
    }
    p.total = o;
    return true;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_wd_walk(const uint8_t *__restrict__ blob, const WFile *__restrict__ files, char *__restrict__ scratch) {
    __shared__ vp::State S;
    __shared__ uint32_t cache[1 << vp::kMaxCacheBits];
    if (threadIdx.x != 0) return;
    const WFile f = files[blockIdx.x];
    vp::Bufs B;
    B.argb = (uint32_t *)(scratch + f.argb_off[0]);
    B.pred = (uint32_t *)(scratch + f.pred_off);
    B.colour = (uint32_t *)(scratch + f.colour_off);
    B.meta = (uint32_t *)(scratch + f.meta_off);
    B.palette = (uint32_t *)(scratch + f.pal_off);
    B.cache = cache;
    B.groups = (vp::Group *)(scratch + f.group_off);
    B.sub_cap = f.sub_cap;
    B.group_cap = f.group_cap;
    vp::Result &R = *(vp::Result *)(scratch + f.res_off);
    if (f.plane) vp::decode_headerless(S, B, blob + f.in_off, (uint32_t)f.in_len, (uint32_t)f.W, (uint32_t)f.H, R);
    else vp::decode_file(S, B, blob + f.in_off, (uint32_t)f.in_len, (uint32_t)f.W, (uint32_t)f.H, R);
}

// ---- the inverse transforms -----------------------------------------------------------------------------------------------------
// grid (groups of kLanes pixels of the largest file, files)
__global__ __launch_bounds__(kLanes) void k_wd_pixel(const WFile *__restrict__ files, char *__restrict__ scratch, int step) {
    const WFile f = files[blockIdx.y];
    const vp::Result &R = *(const vp::Result *)(scratch + f.res_off);
    const int t = R.ntrans - 1 - step;
    if (R.err || t < 0 || R.type[t] == vp::kPredictor) return;
    const uint32_t xs = (uint32_t)R.xs[t];                              // <= W: the walker wrote it
    const uint32_t p = (uint32_t)blockIdx.x * kLanes + threadIdx.x;
    if (p >= xs * (uint32_t)f.H) return;
    const uint32_t y = p / xs, x = p - y * xs;
    const uint32_t *src = (const uint32_t *)(scratch + f.argb_off[step & 1]);
    uint32_t *dst = (uint32_t *)(scratch + f.argb_off[(step + 1) & 1]);
    const int bits = R.bits[t];
    uint32_t v;
    if (R.type[t] == vp::kPalette) {
        v = vp::palette_pixel(src + (size_t)y * vp::subsample(xs, bits), (const uint32_t *)(scratch + f.pal_off), x, bits);
    } else if (R.type[t] == vp::kSubtractGreen) {
        v = vp::add_green(src[p]);
    } else {
        const uint32_t *colour = (const uint32_t *)(scratch + f.colour_off);
        v = vp::cross_colour(src[p], colour[(y >> bits) * vp::subsample(xs, bits) + (x >> bits)]);
    }
    dst[p] = v;
}

// one workgroup per file
__global__ __launch_bounds__(kBandRows) void k_wd_predict(const WFile *__restrict__ files, char *__restrict__ scratch, int step) {
    const WFile f = files[blockIdx.x];
    const vp::Result &R = *(const vp::Result *)(scratch + f.res_off);
    const int t = R.ntrans - 1 - step;
    if (R.err || t < 0 || R.type[t] != vp::kPredictor) return;          // the same for every lane
    __shared__ uint32_t above[2][kBandRows];
    const int xs = R.xs[t], bits = R.bits[t], H = f.H;
    const uint32_t *src = (const uint32_t *)(scratch + f.argb_off[step & 1]);
    uint32_t *dst = (uint32_t *)(scratch + f.argb_off[(step + 1) & 1]);
    const uint32_t *pred = (const uint32_t *)(scratch + f.pred_off);
    const int r = threadIdx.x;
    for (int band = 0; band < H; band += kBandRows) {
        const int rows = min(kBandRows, H - band), row = band + r;
        const bool mine = r < rows;
        uint32_t L = 0, T = 0, TL = 0, first = 0;
        if (mine && r == 0 && row > 0) T = dst[(size_t)(row - 1) * xs];     // lane 0 has no step at x = -1 in which to pick it up
        const int steps = xs + 2 * (rows - 1);
        for (int s = 0; s < steps; ++s) {
            const int x = s - 2 * r;
            if (mine && x >= -1 && x < xs) {
                // pixel x + 1 of the row above: lane r - 1 finished it one step ago
                uint32_t nxt = 0;
                if (x + 1 < xs && row > 0) nxt = r == 0 ? dst[(size_t)(row - 1) * xs + x + 1] : above[(s + 1) & 1][r - 1];
                if (x >= 0) {
                    const uint32_t TR = x + 1 < xs ? nxt : first;
                    const size_t at = (size_t)row * xs + x;
                    const uint32_t px = vp::add_bytes(src[at], vp::predict_at(pred, bits, (uint32_t)xs, (uint32_t)x, (uint32_t)row, L, T, TL, TR));
                    dst[at] = px;
                    above[s & 1][r] = px;
                    if (x == 0) first = px;
                    L = px;
                }
                TL = T; T = nxt;
            }
            __syncthreads();
        }
    }
}

// grid (groups of kLanes pixels of the largest file, files)
__global__ __launch_bounds__(kLanes) void k_wd_store(const WFile *__restrict__ files, const char *__restrict__ scratch, uint8_t *__restrict__ out) {
    const WFile f = files[blockIdx.y];
    const vp::Result &R = *(const vp::Result *)(scratch + f.res_off);
    if (R.err) return;
    const uint32_t p = (uint32_t)blockIdx.x * kLanes + threadIdx.x;
    if (p >= (uint32_t)f.W * (uint32_t)f.H) return;
    const uint32_t v = ((const uint32_t *)(scratch + f.argb_off[R.ntrans & 1]))[p];
    if (f.plane) { out[f.out_off + p] = (uint8_t)(v >> 8); return; }
    uint8_t *q = out + f.out_off + (int64_t)p * f.channels;
    q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16);
    if (f.channels == 4) q[3] = R.has_alpha ? (uint8_t)(v >> 24) : 255;
}

}  // namespace

extern "C" int csm_webp_decode_desc_words(void) { return kDescWords; }

extern "C" size_t csm_webp_decode_scratch_bytes(const int32_t *desc_host, int n) {
    Plan p;
    if (!make_plan(desc_host, n, 0, 0, false, false, p)) return 0;
    return (size_t)p.total;
}

size_t csm::vp8l_scratch_bytes(const int32_t *desc_host, int n, bool planes) {
    Plan p;
    if (!make_plan(desc_host, n, 0, 0, false, planes, p)) return 0;
    return (size_t)p.total;
}

int csm::vp8l_launch(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes, void *scratch,
                     bool planes, hipStream_t st) {
    Plan p;
    if (!make_plan(desc_host, n, blob_bytes, out_bytes, true, planes, p)) return CSM_ERR_ARG;
    char *S = (char *)scratch;
    WFile *files = (WFile *)(S + p.o_files);
    // p.files is pageable host memory: the runtime stages such a copy before hipMemcpyAsync returns
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(WFile), hipMemcpyHostToDevice, st));
    k_wd_walk<<<n, 64, 0, st>>>(blob, files, S);
    int rc = csm::check_launch("k_wd_walk"); if (rc) return rc;
    const dim3 pixel_grid(csm::cdiv(p.max_pixels, kLanes), (unsigned)n);
    for (int step = 0; step < vp::kMaxTransforms; ++step) {
        k_wd_pixel<<<pixel_grid, kLanes, 0, st>>>(files, S, step);
        rc = csm::check_launch("k_wd_pixel"); if (rc) return rc;
        k_wd_predict<<<n, kBandRows, 0, st>>>(files, S, step);
        rc = csm::check_launch("k_wd_predict"); if (rc) return rc;
    }
    k_wd_store<<<pixel_grid, kLanes, 0, st>>>(files, S, out);
    return csm::check_launch("k_wd_store");
}

int csm::vp8l_errors(const void *scratch, int n, uint32_t *err_host, hipStream_t st) {
    std::vector<vp::Result> res(n);
    CSM_HIP(hipMemcpyAsync(res.data(), (const char *)scratch + csm::align16((int64_t)n * sizeof(WFile)), (size_t)n * sizeof(vp::Result),
                           hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) err_host[i] = res[i].err;
    return CSM_OK;
}

extern "C" int csm_webp_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                               void *scratch, int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && out && scratch && blob_bytes > 0 && out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    int rc = csm::vp8l_launch(blob, blob_bytes, desc_host, n, out, out_bytes, scratch, false, st);
    if (rc) return rc;
    std::vector<uint32_t> err(n);
    rc = csm::vp8l_errors(scratch, n, err.data(), st);
    if (rc) return rc;
    int bad = -1;
    for (int i = 0; i < n; ++i) {
        if (info_host) info_host[i] = (int)err[i];
        if ((err[i] & ~(uint32_t)vp::kErrCap) && bad < 0) bad = i;
    }
    if (bad >= 0) {
        csm::set_error("webp decode: file %d of the call has corrupt data (error word 0x%x: see csm_vp8l.h)", bad, err[bad]);
        return CSM_ERR_DATA;
    }
    return CSM_OK;
}
