// webplossy.hip -- lossy WebP files (VP8 key frames, with or without an ALPH chunk) to uint8 B, G, R (, A) on the device, for gfx950.
// The contract is fixed to the byte (the result equals what libwebp decodes) and restated in Python in
// tests/webplossy_restatement.py; the host side (container parser) is cartoonsegmentation_amd/webpread.py; the boolean decoder, the
// parsers and the per-macroblock arithmetic are csm_vp8dec.h, which also compiles for the host.
//
// The boolean-coded partitions are serial per file; everything behind them runs along macroblock diagonals.
//
//   k_vd_walk      one wave per file, one lane of it at work: the frame header, then every macroblock in raster order -- modes from
//                  the first partition, tokens from partition row % parts (up to 8 decoder states, all in LDS with the header and
//                  its probabilities) -- into per-macroblock records and dequantised coefficients.  The inverse WHT of a
//                  whole-block macroblock runs here: whether its inner edges are filtered depends on the DCs it gives
//   k_vd_recon     one workgroup per file: macroblock (x, y) at step x + 2 y (the slope of two is for the sub-blocks' top-right
//                  pixels), kReconMbs macroblocks per step, two lanes each (luma | chroma): prediction from the unfiltered
//                  neighbours, inverse DCT, add and clip into bordered planes
//   k_vd_filter    the simple or the normal loop filter in place, on the same slope-2 wavefront: raster order is the definition,
//                  and macroblock (x, y) needs (x + 1, y - 1) done
//   k_vd_alpha     the ALPH chunk behind its decoder: raw bytes copied (compression 0) or the green bytes the lossless decoder's
//                  kernels left (compression 1; csm_webpdec.h), then filter 1..3 undone on a row wavefront
//   k_vd_store     crop, libwebp's chroma upsampling and colour conversion, B, G, R (, A) bytes
//
// No kernel waits on another workgroup and there is no spin loop on memory.  Every read and store is bounded by sizes from the
// descriptor, whatever the data: a corrupt stream raises bits of the file's error word and leaves the file's pixels undefined.
#include "csm_common.h"
#include "csm_vp8dec.h"
#include "csm_vp8l.h"
#include "csm_webpdec.h"
#include <algorithm>
#include <vector>

namespace {

namespace vd = csm_vp8d;

constexpr int kDescWords = 12;
constexpr int kLanes = 256;
constexpr int kReconMbs = 32;                // macroblocks of one step of k_vd_recon and k_vd_filter (tests/webplossy_cases.py has a longer diagonal)
constexpr int kAlphaRows = 256;              // rows of one band of k_vd_alpha
constexpr int kMaxSide = 16383;

struct VFile {
    // from the caller's descriptor
    int H, W, has_alpha, channels;
    int in_off, in_len, alpha_head, alpha_off, alpha_len;
    int64_t out_off;
    // derived
    int mbw, mbh;
    int64_t frame_off, rec_off, coef_off, modes_off, nz_off, y_off, u_off, v_off, a_off;     // byte offsets in scratch
};

struct Plan {
    std::vector<VFile> files;
    std::vector<int32_t> alpha_desc;         // the lossless decoder's descriptors of the alpha planes of compression 1
    std::vector<int> alpha_file;
    int64_t max_pixels = 0;
    int64_t o_files, o_frames, o_zero, o_vp8l, total;
};

// false: the descriptors are invalid (the error is set)
bool make_plan(const int32_t *desc, int n, int64_t blob_bytes, int64_t out_bytes, bool check_ranges, Plan &p) {
    if (!desc || n < 1 || n > 65535) { csm::set_error("invalid argument: 1 <= n <= 65535 descriptors"); return false; }
    p.files.resize(n);
    int64_t o = 0;
    p.o_files = o;   o += csm::align16((int64_t)n * sizeof(VFile));
    p.o_frames = o;  o += csm::align16((int64_t)n * sizeof(vd::Frame));
    p.o_zero = o;                            // from here to o_vp8l the scratch starts as zeros (the coefficients rely on it)
    for (int i = 0; i < n; ++i) {
        const int32_t *d = desc + (int64_t)i * kDescWords;
        VFile &f = p.files[i];
        f.H = d[0]; f.W = d[1]; f.has_alpha = d[2]; f.channels = d[3]; f.in_off = d[4]; f.in_len = d[5]; f.alpha_head = d[6];
        f.out_off = (int64_t)d[7] | ((int64_t)d[8] << 31);
        f.alpha_off = d[9]; f.alpha_len = d[10];
        bool ok = f.H >= 1 && f.W >= 1 && f.H <= kMaxSide && f.W <= kMaxSide && (f.has_alpha == 0 || f.has_alpha == 1) && (f.channels == 3 || f.channels == 4);
        ok = ok && f.in_off >= 0 && (f.in_off & 15) == 0 && f.in_len >= 10 && d[7] >= 0 && d[8] >= 0 && (f.out_off & 3) == 0;
        if (ok && f.has_alpha) ok = f.alpha_head >= 0 && f.alpha_head <= 255 && f.alpha_off >= 0 && (f.alpha_off & 15) == 0 && f.alpha_len >= 1;
        if (ok && check_ranges) {
            ok = (int64_t)f.in_off + f.in_len <= blob_bytes && f.out_off + (int64_t)f.H * f.W * f.channels <= out_bytes;
            if (ok && f.has_alpha) ok = (int64_t)f.alpha_off + f.alpha_len <= blob_bytes;
        }
        if (!ok) { csm::set_error("invalid argument: descriptor %d of the lossy WebP decode", i); return false; }
        f.mbw = (f.W + 15) >> 4; f.mbh = (f.H + 15) >> 4;
        const int64_t mbs = (int64_t)f.mbw * f.mbh, pixels = (int64_t)f.H * f.W;
        f.frame_off = p.o_frames + (int64_t)i * sizeof(vd::Frame);
        f.rec_off = o;    o += csm::align16(mbs * sizeof(vd::MbRec));
        f.coef_off = o;   o += csm::align16(mbs * vd::kCoefPerMb * 2);
        f.modes_off = o;  o += csm::align16(4 * f.mbw);
        f.nz_off = o;     o += csm::align16(9 * f.mbw);
        f.y_off = o;      o += csm::align16(vd::plane_bytes(f.mbw, f.mbh, 16));
        f.u_off = o;      o += csm::align16(vd::plane_bytes(f.mbw, f.mbh, 8));
        f.v_off = o;      o += csm::align16(vd::plane_bytes(f.mbw, f.mbh, 8));
        const bool plane = f.has_alpha && f.channels == 4;                   // B, G, R output never looks at the ALPH chunk
        f.a_off = o;      o += plane ? csm::align16(pixels) : 0;
        p.max_pixels = std::max(p.max_pixels, pixels);
        if (plane && (f.alpha_head & 3) == 1 && !(f.alpha_head >> 6)) {
            const int32_t a[12] = {f.H, f.W, 1, 1, f.alpha_off, f.alpha_len, 1, (int32_t)(f.a_off & 0x7fffffff), (int32_t)(f.a_off >> 31), 0, 0, 0};
            p.alpha_desc.insert(p.alpha_desc.end(), a, a + 12);
            p.alpha_file.push_back(i);
        }
    }
    p.o_vp8l = o;
    if (!p.alpha_file.empty()) {
        const size_t need = csm::vp8l_scratch_bytes(p.alpha_desc.data(), (int)p.alpha_file.size(), true);
        if (!need) return false;
        o += csm::align16((int64_t)need);
    }
    p.total = o;
    return true;
}

__device__ vd::Plane plane_at(char *scratch, int64_t off, int mbw, int size) {
    return vd::Plane{(uint8_t *)scratch + off + vd::plane_origin(mbw, size), vd::plane_stride(mbw, size)};
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_vd_walk(const uint8_t *__restrict__ blob, const VFile *__restrict__ files, char *__restrict__ scratch) {
    __shared__ vd::Header h;
    __shared__ vd::Bool first, parts[vd::kMaxParts];
    if (threadIdx.x != 0) return;
    const VFile f = files[blockIdx.x];
    vd::WalkBufs B;
    B.top_modes = (uint8_t *)(scratch + f.modes_off);
    B.top_nz = (uint8_t *)(scratch + f.nz_off);
    B.recs = (vd::MbRec *)(scratch + f.rec_off);
    B.coef = (int16_t *)(scratch + f.coef_off);
    vd::Frame &F = *(vd::Frame *)(scratch + f.frame_off);
    vd::walk_frame(h, first, parts, blob + f.in_off, (uint32_t)f.in_len, (uint32_t)f.W, (uint32_t)f.H, B, F);
    if (f.has_alpha && f.channels == 4) {
        const int comp = f.alpha_head & 3;
        if (comp > 1 || (f.alpha_head >> 6) || (comp == 0 && (int64_t)f.alpha_len < (int64_t)f.W * f.H)) F.err |= vd::kErrAlpha;
    }
}

// ---- reconstruction and loop filter: the slope-2 macroblock wavefront ---------------------------------------------------------------
// calls body(x, y) for the macroblocks of step s that this lane pair owns
template <class Body>
__device__ void wavefront(int mbw, int mbh, Body body) {
    const int slot = threadIdx.x >> 1;
    const int steps = (mbw - 1) + 2 * (mbh - 1) + 1;
    for (int s = 0; s < steps; ++s) {
        const int y_hi = min(s >> 1, mbh - 1), y_lo = max(0, (s - (mbw - 1) + 1) >> 1);
        for (int y = y_lo + slot; y <= y_hi; y += kReconMbs) body(s - 2 * y, y);
        __syncthreads();
    }
}

__global__ __launch_bounds__(2 * kReconMbs) void k_vd_recon(const VFile *__restrict__ files, char *__restrict__ scratch) {
    const VFile f = files[blockIdx.x];
    if (((const vd::Frame *)(scratch + f.frame_off))->err) return;           // the same for every lane
    const int mbw = f.mbw, mbh = f.mbh;
    const vd::Plane Y = plane_at(scratch, f.y_off, mbw, 16), U = plane_at(scratch, f.u_off, mbw, 8), V = plane_at(scratch, f.v_off, mbw, 8);
    // what the format predicts from outside the frame
    for (int x = (int)threadIdx.x - 1; x < 16 * mbw + 4; x += blockDim.x) Y.p[-Y.stride + x] = 127;
    for (int x = (int)threadIdx.x - 1; x < 8 * mbw + 4; x += blockDim.x) U.p[-U.stride + x] = V.p[-V.stride + x] = 127;
    for (int y = threadIdx.x; y < 16 * mbh; y += blockDim.x) Y.p[(int64_t)y * Y.stride - 1] = 129;
    for (int y = threadIdx.x; y < 8 * mbh; y += blockDim.x) U.p[(int64_t)y * U.stride - 1] = V.p[(int64_t)y * V.stride - 1] = 129;
    __syncthreads();
    const vd::MbRec *recs = (const vd::MbRec *)(scratch + f.rec_off);
    const int16_t *coef = (const int16_t *)(scratch + f.coef_off);
    const bool chroma = threadIdx.x & 1;
    wavefront(mbw, mbh, [&](int x, int y) {
        const int64_t at = (int64_t)y * mbw + x;
        const vd::MbRec m = recs[at];
        if (chroma) vd::recon_chroma(U, V, x, y, m, coef + at * vd::kCoefPerMb);
        else vd::recon_luma(Y, x, y, mbw, m, coef + at * vd::kCoefPerMb);
    });
}

__global__ __launch_bounds__(2 * kReconMbs) void k_vd_filter(const VFile *__restrict__ files, char *__restrict__ scratch) {
    const VFile f = files[blockIdx.x];
    const vd::Frame &F = *(const vd::Frame *)(scratch + f.frame_off);
    if (F.err || F.filter_type == 0) return;                                 // the same for every lane
    const int mbw = f.mbw, mbh = f.mbh;
    const bool simple = F.filter_type == 1;
    const vd::Plane Y = plane_at(scratch, f.y_off, mbw, 16), U = plane_at(scratch, f.u_off, mbw, 8), V = plane_at(scratch, f.v_off, mbw, 8);
    const vd::MbRec *recs = (const vd::MbRec *)(scratch + f.rec_off);
    const bool chroma = threadIdx.x & 1;
    wavefront(mbw, mbh, [&](int x, int y) {
        const vd::MbRec m = recs[(int64_t)y * mbw + x];
        if (!chroma) {
            vd::filter_mb(Y, 16, x, y, m, simple);
        } else if (!simple) {                                               // the simple filter leaves chroma alone
            vd::filter_mb(U, 8, x, y, m, false);
            vd::filter_mb(V, 8, x, y, m, false);
        }
    });
}

// ---- alpha ------------------------------------------------------------------------------------------------------------------------
// one workgroup per file.  Lane r owns row r of a band of kAlphaRows rows and takes value x = step - r: its left neighbour stays in
// a register, the row above was stored one step earlier
__global__ __launch_bounds__(kAlphaRows) void k_vd_alpha(const uint8_t *__restrict__ blob, const VFile *__restrict__ files, char *__restrict__ scratch) {
    const VFile f = files[blockIdx.x];
    if (!f.has_alpha || f.channels != 4 || ((const vd::Frame *)(scratch + f.frame_off))->err) return;      // the same for every lane
    uint8_t *plane = (uint8_t *)(scratch + f.a_off);
    const int W = f.W, H = f.H, filter = (f.alpha_head >> 2) & 3;
    if ((f.alpha_head & 3) == 0) {
        const uint8_t *raw = blob + f.alpha_off;
        for (int64_t i = threadIdx.x; i < (int64_t)W * H; i += kAlphaRows) plane[i] = raw[i];
        __syncthreads();
    }
    if (filter == 0) return;
    const int r = threadIdx.x;
    for (int band = 0; band < H; band += kAlphaRows) {
        const int rows = min(kAlphaRows, H - band), y = band + r;
        int L = 0, TL = 0;
        const int steps = W + rows - 1;
        for (int s = 0; s < steps; ++s) {
            const int x = s - r;
            if (r < rows && x >= 0 && x < W) {
                uint8_t *p = plane + (int64_t)y * W + x;
                const int T = y ? p[-W] : 0;
                L = (*p + vd::alpha_predict(filter, x, y, L, T, TL)) & 255;
                *p = (uint8_t)L;
                TL = T;
            }
            __syncthreads();
        }
    }
}

// ---- store ------------------------------------------------------------------------------------------------------------------------
// grid (groups of kLanes pixels of the largest file, files)
__global__ __launch_bounds__(kLanes) void k_vd_store(const VFile *__restrict__ files, char *__restrict__ scratch, uint8_t *__restrict__ out) {
    const VFile f = files[blockIdx.y];
    if (((const vd::Frame *)(scratch + f.frame_off))->err) return;
    const uint32_t p = (uint32_t)blockIdx.x * kLanes + threadIdx.x;
    if (p >= (uint32_t)f.W * (uint32_t)f.H) return;
    const int y = (int)(p / (uint32_t)f.W), x = (int)(p - (uint32_t)y * (uint32_t)f.W);
    const vd::Plane Y = plane_at(scratch, f.y_off, f.mbw, 16), U = plane_at(scratch, f.u_off, f.mbw, 8), V = plane_at(scratch, f.v_off, f.mbw, 8);
    const uint32_t v = vd::pixel_bgr(Y, U, V, x, y, f.W, f.H);
    uint8_t *q = out + f.out_off + (int64_t)p * f.channels;
    q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16);
    if (f.channels == 4) q[3] = f.has_alpha ? ((const uint8_t *)(scratch + f.a_off))[p] : 255;
}

}  // namespace

extern "C" int csm_webp_lossy_decode_desc_words(void) { return kDescWords; }

extern "C" size_t csm_webp_lossy_decode_scratch_bytes(const int32_t *desc_host, int n) {
    Plan p;
    if (!make_plan(desc_host, n, 0, 0, false, p)) return 0;
    return (size_t)p.total;
}

extern "C" int csm_webp_lossy_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                                     void *scratch, int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && out && scratch && blob_bytes > 0 && out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    Plan p;
    if (!make_plan(desc_host, n, blob_bytes, out_bytes, true, p)) return CSM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *S = (char *)scratch;
    VFile *files = (VFile *)(S + p.o_files);
    // p.files is pageable host memory: the runtime stages such a copy before hipMemcpyAsync returns
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(VFile), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemsetAsync(S + p.o_zero, 0, (size_t)(p.o_vp8l - p.o_zero), st));
    const int na = (int)p.alpha_file.size();
    int rc;
    if (na) {                                                               // the alpha planes of compression 1, into the files' planes in scratch
        rc = csm::vp8l_launch(blob, blob_bytes, p.alpha_desc.data(), na, (uint8_t *)S, p.o_vp8l, S + p.o_vp8l, true, st);
        if (rc) return rc;
    }
    k_vd_walk<<<n, 64, 0, st>>>(blob, files, S);
    rc = csm::check_launch("k_vd_walk"); if (rc) return rc;
    k_vd_recon<<<n, 2 * kReconMbs, 0, st>>>(files, S);
    rc = csm::check_launch("k_vd_recon"); if (rc) return rc;
    k_vd_filter<<<n, 2 * kReconMbs, 0, st>>>(files, S);
    rc = csm::check_launch("k_vd_filter"); if (rc) return rc;
    k_vd_alpha<<<n, kAlphaRows, 0, st>>>(blob, files, S);
    rc = csm::check_launch("k_vd_alpha"); if (rc) return rc;
    k_vd_store<<<dim3(csm::cdiv(p.max_pixels, kLanes), (unsigned)n), kLanes, 0, st>>>(files, S, out);
    rc = csm::check_launch("k_vd_store"); if (rc) return rc;
    std::vector<vd::Frame> frames(n);
    CSM_HIP(hipMemcpyAsync(frames.data(), S + p.o_frames, (size_t)n * sizeof(vd::Frame), hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> alpha_err(na);
    if (na) { rc = csm::vp8l_errors(S + p.o_vp8l, na, alpha_err.data(), st); if (rc) return rc; }
    CSM_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> err(n);
    for (int i = 0; i < n; ++i) err[i] = frames[i].err;
    for (int k = 0; k < na; ++k) err[p.alpha_file[k]] |= alpha_err[k] << vd::kErrAlphaShift;
    const uint32_t cap = (uint32_t)csm_vp8l::kErrCap << vd::kErrAlphaShift;    // a valid alpha stream with more groups than the cap: not "corrupt"
    int bad = -1;
    for (int i = 0; i < n; ++i) {
        if (info_host) info_host[i] = (int)err[i];
        if ((err[i] & ~cap) && bad < 0) bad = i;
    }
    if (bad >= 0) {
        csm::set_error("webp lossy decode: file %d of the call has corrupt data (error word 0x%x: see csm_vp8dec.h)", bad, err[bad]);
        return CSM_ERR_DATA;
    }
    return CSM_OK;
}
