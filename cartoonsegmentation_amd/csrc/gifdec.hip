// gifdec.hip -- GIF files (GIF87a / GIF89a, animated or not) to uint8 B, G, R (or B, G, R, A) frames on the device, for gfx950.
// The contract is fixed to the byte (frame i equals what Pillow shows after seek(i)) and restated in numpy in
// tests/gifdec_restatement.py; the host side (container parser) is cartoonsegmentation_amd/gifread.py; the code walker is csm_lzw.h,
// which also compiles for the host.
//
// An LZW dictionary entry is always "the previous string plus the first byte of the current one", so every code is a literal or a
// copy (destination, source, length) of bytes already in the output.  The code stream is serial per image; everything behind it is
// not.
//
//   k_gd_identity  src[p] = p for every pixel of every image of the call's group
//   k_gd_walk      one wave per image: the wave stages the compressed bytes through a window in LDS, the dictionary (4096 x offset
//                  and length, 24 KiB) lives in LDS, one lane walks up to 64 codes into records in LDS, then the wave fans them
//                  out: a literal's value to lit[p], a copy's sources to src[p] = source + k (lane per record for the first 8
//                  positions, the whole wave for the rest of a long copy).  No record list in memory
//   k_gd_double    src[p] = src[src[p]], in place, launched ceil(log2(pixels of the largest image)) times; a round whose predecessor
//                  changed nothing in the image returns at once (a device flag per image and round; the host reads nothing)
//   k_gd_gather    idx[p] = lit[src[p]]: the image's indices, 1 byte per pixel, in the caller's index buffer
//   k_gd_compose   one thread per canvas pixel loops over the file's frames in order; the pixel's colour and alpha, the value the
//                  pending disposal will store and the value before the frame stay in registers; it maps the interlaced row order,
//                  tests the rectangle and the transparent index, looks up the local or global table and stores frame f's pixel
//
// Scratch per pixel of a group's images: 4 B of source positions and 1 B of literals; the indices (1 B per pixel) are the only
// bytes that stay until the compose.  No kernel waits on another workgroup and there is no spin loop on memory.  Every read and
// store is bounded by sizes from the descriptors, whatever the data: a corrupt stream raises bits of the image's error word and
// yields garbage inside the image's own buffers.
#include "csm_common.h"
#include "csm_lzw.h"
#include <algorithm>
#include <vector>

namespace {

namespace lzw = csm_lzw;

constexpr int kDescWords = 16;
constexpr int kWindow = 1024;                // bytes of compressed data staged in LDS: 24 KiB + 1 KiB + the batch leave six images per CU
constexpr int kBatch = 64;                   // records per fan-out
constexpr int kShort = 8;                    // positions of a copy that its own lane stores
constexpr int kLanes = 256;
constexpr int kMaxRounds = 31;
constexpr int kFlagWords = 32;               // per image: [r] = doubling round r changed a source
constexpr int64_t kMaxPixels = 0x7FFFFFFF;

struct GImage {
    // from the caller's descriptor
    int H, W, top, left;
    int in_off, in_len, mcs, lace;
    int transparent, disposal, pal_off, pal_len;
    int64_t idx_off;
    int file;
    // derived
    uint32_t npix;
    int rounds, slot;                        // slot: the image's place in the call's group, -1 outside it
    int64_t lit_off, src_off;                // byte offsets in scratch (images of the group only)
};

struct GFile {
    int H, W, first, count;
    int64_t out_off;
    int background, alpha;
};

struct Plan {
    std::vector<GImage> images;
    std::vector<GFile> files;
    uint32_t max_npix = 0, max_canvas = 0;
    int max_rounds = 0;
    int64_t o_images, o_files, o_flags, o_err, o_heavy, total;
};

int64_t wide(int lo, int hi) { return (int64_t)lo | ((int64_t)hi << 31); }

// false: the descriptors are invalid (the error is set)
bool make_plan(const int32_t *desc, int n, const int32_t *fdesc, int nf, int first, int count, int channels, int64_t blob_bytes,
               int64_t idx_bytes, int64_t out_bytes, bool check_ranges, bool compose, Plan &p) {
    if (!desc || !fdesc || n < 1 || n > (1 << 20) || nf < 1 || nf > n) {
        csm::set_error("invalid argument: 1 <= files <= images <= 2^20 descriptors"); return false;
    }
    if (first < 0 || count < 0 || count > 65535 || first > n - count) {
        csm::set_error("invalid argument: the group [first, first + count) lies outside the images, or holds more than 65535"); return false;
    }
    p.images.resize(n);
    p.files.resize(nf);
    for (int j = 0; j < nf; ++j) {
        const int32_t *d = fdesc + (int64_t)j * kDescWords;
        GFile &f = p.files[j];
        f.H = d[0]; f.W = d[1]; f.first = d[2]; f.count = d[3]; f.out_off = wide(d[4], d[5]); f.background = d[6]; f.alpha = d[7] & 1;
        bool ok = f.H >= 1 && f.W >= 1 && (int64_t)f.H * f.W <= kMaxPixels && f.first >= 0 && f.count >= 1 && f.first <= n - f.count;
        ok = ok && d[4] >= 0 && d[5] >= 0 && (f.out_off & 3) == 0 && f.background >= 0 && f.background <= 255;
        if (ok && check_ranges && compose) ok = f.out_off + (int64_t)f.count * f.H * f.W * channels <= out_bytes;
        if (!ok) { csm::set_error("invalid argument: file descriptor %d of the GIF decode", j); return false; }
        p.max_canvas = std::max(p.max_canvas, (uint32_t)(f.H * f.W));
    }
    int64_t o = 0;
    p.o_images = o;  o += csm::align16((int64_t)n * sizeof(GImage));
    p.o_files = o;   o += csm::align16((int64_t)nf * sizeof(GFile));
    p.o_flags = o;   o += csm::align16((int64_t)count * kFlagWords * 4);
    p.o_err = o;     o += csm::align16((int64_t)count * 4);
    p.o_heavy = o;
    for (int i = 0; i < n; ++i) {
        const int32_t *d = desc + (int64_t)i * kDescWords;
        GImage &g = p.images[i];
        g.H = d[0]; g.W = d[1]; g.top = d[2]; g.left = d[3]; g.in_off = d[4]; g.in_len = d[5]; g.mcs = d[6]; g.lace = d[7] & 1;
        g.transparent = d[8]; g.disposal = d[9]; g.pal_off = d[10]; g.pal_len = d[11]; g.idx_off = wide(d[12], d[13]); g.file = d[14];
        bool ok = g.H >= 1 && g.W >= 1 && g.top >= 0 && g.left >= 0 && g.file >= 0 && g.file < nf;
        const int64_t npix = ok ? (int64_t)g.H * g.W : 0;
        if (ok) {
            const GFile &f = p.files[g.file];
            ok = g.top <= f.H - g.H && g.left <= f.W - g.W && i >= f.first && i - f.first < f.count;
        }
        ok = ok && g.in_off >= 0 && (g.in_off & 15) == 0 && g.in_len >= 0 && g.mcs >= 2 && g.mcs <= 8;
        ok = ok && g.transparent >= -1 && g.transparent <= 255 && (g.disposal == 0 || g.disposal == 2 || g.disposal == 3);
        ok = ok && g.pal_off >= 0 && (g.pal_off & 15) == 0 && g.pal_len >= 1 && g.pal_len <= 256;
        ok = ok && d[12] >= 0 && d[13] >= 0 && (g.idx_off & 15) == 0;
        if (ok && check_ranges) {
            ok = csm::align16((int64_t)g.in_off + g.in_len) <= blob_bytes && (int64_t)g.pal_off + 768 <= blob_bytes &&
                 g.idx_off + csm::align16(npix) <= idx_bytes;
        }
        if (!ok) { csm::set_error("invalid argument: image descriptor %d of the GIF decode", i); return false; }
        g.npix = (uint32_t)npix;
        g.rounds = 0;
        while (g.rounds < kMaxRounds && ((int64_t)1 << g.rounds) < npix) ++g.rounds;
        g.slot = -1; g.lit_off = 0; g.src_off = 0;
        if (i >= first && i < first + count) {
            g.slot = i - first;
            g.lit_off = o;  o += csm::align16(npix);
            g.src_off = o;  o += csm::align16(npix * 4);
            p.max_npix = std::max(p.max_npix, g.npix);
            p.max_rounds = std::max(p.max_rounds, g.rounds);
        }
    }
    p.total = o;
    return true;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
struct WalkShared {
    lzw::Table T;
    lzw::State S;
    lzw::Record rec[kBatch];
    int status, n;
};

// one wave per image of the group.  Lane 0 runs the walker; the window and the fan-out are done by the whole wave, under
// wave-uniform control flow.
__global__ __launch_bounds__(64) void k_gd_walk(const uint8_t *__restrict__ blob, const GImage *__restrict__ images, char *__restrict__ scratch,
                                                 uint32_t *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kWindow];
    __shared__ WalkShared sh;
    const GImage g = images[blockIdx.x];
    const int lane = threadIdx.x;
    const uint8_t *in = blob + g.in_off;
    const uint32_t in_len = (uint32_t)g.in_len, npix = g.npix;
    uint8_t *lit = (uint8_t *)(scratch + g.lit_off);
    uint32_t *src = (uint32_t *)(scratch + g.src_off);
    if (lane == 0) lzw::init(sh.S, 0, in_len, g.mcs, npix);               // an empty window: the first step asks for input
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            int n = 0;
            sh.status = lzw::step(sh.S, sh.T, win, sh.rec, kBatch, n);
            sh.n = n;
        }
        __syncthreads();
        const int status = sh.status, n = sh.n;
        lzw::Record r = lzw::Record{0, 0, 0};
        if (lane < n) r = sh.rec[lane];
        const bool literal = (r.len & lzw::kLiteral) != 0;
        uint32_t len = r.len & ~lzw::kLiteral;
        // the walker lists no record that leaves the image or reads from its own destination onwards
        if (r.dst >= npix || len > npix - r.dst || (!literal && r.src >= r.dst)) len = 0;
        if (literal) {
            if (len) lit[r.dst] = (uint8_t)r.src;
        } else {
            for (uint32_t k = 0; k < min(len, (uint32_t)kShort); ++k) src[r.dst + k] = r.src + k;
        }
        unsigned long long longs = __ballot(!literal && len > (uint32_t)kShort);
        while (longs) {
            const int j = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            const uint32_t d = __shfl(r.dst, j), s = __shfl(r.src, j), l = __shfl(len, j);
            for (uint32_t k = kShort + lane; k < l; k += 64) src[d + k] = s + k;
        }
        if (status == lzw::kDone) break;
        if (status == lzw::kNeedInput) {
            const uint32_t base = lzw::byte_position(sh.S) & ~15u;
            // base <= in_len: the walker never asks for input when none is left
            const uint32_t wlen = min((uint32_t)kWindow, in_len - min(base, in_len));
            for (uint32_t i = lane * 16u; i < wlen; i += 64u * 16u)        // the blob holds the stream's bytes rounded up to 16
                *(uint4 *)(win + i) = *(const uint4 *)(in + base + i);
            __syncthreads();
            if (lane == 0) lzw::restage(sh.S, base, wlen);
        }
    }
    if (lane == 0 && sh.S.err) atomicOr(&err[blockIdx.x], sh.S.err);
}

// ---- the resolve --------------------------------------------------------------------------------------------------------------
// grid (groups of 4 * kLanes positions of the largest image, images of the group)
__global__ __launch_bounds__(kLanes) void k_gd_identity(const GImage *__restrict__ images, char *__restrict__ scratch) {
    const GImage g = images[blockIdx.y];
    const uint32_t p = ((uint32_t)blockIdx.x * kLanes + threadIdx.x) * 4u;
    if (p >= g.npix) return;                                           // the array is padded to whole uint4
    *(uint4 *)(scratch + g.src_off + (int64_t)p * 4) = make_uint4(p, p + 1, p + 2, p + 3);
}

// the same grid; round r of the pointer doubling.  A value read is the old or the new ancestor of its position: both are valid, so
// the update is done in place.
__global__ __launch_bounds__(kLanes) void k_gd_double(const GImage *__restrict__ images, char *__restrict__ scratch, int *__restrict__ flags, int round) {
    const GImage g = images[blockIdx.y];
    int *fl = flags + (int64_t)blockIdx.y * kFlagWords;
    if (round >= g.rounds || (round > 0 && fl[round - 1] == 0)) return;
    const uint32_t p = ((uint32_t)blockIdx.x * kLanes + threadIdx.x) * 4u;
    if (p >= g.npix) return;
    uint32_t *src = (uint32_t *)(scratch + g.src_off);
    uint4 v = *(uint4 *)(src + p);
    const uint32_t last = g.npix - 1;
    // positions of the padding hold their own index (>= npix): they stay as they are
    const uint32_t a = v.x != p && v.x <= last ? src[v.x] : v.x;
    const uint32_t b = v.y != p + 1 && v.y <= last ? src[v.y] : v.y;
    const uint32_t c = v.z != p + 2 && v.z <= last ? src[v.z] : v.z;
    const uint32_t d = v.w != p + 3 && v.w <= last ? src[v.w] : v.w;
    if (a != v.x || b != v.y || c != v.z || d != v.w) {
        *(uint4 *)(src + p) = make_uint4(a, b, c, d);
        fl[round] = 1;
    }
}

// the same grid: four indices per thread, one 4-byte store (the index buffer holds every image's pixels rounded up to 16)
__global__ __launch_bounds__(kLanes) void k_gd_gather(const GImage *__restrict__ images, const char *__restrict__ scratch, uint8_t *__restrict__ idx) {
    const GImage g = images[blockIdx.y];
    const uint32_t p = ((uint32_t)blockIdx.x * kLanes + threadIdx.x) * 4u;
    if (p >= g.npix) return;
    const uint8_t *lit = (const uint8_t *)(scratch + g.lit_off);
    const uint4 s = *(const uint4 *)(scratch + g.src_off + (int64_t)p * 4);
    const uint32_t last = g.npix - 1;
    const uint32_t w = (uint32_t)lit[min(s.x, last)] | (uint32_t)lit[min(s.y, last)] << 8 | (uint32_t)lit[min(s.z, last)] << 16 |
                       (uint32_t)lit[min(s.w, last)] << 24;
    *(uint32_t *)(idx + g.idx_off + p) = w;
}

// ---- the compose ----------------------------------------------------------------------------------------------------------------
// B | G << 8 | R << 16 of entry i of a table of 768 bytes R, G, B, zero-padded behind its entries
__device__ __forceinline__ uint32_t colour(const uint8_t *pal, int i) {
    const uint8_t *c = pal + 3 * (i & 255);
    return (uint32_t)c[2] | (uint32_t)c[1] << 8 | (uint32_t)c[0] << 16;
}

// the place of row r of an interlaced image of H rows in the stream's row order
__device__ __forceinline__ int laced_row(int r, int H) {
    if ((r & 7) == 0) return r >> 3;
    const int n1 = (H + 7) >> 3;
    if ((r & 7) == 4) return n1 + (r >> 3);
    const int n2 = (H + 3) >> 3;
    if ((r & 3) == 2) return n1 + n2 + (r >> 2);
    return n1 + n2 + ((H + 1) >> 2) + (r >> 1);
}

// grid (groups of kLanes canvas pixels of the largest file, files).  The rules are those of tests/gifdec_restatement.py.
template <int C>
__global__ __launch_bounds__(kLanes) void k_gd_compose(const uint8_t *__restrict__ blob, const GImage *__restrict__ images, const GFile *__restrict__ files,
                                                        const uint8_t *__restrict__ idx, uint8_t *__restrict__ out) {
    const GFile f = files[blockIdx.y];
    const uint32_t q = (uint32_t)blockIdx.x * kLanes + threadIdx.x;
    if (q >= (uint32_t)(f.H * f.W)) return;
    const int y = (int)(q / (uint32_t)f.W), x = (int)(q - (uint32_t)y * f.W);
    const int64_t frame_bytes = (int64_t)f.H * f.W * C;
    uint8_t *o = out + f.out_off + (int64_t)q * C;
    uint32_t cur = 0, pending = 0;                       // colour | alpha << 24
    bool has_pending = false;
    for (int k = 0; k < f.count; ++k, o += frame_bytes) {
        const GImage g = images[f.first + k];
        const uint8_t *pal = blob + g.pal_off;
        const int t = g.transparent;
        if (has_pending) cur = pending;
        has_pending = false;
        const uint32_t before = cur;
        const int r = y - g.top, c = x - g.left;
        const bool in = r >= 0 && r < g.H && c >= 0 && c < g.W;
        int i = -1;
        if (in) i = idx[g.idx_off + (int64_t)(g.lace ? laced_row(r, g.H) : r) * g.W + c];
        if (k == 0) {
            if (!in) i = t >= 0 ? t : 0;
            cur = colour(pal, i) | (i == t ? 0u : 0xFF000000u);
        } else if (in && i != t) {
            cur = colour(pal, i) | 0xFF000000u;
        }
        o[0] = (uint8_t)cur; o[1] = (uint8_t)(cur >> 8); o[2] = (uint8_t)(cur >> 16);
        if (C == 4) o[3] = f.alpha ? (uint8_t)(cur >> 24) : (uint8_t)255;
        if (in && g.disposal == 2) {
            has_pending = true;
            if (k == 0) pending = t >= 0 ? colour(pal, t) : (colour(pal, f.background) | 0xFF000000u);
            else if (t >= 0) pending = colour(pal, t < g.pal_len ? t : 0);
            else pending = colour(pal, f.background < g.pal_len ? f.background : 0) | 0xFF000000u;
        } else if (in && g.disposal == 3) {
            if (k > 0) { has_pending = true; pending = before; }
            else if (t >= 0) { has_pending = true; pending = colour(pal, t); }
        }
    }
}

}  // namespace

extern "C" int csm_gif_decode_desc_words(void) { return kDescWords; }

extern "C" size_t csm_gif_decode_scratch_bytes(const int32_t *desc_host, int n, const int32_t *file_desc_host, int n_files, int first, int count) {
    Plan p;
    if (!make_plan(desc_host, n, file_desc_host, n_files, first, count, 3, 0, 0, 0, false, false, p)) return 0;
    return (size_t)p.total;
}

extern "C" int csm_gif_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, const int32_t *file_desc_host, int n_files,
                              int first, int count, uint8_t *idx, int64_t idx_bytes, uint8_t *out, int64_t out_bytes, int channels,
                              void *scratch, int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && file_desc_host && idx && scratch && blob_bytes > 0 && idx_bytes > 0);
    CSM_REQUIRE(channels == 3 || channels == 4);
    CSM_REQUIRE(!out || out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)idx & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    Plan p;
    if (!make_plan(desc_host, n, file_desc_host, n_files, first, count, channels, blob_bytes, idx_bytes, out_bytes, true, out != nullptr, p))
        return CSM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *S = (char *)scratch;
    GImage *images = (GImage *)(S + p.o_images);
    GFile *files = (GFile *)(S + p.o_files);
    int *flags = (int *)(S + p.o_flags);
    uint32_t *err = (uint32_t *)(S + p.o_err);
    // p.images and p.files are pageable host memory: the runtime stages such a copy before hipMemcpyAsync returns, so an early return
    // below (a failed launch check) may destroy p while the stream still runs
    CSM_HIP(hipMemcpyAsync(images, p.images.data(), (size_t)n * sizeof(GImage), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n_files * sizeof(GFile), hipMemcpyHostToDevice, st));
    int rc;
    if (count > 0) {
        CSM_HIP(hipMemsetAsync(flags, 0, (size_t)(p.o_heavy - p.o_flags), st));                      // flags, err
        const GImage *group = images + first;
        const dim3 quad_grid(csm::cdiv(p.max_npix, 4 * kLanes), (unsigned)count);
        k_gd_identity<<<quad_grid, kLanes, 0, st>>>(group, S);
        rc = csm::check_launch("k_gd_identity"); if (rc) return rc;
        k_gd_walk<<<count, 64, 0, st>>>(blob, group, S, err);
        rc = csm::check_launch("k_gd_walk"); if (rc) return rc;
        for (int r = 0; r < p.max_rounds; ++r) {
            k_gd_double<<<quad_grid, kLanes, 0, st>>>(group, S, flags, r);
            rc = csm::check_launch("k_gd_double"); if (rc) return rc;
        }
        k_gd_gather<<<quad_grid, kLanes, 0, st>>>(group, S, idx);
        rc = csm::check_launch("k_gd_gather"); if (rc) return rc;
    }
    if (out) {
        const dim3 grid(csm::cdiv(p.max_canvas, kLanes), (unsigned)n_files);
        if (channels == 4) k_gd_compose<4><<<grid, kLanes, 0, st>>>(blob, images, files, idx, out);
        else k_gd_compose<3><<<grid, kLanes, 0, st>>>(blob, images, files, idx, out);
        rc = csm::check_launch("k_gd_compose"); if (rc) return rc;
    }
    if (info_host) { info_host[0] = p.max_rounds; info_host[1] = 0; }
    if (count == 0) return CSM_OK;
    std::vector<uint32_t> err_host(count);
    std::vector<int> flags_host((size_t)count * kFlagWords);
    CSM_HIP(hipMemcpyAsync(err_host.data(), err, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipMemcpyAsync(flags_host.data(), flags, flags_host.size() * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    if (info_host) {
        int used = 0;                                                   // doubling rounds that did work, over the images of the group
        for (int i = 0; i < count; ++i)
            for (int r = 0; r < p.images[first + i].rounds; ++r)
                if (r == 0 || flags_host[(size_t)i * kFlagWords + r - 1]) used = std::max(used, r + 1);
        info_host[1] = used;
    }
    for (int i = 0; i < count; ++i) {
        if (err_host[i]) {
            csm::set_error("gif decode: image %d of the call has corrupt LZW data (error word 0x%x: see csm_lzw.h)", first + i, err_host[i]);
            return CSM_ERR_DATA;
        }
    }
    return CSM_OK;
}
