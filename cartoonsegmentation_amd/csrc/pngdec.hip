// pngdec.hip -- PNG files (8 bit; grey, RGB, palette, grey + alpha, RGBA; not interlaced) to uint8 BGR on the device, for gfx950.
// The contract is fixed to the byte (the result equals utils.io_utils.imread) and restated in numpy in
// tests/pngdec_restatement.py; the host side (chunk parser) is cartoonsegmentation_amd/pngread.py; the symbol walker is
// csm_inflate.h, which also compiles for the host.
//
// Deflate's Huffman stream is serial per file; everything behind it is not.
//
//   k_pd_walk      one wave per file: the wave stages the compressed bytes in LDS and builds each block's decode tables there, one
//                  lane walks the symbols.  Literals go to their own output position; matches are only listed (position, length,
//                  distance); stored blocks are copied by the wave
//   k_pd_identity  src[p] = p for every raw byte
//   k_pd_match     16 lanes per match: src[p] = p - distance for its bytes (overlapping matches need no special case)
//   k_pd_double    src[p] = src[src[p]], in place, launched ceil(log2(raw bytes)) times; a round whose predecessor changed nothing
//                  in the file returns at once (a device flag per file and round; the host reads nothing)
//   k_pd_gather    raw[p] = lit[src[p]] (in place: the sources are literal positions, which keep their value) and the Adler-32
//                  partial sums of every 4096 bytes
//   k_pd_adler     one workgroup per file folds the partials and compares with the zlib trailer: the four bytes behind the end
//                  of the deflate data (bytes behind those are ignored, as zlib ignores them)
//   k_pd_unfilter  one workgroup per file: lane r owns row r of a band of 256 rows and takes pixel x = step - r, the reconstructed
//                  pixel above through LDS, left and upper-left in registers, one barrier per step; colour conversion in the store
//
// No kernel waits on another workgroup and there is no spin loop on memory.  Every read and store is bounded by sizes from the
// descriptor, whatever the data: a corrupt stream raises bits of the file's error word and yields garbage inside the file's own buffers.
#include "csm_common.h"
#include "csm_inflate.h"
#include <algorithm>
#include <vector>

namespace {

namespace inf = csm_inflate;

constexpr int kDescWords = 12;
constexpr int kWindow = 16384;               // bytes of compressed data staged in LDS
constexpr int kLanes = 256;
constexpr int kChunk = 4096;                 // raw bytes per Adler partial (and per workgroup of k_pd_gather)
constexpr int kMaxRounds = 31;
constexpr int kFlagWords = 32;               // per file: [r] = doubling round r changed a source
constexpr uint32_t kAdlerMod = 65521;
constexpr int64_t kMaxRaw = 0x7FFFFFFF;      // positions are 32 bits, sizes and offsets derived from them signed

struct PFile {
    // from the caller's descriptor
    int H, W, ct;
    int in_off, in_len, pal_off;
    int64_t out_off;
    // derived
    int bpp, stride;
    uint32_t raw, match_cap;
    int nchunks, rounds;
    int64_t lit_off, src_off, match_off, part_off;       // byte offsets in scratch
};

struct Plan {
    std::vector<PFile> files;
    uint32_t max_raw = 0;
    int max_rounds = 0;
    int64_t o_files, o_flags, o_err, o_res, total;
};

// false: the descriptors are invalid (the error is set)
bool make_plan(const int32_t *desc, int n, int64_t blob_bytes, int64_t out_bytes, bool check_ranges, Plan &p) {
    if (!desc || n < 1 || n > 65535) { csm::set_error("invalid argument: 1 <= n <= 65535 descriptors"); return false; }
    p.files.resize(n);
    int64_t o = 0;
    p.o_files = o;  o += csm::align16((int64_t)n * sizeof(PFile));
    p.o_flags = o;  o += csm::align16((int64_t)n * kFlagWords * 4);
    p.o_err = o;    o += csm::align16((int64_t)n * 4);
    p.o_res = o;    o += csm::align16((int64_t)n * 16);
    for (int i = 0; i < n; ++i) {
        const int32_t *d = desc + (int64_t)i * kDescWords;
        PFile &f = p.files[i];
        f.H = d[0]; f.W = d[1]; f.ct = d[2]; f.in_off = d[3]; f.in_len = d[4]; f.pal_off = d[5];
        f.out_off = (int64_t)d[7] | ((int64_t)d[8] << 31);
        bool ok = f.H >= 1 && f.W >= 1 && (f.ct == 0 || f.ct == 2 || f.ct == 3 || f.ct == 4 || f.ct == 6);
        ok = ok && f.in_off >= 0 && (f.in_off & 15) == 0 && f.in_len >= 6 && f.pal_off >= 0 && (f.pal_off & 15) == 0;
        ok = ok && d[7] >= 0 && d[8] >= 0 && (f.out_off & 3) == 0;
        f.bpp = f.ct == 2 ? 3 : f.ct == 4 ? 2 : f.ct == 6 ? 4 : 1;
        const int64_t stride = 1 + (int64_t)f.W * f.bpp, raw = ok ? stride * f.H : 0;
        ok = ok && raw <= kMaxRaw;
        if (ok && check_ranges) {
            ok = csm::align16((int64_t)f.in_off + f.in_len) <= blob_bytes && (int64_t)f.pal_off + 768 <= blob_bytes &&
                 f.out_off + (int64_t)f.H * f.W * 3 <= out_bytes;
        }
        if (!ok) { csm::set_error("invalid argument: descriptor %d of the PNG decode", i); return false; }
        f.stride = (int)stride; f.raw = (uint32_t)raw; f.match_cap = f.raw / 3;
        f.nchunks = (int)((raw + kChunk - 1) / kChunk);
        f.rounds = 0;
        while (f.rounds < kMaxRounds && ((int64_t)1 << f.rounds) < raw) ++f.rounds;
        f.lit_off = o;    o += csm::align16(raw);
        f.src_off = o;    o += csm::align16(raw * 4);
        f.match_off = o;  o += csm::align16((int64_t)f.match_cap * 8);
        f.part_off = o;   o += csm::align16((int64_t)f.nchunks * 8);
        p.max_raw = std::max(p.max_raw, f.raw);
        p.max_rounds = std::max(p.max_rounds, f.rounds);
    }
    p.total = o;
    return true;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
struct WalkShared {
    inf::State S;
    inf::Tables T;
    int status;
};

// one wave per file.  Lane 0 runs the walker; whatever it asks for is done by the whole wave, under wave-uniform control flow.
__global__ __launch_bounds__(64) void k_pd_walk(const uint8_t *__restrict__ blob, const PFile *__restrict__ files, char *__restrict__ scratch,
                                                 uint32_t *__restrict__ res, uint32_t *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kWindow];
    __shared__ WalkShared sh;
    const PFile f = files[blockIdx.x];
    const int lane = threadIdx.x;
    const uint8_t *in = blob + f.in_off;
    const uint32_t in_len = (uint32_t)f.in_len - 4;                     // without the Adler-32 trailer
    uint8_t *lit = (uint8_t *)(scratch + f.lit_off);
    uint32_t *matches = (uint32_t *)(scratch + f.match_off);
    if (lane == 0) {
        inf::init(sh.S, 0, in_len, 2, f.raw, f.match_cap);              // behind the zlib header
        sh.status = inf::kNeedInput;
    }
    __syncthreads();
    for (;;) {
        const int status = sh.status;
        if (status == inf::kNeedInput) {
            const uint32_t base = inf::byte_position(sh.S) & ~15u;
            // base <= in_len: the walker never asks for input when none is left
            const uint32_t len = min((uint32_t)kWindow, in_len - min(base, in_len));
            __syncthreads();
            for (uint32_t i = lane * 16u; i < len; i += 64u * 16u)         // the blob holds the file's bytes rounded up to 16
                *(uint4 *)(win + i) = *(const uint4 *)(in + base + i);
            if (lane == 0) inf::restage(sh.S, base, len);
        } else if (status == inf::kBuild) {
            if (lane == 0) inf::prepare(sh.S, sh.T);
            inf::clear_fast(sh.T, lane, 64);
            __syncthreads();
            if (!sh.S.err) inf::fill_fast(sh.S, sh.T, lane, 64);
        } else if (status == inf::kStored) {
            const uint32_t src = sh.S.stored_src, n = sh.S.stored_len, out = sh.S.out;
            for (uint32_t i = lane; i < n; i += 64) lit[out + i] = in[src + i];
            __syncthreads();
            if (lane == 0) inf::stored_done(sh.S);
        } else {
            break;
        }
        __syncthreads();
        if (lane == 0) sh.status = sh.S.err ? (int)inf::kDone : inf::step(sh.S, sh.T, win, lit, matches);
        __syncthreads();
    }
    if (lane == 0) {
        res[4 * blockIdx.x] = sh.S.out;
        res[4 * blockIdx.x + 1] = sh.S.nmatch;
        res[4 * blockIdx.x + 2] = min(inf::byte_position(sh.S), in_len);           // where the trailer stands

        if (sh.S.err) atomicOr(&err[blockIdx.x], sh.S.err);
    }
}

// ---- the resolve --------------------------------------------------------------------------------------------------------------
// grid (groups of 4 * kLanes positions of the largest file, files)
__global__ __launch_bounds__(kLanes) void k_pd_identity(const PFile *__restrict__ files, char *__restrict__ scratch) {
    const PFile f = files[blockIdx.y];
    const uint32_t p = ((uint32_t)blockIdx.x * kLanes + threadIdx.x) * 4u;
    if (p >= f.raw) return;                                            // the array is padded to whole uint4
    *(uint4 *)(scratch + f.src_off + (int64_t)p * 4) = make_uint4(p, p + 1, p + 2, p + 3);
}

// grid (any, files): 16 lanes per match, matches taken with the grid's stride
__global__ __launch_bounds__(kLanes) void k_pd_match(const PFile *__restrict__ files, char *__restrict__ scratch, const uint32_t *__restrict__ res) {
    const PFile f = files[blockIdx.y];
    const uint32_t n = min(res[4 * blockIdx.y + 1], f.match_cap);
    const uint2 *M = (const uint2 *)(scratch + f.match_off);
    uint32_t *src = (uint32_t *)(scratch + f.src_off);
    const uint32_t sub = threadIdx.x & 15;
    for (uint32_t m = (uint32_t)blockIdx.x * (kLanes / 16) + (threadIdx.x >> 4); m < n; m += gridDim.x * (kLanes / 16)) {
        const uint2 r = M[m];
        const uint32_t len = (r.y & 255u) + 3u, dist = (r.y >> 8) + 1u;
        if (r.x < dist || r.x > f.raw || len > f.raw - r.x) continue;   // the walker lists no such match
        for (uint32_t k = sub; k < len; k += 16) src[r.x + k] = r.x + k - dist;
    }
}

// grid (groups of 4 * kLanes positions of the largest file, files); round r of the pointer doubling.  A value read is the old or the
// new ancestor of its position: both are valid, so the update is done in place.
__global__ __launch_bounds__(kLanes) void k_pd_double(const PFile *__restrict__ files, char *__restrict__ scratch, int *__restrict__ flags, int round) {
    const PFile f = files[blockIdx.y];
    int *fl = flags + (int64_t)blockIdx.y * kFlagWords;
    if (round >= f.rounds || (round > 0 && fl[round - 1] == 0)) return;
    const uint32_t p = ((uint32_t)blockIdx.x * kLanes + threadIdx.x) * 4u;
    if (p >= f.raw) return;
    uint32_t *src = (uint32_t *)(scratch + f.src_off);
    uint4 v = *(uint4 *)(src + p);
    const uint32_t last = f.raw - 1;
    // positions of the padding hold their own index (>= raw): they stay as they are
    const uint32_t a = v.x != p && v.x <= last ? src[v.x] : v.x;
    const uint32_t b = v.y != p + 1 && v.y <= last ? src[v.y] : v.y;
    const uint32_t c = v.z != p + 2 && v.z <= last ? src[v.z] : v.z;
    const uint32_t d = v.w != p + 3 && v.w <= last ? src[v.w] : v.w;
    if (a != v.x || b != v.y || c != v.z || d != v.w) {
        *(uint4 *)(src + p) = make_uint4(a, b, c, d);
        fl[round] = 1;
    }
}

// grid (chunks of the largest file, files): 16 bytes per thread, the raw bytes in place of the literals, and the chunk's Adler sums
// A = sum of the bytes, B = sum of (L - i) * byte i over the chunk's L bytes
__global__ __launch_bounds__(kLanes) void k_pd_gather(const PFile *__restrict__ files, char *__restrict__ scratch) {
    const PFile f = files[blockIdx.y];
    if ((int)blockIdx.x >= f.nchunks) return;
    const uint32_t c0 = (uint32_t)blockIdx.x * kChunk;
    const uint32_t L = min((uint32_t)kChunk, f.raw - c0);
    const uint32_t t0 = threadIdx.x * 16u;
    const uint32_t nt = t0 < L ? min(16u, L - t0) : 0u;
    uint8_t *lit = (uint8_t *)(scratch + f.lit_off);
    const uint32_t *src = (const uint32_t *)(scratch + f.src_off);
    uint32_t A = 0, B = 0;
    if (nt) {
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t last = f.raw - 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4u * q >= nt) break;                                   // the source array ends with the quad that holds byte raw - 1
            const uint4 s = *(const uint4 *)(src + c0 + t0 + 4 * q);
            const uint32_t sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = 4 * q + k;
                if (i < nt) {
                    const uint32_t byte = lit[min(sv[k], last)];
                    w[q] |= byte << (8 * k);
                    A += byte;
                    B += (nt - i) * byte;
                }
            }
        }
        *(uint4 *)(lit + c0 + t0) = make_uint4(w[0], w[1], w[2], w[3]);
        B += (L - t0 - nt) * A;                                        // the bytes behind this thread's in the chunk
    }
    unsigned long long a64 = A, b64 = B;
    for (int o = 32; o > 0; o >>= 1) { a64 += __shfl_down(a64, o); b64 += __shfl_down(b64, o); }
    __shared__ unsigned long long sa[kLanes / 64], sb[kLanes / 64];
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = a64; sb[threadIdx.x >> 6] = b64; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kLanes / 64; ++k) { a64 += sa[k]; b64 += sb[k]; }
        uint32_t *part = (uint32_t *)(scratch + f.part_off);
        part[2 * blockIdx.x] = (uint32_t)(a64 % kAdlerMod);
        part[2 * blockIdx.x + 1] = (uint32_t)(b64 % kAdlerMod);
    }
}

// two runs of bytes (A, B, L) one after the other: (A1 + A2, B1 + B2 + L2 * A1, L1 + L2), all mod 65521
__device__ __forceinline__ void adler_append(uint64_t &A, uint64_t &B, uint64_t &L, uint64_t a, uint64_t b, uint64_t l) {
    B = (B + b + l * A) % kAdlerMod;
    A = (A + a) % kAdlerMod;
    L = (L + l) % kAdlerMod;
}

// one workgroup per file
__global__ __launch_bounds__(kLanes) void k_pd_adler(const uint8_t *__restrict__ blob, const PFile *__restrict__ files, const char *__restrict__ scratch,
                                                      const uint32_t *__restrict__ res, uint32_t *__restrict__ err) {
    const PFile f = files[blockIdx.x];
    const uint32_t *part = (const uint32_t *)(scratch + f.part_off);
    const int per = (f.nchunks + kLanes - 1) / kLanes;
    uint64_t A = 0, B = 0, L = 0;
    for (int c = threadIdx.x * per; c < min(f.nchunks, (int)(threadIdx.x + 1) * per); ++c)
        adler_append(A, B, L, part[2 * c], part[2 * c + 1], min((uint32_t)kChunk, f.raw - (uint32_t)c * kChunk) % kAdlerMod);
    __shared__ uint32_t s[3][kLanes];
    s[0][threadIdx.x] = (uint32_t)A; s[1][threadIdx.x] = (uint32_t)B; s[2][threadIdx.x] = (uint32_t)L;
    __syncthreads();
    if (threadIdx.x == 0) {
        A = 0; B = 0; L = 0;
        for (int t = 0; t < kLanes; ++t) adler_append(A, B, L, s[0][t], s[1][t], s[2][t]);
        const uint32_t s1 = (uint32_t)((1 + A) % kAdlerMod), s2 = (uint32_t)((B + L) % kAdlerMod);
        const uint8_t *t = blob + f.in_off + min(res[4 * blockIdx.x + 2], (uint32_t)f.in_len - 4u);       // inside the stream, whatever the data
        const uint32_t trailer = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
        if ((s2 << 16 | s1) != trailer) atomicOr(&err[blockIdx.x], (uint32_t)inf::kErrAdler);
    }
}

// ---- unfilter and colour --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t load_pixel(const uint8_t *p, int bpp) {
    uint32_t v = p[0];
    if (bpp > 1) v |= (uint32_t)p[1] << 8;
    if (bpp > 2) v |= (uint32_t)p[2] << 16;
    if (bpp > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

// the reconstruction of one pixel (bpp bytes, packed) from the filtered bytes x, left a, above b, upper-left c (PNG specification
// 9.2 and 9.4): per byte, mod 256
__device__ __forceinline__ uint32_t reconstruct(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c, int bpp) {
    uint32_t r = 0;
    for (int k = 0; k < bpp; ++k) {
        const int xa = (a >> (8 * k)) & 255, xb = (b >> (8 * k)) & 255, xc = (c >> (8 * k)) & 255;
        int pred = 0;
        if (ft == 1) pred = xa;
        else if (ft == 2) pred = xb;
        else if (ft == 3) pred = (xa + xb) >> 1;
        else if (ft == 4) {
            const int pp = xa + xb - xc, pa = abs(pp - xa), pb = abs(pp - xb), pc = abs(pp - xc);
            pred = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        }
        r |= ((((x >> (8 * k)) & 255u) + (uint32_t)pred) & 255u) << (8 * k);
    }
    return r;
}

// one workgroup per file.  Lane r owns row band + r and takes pixel x = step - r: the pixel above was reconstructed by lane r - 1 one
// step earlier and comes through LDS; the last row of a band is written back in place for the first row of the next band.
__global__ __launch_bounds__(kLanes) void k_pd_unfilter(const uint8_t *__restrict__ blob, const PFile *__restrict__ files, char *__restrict__ scratch,
                                                         uint8_t *__restrict__ out, uint32_t *__restrict__ err) {
    const PFile f = files[blockIdx.x];
    __shared__ uint32_t above[2][kLanes];
    __shared__ uint32_t pal[256];
    const int r = threadIdx.x;
    if (f.ct == 3) {
        const uint8_t *P = blob + f.pal_off + 3 * r;
        pal[r] = (uint32_t)P[2] | (uint32_t)P[1] << 8 | (uint32_t)P[0] << 16;
    }
    __syncthreads();
    uint8_t *raw = (uint8_t *)(scratch + f.lit_off);
    uint8_t *O = out + f.out_off;
    const int bpp = f.bpp;
    bool bad = false;
    for (int band = 0; band < f.H; band += kLanes) {
        const int rows = min(kLanes, f.H - band), row = band + r;
        const bool mine = r < rows;
        uint8_t *line = raw + (int64_t)(mine ? row : band) * f.stride;
        int ft = mine ? line[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        uint32_t a = 0, c = 0;
        const int steps = f.W + rows - 1;
        for (int s = 0; s < steps; ++s) {
            const int x = s - r;
            if (mine && x >= 0 && x < f.W) {
                uint8_t *p = line + 1 + (int64_t)x * bpp;
                const uint32_t v = load_pixel(p, bpp);
                const uint32_t b = row == 0 ? 0u : r == 0 ? load_pixel(p - f.stride, bpp) : above[(s + 1) & 1][r - 1];
                const uint32_t px = reconstruct(ft, v, a, b, c, bpp);
                above[s & 1][r] = px;
                if (r == rows - 1 && band + rows < f.H) {
                    p[0] = (uint8_t)px;
                    if (bpp > 1) p[1] = (uint8_t)(px >> 8);
                    if (bpp > 2) p[2] = (uint8_t)(px >> 16);
                    if (bpp > 3) p[3] = (uint8_t)(px >> 24);
                }
                a = px; c = b;
                uint32_t bgr;
                if (f.ct == 3) bgr = pal[px & 255u];
                else if (f.ct == 0 || f.ct == 4) bgr = (px & 255u) * 0x010101u;
                else bgr = ((px >> 16) & 255u) | (px & 0xFF00u) | (px & 255u) << 16;
                uint8_t *q = O + ((int64_t)row * f.W + x) * 3;
                q[0] = (uint8_t)bgr; q[1] = (uint8_t)(bgr >> 8); q[2] = (uint8_t)(bgr >> 16);
            }
            __syncthreads();
        }
    }
    if (bad) atomicOr(&err[blockIdx.x], (uint32_t)inf::kErrFilter);
}

}  // namespace

extern "C" int csm_png_decode_desc_words(void) { return kDescWords; }

extern "C" size_t csm_png_decode_scratch_bytes(const int32_t *desc_host, int n) {
    Plan p;
    if (!make_plan(desc_host, n, 0, 0, false, p)) return 0;
    return (size_t)p.total;
}

extern "C" int csm_png_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                              void *scratch, int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && out && scratch && blob_bytes > 0 && out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    Plan p;
    if (!make_plan(desc_host, n, blob_bytes, out_bytes, true, p)) return CSM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *S = (char *)scratch;
    PFile *files = (PFile *)(S + p.o_files);
    int *flags = (int *)(S + p.o_flags);
    uint32_t *err = (uint32_t *)(S + p.o_err), *res = (uint32_t *)(S + p.o_res);
    // p.files is pageable host memory: the runtime stages such a copy before hipMemcpyAsync returns, so an early return below (a
    // failed launch check) may destroy p while the stream still runs
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(PFile), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemsetAsync(flags, 0, (size_t)(p.files[0].lit_off - p.o_flags), st));                   // flags, err, res
    k_pd_walk<<<n, 64, 0, st>>>(blob, files, S, res, err);
    int rc = csm::check_launch("k_pd_walk"); if (rc) return rc;
    const dim3 quad_grid(csm::cdiv(p.max_raw, 4 * kLanes), (unsigned)n);
    k_pd_identity<<<quad_grid, kLanes, 0, st>>>(files, S);
    rc = csm::check_launch("k_pd_identity"); if (rc) return rc;
    const unsigned match_blocks = std::min(1024u, std::max(1u, csm::cdiv(p.max_raw / 3, 4 * (kLanes / 16))));
    k_pd_match<<<dim3(match_blocks, (unsigned)n), kLanes, 0, st>>>(files, S, res);
    rc = csm::check_launch("k_pd_match"); if (rc) return rc;
    for (int r = 0; r < p.max_rounds; ++r) {
        k_pd_double<<<quad_grid, kLanes, 0, st>>>(files, S, flags, r);
        rc = csm::check_launch("k_pd_double"); if (rc) return rc;
    }
    k_pd_gather<<<dim3(csm::cdiv(p.max_raw, kChunk), (unsigned)n), kLanes, 0, st>>>(files, S);
    rc = csm::check_launch("k_pd_gather"); if (rc) return rc;
    k_pd_adler<<<n, kLanes, 0, st>>>(blob, files, S, res, err);
    rc = csm::check_launch("k_pd_adler"); if (rc) return rc;
    k_pd_unfilter<<<n, kLanes, 0, st>>>(blob, files, S, out, err);
    rc = csm::check_launch("k_pd_unfilter"); if (rc) return rc;
    std::vector<uint32_t> err_host(n);
    std::vector<int> flags_host((size_t)n * kFlagWords);
    CSM_HIP(hipMemcpyAsync(err_host.data(), err, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipMemcpyAsync(flags_host.data(), flags, flags_host.size() * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    if (info_host) {
        int used = 0;                                                   // doubling rounds that did work, over the files of the call
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < p.files[i].rounds; ++r)
                if (r == 0 || flags_host[(size_t)i * kFlagWords + r - 1]) used = std::max(used, r + 1);
        info_host[0] = p.max_rounds;
        info_host[1] = used;
    }
    for (int i = 0; i < n; ++i) {
        if (err_host[i]) {
            csm::set_error("png decode: file %d of the call has corrupt data (error word 0x%x: see csm_inflate.h)", i, err_host[i]);
            return CSM_ERR_DATA;
        }
    }
    return CSM_OK;
}
