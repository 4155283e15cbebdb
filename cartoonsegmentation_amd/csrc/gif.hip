// gif.hip -- the device half of the GIF writer, for gfx950: one 256-colour palette for a whole clip (a histogram over 15-bit colour
// cells, then an exact nearest-colour search per pixel with an ordered dither) and the LZW stream of every frame (variable-width
// codes, LSB-first).  The contract is fixed to the byte and restated in numpy in tests/gif_restatement.py.  The
// median cut over the cell table, the sub-block framing and the container are host work (gifcode.py).
//
//   histogram: k_gif_hist (a workgroup takes 8192 pixels; counts and low-bit sums of the cells it meets in an LDS table of 4096
//                          slots, one packed 64-bit add per pixel, then integer adds into the global table)
//   map:       k_gif_map (one thread per pixel, the palette in LDS, 256 distances; the lowest index on ties)
//   measure:   k_gif_lzw (one segment of 3839 pixels per wave: greedy LZW from a Clear, codes as uint16 to scratch)
//              -> k_gif_offsets (one workgroup per frame: bit offset of every segment, the frame's bytes)
//              -> k_gif_frame_offsets (one workgroup: byte offset of every frame's stream in the blob)
//   write:     k_gif_pack (one workgroup per segment, 16 codes per thread: the Clear, the codes, the EOI at their bit offsets)
//
// Why a wave per segment and not a lane: LZW is serial in its pixels, so one lane does the walk either way, but the dictionary of a
// lane-per-segment kernel (32 KB each) would live in global memory and every probe would be a dependent global load; a wave keeps
// its dictionary and its pixels in LDS, where a probe costs an LDS round trip, and its 64 lanes clear the table and fetch the pixels
// together.  A workgroup is ONE wave (36.5 KB of LDS, four to a CU) rather than two that share nothing.
// A segment's widths follow from its code count alone: after a Clear the width is 9, and code k (from 0) is written at
// 9 + (k >= 255) + (k >= 767) + (k >= 1791).  So offsets need no serial pass and every code's bit position has a closed form.
// Threads OR whole 32-bit words into the zeroed output: integer ORs of disjoint bits, whose order cannot change a byte.  No float
// atomics, no grid-wide waits, no allocation, no sync; the output is deterministic.
#include "csm_common.h"
#include "csm_bits.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSeg = 3839;                   // pixels of a segment: 257 + kSeg = 4096, the dictionary cannot overflow
constexpr int kSegStride = 3840;             // uint16 codes of a segment in scratch
constexpr int kClear = 256, kEoi = 257;
constexpr int kSlots = 8192;                 // dictionary slots: at most kSeg - 1 = 3838 are ever taken, so a probe always ends
constexpr int kCells = 32768;
constexpr int kHistSlots = 4096;
constexpr int kHistPixels = 8192;            // per workgroup: 7 * 8192 < 65536, so the four packed 16-bit fields cannot carry
constexpr int kPerThread = 16;               // codes a thread of k_gif_pack writes
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

__constant__ uint8_t cBayer[64] = {0, 32, 8, 40, 2, 34, 10, 42, 48, 16, 56, 24, 50, 18, 58, 26, 12, 44, 4, 36, 14, 46, 6, 38,
                                   60, 28, 52, 20, 62, 30, 54, 22, 3, 35, 11, 43, 1, 33, 9, 41, 51, 19, 59, 27, 49, 17, 57, 25,
                                   15, 47, 7, 39, 13, 45, 5, 37, 63, 31, 55, 23, 61, 29, 53, 21};

struct Geo {
    int n, H, W;
    int64_t px;        // pixels of a frame
    int nseg;          // segments of a frame
    int64_t units;     // segments of all frames
};

bool make_geo(int n, int H, int W, Geo &g) {
    if (n < 0 || H < 1 || H > 65535 || W < 1 || W > 65535) return false;
    g.n = n; g.H = H; g.W = W;
    g.px = (int64_t)H * W;
    g.nseg = (int)((g.px + kSeg - 1) / kSeg);
    g.units = (int64_t)n * g.nseg;
    return g.units < (1 << 24);               // one workgroup per segment covers the batch
}

struct Scratch {
    uint16_t *codes;       // [units][kSegStride]
    uint32_t *count;       // [units]: codes of the segment
    int64_t *seg_off;      // [units]: bit offset of the segment's Clear in its frame's stream
    int64_t *frame_bytes;  // [n]
    int64_t *frame_off;    // [n]: byte offset of the frame's stream in the blob (a multiple of 4)
    int64_t total;
};

Scratch make_scratch(const Geo &g, void *base) {
    Scratch s;
    char *p = (char *)base;
    int64_t o = 0;
    s.codes = (uint16_t *)(p + o);      o += csm::align16(g.units * kSegStride * 2);
    s.count = (uint32_t *)(p + o);      o += csm::align16(g.units * 4);
    s.seg_off = (int64_t *)(p + o);     o += csm::align16(g.units * 8);
    s.frame_bytes = (int64_t *)(p + o); o += csm::align16((int64_t)g.n * 8);
    s.frame_off = (int64_t *)(p + o);   o += csm::align16((int64_t)g.n * 8);
    s.total = o;
    return s;
}

// width in force after m codes of a segment (the decoder's extra entry behind the last code counted), m >= 0; also the width
// code m (from 0) is written at
__device__ __forceinline__ int width_after(int m) { return 9 + (m >= 255) + (m >= 767) + (m >= 1791); }

// bits of the first m codes of a segment
__device__ __forceinline__ int code_bits(int m) {
    return 9 * min(m, 255) + 10 * min(max(m - 255, 0), 512) + 11 * min(max(m - 767, 0), 1024) + 12 * max(m - 1791, 0);
}

// ---- palette: histogram and mapping -----------------------------------------------------------------------------------------
// table[cell][4] += count, sum of r & 7, g & 7, b & 7 over the workgroup's pixels.  A cell claims an LDS slot by compare-and-swap
// on its hash; a pixel whose slot another cell holds adds to the global table directly.  Integer adds only: any order, one result.
__global__ __launch_bounds__(kBlock) void k_gif_hist(const uint8_t *__restrict__ frames, int64_t pixels, int swap,
                                                      uint32_t *__restrict__ table) {
    __shared__ uint32_t sKey[kHistSlots];
    __shared__ unsigned long long sVal[kHistSlots];
    const int t = threadIdx.x;
    for (int i = t; i < kHistSlots; i += kBlock) { sKey[i] = kNoCell; sVal[i] = 0; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kHistPixels;
    for (int k = 0; k < kHistPixels / kBlock; ++k) {
        const int64_t p = base + k * kBlock + t;
        if (p >= pixels) break;
        const uint8_t *q = frames + 3 * p;
        const uint32_t c0 = q[0], g = q[1], c2 = q[2];
        const uint32_t r = swap ? c2 : c0, b = swap ? c0 : c2;
        const uint32_t cell = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3);
        const uint32_t slot = (cell * 2654435761u) >> 20;
        const uint32_t old = atomicCAS(&sKey[slot], kNoCell, cell);
        if (old == kNoCell || old == cell) {
            atomicAdd(&sVal[slot], 1ull | (unsigned long long)(r & 7) << 16 | (unsigned long long)(g & 7) << 32 |
                                        (unsigned long long)(b & 7) << 48);
        } else {
            uint32_t *T = table + 4 * cell;
            atomicAdd(T, 1u);
            if (r & 7) atomicAdd(T + 1, r & 7);
            if (g & 7) atomicAdd(T + 2, g & 7);
            if (b & 7) atomicAdd(T + 3, b & 7);
        }
    }
    __syncthreads();
    for (int i = t; i < kHistSlots; i += kBlock) {
        const uint32_t cell = sKey[i];
        if (cell == kNoCell) continue;
        const unsigned long long v = sVal[i];
        uint32_t *T = table + 4 * cell;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t a = (uint32_t)(v >> (16 * c)) & 0xFFFFu;
            if (a) atomicAdd(T + c, a);
        }
    }
}

// one thread per pixel.  A pixel that equals a palette entry takes it (the lowest such index); otherwise the nearest entry of the
// pixel as it is, or with the Bayer offset (cBayer[y & 7][x & 7] >> 3) - 4 added to each channel and clamped.
__global__ __launch_bounds__(kBlock) void k_gif_map(const uint8_t *__restrict__ frames, int64_t pixels, int H, int W, int swap,
                                                     int dither, const uint8_t *__restrict__ palette, uint8_t *__restrict__ indices) {
    __shared__ int sR[256], sG[256], sB[256];
    const int t = threadIdx.x;
    sR[t] = palette[3 * t]; sG[t] = palette[3 * t + 1]; sB[t] = palette[3 * t + 2];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kBlock + t;
    if (p >= pixels) return;
    const uint8_t *q = frames + 3 * p;
    const int c0 = q[0], g = q[1], c2 = q[2];
    const int r = swap ? c2 : c0, b = swap ? c0 : c2;
    int off = 0;
    if (dither) {
        const int x = (int)(p % W), y = (int)((p / W) % H);
        off = (cBayer[(y & 7) * 8 + (x & 7)] >> 3) - 4;
    }
    const int r2 = min(max(r + off, 0), 255), g2 = min(max(g + off, 0), 255), b2 = min(max(b + off, 0), 255);
    int best = INT32_MAX, bi = 0, best2 = INT32_MAX, bi2 = 0;
    for (int j = 0; j < 256; ++j) {
        const int pr = sR[j], pg = sG[j], pb = sB[j];
        const int d = (r - pr) * (r - pr) + (g - pg) * (g - pg) + (b - pb) * (b - pb);
        const int d2 = (r2 - pr) * (r2 - pr) + (g2 - pg) * (g2 - pg) + (b2 - pb) * (b2 - pb);
        if (d < best) { best = d; bi = j; }
        if (d2 < best2) { best2 = d2; bi2 = j; }
    }
    indices[p] = (uint8_t)(best == 0 ? bi : bi2);
}

// ---- LZW --------------------------------------------------------------------------------------------------------------------
// One wave per segment.  The lanes fetch the segment's pixels into LDS and clear the dictionary; lane 0 walks the pixels.  A slot
// holds (prefix code << 8 | byte) << 12 | code, 0 = free (a code is at least 258); linear probing from a multiplicative hash.
__global__ __launch_bounds__(64) void k_gif_lzw(const uint8_t *__restrict__ indices, Geo g, uint16_t *__restrict__ codes,
                                                 uint32_t *__restrict__ count) {
    __shared__ uint32_t sTab[kSlots];
    __shared__ uint8_t sPix[kSegStride];
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int f = (int)(unit / g.nseg), k = (int)(unit - (int64_t)f * g.nseg);
    const int64_t p0 = (int64_t)k * kSeg;
    const int len = (int)min((int64_t)kSeg, g.px - p0);
    const uint8_t *src = indices + (int64_t)f * g.px + p0;
    for (int i = t; i < len; i += 64) sPix[i] = src[i];
    for (int i = t; i < kSlots; i += 64) sTab[i] = 0;
    __syncthreads();
    if (t != 0) return;
    uint16_t *out = codes + unit * kSegStride;
    uint32_t prefix = sPix[0], next = 258;
    int m = 0;
    for (int i = 1; i < len; ++i) {
        const uint32_t c = sPix[i], key = prefix << 8 | c;
        uint32_t h = (key * 2654435761u) >> 19;
        for (;;) {
            const uint32_t e = sTab[h];
            if (e == 0) {                                      // not in the dictionary: the prefix goes out, the pair comes in
                out[m++] = (uint16_t)prefix;
                sTab[h] = key << 12 | next;
                ++next;
                prefix = c;
                break;
            }
            if ((e >> 12) == key) { prefix = e & 0xFFFu; break; }
            h = (h + 1) & (kSlots - 1);
        }
    }
    out[m++] = (uint16_t)prefix;
    count[unit] = (uint32_t)m;
}

// one workgroup per frame: segment k's Clear is written at the width segment k - 1 ended with (9 for the first), so its bits are
// that width plus its codes'; seg_off = the bits of the segments before it; the EOI goes behind the last at the width in force.
__global__ __launch_bounds__(kBlock) void k_gif_offsets(Geo g, const uint32_t *__restrict__ count, int64_t *__restrict__ seg_off,
                                                         int64_t *__restrict__ frame_bytes, int64_t *__restrict__ bytes_out) {
    __shared__ int64_t sScan[kBlock];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint32_t *C = count + (int64_t)f * g.nseg;
    int64_t *O = seg_off + (int64_t)f * g.nseg;
    const int per = (g.nseg + kBlock - 1) / kBlock, k0 = min(g.nseg, t * per), k1 = min(g.nseg, k0 + per);
    int64_t sum = 0, total;
    for (int k = k0; k < k1; ++k) sum += (k ? width_after((int)C[k - 1]) : 9) + code_bits((int)C[k]);
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int k = k0; k < k1; ++k) { O[k] = ex; ex += (k ? width_after((int)C[k - 1]) : 9) + code_bits((int)C[k]); }
    if (t == 0) {
        const int64_t b = (total + width_after((int)C[g.nseg - 1]) + 7) >> 3;
        frame_bytes[f] = b;
        bytes_out[f] = b;
    }
}

// one workgroup: frame_off[f] = the bytes, each rounded up to 4, of the frames before f
__global__ __launch_bounds__(kBlock) void k_gif_frame_offsets(int n, const int64_t *__restrict__ frame_bytes,
                                                               int64_t *__restrict__ frame_off) {
    __shared__ int64_t sScan[kBlock];
    const int t = threadIdx.x;
    const int per = (n + kBlock - 1) / kBlock, f0 = min(n, t * per), f1 = min(n, f0 + per);
    int64_t sum = 0, total;
    for (int f = f0; f < f1; ++f) sum += (frame_bytes[f] + 3) & ~(int64_t)3;
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int f = f0; f < f1; ++f) { frame_off[f] = ex; ex += (frame_bytes[f] + 3) & ~(int64_t)3; }
}

// one workgroup per segment; thread t writes codes [16 t, 16 t + 16), thread 0 the Clear before them, and the thread that holds
// the last code of a frame's last segment the EOI behind it
__global__ __launch_bounds__(kBlock) void k_gif_pack(Geo g, const uint16_t *__restrict__ codes, const uint32_t *__restrict__ count,
                                                      const int64_t *__restrict__ seg_off, const int64_t *__restrict__ frame_bytes,
                                                      const int64_t *__restrict__ frame_off, uint8_t *__restrict__ out,
                                                      int64_t out_bytes) {
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int f = (int)(unit / g.nseg), k = (int)(unit - (int64_t)f * g.nseg);
    const int m = (int)min(count[unit], (uint32_t)kSeg);
    const int j0 = t * kPerThread, j1 = min(m, j0 + kPerThread);
    if (j0 >= m) return;                                       // m >= 1: thread 0 always stays
    const int w0 = k ? width_after((int)count[unit - 1]) : 9;
    const int64_t off = frame_off[f];
    const int64_t limit = min(off + ((frame_bytes[f] + 3) & ~(int64_t)3), out_bytes) >> 2;
    const uint16_t *C = codes + unit * kSegStride;
    csm_bits::BitSink sink;
    sink.open((uint32_t *)out, off * 8 + seg_off[unit] + (t ? w0 + code_bits(j0) : 0), limit);
    if (t == 0) sink.put(kClear, w0);
    for (int j = j0; j < j1; ++j) sink.put(C[j], width_after(j));
    if (k == g.nseg - 1 && j1 == m) sink.put(kEoi, width_after(m));
    sink.close();
}

}  // namespace

extern "C" size_t csm_gif_scratch_bytes(int n, int H, int W) {
    Geo g;
    if (!make_geo(n, H, W, g)) return 0;
    return (size_t)make_scratch(g, nullptr).total;
}

extern "C" int csm_gif_histogram(const uint8_t *frames, int64_t pixels, int flags, uint32_t *table, void *stream) {
    CSM_REQUIRE(pixels >= 0 && pixels < ((int64_t)1 << 29) && (flags & ~1) == 0 && table);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(table, 0, (size_t)kCells * 16, st));
    if (pixels == 0) return CSM_OK;
    CSM_REQUIRE(frames);
    k_gif_hist<<<csm::cdiv(pixels, kHistPixels), kBlock, 0, st>>>(frames, pixels, flags & 1, table);
    return csm::check_launch("k_gif_hist");
}

extern "C" int csm_gif_map(const uint8_t *frames, int n, int H, int W, int flags, const uint8_t *palette, uint8_t *indices,
                           void *stream) {
    CSM_REQUIRE(n >= 0 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && (flags & ~3) == 0);
    const int64_t pixels = (int64_t)n * H * W;
    CSM_REQUIRE(pixels < ((int64_t)1 << 38));                 // one grid of kBlock threads per workgroup covers the clip
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(frames && palette && indices);
    k_gif_map<<<csm::cdiv(pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(frames, pixels, H, W, flags & 1, (flags >> 1) & 1,
                                                                             palette, indices);
    return csm::check_launch("k_gif_map");
}

extern "C" int csm_gif_measure(const uint8_t *indices, int n, int H, int W, int64_t *bytes, void *scratch, void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, g));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(indices && bytes && scratch);
    const Scratch sc = make_scratch(g, scratch);
    hipStream_t st = (hipStream_t)stream;
    k_gif_lzw<<<(unsigned)g.units, 64, 0, st>>>(indices, g, sc.codes, sc.count);
    int rc = csm::check_launch("k_gif_lzw"); if (rc) return rc;
    k_gif_offsets<<<n, kBlock, 0, st>>>(g, sc.count, sc.seg_off, sc.frame_bytes, bytes);
    rc = csm::check_launch("k_gif_offsets"); if (rc) return rc;
    k_gif_frame_offsets<<<1, kBlock, 0, st>>>(n, sc.frame_bytes, sc.frame_off);
    return csm::check_launch("k_gif_frame_offsets");
}

extern "C" int csm_gif_write(int n, int H, int W, uint8_t *out, int64_t out_bytes, void *scratch, void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, g));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(out && scratch && out_bytes > 0 && out_bytes % 4 == 0 && ((uintptr_t)out & 3) == 0);
    const Scratch sc = make_scratch(g, scratch);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(out, 0, (size_t)out_bytes, st));
    k_gif_pack<<<(unsigned)g.units, kBlock, 0, st>>>(g, sc.codes, sc.count, sc.seg_off, sc.frame_bytes, sc.frame_off, out, out_bytes);
    return csm::check_launch("k_gif_pack");
}
