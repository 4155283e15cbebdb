// mjpeg.hip -- baseline JPEG (ITU T.81 SOF0, JFIF) of uint8 BGR frames on the device, for gfx950: the frames of a Motion-JPEG
// AVI (cartoonsegmentation_amd/video.py).  The contract is fixed to the byte and restated in numpy in
// tests/mjpeg_restatement.py: JFIF colour conversion in 16 fractional bits, edge-replicated padding to whole MCUs, 4:2:0 chroma as
// (a + b + c + d + 2) >> 2, a 13-bit integer matrix DCT, the Annex K quantisation tables under the IJG quality rule, the Annex K
// Huffman tables, one interleaved scan, and a restart interval of ONE MCU ROW: every MCU row is a byte-aligned segment whose DC
// predictors start at 0, so the rows are independent on the device.
//
//   measure: k_jpeg_transform (colour, subsampling, DCT, quantisation, zigzag -> int16 coefficients, one wave per 8x8 block)
//            -> k_jpeg_rows<false> (one workgroup per MCU row: stuffed bytes of the row)
//            -> k_jpeg_row_offsets (one workgroup per frame: offsets of the rows, bytes of the frame)
//            -> k_jpeg_frame_offsets (one workgroup: info[f] = {offset, bytes})
//   write:   k_jpeg_rows<true> (the same row work again, now stored at its offset, plus the header, the RST markers and EOI)
//
// k_jpeg_rows per MCU row: bit length of each block -> scan -> assemble the bits -> count the FF bytes -> scan -> stuffed bytes.
// The bits of a row are assembled in LDS (worst case kBlockBytes per block: 83 KB for a 1024-wide 4:2:0 row) or, for rows whose
// worst case does not fit, in a slot of the scratch.  Threads OR whole 32-bit words into the zeroed buffer: integer ORs of disjoint
// bits, whose order cannot change a byte.  No float atomics, no grid-wide waits; the output is deterministic.
#include "csm_common.h"
#include "csm_bits.h"
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kBlockBytes = 216;             // worst case of one 8x8 block: 22 bits of DC + 63 * 26 bits of AC = 1660 bits < 216 B
constexpr int kHeaderBytes = 629;            // SOI 2, APP0 18, DQT 2 * 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int64_t kRowLdsMax = 156 * 1024;   // dynamic LDS of k_jpeg_rows (its static LDS is below 4 KB; 160 KB per workgroup)
constexpr int64_t kRowSlotBudget = 32 << 20; // scratch of the rows too wide for LDS: at most this much (or one row) per launch

// ---- Annex K ---------------------------------------------------------------------------------------------------------------
constexpr uint8_t kQuantLum[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQuantChr[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// kZigzag[i] = natural (row-major) index of the i-th coefficient of the scan
constexpr uint8_t kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Huffman codes by symbol (T.81 Annex C): code | length << 16, 0 = the symbol has no code
struct HuffLut { uint32_t e[256]; };
constexpr HuffLut make_lut(const uint8_t *bits, const uint8_t *vals) {
    HuffLut t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t.e[vals[k++]] = code++ | (unsigned)len << 16;
        code <<= 1;
    }
    return t;
}
// [0] luminance, [1] chrominance; only the 12 categories of the DC tables are used
struct HuffTables { uint32_t dc[2][12]; uint32_t ac[2][256]; };
constexpr HuffTables make_tables() {
    HuffTables t{};
    const HuffLut dl = make_lut(kDcLumBits, kDcVals), dch = make_lut(kDcChrBits, kDcVals);
    const HuffLut al = make_lut(kAcLumBits, kAcLumVals), ach = make_lut(kAcChrBits, kAcChrVals);
    for (int i = 0; i < 12; ++i) { t.dc[0][i] = dl.e[i]; t.dc[1][i] = dch.e[i]; }
    for (int i = 0; i < 256; ++i) { t.ac[0][i] = al.e[i]; t.ac[1][i] = ach.e[i]; }
    return t;
}
__device__ const HuffTables kHuff = make_tables();
// forward DCT matrix C[k][n] = round(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2
__device__ const int kDct[64] = {
    2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896,     4017, 3406, 2276, 799, -799, -2276, -3406, -4017,
    3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784, 3406, -799, -4017, -2276, 2276, 4017, 799, -3406,
    2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896, 2276, -4017, 799, 3406, -3406, -799, 4017, -2276,
    1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567, 799, -2276, 3406, -4017, 4017, -3406, 2276, -799};

// ---- geometry ---------------------------------------------------------------------------------------------------------------
struct Geo {
    int n, H, W;
    int mcu;           // MCU side in pixels: 16 (4:2:0) or 8 (4:4:4)
    int bpm;           // blocks per MCU: 6 or 3
    int mx, my;        // MCUs per row, MCU rows
    int bpr;           // blocks per MCU row
    int64_t units;     // MCU rows of all frames
};

bool make_geo(int n, int H, int W, int subsampling, Geo &g) {
    if (n < 0 || H < 1 || H > 65535 || W < 1 || W > 65535 || (subsampling != 420 && subsampling != 444)) return false;
    g.n = n; g.H = H; g.W = W;
    g.mcu = subsampling == 420 ? 16 : 8;
    g.bpm = subsampling == 420 ? 6 : 3;
    g.mx = (W + g.mcu - 1) / g.mcu;
    g.my = (H + g.mcu - 1) / g.mcu;
    g.bpr = g.mx * g.bpm;
    g.units = (int64_t)n * g.my;
    return true;
}

int64_t row_slot_bytes(const Geo &g) { return (int64_t)g.bpr * kBlockBytes; }
bool rows_in_lds(const Geo &g) { return row_slot_bytes(g) <= kRowLdsMax; }
int64_t units_per_launch(const Geo &g) {
    if (rows_in_lds(g)) return g.units;
    return std::max<int64_t>(1, std::min<int64_t>(g.units, kRowSlotBudget / row_slot_bytes(g)));
}

struct Scratch {
    int16_t *coef;         // [units][bpr][64], zigzag order
    int64_t *row_off;      // [units]: offset of the row's segment inside its frame
    int *row_bytes;        // [units]: stuffed bytes of the row, RST marker included
    uint32_t *slots;       // [units_per_launch][bpr * kBlockBytes / 4], only when the rows do not fit LDS
    int64_t total;
};

Scratch make_scratch(const Geo &g, void *base) {
    Scratch s;
    char *p = (char *)base;
    int64_t o = 0;
    s.coef = (int16_t *)(p + o);     o += csm::align16(g.units * g.bpr * 128);
    s.row_off = (int64_t *)(p + o);  o += csm::align16(g.units * 8);
    s.row_bytes = (int *)(p + o);    o += csm::align16(g.units * 4);
    s.slots = (uint32_t *)(p + o);   o += rows_in_lds(g) ? 0 : units_per_launch(g) * row_slot_bytes(g);
    s.total = o;
    return s;
}

struct QuantTables { uint8_t q[2][64]; uint8_t pos[64]; };   // natural order; [0] luminance, [1] chrominance; pos[natural index] = position in the scan
struct Header { uint8_t b[kHeaderBytes + 3]; };

// IJG jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)
QuantTables make_quant(int quality) {
    QuantTables t;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        t.q[0][i] = (uint8_t)std::min(255, std::max(1, (kQuantLum[i] * s + 50) / 100));
        t.q[1][i] = (uint8_t)std::min(255, std::max(1, (kQuantChr[i] * s + 50) / 100));
        t.pos[kZigzag[i]] = (uint8_t)i;
    }
    return t;
}

Header make_header(const Geo &g, const QuantTables &qt) {
    Header h;
    uint8_t *p = h.b;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (uint8_t)x; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int i = 0; i < 64; ++i) *p++ = qt.q[t][kZigzag[i]];
    }
    put({0xFF, 0xC0, 0, 17, 8, g.H >> 8, g.H & 255, g.W >> 8, g.W & 255, 3, 1, g.mcu == 16 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    const struct { int id; const uint8_t *bits, *vals; int nv; } dht[4] = {
        {0x00, kDcLumBits, kDcVals, 12}, {0x10, kAcLumBits, kAcLumVals, 162}, {0x01, kDcChrBits, kDcVals, 12}, {0x11, kAcChrBits, kAcChrVals, 162}};
    for (const auto &d : dht) {
        put({0xFF, 0xC4, (19 + d.nv) >> 8, (19 + d.nv) & 255, d.id});
        memcpy(p, d.bits, 16); p += 16;
        memcpy(p, d.vals, d.nv); p += d.nv;
    }
    put({0xFF, 0xDD, 0, 4, g.mx >> 8, g.mx & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return h;
}

// ---- transform pass ---------------------------------------------------------------------------------------------------------
struct Ycc { int y, cb, cr; };
__device__ __forceinline__ Ycc ycc_at(const uint8_t *__restrict__ F, int H, int W, int x, int y) {
    const uint8_t *p = F + ((int64_t)min(y, H - 1) * W + min(x, W - 1)) * 3;
    const int B = p[0], G = p[1], R = p[2];
    Ycc r;
    r.y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    r.cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    r.cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    return r;
}

// one wave per 8x8 block, four blocks per workgroup; lane = 8 * row + column of the block
__global__ __launch_bounds__(kBlock) void k_jpeg_transform(const uint8_t *__restrict__ frames, Geo g, QuantTables qt, int64_t blocks,
                                                            int16_t *__restrict__ coef) {
    __shared__ int sC[64];
    __shared__ int sA[4][64], sB[4][64];
    const int t = threadIdx.x, wv = t >> 6, l = t & 63;
    if (t < 64) sC[t] = kDct[t];
    const int64_t blk = (int64_t)blockIdx.x * 4 + wv;
    const bool live = blk < blocks;
    int comp = 0;
    if (live) {
        const int64_t unit = blk / g.bpr;
        const int bi = (int)(blk - unit * g.bpr), m = bi / g.bpm, b = bi - m * g.bpm;
        const int f = (int)(unit / g.my), r = (int)(unit - (int64_t)f * g.my);
        const uint8_t *F = frames + (int64_t)f * g.H * g.W * 3;
        const int y = l >> 3, x = l & 7;
        int s;
        if (g.bpm == 6 && b >= 4) {                   // 4:2:0 chroma: the mean of 2x2 converted samples
            comp = b - 3;
            const int px = m * 16 + 2 * x, py = r * 16 + 2 * y;
            const Ycc a = ycc_at(F, g.H, g.W, px, py), bb = ycc_at(F, g.H, g.W, px + 1, py);
            const Ycc c = ycc_at(F, g.H, g.W, px, py + 1), d = ycc_at(F, g.H, g.W, px + 1, py + 1);
            s = comp == 1 ? (a.cb + bb.cb + c.cb + d.cb + 2) >> 2 : (a.cr + bb.cr + c.cr + d.cr + 2) >> 2;
        } else {
            int px, py;
            if (g.bpm == 6) { px = m * 16 + (b & 1) * 8 + x; py = r * 16 + (b >> 1) * 8 + y; }
            else            { comp = b; px = m * 8 + x; py = r * 8 + y; }
            const Ycc a = ycc_at(F, g.H, g.W, px, py);
            s = comp == 0 ? a.y : comp == 1 ? a.cb : a.cr;
        }
        sA[wv][l] = s - 128;
    }
    __syncthreads();
    if (live) {                                       // row pass: lane (y, k)
        const int y = l >> 3, k = l & 7;
        int acc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += sC[k * 8 + i] * sA[wv][y * 8 + i];
        sB[wv][l] = (acc + 512) >> 10;
    }
    __syncthreads();
    if (live) {                                       // column pass: lane (v, u) = natural index l
        const int v = l >> 3, u = l & 7;
        int acc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += sC[v * 8 + i] * sB[wv][i * 8 + u];
        const int c = (acc + 32768) >> 16;
        const int Q = qt.q[comp ? 1 : 0][l];
        const int a = (abs(c) + (Q >> 1)) / Q;
        coef[blk * 64 + qt.pos[l]] = (int16_t)(c < 0 ? -a : a);
    }
}

// ---- segment pass -----------------------------------------------------------------------------------------------------------
// MSB-first bit writer into a zeroed buffer of 32-bit words (word w holds the stream's bytes 4w..4w+3, first byte on top).  A
// thread ORs each word it completes once; the words at its two ends are shared with its neighbours.
template <bool EMIT> struct BitSink {
    uint32_t *buf;
    uint32_t w, acc;
    int fill, bits;
    __device__ __forceinline__ void open(uint32_t *b, int pos) { buf = b; w = (uint32_t)pos >> 5; fill = pos & 31; acc = 0; bits = 0; }
    // the n low bits of v, 1 <= n <= 27
    __device__ __forceinline__ void put(uint32_t v, int n) {
        bits += n;
        if constexpr (EMIT) {
            const int space = 32 - fill;
            if (n < space) { acc |= v << (space - n); fill += n; }
            else {
                const int rem = n - space;
                atomicOr(buf + w, acc | (v >> rem));
                ++w;
                acc = rem ? v << (32 - rem) : 0u;
                fill = rem;
            }
        }
    }
    __device__ __forceinline__ void close() { if constexpr (EMIT) { if (fill) atomicOr(buf + w, acc); } }
};

__device__ __forceinline__ int bit_size(int a) { return 32 - __clz(a); }       // a >= 0

// the code of one block: c its 64 coefficients in scan order, pred the DC of the previous block of its component
template <bool EMIT> __device__ __forceinline__ void code_block(const int16_t *__restrict__ c, int pred, const uint32_t *dc,
                                                                 const uint32_t *ac, BitSink<EMIT> &sink) {
    const uint4 *q = (const uint4 *)c;
    uint64_t nz = 0;
    int dc0 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = q[i];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        if (i == 0) dc0 = (int)(int16_t)(v.x & 0xFFFF);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (w4[j] & 0xFFFFu) nz |= 1ull << (i * 8 + 2 * j);
            if (w4[j] >> 16)     nz |= 1ull << (i * 8 + 2 * j + 1);
        }
    }
    {
        const int d = dc0 - pred, size = bit_size(abs(d));
        const uint32_t e = dc[size];
        const uint32_t vb = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << size) - 1u);
        sink.put(((e & 0xFFFFu) << size) | vb, (int)(e >> 16) + size);
    }
    nz &= ~1ull;
    int last = 0;
    while (nz) {
        const int k = __ffsll((unsigned long long)nz) - 1;
        nz &= nz - 1;
        int run = k - last - 1;
        last = k;
        for (; run >= 16; run -= 16) sink.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
        const int v = c[k], size = bit_size(abs(v));
        const uint32_t e = ac[(run << 4) | size];
        const uint32_t vb = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        sink.put(((e & 0xFFFFu) << size) | vb, (int)(e >> 16) + size);
    }
    if (last != 63) sink.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

// index (in the row) of the previous block of the same component, -1 for the first
__device__ __forceinline__ int pred_block(int bi, int bpm) {
    if (bpm == 3) return bi - 3;
    const int b = bi % 6;
    if (b >= 4) return bi - 6;
    return b == 0 ? bi - 3 : bi - 1;                  // Y0 follows the previous MCU's Y3
}

// byte i of the assembled stream; a buffer in device memory was filled by atomics at the L2, so it is read past the L1
template <bool LDS> __device__ __forceinline__ uint32_t stream_byte(uint32_t *buf, int i) {
    const uint32_t w = LDS ? buf[i >> 2] : __hip_atomic_load(buf + (i >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (w >> (24 - 8 * (i & 3))) & 0xFFu;
}

// One workgroup per MCU row (unit0 + blockIdx.x).  WRITE = false: row_bytes[unit]; WRITE = true: the row's bytes at
// info[f][0] + row_off[unit] of out, never past the bytes measured for it, plus the frame's header (row 0) and EOI (last row).
template <bool WRITE, bool LDS>
__global__ __launch_bounds__(kBlock) void k_jpeg_rows(const int16_t *__restrict__ coef, Geo g, int64_t unit0, uint32_t *slots,
                                                       int slot_words, int *__restrict__ row_bytes, const int64_t *__restrict__ row_off,
                                                       const int64_t *__restrict__ info, Header hdr, uint8_t *__restrict__ out) {
    extern __shared__ uint32_t lds_bits[];
    __shared__ uint32_t sDc[2][12], sAc[2][256];
    __shared__ int sScan[kBlock];
    const int t = threadIdx.x;
    const int64_t unit = unit0 + blockIdx.x;
    const int f = (int)(unit / g.my), r = (int)(unit - (int64_t)f * g.my);
    const int16_t *C = coef + unit * g.bpr * 64;
    uint32_t *buf = LDS ? lds_bits : slots + (int64_t)blockIdx.x * slot_words;
    for (int i = t; i < 24; i += kBlock) sDc[i / 12][i % 12] = kHuff.dc[i / 12][i % 12];
    for (int i = t; i < 512; i += kBlock) sAc[i >> 8][i & 255] = kHuff.ac[i >> 8][i & 255];
    __syncthreads();

    // 1-2: bits of this thread's run of consecutive blocks, scanned
    const int per = (g.bpr + kBlock - 1) / kBlock, b0 = min(g.bpr, t * per), b1 = min(g.bpr, b0 + per);
    int mybits = 0;
    for (int bi = b0; bi < b1; ++bi) {
        const int chroma = g.bpm == 3 ? bi % 3 != 0 : bi % 6 >= 4, pb = pred_block(bi, g.bpm);
        BitSink<false> len;
        len.open(nullptr, 0);
        code_block<false>(C + (int64_t)bi * 64, pb >= 0 ? C[(int64_t)pb * 64] : 0, sDc[chroma], sAc[chroma], len);
        mybits += len.bits;
    }
    int total_bits;
    const int start = csm_bits::block_exclusive<kBlock>(mybits, sScan, total_bits);
    const int nbytes = (total_bits + 7) >> 3, nwords = (nbytes + 3) >> 2;
    if (nwords > slot_words) return;                  // cannot happen (kBlockBytes is the worst case); never write past the buffer

    // 3: assemble
    for (int i = t; i < nwords; i += kBlock) buf[i] = 0;
    __syncthreads();
    {
        BitSink<true> sink;
        sink.open(buf, start);
        for (int bi = b0; bi < b1; ++bi) {
            const int chroma = g.bpm == 3 ? bi % 3 != 0 : bi % 6 >= 4, pb = pred_block(bi, g.bpm);
            code_block<true>(C + (int64_t)bi * 64, pb >= 0 ? C[(int64_t)pb * 64] : 0, sDc[chroma], sAc[chroma], sink);
        }
        sink.close();
    }
    if (t == 0 && (total_bits & 7)) {                 // pad the last byte with 1-bits
        const int pad = 8 - (total_bits & 7), off = total_bits & 31;
        atomicOr(buf + (total_bits >> 5), ((1u << pad) - 1u) << (32 - off - pad));
    }
    __syncthreads();

    // 4-5: FF bytes of this thread's run of consecutive bytes, scanned
    const int bper = (nbytes + kBlock - 1) / kBlock, i0 = min(nbytes, t * bper), i1 = min(nbytes, i0 + bper);
    int ff = 0;
    for (int i = i0; i < i1; ++i) ff += stream_byte<LDS>(buf, i) == 0xFFu;
    int total_ff;
    const int ff_before = csm_bits::block_exclusive<kBlock>(ff, sScan, total_ff);
    const bool last_row = r == g.my - 1;
    const int seg = nbytes + total_ff + (last_row ? 0 : 2);
    if constexpr (!WRITE) {
        if (t == 0) row_bytes[unit] = seg;
    } else {
        // 6: stuffed bytes, the marker after them, and the frame's header and EOI
        uint8_t *O = out + info[2 * f];
        const int64_t base = row_off[unit], end = base + row_bytes[unit];
        int64_t pos = base + i0 + ff_before;
        for (int i = i0; i < i1; ++i) {
            const uint32_t v = stream_byte<LDS>(buf, i);
            if (pos < end) O[pos] = (uint8_t)v;
            ++pos;
            if (v == 0xFFu) { if (pos < end) O[pos] = 0; ++pos; }
        }
        if (t == 0 && seg == row_bytes[unit]) {
            if (last_row) { O[end] = 0xFF; O[end + 1] = 0xD9; }
            else          { O[end - 2] = 0xFF; O[end - 1] = (uint8_t)(0xD0 + (r & 7)); }
        }
        if (r == 0) for (int i = t; i < kHeaderBytes; i += kBlock) O[i] = hdr.b[i];
    }
}

// one workgroup per frame: row_off[unit] = header + bytes of the rows before it; frame_bytes[f] = header + rows + EOI
__global__ __launch_bounds__(kBlock) void k_jpeg_row_offsets(int my, const int *__restrict__ row_bytes, int64_t *__restrict__ row_off,
                                                              int64_t *__restrict__ info) {
    __shared__ int64_t sScan[kBlock];
    const int f = blockIdx.x, t = threadIdx.x;
    const int per = (my + kBlock - 1) / kBlock, r0 = min(my, t * per), r1 = min(my, r0 + per);
    const int *B = row_bytes + (int64_t)f * my;
    int64_t *O = row_off + (int64_t)f * my;
    int64_t sum = 0, total;
    for (int r = r0; r < r1; ++r) sum += B[r];
    int64_t ex = kHeaderBytes + csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int r = r0; r < r1; ++r) { O[r] = ex; ex += B[r]; }
    if (t == 0) info[2 * f + 1] = kHeaderBytes + total + 2;
}

// one workgroup: info[f][0] = sum of info[k][1] over k < f
__global__ __launch_bounds__(kBlock) void k_jpeg_frame_offsets(int n, int64_t *__restrict__ info) {
    __shared__ int64_t sh[kBlock];
    const int t = threadIdx.x;
    const int per = (n + kBlock - 1) / kBlock, f0 = min(n, t * per), f1 = min(n, f0 + per);
    int64_t sum = 0, total;
    for (int f = f0; f < f1; ++f) sum += info[2 * f + 1];
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sh, total);
    for (int f = f0; f < f1; ++f) { info[2 * f] = ex; ex += info[2 * f + 1]; }
}

template <bool WRITE>
int launch_rows(const Geo &g, const Scratch &sc, const int64_t *info, const Header &hdr, uint8_t *out, hipStream_t st) {
    const bool lds = rows_in_lds(g);
    const int slot_words = (int)(row_slot_bytes(g) / 4);
    const size_t dyn = lds ? (size_t)row_slot_bytes(g) : 0;
    if (lds && dyn > 48 * 1024) {
        CSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_jpeg_rows<WRITE, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)kRowLdsMax));
    }
    const int64_t step = units_per_launch(g);
    for (int64_t u0 = 0; u0 < g.units; u0 += step) {
        const unsigned grid = (unsigned)std::min<int64_t>(step, g.units - u0);
        if (lds) k_jpeg_rows<WRITE, true><<<grid, kBlock, dyn, st>>>(sc.coef, g, u0, nullptr, slot_words, sc.row_bytes, sc.row_off, info, hdr, out);
        else     k_jpeg_rows<WRITE, false><<<grid, kBlock, 0, st>>>(sc.coef, g, u0, sc.slots, slot_words, sc.row_bytes, sc.row_off, info, hdr, out);
        const int rc = csm::check_launch("k_jpeg_rows");
        if (rc) return rc;
    }
    return CSM_OK;
}

}  // namespace

extern "C" size_t csm_jpeg_scratch_bytes(int n, int H, int W, int subsampling) {
    Geo g;
    if (!make_geo(n, H, W, subsampling, g)) return 0;
    return (size_t)make_scratch(g, nullptr).total;
}

extern "C" int csm_jpeg_header_bytes(void) { return kHeaderBytes; }

extern "C" int csm_jpeg_measure(const uint8_t *frames, int n, int H, int W, int quality, int subsampling, int64_t *info, void *scratch,
                                void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, subsampling, g));
    CSM_REQUIRE(quality >= 1 && quality <= 100);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(frames && info && scratch);
    const int64_t blocks = g.units * g.bpr;
    CSM_REQUIRE(blocks / 4 < INT32_MAX && g.units < INT32_MAX);
    const Scratch sc = make_scratch(g, scratch);
    const QuantTables qt = make_quant(quality);
    const Header hdr = make_header(g, qt);
    hipStream_t st = (hipStream_t)stream;
    k_jpeg_transform<<<csm::cdiv(blocks, 4), kBlock, 0, st>>>(frames, g, qt, blocks, sc.coef);
    int rc = csm::check_launch("k_jpeg_transform"); if (rc) return rc;
    rc = launch_rows<false>(g, sc, info, hdr, nullptr, st); if (rc) return rc;
    k_jpeg_row_offsets<<<n, kBlock, 0, st>>>(g.my, sc.row_bytes, sc.row_off, info);
    rc = csm::check_launch("k_jpeg_row_offsets"); if (rc) return rc;
    k_jpeg_frame_offsets<<<1, kBlock, 0, st>>>(n, info);
    return csm::check_launch("k_jpeg_frame_offsets");
}

extern "C" int csm_jpeg_write(int n, int H, int W, int quality, int subsampling, const int64_t *info, uint8_t *out, void *scratch,
                              void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, subsampling, g));
    CSM_REQUIRE(quality >= 1 && quality <= 100);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(info && out && scratch && g.units < INT32_MAX);
    const Scratch sc = make_scratch(g, scratch);
    const Header hdr = make_header(g, make_quant(quality));
    return launch_rows<true>(g, sc, info, hdr, out, (hipStream_t)stream);
}
