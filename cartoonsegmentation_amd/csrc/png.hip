// png.hip -- the zlib stream (RFC 1950 / 1951) of a PNG's IDAT chunk, from uint8 images on the device, for gfx950.  The contract
// is fixed to the byte and restated in numpy in tests/png_restatement.py: per-scanline choice among the five PNG
// filters by the smallest sum of min(r, 256 - r), a parse into runs of equal bytes that never cross a scanline (a literal, then
// distance-1 matches), ONE deflate block per image whose code the host builds from the image's 286-entry histogram, and the
// Adler-32 of the filtered bytes.  Signature, IHDR, chunk lengths and CRCs are host work (ops.png_encode).
//
//   measure: k_png_filter (one workgroup per scanline: the five filter sums, the chosen filter's bytes to scratch, the row's
//                          Adler partial)
//            -> k_png_parse<kHist> (one workgroup per scanline: symbol counts in LDS, then integer adds into the image's table)
//            -> k_png_adler (one workgroup per image: the Adler-32 from the row partials, and the one end-of-block symbol)
//   write:   k_png_parse<kBits> (bits of every scanline under the host's code) -> k_png_row_offsets (one workgroup per image)
//            -> k_png_parse<kEmit> (every scanline's bits at its bit offset, the block header with row 0, the end-of-block
//                                   symbol and the Adler-32 with the last row)
//
// No row is ever staged in LDS: the kernels stream a scanline from global memory (its second reading comes from the L2), so
// there is one path for every width.  Deflate packs bits LSB-first; the host hands the Huffman codes over already bit-reversed.
// Threads OR whole 32-bit words into the zeroed output: integer ORs of disjoint bits, whose order cannot change a byte.  No float
// atomics, no grid-wide waits, no allocation, no sync; the output is deterministic.
#include "csm_common.h"
#include "csm_bits.h"

namespace {

using csm_bits::BitSink;
using csm_bits::parse_chunk;

constexpr int kBlock = 256;                  // threads of every workgroup: the size csm_bits.h's helpers are instantiated for
constexpr uint32_t kAdlerMod = 65521;
constexpr int kSyms = 286;                   // literal / length alphabet
constexpr int kEob = 256;
constexpr int kMaxMatch = 258;
constexpr int kMeasureWords = 288;           // device table per image: 286 counts, the Adler-32, one spare
// host table per image (uint32 words)
constexpr int kTabWords = 384;
constexpr int kTabHdrBits = 286;             // bits before the first scanline's symbols: zlib header + block header
constexpr int kTabAdler = 287;
constexpr int kTabOffLo = 288, kTabOffHi = 289;   // byte offset of the stream in the blob (a multiple of 4)
constexpr int kTabDistBits = 290;            // bits of the distance code of every match (all zero): 1 dynamic, 5 fixed
constexpr int kTabBytes = 291;               // bytes of the stream
constexpr int kTabHdr = 292;                 // the header bits, LSB-first, at most 92 words
constexpr int kHdrWordsMax = kTabWords - kTabHdr;

enum { kHist = 0, kBits = 1, kEmit = 2 };

struct Geo {
    int n, H, W, C;
    int Wb;            // raw bytes of a scanline
    int L;             // filtered bytes of a scanline: the type byte + Wb
    int swap;          // colour: memory is B, G, R (written as R, G, B)
    int mask;          // grey: any non-zero byte is written as 255
    int64_t units;     // scanlines of all images
};

bool make_geo(int n, int H, int W, int C, int flags, Geo &g) {
    if (n < 0 || H < 1 || H > 65535 || W < 1 || W > 65535 || (C != 1 && C != 3)) return false;
    g.n = n; g.H = H; g.W = W; g.C = C;
    g.Wb = W * C;
    g.L = g.Wb + 1;
    g.swap = (C == 3) && (flags & 1);
    g.mask = (C == 1) && (flags & 2);
    g.units = (int64_t)n * H;
    // the counts of one image are 32-bit, and one grid of kBlock threads per scanline covers the batch
    return (int64_t)H * g.L < INT32_MAX && g.units < (1 << 24);
}

struct Scratch {
    uint8_t *filt;         // [units][L]: filtered scanlines
    int64_t *row_off;      // [units]: bit offset of the scanline's symbols behind the block header
    uint32_t *row_bits;    // [units]
    uint32_t *ad_a, *ad_b; // [units]: Adler partials of the scanline from (0, 0)
    int64_t total;
};

Scratch make_scratch(const Geo &g, void *base) {
    Scratch s;
    char *p = (char *)base;
    int64_t o = 0;
    s.filt = (uint8_t *)(p + o);      o += csm::align16(g.units * g.L);
    s.row_off = (int64_t *)(p + o);   o += csm::align16(g.units * 8);
    s.row_bits = (uint32_t *)(p + o); o += csm::align16(g.units * 4);
    s.ad_a = (uint32_t *)(p + o);     o += csm::align16(g.units * 4);
    s.ad_b = (uint32_t *)(p + o);     o += csm::align16(g.units * 4);
    s.total = o;
    return s;
}

// ---- filter pass ------------------------------------------------------------------------------------------------------------
// byte j of a raw scanline as the file holds it (R, G, B; masks as 0 / 255); j < 0 is left of the first pixel
__device__ __forceinline__ int raw_byte(const uint8_t *__restrict__ row, int j, const Geo &g) {
    if (j < 0 || !row) return 0;
    if (g.C == 3) {
        if (!g.swap) return row[j];
        const int p = j / 3, ch = j - 3 * p;
        return row[3 * p + 2 - ch];
    }
    const int v = row[j];
    return g.mask ? (v ? 255 : 0) : v;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int cost(int r) { r &= 255; return min(r, 256 - r); }

// one workgroup per scanline
__global__ __launch_bounds__(kBlock) void k_png_filter(const uint8_t *__restrict__ images, Geo g, uint8_t *__restrict__ filt,
                                                        uint32_t *__restrict__ ad_a, uint32_t *__restrict__ ad_b) {
    __shared__ int sInt[kBlock];
    __shared__ unsigned long long sLong[kBlock];
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int r = (int)(unit % g.H);
    const uint8_t *cur = images + unit * g.Wb;              // the images are contiguous: scanline `unit` of the batch
    const uint8_t *up = r ? cur - g.Wb : nullptr;
    int s[5] = {0, 0, 0, 0, 0};
    for (int j = t; j < g.Wb; j += kBlock) {
        const int x = raw_byte(cur, j, g), a = raw_byte(cur, j - g.C, g), b = raw_byte(up, j, g), c = raw_byte(up, j - g.C, g);
        s[0] += cost(x);
        s[1] += cost(x - a);
        s[2] += cost(x - b);
        s[3] += cost(x - ((a + b) >> 1));
        s[4] += cost(x - paeth(a, b, c));
    }
    int type = 0, best = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int v = csm_bits::block_sum<kBlock>(s[k], sInt);
        if (k == 0 || v < best) { best = v; type = k; }      // ties go to the lowest type
    }
    uint8_t *F = filt + unit * g.L;
    // Adler partial from (0, 0): A = sum of the bytes, B = sum of (L - i) * byte i
    unsigned long long A = 0, B = 0;
    if (t == 0) { F[0] = (uint8_t)type; A = (unsigned)type; B = (unsigned long long)g.L * (unsigned)type; }
    for (int j = t; j < g.Wb; j += kBlock) {
        const int x = raw_byte(cur, j, g);
        int v = x;
        if (type == 1) v = x - raw_byte(cur, j - g.C, g);
        else if (type == 2) v = x - raw_byte(up, j, g);
        else if (type == 3) v = x - ((raw_byte(cur, j - g.C, g) + raw_byte(up, j, g)) >> 1);
        else if (type == 4) v = x - paeth(raw_byte(cur, j - g.C, g), raw_byte(up, j, g), raw_byte(up, j - g.C, g));
        v &= 255;
        F[1 + j] = (uint8_t)v;
        A += (unsigned)v;
        B += (unsigned long long)(g.L - 1 - j) * (unsigned)v;
    }
    A = csm_bits::block_sum<kBlock>(A, sLong);
    B = csm_bits::block_sum<kBlock>(B, sLong);
    if (t == 0) { ad_a[unit] = (uint32_t)(A % kAdlerMod); ad_b[unit] = (uint32_t)(B % kAdlerMod); }
}

// one workgroup per image: the Adler-32 of its H scanlines of L bytes from their partials.  From (s1, s2) a scanline with the
// partial (A, B) leads to (s1 + A, s2 + L * s1 + B); from (1, 0) that sums to s1 = 1 + sum A_k and
// s2 = sum B_k + L * H + L * sum A_k * (H - 1 - k), all mod 65521.  It also counts the one end-of-block symbol.
__global__ __launch_bounds__(kBlock) void k_png_adler(Geo g, const uint32_t *__restrict__ ad_a, const uint32_t *__restrict__ ad_b,
                                                       uint32_t *__restrict__ table) {
    __shared__ unsigned long long sLong[kBlock];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint32_t *A = ad_a + (int64_t)f * g.H, *B = ad_b + (int64_t)f * g.H;
    unsigned long long sa = 0, sb = 0, sw = 0;
    for (int k = t; k < g.H; k += kBlock) {
        sa += A[k];
        sb += B[k];
        sw += (unsigned long long)A[k] * (unsigned)(g.H - 1 - k) % kAdlerMod;
    }
    sa = csm_bits::block_sum<kBlock>(sa, sLong);
    sb = csm_bits::block_sum<kBlock>(sb, sLong);
    sw = csm_bits::block_sum<kBlock>(sw, sLong);
    if (t == 0) {
        const unsigned long long Lm = (unsigned)g.L % kAdlerMod;
        const unsigned long long s1 = (1 + sa) % kAdlerMod;
        const unsigned long long s2 = (sb % kAdlerMod + Lm * (unsigned)g.H % kAdlerMod + Lm * (sw % kAdlerMod) % kAdlerMod) % kAdlerMod;
        uint32_t *T = table + (int64_t)f * kMeasureWords;
        T[kEob] = 1;
        T[286] = (uint32_t)(s2 << 16 | s1);
        T[287] = 0;
    }
}

// ---- parse ------------------------------------------------------------------------------------------------------------------
// length 3..258 -> symbol | extra bits << 16 | extra value << 24 (RFC 1951 §3.2.5)
__device__ __forceinline__ uint32_t length_entry(int len) {
    if (len == kMaxMatch) return 285u;
    const int m = len - 3;                                 // 0..254
    if (m < 8) return 257u + m;
    const int e = 29 - __clz(m);                           // extra bits: 1 for 8..15, 2 for 16..31, ... 5 for 128..254
    const int sym = 261 + 4 * e + ((m >> e) & 3);
    return (uint32_t)sym | (uint32_t)e << 16 | (uint32_t)(m & ((1 << e) - 1)) << 24;
}

// what one run of `len` equal bytes v costs or emits: the literal, (len - 1) / 258 matches of 258, then one match of the
// remainder if that is 3 or more, else the remainder as literals.  code[s] = reversed code | length << 16.
template <int MODE> struct RunSink {
    uint32_t *hist;            // kHist: LDS counts
    const uint32_t *code;      // kBits, kEmit: LDS
    int dist_bits;
    unsigned bits;             // kBits
    BitSink sink;              // kEmit
    __device__ __forceinline__ void symbol(int s, int times) {
        if constexpr (MODE == kHist) atomicAdd(hist + s, (uint32_t)times);
        else if constexpr (MODE == kBits) bits += (code[s] >> 16) * times;
        else { const uint32_t e = code[s]; for (int k = 0; k < times; ++k) sink.put(e & 0xFFFFu, (int)(e >> 16)); }
    }
    __device__ __forceinline__ void match(int len, int times) {
        const uint32_t le = length_entry(len);
        const int s = (int)(le & 0xFFFFu), eb = (int)(le >> 16) & 0xFF;
        if constexpr (MODE == kHist) atomicAdd(hist + s, (uint32_t)times);
        else if constexpr (MODE == kBits) bits += ((code[s] >> 16) + eb + dist_bits) * times;
        else {
            const uint32_t e = code[s];
            const int cl = (int)(e >> 16);
            // code, extra bits of the length, the all-zero distance code: at most 15 + 5 + 5 bits
            const uint32_t v = (e & 0xFFFFu) | (le >> 24) << cl;
            for (int k = 0; k < times; ++k) sink.put(v, cl + eb + dist_bits);
        }
    }
    __device__ __forceinline__ void run(int v, int len) {
        const int R = len - 1, q = R / kMaxMatch, rem = R - q * kMaxMatch;
        symbol(v, 1);
        if (q) match(kMaxMatch, q);
        if (rem >= 3) match(rem, 1);
        else if (rem) symbol(v, rem);
    }
};

// One workgroup per scanline.  Every thread takes a stretch of consecutive bytes and the runs that start there.
//   kHist: counts into table[f][0..285] (device table of the measure call)
//   kBits: row_bits[unit] under the code of host[f]
//   kEmit: the bits at host[f].offset, bit host[f].hdr_bits + row_off[unit]; row 0 adds the header, the last row the
//          end-of-block symbol and the Adler-32
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_png_parse(const uint8_t *__restrict__ filt, Geo g, uint32_t *__restrict__ table,
                                                       const uint32_t *__restrict__ host, uint32_t *__restrict__ row_bits,
                                                       const int64_t *__restrict__ row_off, uint8_t *__restrict__ out) {
    __shared__ uint32_t sTab[kSyms];                        // kHist: counts; otherwise the code
    __shared__ int sScan[kBlock];
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int f = (int)(unit / g.H), r = (int)(unit - (int64_t)f * g.H);
    const uint8_t *F = filt + unit * g.L;
    const uint32_t *T = MODE == kHist ? nullptr : host + (int64_t)f * kTabWords;
    for (int i = t; i < kSyms; i += kBlock) sTab[i] = MODE == kHist ? 0u : T[i];

    const csm_bits::RunStretch my = csm_bits::run_stretch<kBlock>(F, g.L, sScan);   // (its barriers also publish sTab)

    RunSink<MODE> rs;
    rs.hist = sTab; rs.code = sTab; rs.bits = 0;
    rs.dist_bits = MODE == kHist ? 0 : (int)T[kTabDistBits];
    if constexpr (MODE == kHist) {
        parse_chunk(F, my, rs);
        __syncthreads();
        uint32_t *G = table + (int64_t)f * kMeasureWords;
        for (int i = t; i < kSyms; i += kBlock) if (sTab[i]) atomicAdd(G + i, sTab[i]);
    } else {
        {
            RunSink<kBits> len;
            len.hist = nullptr; len.code = sTab; len.bits = 0; len.dist_bits = rs.dist_bits;
            parse_chunk(F, my, len);
            rs.bits = len.bits;
        }
        int total;
        const int start = csm_bits::block_exclusive<kBlock>((int)rs.bits, sScan, total);
        if constexpr (MODE == kBits) {
            if (t == 0) row_bits[unit] = (uint32_t)total;
        } else {
            const int64_t off = (int64_t)T[kTabOffLo] | (int64_t)T[kTabOffHi] << 32;
            const int64_t limit = ((int64_t)T[kTabBytes] + 3) >> 2;
            uint32_t *O = (uint32_t *)(out + off);
            const int64_t base = (int64_t)T[kTabHdrBits] + row_off[unit];
            rs.sink.open(O, base + start, limit);
            parse_chunk(F, my, rs);
            rs.sink.close();
            if (r == 0) {
                const int hw = min(kHdrWordsMax, ((int)T[kTabHdrBits] + 31) >> 5);
                for (int i = t; i < hw; i += kBlock) if (T[kTabHdr + i] && i < limit) atomicOr(O + i, T[kTabHdr + i]);
            }
            if (r == g.H - 1 && t == 0) {
                BitSink tail;
                tail.open(O, base + total, limit);
                tail.put(sTab[kEob] & 0xFFFFu, (int)(sTab[kEob] >> 16));
                if (tail.fill & 7) tail.put(0, 8 - (tail.fill & 7));
                const uint32_t ad = T[kTabAdler];
                tail.put((ad >> 24) | (ad >> 8 & 0xFF00u) | (ad << 8 & 0xFF0000u) | ad << 24, 32);   // big-endian
                tail.close();
            }
        }
    }
}

// one workgroup per image: row_off[unit] = bits of the image's scanlines before it
__global__ __launch_bounds__(kBlock) void k_png_row_offsets(int H, const uint32_t *__restrict__ row_bits, int64_t *__restrict__ row_off) {
    __shared__ int64_t sScan[kBlock];
    const int f = blockIdx.x, t = threadIdx.x;
    const int per = (H + kBlock - 1) / kBlock, r0 = min(H, t * per), r1 = min(H, r0 + per);
    const uint32_t *B = row_bits + (int64_t)f * H;
    int64_t *O = row_off + (int64_t)f * H;
    int64_t sum = 0, total;
    for (int r = r0; r < r1; ++r) sum += B[r];
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int r = r0; r < r1; ++r) { O[r] = ex; ex += B[r]; }
}

}  // namespace

extern "C" size_t csm_png_scratch_bytes(int n, int H, int W, int channels) {
    Geo g;
    if (!make_geo(n, H, W, channels, 0, g)) return 0;
    return (size_t)make_scratch(g, nullptr).total;
}

extern "C" int csm_png_table_words(void) { return kTabWords; }

extern "C" int csm_png_measure(const uint8_t *images, int n, int H, int W, int channels, int flags, uint32_t *table, void *scratch,
                               void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, channels, flags, g));
    CSM_REQUIRE((flags & ~3) == 0);
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(images && table && scratch);
    const Scratch sc = make_scratch(g, scratch);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(table, 0, (size_t)n * kMeasureWords * 4, st));
    k_png_filter<<<(unsigned)g.units, kBlock, 0, st>>>(images, g, sc.filt, sc.ad_a, sc.ad_b);
    int rc = csm::check_launch("k_png_filter"); if (rc) return rc;
    k_png_parse<kHist><<<(unsigned)g.units, kBlock, 0, st>>>(sc.filt, g, table, nullptr, nullptr, nullptr, nullptr);
    rc = csm::check_launch("k_png_parse<hist>"); if (rc) return rc;
    k_png_adler<<<n, kBlock, 0, st>>>(g, sc.ad_a, sc.ad_b, table);
    return csm::check_launch("k_png_adler");
}

extern "C" int csm_png_write(int n, int H, int W, int channels, const uint32_t *host_table, uint8_t *out, int64_t out_bytes,
                             void *scratch, void *stream) {
    Geo g;
    CSM_REQUIRE(make_geo(n, H, W, channels, 0, g));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(host_table && out && scratch && out_bytes > 0 && out_bytes % 4 == 0 && ((uintptr_t)out & 3) == 0);
    const Scratch sc = make_scratch(g, scratch);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(out, 0, (size_t)out_bytes, st));
    k_png_parse<kBits><<<(unsigned)g.units, kBlock, 0, st>>>(sc.filt, g, nullptr, host_table, sc.row_bits, nullptr, nullptr);
    int rc = csm::check_launch("k_png_parse<bits>"); if (rc) return rc;
    k_png_row_offsets<<<n, kBlock, 0, st>>>(g.H, sc.row_bits, sc.row_off);
    rc = csm::check_launch("k_png_row_offsets"); if (rc) return rc;
    k_png_parse<kEmit><<<(unsigned)g.units, kBlock, 0, st>>>(sc.filt, g, nullptr, host_table, nullptr, sc.row_off, out);
    return csm::check_launch("k_png_parse<emit>");
}
