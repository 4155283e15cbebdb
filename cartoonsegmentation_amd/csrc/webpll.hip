// webpll.hip -- the VP8L payload of a lossless WebP file, from uint8 images on the device, for gfx950.  The contract is fixed to
// the byte and restated in numpy in tests/webpll_restatement.py: subtract-green, the predictor transform with
// one mode per 16 x 16 block (the mode 0..12 with the smallest sum of min(r, 256 - r) over the block's residual bytes), a parse of
// every row into runs of equal ARGB pixels (four literals, then distance-1 references of up to 4096), and ONE group of five prefix
// codes per plane, which the host builds from the plane's histograms.  An image has two planes: the mode image of the predictor
// transform and the residual image; both go through the same parse and coder.  Images of different sizes and channel counts
// share a call through the descriptor table.  The RIFF container is host work (webpcode.lossless_file).
//
//   measure: k_ll_predict (one workgroup per 16 x 16 block: the 13 sums, the mode, the block's residual pixels to scratch)
//            -> k_ll_parse<kHist> (one workgroup per row of a plane: counts in LDS, then integer adds into the plane's table)
//   write:   k_ll_parse<kBits> (bits of every row under the host's codes) -> k_ll_row_offsets (one workgroup per plane)
//            -> k_ll_parse<kEmit> (every row's bits at its bit offset; a plane's first row adds the header bits in front of it)
//
// Coding is lossless, so every prediction reads input pixels: no pass waits for another pixel's result.  VP8L packs bits
// LSB-first; the host hands the prefix codes over bit-reversed.  Threads OR whole 32-bit words into the zeroed output: integer ORs
// of disjoint bits, whose order cannot change a byte.  No float atomics, no grid-wide waits, no allocation, no sync.
#include "csm_common.h"
#include "csm_bits.h"

namespace {

using csm_bits::BitSink;
using csm_bits::parse_chunk;

constexpr int kBlock = 256;                              // threads of every workgroup: the size csm_bits.h's helpers are instantiated for
constexpr int kBlkBits = 4, kBlk = 1 << kBlkBits;        // kBlk * kBlk == kBlock: one thread per pixel of a block
constexpr int kModes = 13;
constexpr int kMaxRef = 4096;
constexpr int kMaxSide = 16384;
constexpr int kSyms = 1088;                              // green + 24 length prefixes, red, blue, alpha, 40 distance prefixes
constexpr int kGreen = 0, kRed = 280, kBlue = 536, kAlpha = 792, kDist = 1048;
constexpr int kDistLeft = kDist + 1;                     // plane code 2, "the pixel to the left": prefix symbol 1, no extra bits
// host table per plane (uint32 words)
constexpr int kTabWords = 1352;
constexpr int kTabOffLo = 1088, kTabOffHi = 1089;        // byte offset of the image's payload in the blob (a multiple of 4)
constexpr int kTabBytes = 1090;                          // bytes of the payload
constexpr int kTabStartLo = 1091, kTabStartHi = 1092;    // the bit at which the plane's pixels begin
constexpr int kTabHdrWord = 1093, kTabHdrCount = 1094;   // first word and number of words of the header bits in front of them
constexpr int kTabHdr = 1095;                            // those words, shifted onto the payload's word grid
constexpr int kHdrWordsMax = 256;
static_assert(kTabHdr + kHdrWordsMax <= kTabWords, "table row");
// descriptor per image (int64 words)
constexpr int kDescWords = 8;
enum { dPtr = 0, dH = 1, dW = 2, dChan = 3, dPix = 4, dBlk = 5, dUnit = 6 };

enum { kHist = 0, kBits = 1, kEmit = 2 };

struct Plan {
    int64_t pixels, blocks, units;       // of all images: residual pixels, 16 x 16 blocks, rows of both planes
    uint32_t *res;                       // [pixels] residual ARGB
    uint32_t *modes;                     // [blocks] mode image ARGB
    uint32_t *row_bits;                  // [units]
    int64_t *row_off;                    // [units] bit offset of the row behind the first bit of its plane's pixels
    int64_t total;
};

// checks every descriptor; fill: writes the derived words [4..6]; otherwise they must hold what fill would write
bool make_plan(int64_t *desc, int n, bool fill, void *base, Plan &p) {
    if (n < 0 || (n > 0 && !desc)) return false;
    int64_t pix = 0, blk = 0, unit = 0;
    for (int i = 0; i < n; ++i) {
        int64_t *d = desc + (int64_t)i * kDescWords;
        const int64_t H = d[dH], W = d[dW], C = d[dChan] & 255, flags = d[dChan] >> 8;
        if (!d[dPtr] || H < 1 || H > kMaxSide || W < 1 || W > kMaxSide || (C != 1 && C != 3 && C != 4)) return false;
        if (flags & ~(int64_t)1 || (flags && C != 1)) return false;
        if (fill) { d[dPix] = pix; d[dBlk] = blk; d[dUnit] = unit; d[7] = 0; }
        else if (d[dPix] != pix || d[dBlk] != blk || d[dUnit] != unit) return false;
        const int64_t hb = (H + kBlk - 1) >> kBlkBits, wb = (W + kBlk - 1) >> kBlkBits;
        pix += H * W; blk += hb * wb; unit += hb + H;
    }
    if (blk >= INT32_MAX || unit >= INT32_MAX) return false;      // one workgroup per block, one per row
    p.pixels = pix; p.blocks = blk; p.units = unit;
    char *b = (char *)base;
    int64_t o = 0;
    p.res = (uint32_t *)(b + o);      o += csm::align16(pix * 4);
    p.modes = (uint32_t *)(b + o);    o += csm::align16(blk * 4);
    p.row_bits = (uint32_t *)(b + o); o += csm::align16(unit * 4);
    p.row_off = (int64_t *)(b + o);   o += csm::align16(unit * 8);
    p.total = o;
    return true;
}

// the image whose first block / row unit (desc word `field`) is the last one not above u
__device__ __forceinline__ int find_image(const int64_t *__restrict__ desc, int n, int field, int64_t u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * kDescWords + field] <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- predictor pass -----------------------------------------------------------------------------------------------------------
struct Img {
    const uint8_t *p;
    int H, W, C, mask;
};

__device__ __forceinline__ Img load_img(const int64_t *__restrict__ d) {
    Img im;
    im.p = (const uint8_t *)(uintptr_t)d[dPtr];
    im.H = (int)d[dH]; im.W = (int)d[dW]; im.C = (int)(d[dChan] & 255); im.mask = (int)(d[dChan] >> 8) & 1;
    return im;
}

// pixel (y, x) as A << 24 | R << 16 | G << 8 | B after subtract-green; memory is grey, B G R or B G R A
__device__ __forceinline__ uint32_t load_px(const Img &im, int y, int x) {
    const uint8_t *q = im.p + ((int64_t)y * im.W + x) * im.C;
    if (im.C == 1) {
        uint32_t g = q[0];
        if (im.mask) g = g ? 255u : 0u;
        return 0xff000000u | g << 8;                         // red - green and blue - green are 0
    }
    const uint32_t b = q[0], g = q[1], r = q[2], a = im.C == 4 ? q[3] : 255u;
    return a << 24 | ((r - g) & 255u) << 16 | g << 8 | ((b - g) & 255u);
}

__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }

// a - b per channel, mod 256
__device__ __forceinline__ uint32_t sub_px(uint32_t a, uint32_t b) {
    const uint32_t ag = 0x00ff00ffu + (a & 0xff00ff00u) - (b & 0xff00ff00u);
    const uint32_t rb = 0xff00ff00u + (a & 0x00ff00ffu) - (b & 0x00ff00ffu);
    return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}

__device__ __forceinline__ int chan(uint32_t v, int k) { return (int)(v >> (8 * k)) & 255; }

__device__ __forceinline__ int cost_px(uint32_t r) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int c = chan(r, k); s += min(c, 256 - c); }
    return s;
}

__device__ __forceinline__ uint32_t select_px(uint32_t L, uint32_t T, uint32_t TL) {
    int dl = 0, dt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { dl += abs(chan(L, k) - chan(TL, k)); dt += abs(chan(T, k) - chan(TL, k)); }
    return dt < dl ? L : T;
}

__device__ __forceinline__ uint32_t clamp_add_sub(uint32_t L, uint32_t T, uint32_t TL) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) out |= (uint32_t)min(255, max(0, chan(L, k) + chan(T, k) - chan(TL, k))) << (8 * k);
    return out;
}

__device__ __forceinline__ uint32_t predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
    case 0: return 0xff000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return avg2(avg2(L, TR), T);
    case 6: return avg2(L, TL);
    case 7: return avg2(L, T);
    case 8: return avg2(TL, T);
    case 9: return avg2(T, TR);
    case 10: return avg2(avg2(L, TL), avg2(T, TR));
    case 11: return select_px(L, T, TL);
    default: return clamp_add_sub(L, T, TL);
    }
}

// one workgroup per 16 x 16 block, one thread per pixel
__global__ __launch_bounds__(kBlock) void k_ll_predict(const int64_t *__restrict__ desc, int n, uint32_t *__restrict__ res,
                                                        uint32_t *__restrict__ modes) {
    __shared__ int sCost[kModes];
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int64_t *d = desc + (int64_t)find_image(desc, n, dBlk, unit) * kDescWords;
    const Img im = load_img(d);
    const int wb = (im.W + kBlk - 1) >> kBlkBits;
    const int b = (int)(unit - d[dBlk]), by = b / wb, bx = b - by * wb;
    const int y = by * kBlk + (t >> kBlkBits), x = bx * kBlk + (t & (kBlk - 1));
    const bool inside = y < im.H && x < im.W, inner = inside && y > 0 && x > 0;
    if (t < kModes) sCost[t] = 0;
    __syncthreads();
    uint32_t px = 0, L = 0, T = 0, TL = 0, TR = 0;
    if (inside) {
        px = load_px(im, y, x);
        if (x > 0) L = load_px(im, y, x - 1);
        if (y > 0) T = load_px(im, y - 1, x);
    }
    if (inner) {
        TL = load_px(im, y - 1, x - 1);
        TR = x + 1 < im.W ? load_px(im, y - 1, x + 1) : load_px(im, y, 0);   // behind the last column: the row's first pixel
#pragma unroll
        for (int m = 0; m < kModes; ++m) {
            const int c = cost_px(sub_px(px, predict(m, L, T, TL, TR)));
            if (c) atomicAdd(sCost + m, c);
        }
    }
    __syncthreads();
    int best = 0, low = sCost[0];
#pragma unroll
    for (int m = 1; m < kModes; ++m) {
        const int c = sCost[m];
        if (c < low) { low = c; best = m; }                  // ties go to the lowest mode
    }
    if (inside) {
        // the format's border rules override the mode: (0, 0) from opaque black, row 0 from L, column 0 from T
        const uint32_t pred = inner ? predict(best, L, T, TL, TR) : (y == 0 ? (x == 0 ? 0xff000000u : L) : T);
        res[d[dPix] + (int64_t)y * im.W + x] = sub_px(px, pred);
    }
    if (t == 0) modes[unit] = 0xff000000u | (uint32_t)best << 8;
}

// ---- parse ------------------------------------------------------------------------------------------------------------------
// length 1..4096 -> prefix symbol | extra bits << 8 | extra value << 16
__device__ __forceinline__ uint32_t length_entry(int len) {
    const int v = len - 1;
    if (v < 4) return (uint32_t)v;
    const int hb = 31 - __clz(v), eb = hb - 1;
    return (uint32_t)(2 * hb + ((v >> eb) & 1)) | (uint32_t)eb << 8 | (uint32_t)(v & ((1 << eb) - 1)) << 16;
}

// what one run of `len` equal pixels v costs or emits: four literals, (len - 1) / 4096 references of 4096, then one reference of
// the remainder if there is one.  code[s] = reversed code | length << 16; a length of 0 (the one symbol of a simple code) costs
// and writes nothing.
template <int MODE> struct RunSink {
    uint32_t *hist;            // kHist: LDS counts
    const uint32_t *code;      // kBits, kEmit: LDS
    unsigned bits;             // kBits
    BitSink sink;              // kEmit
    __device__ __forceinline__ void symbol(int s) {
        if constexpr (MODE == kHist) atomicAdd(hist + s, 1u);
        else if constexpr (MODE == kBits) bits += code[s] >> 16;
        else { const uint32_t e = code[s]; sink.put(e & 0xFFFFu, (int)(e >> 16)); }
    }
    __device__ __forceinline__ void reference(int len, int times) {
        const uint32_t le = length_entry(len);
        const int s = kGreen + 256 + (int)(le & 255u), eb = (int)(le >> 8) & 255;
        if constexpr (MODE == kHist) { atomicAdd(hist + s, (uint32_t)times); atomicAdd(hist + kDistLeft, (uint32_t)times); }
        else if constexpr (MODE == kBits) bits += ((code[s] >> 16) + eb + (code[kDistLeft] >> 16)) * times;
        else {
            const uint32_t e = code[s], dc = code[kDistLeft];
            const int cl = (int)(e >> 16);
            const uint32_t v = (e & 0xFFFFu) | (le >> 16) << cl;         // the code, then the extra bits: at most 15 + 10 bits
            for (int k = 0; k < times; ++k) { sink.put(v, cl + eb); sink.put(dc & 0xFFFFu, (int)(dc >> 16)); }
        }
    }
    __device__ __forceinline__ void run(uint32_t v, int len) {
        symbol(kGreen + (int)(v >> 8 & 255u));
        symbol(kRed + (int)(v >> 16 & 255u));
        symbol(kBlue + (int)(v & 255u));
        symbol(kAlpha + (int)(v >> 24));
        const int R = len - 1, q = R / kMaxRef, rem = R - q * kMaxRef;
        if (q) reference(kMaxRef, q);
        if (rem) reference(rem, 1);
    }
};

// One workgroup per row of a plane.  Every thread takes a stretch of consecutive pixels and the runs that start there.
//   kHist: counts into table[plane][0..1087] (device table of the measure call)
//   kBits: row_bits[unit] under the codes of host[plane]
//   kEmit: the bits at host[plane]'s offset, bit start + row_off[unit]; the plane's first row adds the header words
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_ll_parse(const int64_t *__restrict__ desc, int n, const uint32_t *__restrict__ res,
                                                      const uint32_t *__restrict__ modes, uint32_t *__restrict__ table,
                                                      const uint32_t *__restrict__ host, uint32_t *__restrict__ row_bits,
                                                      const int64_t *__restrict__ row_off, uint8_t *__restrict__ out, int64_t out_bytes) {
    __shared__ uint32_t sTab[kSyms];                        // kHist: counts; otherwise the codes
    __shared__ int sScan[kBlock];
    const int t = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int f = find_image(desc, n, dUnit, unit);
    const int64_t *d = desc + (int64_t)f * kDescWords;
    const int H = (int)d[dH], W = (int)d[dW];
    const int hb = (H + kBlk - 1) >> kBlkBits, wb = (W + kBlk - 1) >> kBlkBits;
    const int r = (int)(unit - d[dUnit]);
    const int plane = r >= hb, row = plane ? r - hb : r, L = plane ? W : wb;
    const uint32_t *F = plane ? res + d[dPix] + (int64_t)row * W : modes + d[dBlk] + (int64_t)row * wb;
    const int64_t pl = 2 * (int64_t)f + plane;
    const uint32_t *T = MODE == kHist ? nullptr : host + pl * kTabWords;
    for (int i = t; i < kSyms; i += kBlock) sTab[i] = MODE == kHist ? 0u : T[i];

    const csm_bits::RunStretch my = csm_bits::run_stretch<kBlock>(F, L, sScan);     // (its barriers also publish sTab)

    RunSink<MODE> rs;
    rs.hist = sTab; rs.code = sTab; rs.bits = 0;
    if constexpr (MODE == kHist) {
        parse_chunk(F, my, rs);
        __syncthreads();
        uint32_t *G = table + pl * kSyms;
        for (int i = t; i < kSyms; i += kBlock) if (sTab[i]) atomicAdd(G + i, sTab[i]);
    } else {
        {
            RunSink<kBits> len;
            len.hist = nullptr; len.code = sTab; len.bits = 0;
            parse_chunk(F, my, len);
            rs.bits = len.bits;
        }
        int total;
        const int start = csm_bits::block_exclusive<kBlock>((int)rs.bits, sScan, total);
        if constexpr (MODE == kBits) {
            if (t == 0) row_bits[unit] = (uint32_t)total;
        } else {
            const int64_t off = (int64_t)T[kTabOffLo] | (int64_t)T[kTabOffHi] << 32;
            // words of the payload, and never past the blob whatever the table says
            const int64_t limit = off < 0 || off > out_bytes ? 0 : min(((int64_t)T[kTabBytes] + 3) >> 2, (out_bytes - off) >> 2);
            uint32_t *O = (uint32_t *)(out + off);
            const int64_t base = ((int64_t)T[kTabStartLo] | (int64_t)T[kTabStartHi] << 32) + row_off[unit];
            rs.sink.open(O, base + start, limit);
            parse_chunk(F, my, rs);
            rs.sink.close();
            if (row == 0) {
                const int64_t w0 = T[kTabHdrWord];
                const int hw = min(kHdrWordsMax, (int)T[kTabHdrCount]);
                for (int i = t; i < hw; i += kBlock) if (T[kTabHdr + i] && w0 + i < limit) atomicOr(O + w0 + i, T[kTabHdr + i]);
            }
        }
    }
}

// one workgroup per plane: row_off[unit] = bits of the plane's rows before it
__global__ __launch_bounds__(kBlock) void k_ll_row_offsets(const int64_t *__restrict__ desc, const uint32_t *__restrict__ row_bits,
                                                            int64_t *__restrict__ row_off) {
    __shared__ int64_t sScan[kBlock];
    const int f = blockIdx.x >> 1, plane = blockIdx.x & 1, t = threadIdx.x;
    const int64_t *d = desc + (int64_t)f * kDescWords;
    const int H = (int)d[dH], hb = (H + kBlk - 1) >> kBlkBits;
    const int rows = plane ? H : hb;
    const int64_t u0 = d[dUnit] + (plane ? hb : 0);
    const int per = (rows + kBlock - 1) / kBlock, r0 = min(rows, t * per), r1 = min(rows, r0 + per);
    const uint32_t *B = row_bits + u0;
    int64_t *O = row_off + u0;
    int64_t sum = 0, total;
    for (int r = r0; r < r1; ++r) sum += B[r];
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sScan, total);
    for (int r = r0; r < r1; ++r) { O[r] = ex; ex += B[r]; }
}

}  // namespace

extern "C" int csm_webpll_desc_words(void) { return kDescWords; }
extern "C" int csm_webpll_measure_words(void) { return kSyms; }
extern "C" int csm_webpll_table_words(void) { return kTabWords; }

extern "C" size_t csm_webpll_plan(int64_t *desc_host, int n) {
    Plan p;
    if (n < 1 || !make_plan(desc_host, n, true, nullptr, p)) return 0;
    return (size_t)p.total;
}

extern "C" int csm_webpll_measure(const int64_t *desc_host, const int64_t *desc_dev, int n, uint32_t *table, void *scratch,
                                  void *stream) {
    Plan p;
    CSM_REQUIRE(make_plan(const_cast<int64_t *>(desc_host), n, false, scratch, p));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(desc_dev && table && scratch);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(table, 0, (size_t)n * 2 * kSyms * 4, st));
    k_ll_predict<<<(unsigned)p.blocks, kBlock, 0, st>>>(desc_dev, n, p.res, p.modes);
    int rc = csm::check_launch("k_ll_predict"); if (rc) return rc;
    k_ll_parse<kHist><<<(unsigned)p.units, kBlock, 0, st>>>(desc_dev, n, p.res, p.modes, table, nullptr, nullptr, nullptr, nullptr, 0);
    return csm::check_launch("k_ll_parse<hist>");
}

extern "C" int csm_webpll_write(const int64_t *desc_host, const int64_t *desc_dev, int n, const uint32_t *host_table, uint8_t *out,
                                int64_t out_bytes, void *scratch, void *stream) {
    Plan p;
    CSM_REQUIRE(make_plan(const_cast<int64_t *>(desc_host), n, false, scratch, p));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(desc_dev && host_table && out && scratch && out_bytes > 0 && out_bytes % 4 == 0 && ((uintptr_t)out & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    CSM_HIP(hipMemsetAsync(out, 0, (size_t)out_bytes, st));
    k_ll_parse<kBits><<<(unsigned)p.units, kBlock, 0, st>>>(desc_dev, n, p.res, p.modes, nullptr, host_table, p.row_bits, nullptr, nullptr, 0);
    int rc = csm::check_launch("k_ll_parse<bits>"); if (rc) return rc;
    k_ll_row_offsets<<<2 * n, kBlock, 0, st>>>(desc_dev, p.row_bits, p.row_off);
    rc = csm::check_launch("k_ll_row_offsets"); if (rc) return rc;
    k_ll_parse<kEmit><<<(unsigned)p.units, kBlock, 0, st>>>(desc_dev, n, p.res, p.modes, nullptr, host_table, nullptr, p.row_off, out, out_bytes);
    return csm::check_launch("k_ll_parse<emit>");
}
