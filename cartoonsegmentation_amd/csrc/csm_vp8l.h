// csm_vp8l.h -- the bit reader, the code builder and the symbol walker of the lossless WebP decoder (VP8L; contract DESIGN.md §4.15),
// and the per-pixel arithmetic of the four inverse transforms, written so that the same text compiles for the device
// (csrc/webpdec.hip: one lane of a wave runs decode_file()) and for the host (tools/vp8l_host_check.cpp, where corrupt streams are
// exercised under the sanitizers).
//
// decode_file() walks one VP8L payload from its first byte: the 5-byte header, the transforms with their sub-images, the colour
// cache, the entropy image, every prefix-code group, and the entropy-coded pixels.  It leaves the ARGB values in front of the
// inverse transforms in B.argb, the sub-images in their own buffers, and in Result the list of transforms in stream order.  The
// transforms themselves are applied by the caller (kernels on the device, apply_transforms_host() here) in reverse order.
//
// Every read of the input is bounded by its length (bytes behind the end read as zero and raise kErrEnd), every store by the sizes
// in Bufs, whatever the data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSM_VP8L_FN __host__ __device__ inline
#else
#define CSM_VP8L_FN inline
#endif

namespace csm_vp8l {

constexpr int kMaxCacheBits = 11;
constexpr int kGreenMax = 256 + 24 + (1 << kMaxCacheBits);       // the largest first alphabet
constexpr int kSymbolsPerGroup = kGreenMax + 3 * 256 + 40;
constexpr int kFastBits = 8;
constexpr uint32_t kGroupCap = 2600;                            // prefix-code groups of a file (libwebp's encoder emits no more)
constexpr int kMaxTransforms = 4;

enum : uint32_t {                                               // bits of the error word of a file
    kErrCode = 1,        // an over-subscribed or incomplete code, no used symbol, a bad run of code lengths, max_symbol too large
    kErrRef = 2,         // a backward reference that starts before the first pixel or runs past the last
    kErrTransform = 4,   // a second transform of one type
    kErrCache = 8,       // colour-cache bits outside 1..11, or a cache index at or beyond the cache size
    kErrEnd = 16,        // the stream ended early
    kErrCap = 32,        // more prefix-code groups than the cap: the file is valid but not taken (not "corrupt")
    kErrHeader = 64,     // the signature, the version or the size in the 5-byte header is not what the descriptor says
};

enum : int { kPredictor = 0, kCrossColour = 1, kSubtractGreen = 2, kPalette = 3 };

struct Code {
    uint16_t count[16];                  // codes per length; count[0] != 0: a code of one symbol, which takes no bits
    uint16_t fast[1 << kFastBits];       // by the next 8 bits: length << 12 | symbol of a code of up to 8 bits, else 0
};

struct Group {
    Code c[5];                           // green + length prefixes + cache indices, red, blue, alpha, distance prefixes
    uint16_t sorted[kSymbolsPerGroup];   // the symbols of each code in canonical order
};

CSM_VP8L_FN int sorted_offset(int k) { return k == 0 ? 0 : kGreenMax + (k - 1) * 256; }

struct Result {
    uint32_t err;
    int32_t ntrans, type[kMaxTransforms], bits[kMaxTransforms], xs[kMaxTransforms];   // in stream order; xs: the width the transform gives back
    int32_t pal_n, main_xs, has_alpha;
    uint32_t ngroups, meta_bits, cache_bits, bytes_used;
};

struct Bufs {
    uint32_t *argb;                      // W * H
    uint32_t *pred, *colour, *meta;      // sub_cap each
    uint32_t *palette;                   // 256
    uint32_t *cache;                     // 1 << kMaxCacheBits
    Group *groups;                       // group_cap
    uint32_t sub_cap, group_cap;
};

struct State {
    const uint8_t *in;
    uint32_t in_len;
    uint64_t pos;                        // the next bit
    uint64_t val;                        // the eight bytes from byte `base`
    uint32_t base;
    uint32_t err;
    Code clc;                            // the code of the code lengths
    uint16_t cl_sorted[19];
    uint8_t lens[kGreenMax];
};

CSM_VP8L_FN uint32_t subsample(uint32_t v, int bits) { return (v + (1u << bits) - 1) >> bits; }

// ---- bits ---------------------------------------------------------------------------------------------------------------------
CSM_VP8L_FN uint64_t load8(const uint8_t *p, uint32_t len, uint32_t byte) {
    uint64_t v = 0;
    if (byte + 8 <= len && byte + 8 > byte) {
        __builtin_memcpy(&v, p + byte, 8);
    } else {
        for (uint32_t k = 0; k < 8; ++k)
            if (byte + k < len && byte + k >= byte) v |= (uint64_t)p[byte + k] << (8 * k);
    }
    return v;
}

CSM_VP8L_FN void start(State &S, const uint8_t *in, uint32_t len) {
    S.in = in; S.in_len = len; S.pos = 0; S.base = 0; S.err = 0;
    S.val = load8(in, len, 0);
}

// the next n <= 32 bits, not consumed
CSM_VP8L_FN uint32_t peek(State &S, int n) {
    const uint64_t byte = S.pos >> 3;
    if (byte >= S.in_len) return 0;
    if (S.pos - 8ull * S.base > 32 || byte < S.base) {
        S.base = (uint32_t)byte;
        S.val = load8(S.in, S.in_len, S.base);
    }
    const uint64_t v = S.val >> (S.pos - 8ull * S.base);
    return n >= 32 ? (uint32_t)v : (uint32_t)v & ((1u << n) - 1u);
}

CSM_VP8L_FN uint32_t take(State &S, int n) {
    if (n == 0) return 0;
    const uint32_t v = peek(S, n);
    S.pos += n;
    return v;
}

CSM_VP8L_FN bool past_end(const State &S) { return S.pos > 8ull * S.in_len; }

// ---- codes --------------------------------------------------------------------------------------------------------------------
// lens[0, n) <= 15.  false: no symbol is used, or the code is incomplete or over-subscribed
CSM_VP8L_FN bool build_code(const uint8_t *lens, int n, Code &c, uint16_t *sorted) {
    uint16_t offs[16], next[16];
    for (int l = 0; l < 16; ++l) c.count[l] = 0;
    for (int s = 0; s < n; ++s) ++c.count[lens[s] & 15];
    const int used = n - c.count[0];
    c.count[0] = 0;
    if (used == 0) return false;
    if (used == 1) {
        for (int s = 0; s < n; ++s)
            if (lens[s]) sorted[0] = (uint16_t)s;
        for (int l = 1; l < 16; ++l) c.count[l] = 0;
        c.count[0] = 1;
        return true;
    }
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = 2 * left - c.count[l];
        if (left < 0) return false;
    }
    if (left != 0) return false;
    uint32_t o = 0, code = 0;
    offs[0] = 0; next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        offs[l] = (uint16_t)o; o += c.count[l];
        code = (code + c.count[l - 1]) << 1;                        // count[0] is 0 here
        next[l] = (uint16_t)code;
    }
    for (int i = 0; i < (1 << kFastBits); ++i) c.fast[i] = 0;
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        if (!l) continue;
        sorted[offs[l]++] = (uint16_t)s;
        const uint32_t cd = next[l]++;
        if (l <= kFastBits) {
            uint32_t rev = 0;
            for (int k = 0; k < l; ++k) rev |= ((cd >> k) & 1u) << (l - 1 - k);
            for (uint32_t i = rev; i < (1u << kFastBits); i += 1u << l) c.fast[i] = (uint16_t)(l << 12 | s);
        }
    }
    return true;
}

// the next symbol of a code; -1 cannot happen with a code build_code accepted
CSM_VP8L_FN int read_symbol(State &S, const Code &c, const uint16_t *sorted) {
    if (c.count[0]) return sorted[0];
    uint32_t v = peek(S, 15);
    const uint16_t e = c.fast[v & ((1u << kFastBits) - 1u)];
    if (e) { S.pos += e >> 12; return e & 0xfff; }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(v & 1u); v >>= 1;
        const int cnt = c.count[l];
        if (code - cnt < first) { S.pos += l; return sorted[index + (code - first)]; }
        index += cnt; first += cnt; first <<= 1; code <<= 1;
    }
    S.pos += 15;
    return -1;
}

// one prefix code of an alphabet of n symbols from the stream
CSM_VP8L_FN void read_code(State &S, int n, Code &c, uint16_t *sorted) {
    const int order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    for (int s = 0; s < n; ++s) S.lens[s] = 0;
    if (take(S, 1)) {                                               // a simple code
        const int two = (int)take(S, 1);
        const int s0 = (int)take(S, take(S, 1) ? 8 : 1);
        if (s0 < n) S.lens[s0] = 1;
        if (two) {
            const int s1 = (int)take(S, 8);
            if (s1 < n) S.lens[s1] = 1;
        }
    } else {
        uint8_t cl[19];
        for (int k = 0; k < 19; ++k) cl[k] = 0;
        const int ncl = 4 + (int)take(S, 4);
        if (ncl > 19) { S.err |= kErrCode; return; }
        for (int k = 0; k < ncl; ++k) cl[order[k]] = (uint8_t)take(S, 3);
        if (!build_code(cl, 19, S.clc, S.cl_sorted)) { S.err |= kErrCode; return; }
        int max_symbol = n;
        if (take(S, 1)) {
            const int nbits = 2 + 2 * (int)take(S, 3);
            max_symbol = 2 + (int)take(S, nbits);
            if (max_symbol > n) { S.err |= kErrCode; return; }
        }
        int s = 0, prev = 8;
        while (s < n) {
            if (max_symbol-- == 0) break;
            if (past_end(S)) { S.err |= kErrEnd; return; }
            const int l = read_symbol(S, S.clc, S.cl_sorted);
            if (l < 0) { S.err |= kErrCode; return; }
            if (l < 16) {
                S.lens[s++] = (uint8_t)l;
                if (l) prev = l;
            } else {
                const int extra = l == 16 ? 2 : l == 17 ? 3 : 7, offset = l == 18 ? 11 : 3;
                const int repeat = (int)take(S, extra) + offset;
                if (s + repeat > n) { S.err |= kErrCode; return; }
                const uint8_t fill = l == 16 ? (uint8_t)prev : 0;
                for (int k = 0; k < repeat; ++k) S.lens[s++] = fill;
            }
        }
    }
    if (past_end(S)) { S.err |= kErrEnd; return; }
    if (!build_code(S.lens, n, c, sorted)) S.err |= kErrCode;
}

CSM_VP8L_FN void read_group(State &S, Group &g, int cache_bits) {
    for (int k = 0; k < 5 && !S.err; ++k) {
        const int n = k == 0 ? 256 + 24 + (cache_bits ? 1 << cache_bits : 0) : k == 4 ? 40 : 256;
        read_code(S, n, g.c[k], g.sorted + sorted_offset(k));
    }
}

// the value of a length or distance prefix symbol and its extra bits
CSM_VP8L_FN uint32_t prefix_value(State &S, int sym) {
    if (sym < 4) return (uint32_t)sym + 1;
    const int extra = (sym - 2) >> 1;
    const uint32_t offset = (uint32_t)(2 + (sym & 1)) << extra;
    return offset + take(S, extra) + 1;
}

// the 120 short distance codes: (dx, dy) packed as (dy << 4) | (8 - dx)
CSM_VP8L_FN uint32_t plane_distance(uint32_t code, uint32_t xs) {
    const uint8_t map[120] = {
        0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
        0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
        0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
        0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
        0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
        0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
    if (code > 120) return code - 120;
    const int m = map[code - 1];
    const int d = (m >> 4) * (int)xs + (8 - (m & 15));
    return d < 1 ? 1u : (uint32_t)d;
}

CSM_VP8L_FN uint32_t cache_key(uint32_t argb, int bits) { return (0x1e35a7bdu * argb) >> (32 - bits); }

// the entropy-coded pixels of one image of xs * ys values into out.  meta == nullptr: one group
CSM_VP8L_FN void decode_pixels(State &S, const Bufs &B, uint32_t *out, uint32_t xs, uint32_t ys, int cache_bits, const uint32_t *meta, int meta_bits,
                               uint32_t meta_w) {
    const uint32_t total = xs * ys;
    const uint32_t cache_size = cache_bits ? 1u << cache_bits : 0u;
    for (uint32_t i = 0; i < cache_size; ++i) B.cache[i] = 0;
    const uint32_t mask = meta ? (1u << meta_bits) - 1u : 0xffffffffu;
    uint32_t pos = 0, x = 0, y = 0;
    const Group *g = B.groups;
    bool fetch = true;
    while (pos < total) {
        if (past_end(S)) { S.err |= kErrEnd; return; }
        if (fetch || (x & mask) == 0) {
            if (meta) g = B.groups + ((meta[(y >> meta_bits) * meta_w + (x >> meta_bits)] >> 8) & 0xffffu);
            fetch = false;
        }
        const int sym = read_symbol(S, g->c[0], g->sorted);
        if (sym < 0) { S.err |= kErrCode; return; }
        if (sym < 256) {
            const int r = read_symbol(S, g->c[1], g->sorted + sorted_offset(1));
            const int b = read_symbol(S, g->c[2], g->sorted + sorted_offset(2));
            const int a = read_symbol(S, g->c[3], g->sorted + sorted_offset(3));
            if ((r | b | a) < 0) { S.err |= kErrCode; return; }
            const uint32_t px = (uint32_t)a << 24 | (uint32_t)r << 16 | (uint32_t)sym << 8 | (uint32_t)b;
            out[pos++] = px;
            if (cache_size) B.cache[cache_key(px, cache_bits)] = px;
            if (++x >= xs) { x = 0; ++y; }
        } else if (sym < 256 + 24) {
            const uint32_t len = prefix_value(S, sym - 256);
            const int dsym = read_symbol(S, g->c[4], g->sorted + sorted_offset(4));
            if (dsym < 0) { S.err |= kErrCode; return; }
            const uint32_t dist = plane_distance(prefix_value(S, dsym), xs);
            if (dist > pos || len > total - pos) { S.err |= kErrRef; return; }
            uint32_t k = 0;
            if (dist >= 8) {                                        // eight loads in flight: the sources are final
                for (; k + 8 <= len; k += 8) {
                    uint32_t v[8];
                    for (int j = 0; j < 8; ++j) v[j] = out[pos + k + j - dist];
                    for (int j = 0; j < 8; ++j) out[pos + k + j] = v[j];
                    if (cache_size)
                        for (int j = 0; j < 8; ++j) B.cache[cache_key(v[j], cache_bits)] = v[j];
                }
            }
            for (; k < len; ++k) {
                const uint32_t v = out[pos + k - dist];
                out[pos + k] = v;
                if (cache_size) B.cache[cache_key(v, cache_bits)] = v;
            }
            pos += len;
            x += len;
            while (x >= xs) { x -= xs; ++y; }
            fetch = true;
        } else {
            const uint32_t idx = (uint32_t)sym - (256 + 24);
            if (idx >= cache_size) { S.err |= kErrCache; return; }
            out[pos++] = B.cache[idx];
            if (++x >= xs) { x = 0; ++y; }
        }
    }
    if (past_end(S)) S.err |= kErrEnd;
}

// false: invalid cache bits
CSM_VP8L_FN bool read_cache_bits(State &S, int &cache_bits) {
    cache_bits = 0;
    if (take(S, 1)) {
        cache_bits = (int)take(S, 4);
        if (cache_bits < 1 || cache_bits > kMaxCacheBits) { S.err |= kErrCache; return false; }
    }
    return true;
}

// a sub-image (entropy-coded image without transforms and without meta codes) of xs * ys <= the buffer's capacity
CSM_VP8L_FN void decode_sub(State &S, const Bufs &B, uint32_t *out, uint32_t xs, uint32_t ys) {
    int cache_bits;
    if (!read_cache_bits(S, cache_bits)) return;
    read_group(S, B.groups[0], cache_bits);
    if (S.err) return;
    decode_pixels(S, B, out, xs, ys, cache_bits, nullptr, 0, 0);
}

CSM_VP8L_FN uint32_t add_bytes(uint32_t a, uint32_t b) {
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}

// one VP8L payload of a W * H image.  B.sub_cap >= subsample(W, 2) * subsample(H, 2), B.group_cap >= 1
CSM_VP8L_FN void decode_file(State &S, const Bufs &B, const uint8_t *in, uint32_t in_len, uint32_t W, uint32_t H, Result &R) {
    start(S, in, in_len);
    R.ntrans = 0; R.pal_n = 0; R.main_xs = (int32_t)W; R.ngroups = 0; R.meta_bits = 0; R.cache_bits = 0; R.bytes_used = 0; R.has_alpha = 0;
    const uint32_t sig = take(S, 8), w = take(S, 14) + 1, h = take(S, 14) + 1;
    R.has_alpha = (int32_t)take(S, 1);
    const uint32_t version = take(S, 3);
    if (sig != 0x2f || w != W || h != H || version != 0 || in_len < 5) { S.err |= kErrHeader; R.err = S.err; return; }
    uint32_t xs = W, seen = 0;
    while (!S.err && take(S, 1)) {
        if (past_end(S)) { S.err |= kErrEnd; break; }
        const int type = (int)take(S, 2);
        if (seen >> type & 1u) { S.err |= kErrTransform; break; }
        seen |= 1u << type;
        const int t = R.ntrans++;
        R.type[t] = type; R.xs[t] = (int32_t)xs; R.bits[t] = 0;
        if (type == kPredictor || type == kCrossColour) {
            const int bits = (int)take(S, 3) + 2;
            R.bits[t] = bits;
            decode_sub(S, B, type == kPredictor ? B.pred : B.colour, subsample(xs, bits), subsample(H, bits));
        } else if (type == kPalette) {
            const int n = (int)take(S, 8) + 1;
            const int bits = n > 16 ? 0 : n > 4 ? 1 : n > 2 ? 2 : 3;
            R.bits[t] = bits; R.pal_n = n;
            decode_sub(S, B, B.palette, (uint32_t)n, 1);
            if (S.err) break;
            for (int i = 1; i < n; ++i) B.palette[i] = add_bytes(B.palette[i], B.palette[i - 1]);
            for (int i = n; i < 256; ++i) B.palette[i] = 0;
            xs = subsample(xs, bits);
        }
    }
    int cache_bits = 0;
    const uint32_t *meta = nullptr;
    uint32_t meta_w = 0, ngroups = 1;
    int meta_bits = 0;
    if (!S.err && read_cache_bits(S, cache_bits)) {
        if (take(S, 1)) {
            meta_bits = (int)take(S, 3) + 2;
            meta_w = subsample(xs, meta_bits);
            const uint32_t meta_h = subsample(H, meta_bits);
            decode_sub(S, B, B.meta, meta_w, meta_h);
            if (!S.err) {
                uint32_t top = 0;
                for (uint32_t i = 0; i < meta_w * meta_h; ++i) {
                    const uint32_t v = (B.meta[i] >> 8) & 0xffffu;
                    top = v > top ? v : top;
                }
                ngroups = top + 1;
                meta = B.meta;
            }
        }
        R.ngroups = ngroups; R.meta_bits = (uint32_t)meta_bits; R.cache_bits = (uint32_t)cache_bits;
        if (!S.err && ngroups > B.group_cap) S.err |= kErrCap;
        for (uint32_t k = 0; k < ngroups && !S.err; ++k) read_group(S, B.groups[k], cache_bits);
        if (!S.err) decode_pixels(S, B, B.argb, xs, H, cache_bits, meta, meta_bits, meta_w);
    }
    R.main_xs = (int32_t)xs;
    R.bytes_used = (uint32_t)((S.pos + 7) >> 3);
    R.err = S.err;
}

// The same walk for a stream that begins behind the 5-byte header: the alpha plane of a lossy file (an ALPH chunk of compression 1;
// csm_vp8dec.h), whose size is the frame's and whose values are the green channel.
CSM_VP8L_FN void decode_headerless(State &S, const Bufs &B, const uint8_t *in, uint32_t in_len, uint32_t W, uint32_t H, Result &R) {
    start(S, in, in_len);
    R.ntrans = 0; R.pal_n = 0; R.main_xs = (int32_t)W; R.ngroups = 0; R.meta_bits = 0; R.cache_bits = 0; R.bytes_used = 0; R.has_alpha = 0;
    uint32_t xs = W, seen = 0;
    while (!S.err && take(S, 1)) {
        if (past_end(S)) { S.err |= kErrEnd; break; }
        const int type = (int)take(S, 2);
        if (seen >> type & 1u) { S.err |= kErrTransform; break; }
        seen |= 1u << type;
        const int t = R.ntrans++;
        R.type[t] = type; R.xs[t] = (int32_t)xs; R.bits[t] = 0;
        if (type == kPredictor || type == kCrossColour) {
            const int bits = (int)take(S, 3) + 2;
            R.bits[t] = bits;
            decode_sub(S, B, type == kPredictor ? B.pred : B.colour, subsample(xs, bits), subsample(H, bits));
        } else if (type == kPalette) {
            const int n = (int)take(S, 8) + 1;
            const int bits = n > 16 ? 0 : n > 4 ? 1 : n > 2 ? 2 : 3;
            R.bits[t] = bits; R.pal_n = n;
            decode_sub(S, B, B.palette, (uint32_t)n, 1);
            if (S.err) break;
            for (int i = 1; i < n; ++i) B.palette[i] = add_bytes(B.palette[i], B.palette[i - 1]);
            for (int i = n; i < 256; ++i) B.palette[i] = 0;
            xs = subsample(xs, bits);
        }
    }
    int cache_bits = 0;
    const uint32_t *meta = nullptr;
    uint32_t meta_w = 0, ngroups = 1;
    int meta_bits = 0;
    if (!S.err && read_cache_bits(S, cache_bits)) {
        if (take(S, 1)) {
            meta_bits = (int)take(S, 3) + 2;
            meta_w = subsample(xs, meta_bits);
            const uint32_t meta_h = subsample(H, meta_bits);
            decode_sub(S, B, B.meta, meta_w, meta_h);
            if (!S.err) {
                uint32_t top = 0;
                for (uint32_t i = 0; i < meta_w * meta_h; ++i) {
                    const uint32_t v = (B.meta[i] >> 8) & 0xffffu;
                    top = v > top ? v : top;
                }
                ngroups = top + 1;
                meta = B.meta;
            }
        }
        R.ngroups = ngroups; R.meta_bits = (uint32_t)meta_bits; R.cache_bits = (uint32_t)cache_bits;
        if (!S.err && ngroups > B.group_cap) S.err |= kErrCap;
        for (uint32_t k = 0; k < ngroups && !S.err; ++k) read_group(S, B.groups[k], cache_bits);
        if (!S.err) decode_pixels(S, B, B.argb, xs, H, cache_bits, meta, meta_bits, meta_w);
    }
    R.main_xs = (int32_t)xs;
    R.bytes_used = (uint32_t)((S.pos + 7) >> 3);
    R.err = S.err;
}

// ---- the inverse transforms, per pixel ------------------------------------------------------------------------------------------
CSM_VP8L_FN uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }

CSM_VP8L_FN int absdiff(uint32_t a, uint32_t b, int shift) {
    const int d = (int)((a >> shift) & 255u) - (int)((b >> shift) & 255u);
    return d < 0 ? -d : d;
}

CSM_VP8L_FN uint32_t clamp255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// the prediction of mode 0..13 (14 and 15 predict like 0) from left, top, top-left, top-right
CSM_VP8L_FN uint32_t predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
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
    case 11: {
        int pl = 0, pt = 0;
        for (int s = 0; s < 32; s += 8) { pl += absdiff(T, TL, s); pt += absdiff(L, TL, s); }
        return pl < pt ? L : T;
    }
    case 12: {
        uint32_t r = 0;
        for (int s = 0; s < 32; s += 8)
            r |= clamp255((int)((L >> s) & 255u) + (int)((T >> s) & 255u) - (int)((TL >> s) & 255u)) << s;
        return r;
    }
    case 13: {
        const uint32_t a = avg2(L, T);
        uint32_t r = 0;
        for (int s = 0; s < 32; s += 8) {
            const int av = (int)((a >> s) & 255u), c = (int)((TL >> s) & 255u);
            r |= clamp255(av + (av - c) / 2) << s;
        }
        return r;
    }
    default: return 0xff000000u;
    }
}

CSM_VP8L_FN uint32_t add_green(uint32_t v) {
    const uint32_t g = (v >> 8) & 255u;
    return (v & 0xff00ff00u) | (((v & 0x00ff00ffu) + (g << 16 | g)) & 0x00ff00ffu);
}

CSM_VP8L_FN int colour_delta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }

// m: the block's element of the cross-colour sub-image (red_to_blue << 16 | green_to_blue << 8 | green_to_red)
CSM_VP8L_FN uint32_t cross_colour(uint32_t v, uint32_t m) {
    const uint32_t g = (v >> 8) & 255u;
    const uint32_t r = ((v >> 16) + (uint32_t)colour_delta(m & 255u, g)) & 255u;
    const uint32_t b = (v + (uint32_t)colour_delta((m >> 8) & 255u, g) + (uint32_t)colour_delta((m >> 16) & 255u, r)) & 255u;
    return (v & 0xff00ff00u) | r << 16 | b;
}

// pixel x of a row of packed palette indices (bits 0..3: 1 << bits pixels per packed pixel)
CSM_VP8L_FN uint32_t palette_pixel(const uint32_t *row, const uint32_t *palette, uint32_t x, int bits) {
    const uint32_t packed = (row[x >> bits] >> 8) & 255u;
    const int per = 8 >> bits;
    const uint32_t idx = bits ? (packed >> ((x & ((1u << bits) - 1u)) * per)) & ((1u << per) - 1u) : packed;
    return palette[idx];
}

// the prediction of pixel (x, y) of a predictor transform: the border rules, then the block's mode
CSM_VP8L_FN uint32_t predict_at(const uint32_t *pred, int bits, uint32_t xs, uint32_t x, uint32_t y, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    if (y == 0) return x == 0 ? 0xff000000u : L;
    if (x == 0) return T;
    const int mode = (int)((pred[(y >> bits) * subsample(xs, bits) + (x >> bits)] >> 8) & 15u);
    return predict(mode, L, T, TL, TR);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the inverse transforms in reverse stream order, serially; a and b are W * H buffers, a holds decode_file's B.argb.  Returns the
// buffer that holds the image
inline uint32_t *apply_transforms_host(const Result &R, const Bufs &B, uint32_t *a, uint32_t *b, uint32_t H) {
    for (int t = R.ntrans - 1; t >= 0; --t) {
        const uint32_t xs = (uint32_t)R.xs[t];
        const int bits = R.bits[t];
        if (R.type[t] == kPalette) {
            const uint32_t in_w = subsample(xs, bits);
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < xs; ++x) b[y * xs + x] = palette_pixel(a + y * in_w, B.palette, x, bits);
        } else if (R.type[t] == kPredictor) {
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < xs; ++x) {
                    const uint32_t L = x ? b[y * xs + x - 1] : 0, T = y ? b[(y - 1) * xs + x] : 0, TL = x && y ? b[(y - 1) * xs + x - 1] : 0;
                    const uint32_t TR = !y ? 0 : x + 1 < xs ? b[(y - 1) * xs + x + 1] : b[y * xs];
                    b[y * xs + x] = add_bytes(a[y * xs + x], predict_at(B.pred, bits, xs, x, y, L, T, TL, TR));
                }
        } else {
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < xs; ++x) {
                    const uint32_t v = a[y * xs + x];
                    b[y * xs + x] = R.type[t] == kSubtractGreen ? add_green(v) : cross_colour(v, B.colour[(y >> bits) * subsample(xs, bits) + (x >> bits)]);
                }
        }
        uint32_t *s = a; a = b; b = s;
    }
    return a;
}
#endif

}  // namespace csm_vp8l
