// csm_inflate.h -- the symbol walker of the PNG decoder (RFC 1951 inflate; contract DESIGN.md §4.9), written so that the same text
// compiles for the device (csrc/pngdec.hip: one lane of a wave runs step(), the wave runs the marked helpers together) and for the host
// (tools/inflate_host_check.cpp, where corrupt streams are exercised under the sanitizers).
//
// The walker does not copy matches.  It walks the Huffman stream once and leaves
//   lit[p]                       the byte of every literal (and of every stored block) at its own output position p
//   matches[2m], matches[2m+1]   for match m: its output position, and (length - 3) | (distance - 1) << 8
// for the resolve stage.  The input is read through a window (the device stages it in LDS, the host passes the whole stream); every
// read is bounded by the window, every store by raw_cap / match_cap, whatever the data.
//
//   step(S, T, ..)    runs until something needs the caller: kNeedInput (restage the window: restage()), kBuild (code lengths are in
//                     T.lens: prepare(), then clear_fast() and fill_fast() by any number of lanes), kStored (copy S.stored_len bytes
//                     from input offset S.stored_src to lit + S.out, then stored_done()), kDone (S.err tells how it ended)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSM_INF_FN __host__ __device__ inline
#else
#define CSM_INF_FN inline
#endif

namespace csm_inflate {

constexpr int kLitBits = 11, kDistBits = 9;          // index bits of the two direct tables; longer codes take the canonical walk
constexpr int kMaxLit = 288, kMaxDist = 32;
constexpr uint32_t kHeaderGuard = 640;               // bytes a block header may take (dynamic: 14 + 19 * 3 + 316 * 14 bits)
constexpr uint32_t kSymbolGuard = 8;                 // bytes the two refills of a literal/length + distance pair may take (20 + 28 bits)

enum : uint32_t {                                    // bits of the error word of a file
    kErrCode = 1,        // a code that is over-subscribed, or incomplete where RFC 1951 forbids it; a bad run of code lengths
    kErrSymbol = 2,      // an unassigned code, literal/length symbol 286 / 287, distance symbol 30 / 31, too many symbols
    kErrDistance = 4,    // a distance that reaches before byte 0
    kErrOutput = 8,      // output beyond the raw size
    kErrInput = 16,      // the input ran out
    kErrMatches = 32,    // the match list is full
    kErrBlock = 64,      // block type 3, or a stored block whose length check fails
    kErrShort = 128,     // the stream ended before the raw size
    kErrAdler = 256,     // the Adler-32 of the raw bytes is not the trailer's
    kErrFilter = 512,    // a scanline with a filter type above 4
};

enum Status : int { kNeedInput = 1, kBuild = 2, kStored = 3, kDone = 4 };

struct Tables {
    uint16_t lit_fast[1 << kLitBits];     // by the next kLitBits bits: length << 9 | symbol of a code of up to kLitBits bits, else 0
    uint16_t dist_fast[1 << kDistBits];
    uint16_t lit_count[16], dist_count[16];              // codes per length
    uint16_t lit_symbol[kMaxLit], dist_symbol[kMaxDist]; // symbols in canonical order
    uint16_t code[kMaxLit + kMaxDist];                   // bit-reversed canonical code of every symbol
    uint8_t lens[kMaxLit + kMaxDist];                    // code length of every symbol: nlit literal/length ones, then ndist
    uint16_t cl_count[16], cl_symbol[19], work[32];      // the code-length code of a dynamic header; make_code's running offsets
    uint8_t cl[20];
};

struct State {
    // the input window: the caller's win[0, win_len) holds bytes [win_base, win_base + win_len) of the in_len input bytes
    uint32_t win_base, win_len, in_len;
    uint32_t pos;            // next byte of the window to feed (may pass win_len: zeros are fed, and counted as missing input)
    uint64_t bits;
    int nbits;
    // output: positions in the caller's lit[0, raw_cap) and matches[0, 2 * match_cap)
    uint32_t raw_cap, match_cap, out, nmatch;
    // block state
    int in_block, last, nlit, ndist, fixed_built;
    uint32_t stored_src, stored_len;
    uint32_t err;
};

CSM_INF_FN void init(State &S, uint32_t win_len, uint32_t in_len, uint32_t start, uint32_t raw_cap, uint32_t match_cap) {
    S.win_base = 0; S.win_len = win_len; S.in_len = in_len; S.pos = start; S.bits = 0; S.nbits = 0;
    S.raw_cap = raw_cap; S.match_cap = match_cap; S.out = 0; S.nmatch = 0;
    S.in_block = 0; S.last = 0; S.nlit = 0; S.ndist = 0; S.fixed_built = 0; S.stored_src = 0; S.stored_len = 0; S.err = 0;
}

// input offset of the first byte none of whose bits has been fed to the reader's unread whole bytes: the byte BEHIND a started byte
// (nbits & 7 != 0, whose unread bits stay in the register across restage()), the byte of the next bit otherwise.  After the last
// block this is the offset of the zlib trailer.
CSM_INF_FN uint32_t byte_position(const State &S) { return S.win_base + S.pos - (uint32_t)(S.nbits >> 3); }

// the window is about to be refilled from input offset `base` (at or before byte_position) with `len` bytes: whole unread bytes go
// back, the unread bits of a started byte stay
CSM_INF_FN void restage(State &S, uint32_t base, uint32_t len) {
    const uint32_t bp = byte_position(S);
    S.nbits &= 7;
    S.bits &= (1ull << S.nbits) - 1;
    S.win_base = base; S.win_len = len; S.pos = bp - base;
}

// the bit reader over the window, on local copies of the state
struct Bits {
    const uint8_t *win;
    uint32_t win_len, pos;
    uint64_t bits;
    int nbits;
    // at least 33 bits afterwards: four bytes at once (the loads do not depend on one another), zeros beyond the window
    CSM_INF_FN void refill() {
        if (nbits > 32) return;
        uint32_t w;
        if (pos + 4 <= win_len) {
            w = (uint32_t)win[pos] | (uint32_t)win[pos + 1] << 8 | (uint32_t)win[pos + 2] << 16 | (uint32_t)win[pos + 3] << 24;
        } else {
            w = 0;
            for (uint32_t k = 0; k < 4; ++k)
                if (pos + k < win_len) w |= (uint32_t)win[pos + k] << (8 * k);
        }
        bits |= (uint64_t)w << nbits;
        nbits += 32; pos += 4;
    }
    CSM_INF_FN uint32_t peek(int n) const { return (uint32_t)bits & ((1u << n) - 1u); }
    CSM_INF_FN void skip(int n) { bits >>= n; nbits -= n; }
    CSM_INF_FN uint32_t get(int n) { const uint32_t v = peek(n); skip(n); return v; }
};

// canonical walk, one bit at a time (codes longer than the direct table, and the code-length code): the symbol, or -1 for a bit
// pattern no code has.  At least 15 bits are in the reader.
CSM_INF_FN int decode_slow(Bits &B, const uint16_t *count, const uint16_t *symbol) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((B.bits >> (len - 1)) & 1);
        const int c = count[len];
        if (code - c < first) { B.skip(len); return symbol[index + (code - first)]; }
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// counts, canonical order and bit-reversed codes of the n symbols whose lengths are lens[0, n).  Returns 0, or kErrCode for an
// over-subscribed code or an incomplete one (allowed: a code with no symbols when may_be_empty, and one single code of one bit).
CSM_INF_FN uint32_t make_code(const uint8_t *lens, int n, uint16_t *count, uint16_t *symbol, uint16_t *code, uint16_t *work,
                              bool may_be_empty, bool may_be_single) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s]];
    int left = 1, maxlen = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return kErrCode;
        if (count[l]) maxlen = l;
    }
    if (left > 0 && !((maxlen == 0 && may_be_empty) || (maxlen == 1 && may_be_single))) return kErrCode;
    uint16_t *offs = work, *next = work + 16;
    offs[1] = 0; next[0] = 0; next[1] = 0;
    for (int l = 1; l < 15; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        next[l + 1] = (uint16_t)((next[l] + count[l]) << 1);
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (!l) continue;
        symbol[offs[l]++] = (uint16_t)s;
        uint32_t c = next[l]++, r = 0;
        for (int k = 0; k < l; ++k) { r = (r << 1) | (c & 1); c >>= 1; }
        if (code) code[s] = (uint16_t)r;
    }
    count[0] = 0;
    return 0;
}

// after kBuild, by one lane: both codes from T.lens
CSM_INF_FN void prepare(State &S, Tables &T) {
    S.err |= make_code(T.lens, S.nlit, T.lit_count, T.lit_symbol, T.code, T.work, false, true);
    S.err |= make_code(T.lens + S.nlit, S.ndist, T.dist_count, T.dist_symbol, T.code + S.nlit, T.work, true, true);
}

// after prepare, by `lanes` lanes (lane = 0 .. lanes - 1) with a barrier between the two: the direct tables
CSM_INF_FN void clear_fast(Tables &T, int lane, int lanes) {
    for (int i = lane; i < (1 << kLitBits); i += lanes) T.lit_fast[i] = 0;
    for (int i = lane; i < (1 << kDistBits); i += lanes) T.dist_fast[i] = 0;
}
CSM_INF_FN void fill_fast(const State &S, Tables &T, int lane, int lanes) {
    for (int s = lane; s < S.nlit + S.ndist; s += lanes) {
        const int l = T.lens[s];
        const bool dist = s >= S.nlit;
        const int bitsn = dist ? kDistBits : kLitBits;
        if (!l || l > bitsn) continue;
        uint16_t *fast = dist ? T.dist_fast : T.lit_fast;
        const uint16_t e = (uint16_t)(l << 9 | (dist ? s - S.nlit : s));
        for (int k = T.code[s]; k < (1 << bitsn); k += 1 << l) fast[k] = e;
    }
}

// after the caller has copied a stored block
CSM_INF_FN void stored_done(State &S) {
    S.out += S.stored_len;
    S.pos = S.stored_src + S.stored_len - S.win_base;
    S.bits = 0; S.nbits = 0;
}

CSM_INF_FN bool more_input(const State &S) { return S.win_base + S.win_len < S.in_len; }

// by one lane.  The window, the literals and the match list are arguments rather than members of S, so that a kernel's compiler
// sees which memory each of them is (LDS, global) and the loop's stores do not force its table reads to be repeated.
CSM_INF_FN int step(State &S, Tables &T, const uint8_t *win, uint8_t *lit, uint32_t *matches) {
    Bits B{win, S.win_len, S.pos, S.bits, S.nbits};
    const uint32_t raw_cap = S.raw_cap, match_cap = S.match_cap;
    const bool more = more_input(S);
#define CSM_INF_SAVE() do { S.pos = B.pos; S.bits = B.bits; S.nbits = B.nbits; } while (0)
#define CSM_INF_FAIL(e) do { CSM_INF_SAVE(); S.err |= (e); return kDone; } while (0)
    // the bits taken so far lie inside the input
#define CSM_INF_INSIDE() ((uint64_t)(S.win_base + (uint64_t)B.pos) * 8 - (uint64_t)B.nbits <= (uint64_t)S.in_len * 8)
    for (;;) {
        if (S.err) { CSM_INF_SAVE(); return kDone; }
        if (!S.in_block) {
            if (S.last) {
                CSM_INF_SAVE();
                if (S.out != S.raw_cap) S.err |= kErrShort;
                return kDone;
            }
            if ((uint64_t)B.pos + kHeaderGuard > B.win_len && more) { CSM_INF_SAVE(); return kNeedInput; }
            B.refill();
            S.last = (int)B.get(1);
            const uint32_t type = B.get(2);
            if (type == 3) CSM_INF_FAIL(kErrBlock);
            if (type == 0) {
                B.skip(B.nbits & 7);
                B.refill();
                const uint32_t len = B.get(16), nlen = B.get(16);
                if (!CSM_INF_INSIDE()) CSM_INF_FAIL(kErrInput);
                if ((len ^ nlen) != 0xFFFFu) CSM_INF_FAIL(kErrBlock);
                CSM_INF_SAVE();
                const uint32_t src = byte_position(S);
                if (src > S.in_len || len > S.in_len - src) { S.err |= kErrInput; return kDone; }
                if (len > S.raw_cap - S.out) { S.err |= kErrOutput; return kDone; }
                S.stored_src = src; S.stored_len = len;
                return kStored;
            }
            if (type == 1) {
                S.in_block = 1;
                if (S.fixed_built) continue;
                for (int s = 0; s < 288; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (int s = 0; s < 32; ++s) T.lens[288 + s] = 5;
                S.nlit = 288; S.ndist = 32; S.fixed_built = 1;
                CSM_INF_SAVE();
                return kBuild;
            }
            // a dynamic block: the code-length code, then the lengths of both codes
            S.fixed_built = 0;
            const int nlit = (int)B.get(5) + 257, ndist = (int)B.get(5) + 1, ncl = (int)B.get(4) + 4;
            if (nlit > 286 || ndist > 30) CSM_INF_FAIL(kErrSymbol);
            uint8_t *cl = T.cl;
            for (int i = 0; i < 19; ++i) cl[i] = 0;
            for (int i = 0; i < ncl; ++i) {
                // the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - (i - 3) / 2 : 8 + (i - 4) / 2;
                B.refill();
                cl[at] = (uint8_t)B.get(3);
            }
            uint16_t *cl_count = T.cl_count, *cl_symbol = T.cl_symbol;
            if (make_code(cl, 19, cl_count, cl_symbol, nullptr, T.work, false, false)) CSM_INF_FAIL(kErrCode);
            int have = 0, prev = 0;
            while (have < nlit + ndist) {
                B.refill();
                const int sym = decode_slow(B, cl_count, cl_symbol);
                if (sym < 0) CSM_INF_FAIL(kErrSymbol);
                if (sym < 16) { T.lens[have++] = (uint8_t)sym; prev = sym; continue; }
                int rep, val = 0;
                if (sym == 16) {
                    if (!have) CSM_INF_FAIL(kErrCode);
                    val = prev; rep = 3 + (int)B.get(2);
                } else if (sym == 17) rep = 3 + (int)B.get(3);
                else rep = 11 + (int)B.get(7);
                if (have + rep > nlit + ndist) CSM_INF_FAIL(kErrCode);
                for (int k = 0; k < rep; ++k) T.lens[have++] = (uint8_t)val;
                prev = val;
            }
            if (!CSM_INF_INSIDE()) CSM_INF_FAIL(kErrInput);
            if (T.lens[256] == 0) CSM_INF_FAIL(kErrCode);
            S.nlit = nlit; S.ndist = ndist; S.in_block = 1;
            CSM_INF_SAVE();
            return kBuild;
        }
        // symbols of the block
        uint32_t out = S.out, nmatch = S.nmatch;
        uint32_t fail = 0;
        bool need = false;
        for (;;) {
            if ((uint64_t)B.pos + kSymbolGuard > B.win_len && more) { need = true; break; }
            B.refill();
            int e = T.lit_fast[B.peek(kLitBits)], sym;
            if (e) { B.skip(e >> 9); sym = e & 511; }
            else {
                sym = decode_slow(B, T.lit_count, T.lit_symbol);
                if (sym < 0) { fail = kErrSymbol; break; }
            }
            if (sym < 256) {
                if (out >= raw_cap) { fail = kErrOutput; break; }
                lit[out++] = (uint8_t)sym;
                continue;
            }
            if (sym == 256) { S.in_block = 0; break; }
            if (sym > 285) { fail = kErrSymbol; break; }
            uint32_t len;
            if (sym < 265) len = (uint32_t)sym - 254;
            else if (sym == 285) len = 258;
            else {
                const int x = (sym - 261) >> 2;
                len = 3 + ((4 + ((uint32_t)(sym - 265) & 3)) << x) + B.get(x);
            }
            int d;
            B.refill();
            e = T.dist_fast[B.peek(kDistBits)];
            if (e) { B.skip(e >> 9); d = e & 511; }
            else {
                d = decode_slow(B, T.dist_count, T.dist_symbol);
                if (d < 0) { fail = kErrSymbol; break; }
            }
            if (d > 29) { fail = kErrSymbol; break; }
            uint32_t dist;
            if (d < 4) dist = (uint32_t)d + 1;
            else {
                const int x = (d >> 1) - 1;
                dist = 1 + ((2 + ((uint32_t)d & 1)) << x) + B.get(x);
            }
            if (dist > out) { fail = kErrDistance; break; }
            if (len > raw_cap - out) { fail = kErrOutput; break; }
            if (nmatch >= match_cap) { fail = kErrMatches; break; }
            matches[2 * (uint64_t)nmatch] = out;
            matches[2 * (uint64_t)nmatch + 1] = (len - 3) | (dist - 1) << 8;
            ++nmatch;
            out += len;
        }
        S.out = out; S.nmatch = nmatch;
        if (!fail && !CSM_INF_INSIDE()) fail = kErrInput;
        if (fail) CSM_INF_FAIL(fail);
        if (need) { CSM_INF_SAVE(); return kNeedInput; }
    }
#undef CSM_INF_SAVE
#undef CSM_INF_FAIL
#undef CSM_INF_INSIDE
}

}  // namespace csm_inflate
