// csm_lzw.h -- the code walker of the GIF decoder (variable-width LZW; contract DESIGN.md §4.17), written so that the same text
// compiles for the device (csrc/gifdec.hip: one lane of a wave runs step(), the wave fans its records out) and for the host
// (tools/lzw_host_check.cpp, where corrupt streams are exercised under the sanitizers).
//
// The walker copies no strings.  A dictionary entry is always "the previous string plus the first byte of the current one", and
// those bytes lie next to each other in the output.  So an entry is (output offset, length), and every code is either a literal or
// a copy of `length` bytes from an earlier output offset, which may overlap its destination (the "code equals the next free entry"
// case).  step() walks codes into records
//   rec[k] = (destination, literal value or source offset, length | kLiteral for a literal)
// for the resolve stage.  The input is read through a window (the device stages it in LDS, the host may pass the whole stream);
// every read is bounded by the window, every record by the image's pixel count, every table index by 4096, whatever the data.
//
//   step(S, T, win, rec, cap, n)    walks until `cap` records are listed (kBatch), the window is used up (kNeedInput: restage()),
//                                   or the image is done (kDone: S.err tells how it ended).  n receives the records listed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSM_LZW_FN __host__ __device__ inline
#else
#define CSM_LZW_FN inline
#endif

namespace csm_lzw {

constexpr int kEntries = 4096;
constexpr uint32_t kLiteral = 0x80000000u;

enum : uint32_t {                                    // bits of the error word of an image
    kErrCode = 1,        // a code above the next free entry
    kErrFirst = 2,       // the first code after a clear (or of the stream) is not a literal
    kErrEarly = 4,       // the data or the end code came before the rectangle was full
};

enum Status : int { kNeedInput = 1, kBatch = 2, kDone = 3 };

struct Table {                                       // 24 KiB: the string of code c is out[off[c], off[c] + len[c])
    uint32_t off[kEntries];
    uint16_t len[kEntries];
};

struct Record { uint32_t dst, src, len; };

struct State {
    // the input window: the caller's win[0, win_len) holds bytes [win_base, win_base + win_len) of the in_len input bytes
    uint32_t win_base, win_len, in_len;
    uint32_t pos;            // next input byte to feed (absolute)
    uint64_t acc;            // the bits fed and not yet taken, lowest first
    int nbits;
    int min_code, width;     // 2 .. 8; min_code + 1 .. 12
    uint32_t clear, next;    // the clear code (the end code is clear + 1); the next free entry, 4096 when the dictionary is full
    uint32_t prev_off, prev_len;         // the string of the code before; prev_len == 0: none since the last clear
    uint32_t out, npix;      // pixels listed so far, pixels of the rectangle
    uint32_t err;
};

// min_code outside 2 .. 8 is the caller's to refuse; it is clamped here so that no table index can leave the table
CSM_LZW_FN void init(State &S, uint32_t win_len, uint32_t in_len, int min_code, uint32_t npix) {
    S.win_base = 0; S.win_len = win_len; S.in_len = in_len;
    S.pos = 0; S.acc = 0; S.nbits = 0;
    S.min_code = min_code < 2 ? 2 : min_code > 8 ? 8 : min_code;
    S.width = S.min_code + 1;
    S.clear = 1u << S.min_code; S.next = S.clear + 2;
    S.prev_off = 0; S.prev_len = 0;
    S.out = 0; S.npix = npix; S.err = 0;
}

CSM_LZW_FN uint32_t byte_position(const State &S) { return S.pos; }

// the caller has staged bytes [base, base + len) of the input at win[0, len); base <= byte_position, base a multiple of 4, win
// 4-byte aligned
CSM_LZW_FN void restage(State &S, uint32_t base, uint32_t len) { S.win_base = base; S.win_len = len; }

// The state is worked on in a copy (registers on the device: the stores to T and rec cannot alias it) and written back on return.
CSM_LZW_FN int step(State &state, Table &T, const uint8_t *win, Record *rec, int cap, int &n) {
    State S = state;
    int status = kDone;
    n = 0;
    while (S.out < S.npix) {
        if (n >= cap) { status = kBatch; break; }
        if (S.nbits < S.width) {
            if (S.pos >= S.in_len) { S.err |= kErrEarly; break; }
            const uint32_t at = S.pos - S.win_base;               // pos >= win_base by restage's rule; a wrapped value is refused too
            if (at >= S.win_len) { status = kNeedInput; break; }
            if ((at & 3u) == 0 && S.win_len - at >= 4) {          // four bytes at once: win and win_base are 4-byte aligned
                uint32_t w;
                __builtin_memcpy(&w, __builtin_assume_aligned(win + at, 4), 4);
                S.acc |= (uint64_t)w << S.nbits;                  // nbits <= 11: no bit is lost
                S.nbits += 32;
                S.pos += 4;
            } else {
                S.acc |= (uint64_t)win[at] << S.nbits;
                S.nbits += 8;
                ++S.pos;
                continue;                                         // a width of 9 .. 12 may take a second byte
            }
        }
        const uint32_t code = (uint32_t)S.acc & ((1u << S.width) - 1u);
        S.acc >>= S.width;
        S.nbits -= S.width;
        if (code == S.clear) {
            S.width = S.min_code + 1; S.next = S.clear + 2; S.prev_len = 0;
            continue;
        }
        if (code == S.clear + 1) { S.err |= kErrEarly; break; }
        const uint32_t room = S.npix - S.out;
        if (S.prev_len == 0) {
            if (code > S.clear) { S.err |= kErrFirst; break; }
            rec[n++] = Record{S.out, code, 1u | kLiteral};
            S.prev_off = S.out; S.prev_len = 1;
            ++S.out;
            continue;
        }
        if (code > S.next || code >= (uint32_t)kEntries) { S.err |= kErrCode; break; }          // a 12-bit code is below 4096 anyway
        uint32_t len = 1;
        if (code < S.clear) {
            rec[n++] = Record{S.out, code, 1u | kLiteral};
        } else {
            uint32_t off;
            if (code == S.next) { off = S.prev_off; len = S.prev_len + 1; }     // next < 4096 here: code < 4096
            else { off = T.off[code]; len = T.len[code]; }
            // off < out, and off + len <= out + 1 (an entry ends with the first byte of the string behind it): sources lie inside the image
            rec[n++] = Record{S.out, off, len < room ? len : room};
        }
        if (S.next < (uint32_t)kEntries) {
            T.off[S.next] = S.prev_off;
            T.len[S.next] = (uint16_t)(S.prev_len + 1);           // at most 4096 - clear - 1 entries since the clear, each one longer by 1
            ++S.next;
            if (S.next == (1u << S.width) && S.width < 12) ++S.width;
        }
        S.prev_off = S.out; S.prev_len = len;
        S.out += len < room ? len : room;
    }
    state = S;
    return status;
}

}  // namespace csm_lzw
