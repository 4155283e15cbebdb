// csm_boolenc.h -- the VP8 boolean (arithmetic) coder of the WebP writer (webp.hip), one instance per lane.
// Plain C++ that compiles for the device and for the host: tests/test_webp.py builds it with the host compiler and drives it
// against a segment that is too short, which no device input can do (the segments are sized from a proven bound).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSM_BOOLENC_FN __host__ __device__ __forceinline__
#else
#define CSM_BOOLENC_FN inline
#endif

namespace csm {

// The format's coder in its byte-wise form: range holds the range minus one (127..254 between calls), value the low end, nb_bits
// the bits of value past the next whole byte.  A finished byte is held back while it may still take a carry: the last byte that
// is not 0xFF in `held`, the 0xFF bytes behind it as the count `run`.  Bytes go out front to back and every one of them through
// emit(): nothing is written at or past `cap`, `over` remembers that the cursor met it, and `pos` goes on counting, so finish()
// returns the bytes the stream needs whether or not they fitted.  run never exceeds the bytes finished so far (at most 7 bits per
// coded pair), which bounds its loops.
struct BoolEnc {
    uint8_t *out;
    int64_t pos, cap;
    int range, nb_bits, run, held, over;
    uint32_t value;
    CSM_BOOLENC_FN void open(uint8_t *o, int64_t c) {
        out = o; pos = 0; cap = c; range = 254; nb_bits = -8; run = 0; held = -1; over = 0; value = 0;
    }
    CSM_BOOLENC_FN void emit(int byte) {
        if (pos < cap) out[pos] = (uint8_t)byte; else over = 1;
        ++pos;
    }
    CSM_BOOLENC_FN void flush() {
        const int s = 8 + nb_bits;
        const uint32_t bits = value >> s;
        value -= bits << s;
        nb_bits -= 8;
        if ((bits & 0xFF) != 0xFF) {
            const int carry = (int)(bits >> 8) & 1;
            if (held >= 0) emit(held + carry);
            for (; run > 0; --run) emit(carry ? 0x00 : 0xFF);
            held = (int)(bits & 0xFF);
        } else {
            ++run;
        }
    }
    CSM_BOOLENC_FN void put(int prob, int bit) {
        const int split = (range * prob) >> 8;
        if (bit) { value += split + 1; range -= split + 1; } else { range = split; }
        if (range < 127) {
            const int shift = __builtin_clz((unsigned)(range + 1)) - 24;
            range = ((range + 1) << shift) - 1;
            value <<= shift;
            nb_bits += shift;
            if (nb_bits > 0) flush();
        }
    }
    CSM_BOOLENC_FN void put_bits(int v, int n) {
        for (int k = n - 1; k >= 0; --k) put(128, (v >> k) & 1);
    }
    CSM_BOOLENC_FN int64_t finish() {
        put_bits(0, 9 - nb_bits);
        nb_bits = 0;
        flush();
        if (held >= 0) emit(held);
        for (; run > 0; --run) emit(0xFF);
        return pos;
    }
};

}  // namespace csm
