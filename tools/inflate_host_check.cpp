// inflate_host_check.cpp -- the symbol walker of the PNG decoder (cartoonsegmentation_amd/csrc/csm_inflate.h) on the host, with a
// plain serial resolve behind it.  Built with the host compiler under -fsanitize=address,undefined (tests/test_pngdec.py), this is
// where truncated and mutated streams are exercised: every read and store of the walker has to stay inside its buffers.
//
//   inflate_host_check RAW_SIZE FILE...      each FILE holds one zlib stream (RFC 1950); RAW_SIZE is the size its data must have
//   inflate_host_check - < LIST              lines "RAW_SIZE FILE"
//   inflate_host_check -w BYTES - < LIST     the same through a staging window of BYTES bytes (a multiple of 16, at least 1024), as
//                                            the kernel reads its input; without -w the window is the whole stream
// prints one line per file: the error word, the bytes produced, their Adler-32 (hexadecimal; 0 when the error word is not 0).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csm_inflate.h"

namespace inf = csm_inflate;

static uint32_t g_window = 0;

static int run(const char *path, uint32_t raw_size) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fp);
    uint32_t err = 0, out = 0, adler = 0;
    if (in.size() < 6) {
        err = inf::kErrInput;
    } else {
        // exact sizes, so that the sanitizer sees every byte past a bound
        const uint32_t in_len = (uint32_t)in.size() - 4, cap = raw_size / 3;
        const std::vector<uint8_t> data(in.begin(), in.begin() + in_len);
        std::vector<uint8_t> win(g_window ? g_window : in_len), lit(raw_size);
        if (!g_window) win = data;
        std::vector<uint32_t> matches(2 * (size_t)cap);
        inf::State S;
        inf::Tables *T = new inf::Tables;
        inf::init(S, g_window ? 0 : in_len, in_len, 2, raw_size, cap);
        bool begin = g_window != 0;
        for (;;) {
            const int status = begin ? (int)inf::kNeedInput : S.err ? (int)inf::kDone : inf::step(S, *T, win.data(), lit.data(), matches.data());
            begin = false;
            if (status == inf::kNeedInput) {
                if (!g_window) { S.err |= inf::kErrInput; continue; }          // the window is the whole input: nothing to stage
                const uint32_t base = inf::byte_position(S) & ~15u;
                const uint32_t len = std::min(g_window, in_len - std::min(base, in_len));
                if (len) std::memcpy(win.data(), data.data() + base, len);
                inf::restage(S, base, len);
            } else if (status == inf::kBuild) {
                inf::prepare(S, *T);
                inf::clear_fast(*T, 0, 1);
                if (!S.err) inf::fill_fast(S, *T, 0, 1);
            } else if (status == inf::kStored) {
                if (S.stored_len) std::memcpy(lit.data() + S.out, data.data() + S.stored_src, S.stored_len);
                inf::stored_done(S);
            } else {
                break;
            }
        }
        delete T;
        err = S.err; out = S.out;
        if (!err) {
            for (uint32_t m = 0; m < S.nmatch; ++m) {           // in stream order every source byte is final
                const uint32_t p = matches[2 * (size_t)m], len = (matches[2 * (size_t)m + 1] & 255u) + 3u,
                               dist = (matches[2 * (size_t)m + 1] >> 8) + 1u;
                for (uint32_t k = 0; k < len; ++k) lit[p + k] = lit[p + k - dist];
            }
            uint32_t s1 = 1, s2 = 0;
            for (uint32_t i = 0; i < out; ++i) { s1 = (s1 + lit[i]) % 65521u; s2 = (s2 + s1) % 65521u; }
            adler = s2 << 16 | s1;
            const uint8_t *t = in.data() + std::min(inf::byte_position(S), in_len);          // the trailer stands behind the deflate data
            if (adler != ((uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3])) err |= inf::kErrAdler;
        }
    }
    std::printf("%u %u %08x\n", err, out, err & ~(uint32_t)inf::kErrAdler ? 0u : adler);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::strcmp(argv[1], "-w") == 0) {
        g_window = (uint32_t)std::strtoul(argv[2], nullptr, 10);
        if (g_window < 1024 || (g_window & 15)) { std::fprintf(stderr, "-w: a multiple of 16, at least 1024\n"); return 2; }
        argv += 2; argc -= 2;
    }
    if (argc == 2 && std::strcmp(argv[1], "-") == 0) {
        char path[4096];
        unsigned long raw;
        while (std::scanf("%lu %4095s", &raw, path) == 2)
            if (int rc = run(path, (uint32_t)raw)) return rc;
        return 0;
    }
    if (argc < 3) { std::fprintf(stderr, "usage: %s RAW_SIZE FILE... | %s - < LIST\n", argv[0], argv[0]); return 2; }
    const uint32_t raw = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    for (int i = 2; i < argc; ++i)
        if (int rc = run(argv[i], raw)) return rc;
    return 0;
}
