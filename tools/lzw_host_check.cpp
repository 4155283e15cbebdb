// lzw_host_check.cpp -- the code walker of the GIF decoder (cartoonsegmentation_amd/csrc/csm_lzw.h) on the host, with a plain
// serial resolve behind it.  Built with the host compiler under -fsanitize=address,undefined (tests/test_gifdec.py), this is where
// truncated and mutated streams are exercised: every read and store of the walker has to stay inside its buffers.
//
//   lzw_host_check [-w BYTES] [-b RECORDS] [-x] - < LIST      lines "PIXELS MIN_CODE_SIZE FILE"; each FILE holds one image's LZW bytes
//     -w   read through a staging window of BYTES bytes (a multiple of 16, at least 16), as the kernel reads its input; without
//          it the window is the whole stream
//     -b   records per batch (default 64, the kernel's)
//     -x   print the indices too, in hexadecimal
// prints one line per file: the error word, the pixels produced, the FNV-1a hash of the indices (hexadecimal; 0 when the error
// word is not 0) and with -x the indices.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm_lzw.h"

namespace lzw = csm_lzw;

static uint32_t g_window = 0;
static int g_batch = 64;
static bool g_hex = false;

static int run(const char *path, uint32_t npix, int mcs) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fp);
    // exact sizes, so that the sanitizer sees every byte past a bound
    const uint32_t in_len = (uint32_t)in.size();
    std::vector<uint8_t> win(g_window ? g_window : in_len), idx(npix);
    if (!g_window) win = in;
    std::vector<lzw::Record> rec(g_batch);
    lzw::State S;
    lzw::Table *T = new lzw::Table;
    lzw::init(S, g_window ? 0 : in_len, in_len, mcs, npix);
    bool bad = false;
    for (;;) {
        int n = 0;
        const int status = lzw::step(S, *T, win.data(), rec.data(), g_batch, n);
        for (int k = 0; k < n; ++k) {                       // in stream order every source byte is final
            const lzw::Record r = rec[k];
            const uint32_t len = r.len & ~lzw::kLiteral;
            if (r.dst >= npix || len > npix - r.dst) { bad = true; break; }
            if (r.len & lzw::kLiteral) { idx[r.dst] = (uint8_t)r.src; continue; }
            if (r.src >= r.dst) { bad = true; break; }
            for (uint32_t i = 0; i < len; ++i) idx[r.dst + i] = idx[r.src + i];
        }
        if (bad || status == lzw::kDone) break;
        if (status == lzw::kNeedInput) {
            if (!g_window) { bad = true; break; }           // the window is the whole input: the walker must not ask
            const uint32_t base = lzw::byte_position(S) & ~15u;
            const uint32_t len = std::min(g_window, in_len - std::min(base, in_len));
            if (len) std::memcpy(win.data(), in.data() + base, len);
            lzw::restage(S, base, len);
        }
    }
    delete T;
    if (bad) { std::fprintf(stderr, "%s: a record outside the image\n", path); return 3; }
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < S.out; ++i) h = (h ^ idx[i]) * 16777619u;
    std::printf("%u %u %08x", S.err, S.out, S.err ? 0u : h);
    if (g_hex) {
        std::printf(" ");
        for (uint32_t i = 0; i < S.out; ++i) std::printf("%02x", idx[i]);
    }
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    while (argc >= 2 && argv[1][0] == '-' && argv[1][1]) {
        if (std::strcmp(argv[1], "-x") == 0) { g_hex = true; ++argv; --argc; continue; }
        if (argc < 3) break;
        if (std::strcmp(argv[1], "-w") == 0) {
            g_window = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            if (g_window < 16 || (g_window & 15)) { std::fprintf(stderr, "-w: a multiple of 16, at least 16\n"); return 2; }
        } else if (std::strcmp(argv[1], "-b") == 0) {
            g_batch = std::atoi(argv[2]);
            if (g_batch < 1 || g_batch > 65536) { std::fprintf(stderr, "-b: 1 .. 65536\n"); return 2; }
        } else {
            break;
        }
        argv += 2; argc -= 2;
    }
    if (argc == 2 && std::strcmp(argv[1], "-") == 0) {
        char path[4096];
        unsigned long npix;
        int mcs;
        while (std::scanf("%lu %d %4095s", &npix, &mcs, path) == 3)
            if (int rc = run(path, (uint32_t)npix, mcs)) return rc;
        return 0;
    }
    std::fprintf(stderr, "usage: %s [-w BYTES] [-b RECORDS] [-x] - < LIST\n", argv[0]);
    return 2;
}
