// vp8l_host_check.cpp -- the symbol walker of the lossless WebP decoder (cartoonsegmentation_amd/csrc/csm_vp8l.h) on the host, with
// the inverse transforms applied serially behind it.  Built with the host compiler under -fsanitize=address,undefined
// (tests/test_webpdec.py), this is where truncated and mutated streams are exercised: every read and store of the walker has to stay
// inside its buffers.
//
//   vp8l_host_check - < LIST      lines "WIDTH HEIGHT IN OUT": IN holds one VP8L payload (the chunk's bytes), WIDTH and HEIGHT are
//                                 what the container's parser read from its header; OUT receives the decoded pixels as little-endian
//                                 uint32 ARGB [HEIGHT][WIDTH] when the error word is 0 ("-": nothing is written)
// prints one line per file: the error word (csm_vp8l.h), the prefix-code groups, the bytes of the payload the walker consumed, the
// header's alpha flag.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm_vp8l.h"

namespace vp = csm_vp8l;

static int run(unsigned W, unsigned H, const char *path, const char *out_path) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fp);
    if (W < 1 || H < 1 || W > 16384 || H > 16384) { std::fprintf(stderr, "invalid size\n"); return 2; }
    // exact sizes, as the kernel's plan gives them, so that the sanitizer sees every element past a bound
    const uint32_t sub_cap = vp::subsample(W, 2) * vp::subsample(H, 2), group_cap = sub_cap < vp::kGroupCap ? sub_cap : vp::kGroupCap;
    const std::vector<uint8_t> data(in.begin(), in.end());
    std::vector<uint32_t> a((size_t)W * H), b((size_t)W * H), pred(sub_cap), colour(sub_cap), meta(sub_cap), palette(256), cache(1 << vp::kMaxCacheBits);
    std::vector<vp::Group> groups(group_cap);
    vp::Bufs B;
    B.argb = a.data(); B.pred = pred.data(); B.colour = colour.data(); B.meta = meta.data(); B.palette = palette.data();
    B.cache = cache.data(); B.groups = groups.data(); B.sub_cap = sub_cap; B.group_cap = group_cap;
    vp::State *S = new vp::State;
    vp::Result R;
    std::memset(&R, 0, sizeof R);
    vp::decode_file(*S, B, data.data(), (uint32_t)data.size(), W, H, R);
    delete S;
    if (!R.err && std::strcmp(out_path, "-") != 0) {
        const uint32_t *px = vp::apply_transforms_host(R, B, a.data(), b.data(), H);
        FILE *fo = std::fopen(out_path, "wb");
        if (!fo) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
        std::fwrite(px, 4, (size_t)W * H, fo);
        std::fclose(fo);
    }
    std::printf("%u %u %u %d\n", R.err, R.ngroups, R.bytes_used, R.has_alpha);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2 || std::strcmp(argv[1], "-") != 0) { std::fprintf(stderr, "usage: %s - < LIST   (lines: WIDTH HEIGHT IN OUT)\n", argv[0]); return 2; }
    char path[4096], out_path[4096];
    unsigned W, H;
    while (std::scanf("%u %u %4095s %4095s", &W, &H, path, out_path) == 4)
        if (int rc = run(W, H, path, out_path)) return rc;
    return 0;
}
