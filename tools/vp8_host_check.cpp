// vp8_host_check.cpp -- the VP8 key-frame decoder of the lossy WebP reader (cartoonsegmentation_amd/csrc/csm_vp8dec.h) on the host:
// the walk over a frame's partitions, then reconstruction, loop filter and colour conversion macroblock by macroblock in raster
// order, with the same functions the kernels of csrc/webplossy.hip call.  Built with the host compiler under
// -fsanitize=address,undefined (tests/test_webplossy.py), this is where truncated and mutated streams are exercised: every read and
// store has to stay inside its buffers.
//
//   vp8_host_check - < LIST      lines "V WIDTH HEIGHT IN OUT": IN holds one VP8 chunk's bytes, WIDTH and HEIGHT are what the
//                                container's parser read from its header.  When the error word is 0, OUT ("-": nothing is written)
//                                receives int32 mbw, mbh, then per macroblock its 24-byte record, then the int16 coefficients
//                                [mbh * mbw][25][16], then the pixels as B, G, R bytes [HEIGHT][WIDTH][3].
//                                lines "A WIDTH HEIGHT IN OUT": IN holds one ALPH chunk's bytes; OUT receives the plane [HEIGHT][WIDTH]
// prints one line per file.  V: the error word (csm_vp8dec.h), partitions, filter type, probability updates, the bytes used of the
// first partition and of every token partition.  A: the error word, the VP8L stream's prefix-code groups.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm_vp8dec.h"
#include "csm_vp8l.h"

namespace vd = csm_vp8d;
namespace vp = csm_vp8l;

static bool read_file(const char *path, std::vector<uint8_t> &in) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return false; }
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fp);
    return true;
}

static vd::Plane make_plane(std::vector<uint8_t> &store, int mbw, int mbh, int size) {
    store.assign((size_t)vd::plane_bytes(mbw, mbh, size), 0);
    vd::Plane P{store.data() + vd::plane_origin(mbw, size), vd::plane_stride(mbw, size)};
    for (int x = -1; x < mbw * size + 4; ++x) P.p[-P.stride + x] = 127;
    for (int y = 0; y < mbh * size; ++y) P.p[(int64_t)y * P.stride - 1] = 129;
    return P;
}

static int run_vp8(unsigned W, unsigned H, const char *path, const char *out_path) {
    std::vector<uint8_t> in;
    if (!read_file(path, in)) return 2;
    const std::vector<uint8_t> data(in.begin(), in.end());             // exact size: the sanitizer sees every byte past the end
    const int mbw = (int)((W + 15) >> 4), mbh = (int)((H + 15) >> 4);
    std::vector<uint8_t> top_modes((size_t)4 * mbw), top_nz((size_t)9 * mbw);
    std::vector<vd::MbRec> recs((size_t)mbw * mbh);
    std::vector<int16_t> coef((size_t)mbw * mbh * vd::kCoefPerMb, 0);
    vd::WalkBufs B{top_modes.data(), top_nz.data(), recs.data(), coef.data()};
    vd::Header *h = new vd::Header;
    vd::Bool first, parts[vd::kMaxParts];
    vd::Frame F;
    vd::walk_frame(*h, first, parts, data.data(), (uint32_t)data.size(), W, H, B, F);
    delete h;
    if (!F.err && std::strcmp(out_path, "-") != 0) {
        std::vector<uint8_t> sy, su, sv;
        const vd::Plane Y = make_plane(sy, mbw, mbh, 16), U = make_plane(su, mbw, mbh, 8), V = make_plane(sv, mbw, mbh, 8);
        for (int y = 0; y < mbh; ++y)
            for (int x = 0; x < mbw; ++x) {
                const vd::MbRec &m = recs[(size_t)y * mbw + x];
                const int16_t *c = coef.data() + ((size_t)y * mbw + x) * vd::kCoefPerMb;
                vd::recon_luma(Y, x, y, mbw, m, c);
                vd::recon_chroma(U, V, x, y, m, c);
            }
        if (F.filter_type)
            for (int y = 0; y < mbh; ++y)
                for (int x = 0; x < mbw; ++x) {
                    const vd::MbRec &m = recs[(size_t)y * mbw + x];
                    vd::filter_mb(Y, 16, x, y, m, F.filter_type == 1);
                    if (F.filter_type == 2) { vd::filter_mb(U, 8, x, y, m, false); vd::filter_mb(V, 8, x, y, m, false); }
                }
        std::vector<uint8_t> px((size_t)W * H * 3);
        for (unsigned y = 0; y < H; ++y)
            for (unsigned x = 0; x < W; ++x) {
                const uint32_t v = vd::pixel_bgr(Y, U, V, (int)x, (int)y, (int)W, (int)H);
                uint8_t *q = px.data() + ((size_t)y * W + x) * 3;
                q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16);
            }
        FILE *fo = std::fopen(out_path, "wb");
        if (!fo) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
        const int32_t dims[2] = {mbw, mbh};
        std::fwrite(dims, 4, 2, fo);
        std::fwrite(recs.data(), sizeof(vd::MbRec), recs.size(), fo);
        std::fwrite(coef.data(), 2, coef.size(), fo);
        std::fwrite(px.data(), 1, px.size(), fo);
        std::fclose(fo);
    }
    std::printf("%u %d %d %u", F.err, F.nparts, F.filter_type, F.prob_updates);
    for (int k = 0; k <= vd::kMaxParts; ++k) std::printf(" %u", F.used[k]);
    std::printf("\n");
    return 0;
}

static int run_alpha(unsigned W, unsigned H, const char *path, const char *out_path) {
    std::vector<uint8_t> in;
    if (!read_file(path, in)) return 2;
    const std::vector<uint8_t> data(in.begin(), in.end());
    uint32_t err = 0, ngroups = 0;
    std::vector<uint8_t> plane((size_t)W * H, 0);
    const int head = data.empty() ? 0xff : data[0], comp = head & 3, filter = (head >> 2) & 3;
    if (data.empty() || comp > 1 || (head >> 6)) {
        err = vd::kErrAlpha;
    } else if (comp == 0) {
        if (data.size() - 1 < plane.size()) err = vd::kErrAlpha;
        else std::memcpy(plane.data(), data.data() + 1, plane.size());
    } else {
        const uint32_t sub_cap = vp::subsample(W, 2) * vp::subsample(H, 2), group_cap = sub_cap < vp::kGroupCap ? sub_cap : vp::kGroupCap;
        std::vector<uint32_t> a((size_t)W * H), b((size_t)W * H), pred(sub_cap), colour(sub_cap), meta(sub_cap), palette(256), cache(1 << vp::kMaxCacheBits);
        std::vector<vp::Group> groups(group_cap);
        vp::Bufs B;
        B.argb = a.data(); B.pred = pred.data(); B.colour = colour.data(); B.meta = meta.data(); B.palette = palette.data();
        B.cache = cache.data(); B.groups = groups.data(); B.sub_cap = sub_cap; B.group_cap = group_cap;
        vp::State *S = new vp::State;
        vp::Result R;
        std::memset(&R, 0, sizeof R);
        const std::vector<uint8_t> stream(data.begin() + 1, data.end());
        vp::decode_headerless(*S, B, stream.data(), (uint32_t)stream.size(), W, H, R);
        delete S;
        ngroups = R.ngroups;
        if (R.err) {
            err = R.err << vd::kErrAlphaShift;
        } else {
            const uint32_t *px = vp::apply_transforms_host(R, B, a.data(), b.data(), H);
            for (size_t i = 0; i < plane.size(); ++i) plane[i] = (uint8_t)(px[i] >> 8);
        }
    }
    if (!err && filter)
        for (unsigned y = 0; y < H; ++y)
            for (unsigned x = 0; x < W; ++x) {
                uint8_t *p = plane.data() + (size_t)y * W + x;
                const int L = x ? p[-1] : 0, T = y ? p[-(int64_t)W] : 0, TL = x && y ? p[-(int64_t)W - 1] : 0;
                *p = (uint8_t)(*p + vd::alpha_predict(filter, (int)x, (int)y, L, T, TL));
            }
    if (!err && std::strcmp(out_path, "-") != 0) {
        FILE *fo = std::fopen(out_path, "wb");
        if (!fo) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
        std::fwrite(plane.data(), 1, plane.size(), fo);
        std::fclose(fo);
    }
    std::printf("%u %u\n", err, ngroups);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2 || std::strcmp(argv[1], "-") != 0) { std::fprintf(stderr, "usage: %s - < LIST   (lines: V|A WIDTH HEIGHT IN OUT)\n", argv[0]); return 2; }
    char kind[8], path[4096], out_path[4096];
    unsigned W, H;
    while (std::scanf("%7s %u %u %4095s %4095s", kind, &W, &H, path, out_path) == 5) {
        if (W < 1 || H < 1 || W > 16383 || H > 16383) { std::fprintf(stderr, "invalid size\n"); return 2; }
        if (int rc = kind[0] == 'A' ? run_alpha(W, H, path, out_path) : run_vp8(W, H, path, out_path)) return rc;
    }
    return 0;
}
