// overlay.hip -- instance overlays (box outlines, alpha-blended masks, contours) drawn on the device, for gfx950.
//
//   csm_overlay_plan      checks the host job table and fills its tile words
//   csm_draw_instances    one launch (k_overlay) for a chunk of frames of any sizes; every tile walks its frame's whole draw list
//
// Every mask byte is read exactly once, which no exact form can undercut: per-tile instance lists need each mask's tight box, and
// csm_mask_bbox reads every mask byte to find it.  The binned form was built and measured; it lost at 100, 10 and 1 instances
//  and is not kept.
//
// A tile is 128 x 8 pixels and one workgroup; a lane owns 4 consecutive pixels of a row, so a mask row costs one 4-byte load per lane
// and instance (two where the row's address is not a multiple of 4: the two aligned words are funnel-shifted).  Colours, boxes and
// list entries are read at wave-uniform addresses.  The chain is d = fl(fl(d * (1 - a)) + fl(a * c)) in fp32 without contraction;
// no atomics, no float reduction: the bytes are deterministic.
#include "csm_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 128, kTileH = 8;  // 32 lanes x 4 px per row, 8 rows
constexpr int kJobWords = 16;
enum { jImg = 0, jOut = 1, jMasks = 2, jBoxes = 3, jH = 4, jW = 5, jN = 6, jK = 7, jFirst = 8, jLine = 9,
       jTile0 = 10, jTilesX = 11, jTiles = 12 };
enum { fBox = 1, fMask = 2, fContour = 4 };

struct Frame {
    const uint8_t *img, *masks;
    uint8_t *out;
    const int32_t *boxes;
    int H, W, k, first, a, b;
};

__device__ inline Frame load_frame(const int64_t *J) {
    Frame f;
    f.img = (const uint8_t *)J[jImg]; f.out = (uint8_t *)J[jOut]; f.masks = (const uint8_t *)J[jMasks];
    f.boxes = (const int32_t *)J[jBoxes];
    f.H = (int)J[jH]; f.W = (int)J[jW]; f.k = (int)J[jK]; f.first = (int)J[jFirst];
    f.a = (int)J[jLine] / 2; f.b = (int)J[jLine] - f.a;
    return f;
}

__device__ inline int find_job(const int64_t *jobs, int n_jobs, int tile) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[(int64_t)mid * kJobWords + jTile0] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline uint32_t nonzero_bytes(uint32_t v) {       // 0x01 in every byte of v that is not zero
    return ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) >> 7;
}

// the mask bytes of pixels x .. x + 3 of row y as 0 / 1 bytes (0 outside the frame).  Only aligned 4-byte words that hold at least
// one byte of the row are read.
__device__ inline uint32_t mask4(const uint8_t *M, int H, int W, int y, int x) {
    if (y < 0 || y >= H || x >= W) return 0;
    const int count = min(4, W - x);
    const uintptr_t p = (uintptr_t)(M + (int64_t)y * W + x);
    const uint32_t *q = (const uint32_t *)(p & ~(uintptr_t)3);
    const int sh = (int)(p & 3) * 8;
    uint32_t v = q[0] >> sh;
    if (sh && (int)(p & 3) + count > 4) v |= q[1] << (32 - sh);
    if (count < 4) v &= (1u << (8 * count)) - 1u;
    return nonzero_bytes(v);
}

__device__ inline uint32_t mask1(const uint8_t *M, int H, int W, int y, int x) {
    return (y >= 0 && y < H && x >= 0 && x < W && M[(int64_t)y * W + x]) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_overlay(const int64_t *__restrict__ jobs, int n_jobs, const int32_t *__restrict__ entries,
                                                     const uint8_t *__restrict__ colors, int flags, float alpha, float rest) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const int64_t *J = jobs + (int64_t)find_job(jobs, n_jobs, tile) * kJobWords;
    const Frame f = load_frame(J);
    const int tl = tile - (int)J[jTile0], tilesX = (int)J[jTilesX];
    const int x0 = (tl % tilesX) * kTileW, y0 = (tl / tilesX) * kTileH;
    const int x = x0 + (t & 31) * 4, y = y0 + (t >> 5);
    const int count = (y < f.H && x < f.W) ? min(4, f.W - x) : 0;          // this lane's pixels

    float d[12];
    const int64_t off = ((int64_t)y * f.W + x) * 3;
    const bool wide = count == 4 && (((uintptr_t)(f.img + off) | (uintptr_t)(f.out + off)) & 3) == 0;
    if (wide) {
        const uint32_t *s = (const uint32_t *)(f.img + off);
        for (int i = 0; i < 3; ++i) {
            const uint32_t v = s[i];
            for (int j = 0; j < 4; ++j) d[4 * i + j] = (float)((v >> (8 * j)) & 255u);
        }
    } else {
        for (int i = 0; i < 12; ++i) d[i] = i < 3 * count ? (float)f.img[off + i] : 0.0f;
    }

    // the frame's draw list, in list order: walk(body) calls body(instance, its colour)
    auto walk = [&](auto body) {
        for (int e = 0; e < f.k; ++e) body(entries[f.first + e], colors + 3 * (int64_t)(f.first + e));
    };

    if (flags & fBox) {
        walk([&](int inst, const uint8_t *c) {
            const int32_t *B = f.boxes + 4 * (int64_t)inst;
            const int64_t bx = B[0], by = B[1], ex = bx + B[2], ey = by + B[3];
            if (y < by - f.a || y > ey + f.a) return;
            const bool rowInside = y >= by + f.b && y <= ey - f.b;
            for (int p = 0; p < 4; ++p) {
                const int64_t px = x + p;
                if (px < bx - f.a || px > ex + f.a) continue;
                if (rowInside && px >= bx + f.b && px <= ex - f.b) continue;
                for (int ch = 0; ch < 3; ++ch) d[3 * p + ch] = (float)c[ch];
            }
        });
    }
    if (flags & fMask) {
        walk([&](int inst, const uint8_t *c) {
            const uint32_t m = mask4(f.masks + (int64_t)inst * f.H * f.W, f.H, f.W, y, x);
            if (!m) return;
            float ac[3];
            for (int ch = 0; ch < 3; ++ch) ac[ch] = __fmul_rn(alpha, (float)c[ch]);
            for (int p = 0; p < 4; ++p)
                if ((m >> (8 * p)) & 1u)
                    for (int ch = 0; ch < 3; ++ch) d[3 * p + ch] = __fadd_rn(__fmul_rn(d[3 * p + ch], rest), ac[ch]);
        });
        for (int i = 0; i < 12; ++i) d[i] = (float)(int)d[i];             // astype(uint8) of a value in [0, 255]: truncation
    }
    if (flags & fContour) {
        walk([&](int inst, const uint8_t *c) {
            const uint8_t *M = f.masks + (int64_t)inst * f.H * f.W;
            const uint32_t m = mask4(M, f.H, f.W, y, x);
            if (!m) return;
            const uint32_t left = (m << 8) | mask1(M, f.H, f.W, y, x - 1), right = (m >> 8) | (mask1(M, f.H, f.W, y, x + 4) << 24);
            const uint32_t edge = m & ~(mask4(M, f.H, f.W, y - 1, x) & mask4(M, f.H, f.W, y + 1, x) & left & right);
            for (int p = 0; p < 4; ++p)
                if ((edge >> (8 * p)) & 1u)
                    for (int ch = 0; ch < 3; ++ch) d[3 * p + ch] = (float)c[ch];
        });
    }

    if (wide) {
        uint32_t *o = (uint32_t *)(f.out + off);
        for (int i = 0; i < 3; ++i) {
            uint32_t v = 0;
            for (int j = 0; j < 4; ++j) v |= (uint32_t)(int)d[4 * i + j] << (8 * j);
            o[i] = v;
        }
    } else {
        for (int i = 0; i < 3 * count; ++i) f.out[off + i] = (uint8_t)(int)d[i];
    }
}

// the checks of a job that both entry points share; fills nothing
bool job_ok(const int64_t *J, int n_entries) {
    return J[jImg] && J[jOut] && J[jImg] != J[jOut] && J[jH] >= 1 && J[jW] >= 1 && J[jH] * J[jW] < INT32_MAX && J[jN] >= 0 &&
           J[jN] < INT32_MAX / 4 && J[jK] >= 0 && J[jFirst] >= 0 && J[jFirst] + J[jK] <= n_entries && J[jLine] >= 1 &&
           J[jLine] < (1 << 30) && (J[jK] == 0 || (J[jMasks] && J[jBoxes]));
}

}  // namespace

extern "C" int csm_overlay_job_words(void) { return kJobWords; }

extern "C" int csm_overlay_plan(int64_t *jobs_host, int n_jobs, int n_entries) {
    if (!jobs_host || n_jobs < 1 || n_entries < 0) return 0;
    int64_t tiles = 0;
    for (int i = 0; i < n_jobs; ++i) {
        int64_t *J = jobs_host + (int64_t)i * kJobWords;
        if (!job_ok(J, n_entries)) return 0;
        J[jTilesX] = (J[jW] + kTileW - 1) / kTileW;
        J[jTiles] = J[jTilesX] * ((J[jH] + kTileH - 1) / kTileH);
        J[jTile0] = tiles; J[13] = 0; J[14] = 0; J[15] = 0;
        tiles += J[jTiles];
        if (tiles >= INT32_MAX) return 0;
    }
    return (int)tiles;
}

extern "C" int csm_draw_instances(const int64_t *jobs_host, const int64_t *jobs_dev, int n_jobs, const int32_t *entries_host,
                                  const int32_t *entries_dev, const uint8_t *colors_dev, int n_entries, int flags, float alpha,
                                  float one_minus_alpha, void *stream) {
    CSM_REQUIRE(n_jobs >= 0 && n_entries >= 0 && (flags & ~(fBox | fMask | fContour)) == 0);
    if (n_jobs == 0) return CSM_OK;
    CSM_REQUIRE(jobs_host && jobs_dev && (n_entries == 0 || (entries_host && entries_dev && colors_dev)));
    int64_t tiles = 0;
    for (int i = 0; i < n_jobs; ++i) {                       // every job as csm_overlay_plan left it, every entry inside its frame's masks
        const int64_t *J = jobs_host + (int64_t)i * kJobWords;
        CSM_REQUIRE(job_ok(J, n_entries));
        CSM_REQUIRE(J[jTilesX] == (J[jW] + kTileW - 1) / kTileW && J[jTiles] == J[jTilesX] * ((J[jH] + kTileH - 1) / kTileH));
        CSM_REQUIRE(J[jTile0] == tiles);
        for (int64_t e = J[jFirst]; e < J[jFirst] + J[jK]; ++e) CSM_REQUIRE(entries_host[e] >= 0 && entries_host[e] < J[jN]);
        tiles += J[jTiles];
        CSM_REQUIRE(tiles < INT32_MAX);
    }
    k_overlay<<<(unsigned)tiles, kBlock, 0, (hipStream_t)stream>>>(jobs_dev, n_jobs, entries_dev, colors_dev, flags, alpha, one_minus_alpha);
    return csm::check_launch("k_overlay");
}
