// patchmatch.hip -- PatchMatch inpainting on the device, for gfx950 (Barnes et al. 2009 nearest-neighbour search, coarse-to-fine
// EM completion after Wexler et al. 2007): the `patch_match.inpaint(img, mask, patch_size)` of the Ken Burns patchmatch path,
// repaint_person.py and run_style.py.  The contract is ours, integer-exact and deterministic; the numpy
// restatement tests/patchmatch_restatement.py returns the same bytes.
//
// Pyramid: level l + 1 = ceil(h / 2) x ceil(w / 2); a pixel is known when one of its 2x2 children is (rounded integer mean of the
// known ones), excluded when one is.  Centres are the interior pixels [r, h - r) x [r, w - r), r = p / 2; a valid source is a
// centre whose window holds no hole and no excluded pixel, a target one whose window touches a hole.  The texels are RGBA8 (one
// 4-byte load per pixel); the NNF holds level-local source indices sy * w + sx.
//
//   prepare: k_pm_init (level 0) -> k_pm_down per level -> k_pm_roles (roles + per-block counts, every level in one launch)
//            -> k_pm_scan (one block per level: block offsets, info) -> k_pm_lists (ordered compaction of the valid sources,
//            targets and hole pixels of every level)
//   run:     coarsest: k_pm_mean_sum, k_pm_mean_fill, k_pm_nnf_init; finer: k_pm_upsample, k_pm_nnf_init; every level
//            em_iters x (nnf_passes x k_pm_nnf_pass, k_pm_vote); k_pm_output
// The run kernels launch over the compacted targets / hole pixels of a level, so the work follows the hole area.  No atomics but
// the integer sums of the coarsest mean (order-free), no grid-wide waits; the host reads the info array once, between the calls.
#include "csm_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxLevels = 32;
constexpr int kJump = 4;                      // the longer propagation step
constexpr unsigned kInitPass = 0xFFFF;        // the `pass` field of the hash for the initial draws
constexpr uint8_t kKnown = 1, kExcl = 2;      // flags
constexpr uint8_t kValid = 1, kTarget = 2, kHole = 4;   // roles

struct Levels {
    int n;
    int off[kMaxLevels];     // first pixel of the level in the concatenated (256-padded) arrays
    int h[kMaxLevels], w[kMaxLevels];
};

int em_iters(int l) { return l < 4 ? 2 + 2 * l : 10; }
int nnf_passes(int l) { return l < 4 ? 2 + l : 6; }

__host__ __device__ inline int64_t pad256(int64_t n) { return (n + 255) / 256 * 256; }

bool shape_ok(int H, int W, int p) {
    return p >= 3 && p <= 15 && (p & 1) && H >= p && W >= p && (int64_t)H * W <= (1 << 28);
}

Levels make_levels(int H, int W, int p) {
    Levels L{};
    int h = H, w = W;
    int64_t off = 0;
    for (;;) {
        L.off[L.n] = (int)off; L.h[L.n] = h; L.w[L.n] = w;
        off += pad256((int64_t)h * w);
        ++L.n;
        if (L.n == kMaxLevels || (h + 1) / 2 <= p || (w + 1) / 2 <= p) break;
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    return L;
}

int64_t total_pixels(const Levels &L) { return L.off[L.n - 1] + pad256((int64_t)L.h[L.n - 1] * L.w[L.n - 1]); }

struct Scratch {
    uint32_t *col;           // RGBA8 texels
    uint8_t *flags, *roles;
    int *nnf[2];
    uint32_t *wgt;           // vote weight of each target's match
    int *lists[3];           // valid sources, targets, hole pixels (level-local indices, ascending)
    int *blk;                // per 256-pixel block: [3] counts, then exclusive offsets
    unsigned long long *sums;   // coarsest mean: r, g, b, n
    size_t bytes;
};

Scratch layout(const Levels &L, void *base) {
    const int64_t N = total_pixels(L);
    char *p = (char *)base;
    size_t o = 0;
    auto take = [&](size_t b) { char *q = p + o; o += (b + 255) / 256 * 256; return q; };
    Scratch s;
    s.col = (uint32_t *)take(N * 4);
    s.flags = (uint8_t *)take(N);
    s.roles = (uint8_t *)take(N);
    s.nnf[0] = (int *)take(N * 4);
    s.nnf[1] = (int *)take(N * 4);
    s.wgt = (uint32_t *)take(N * 4);
    for (int k = 0; k < 3; ++k) s.lists[k] = (int *)take(N * 4);
    s.blk = (int *)take(N / 256 * 3 * 4);
    s.sums = (unsigned long long *)take(4 * 8);
    s.bytes = o;
    return s;
}

// ---- hash (tests/patchmatch_restatement.py rng) ------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    return x ^ (x >> 16);
}

// the per-(seed, level, iteration, pass) prefix of the hash; the kernels finish it with the pixel and the sample
uint32_t hash_base(uint32_t seed, int level, int it, unsigned pass) {
    uint32_t h = mix32(seed ^ 0x9E3779B9u);
    h = mix32(h ^ (uint32_t)level);
    h = mix32(h ^ (uint32_t)it);
    return mix32(h ^ pass);
}

__device__ __forceinline__ uint32_t hash_px(uint32_t base, int pixel, uint32_t sample) {
    return mix32(mix32(base ^ (uint32_t)pixel) ^ sample);
}

__device__ __forceinline__ int level_of(const Levels &L, int g) {
    int l = 0;
    while (l + 1 < L.n && g >= L.off[l + 1]) ++l;
    return l;
}

// ---- prepare ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_pm_init(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask,
                                                     const uint8_t *__restrict__ gmask, int n, uint32_t *__restrict__ col,
                                                     uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    col[i] = img[3 * i] | (img[3 * i + 1] << 8) | (img[3 * i + 2] << 16);
    flags[i] = (mask[i] ? 0 : kKnown) | (gmask && gmask[i] ? kExcl : 0);
}

__global__ __launch_bounds__(kBlock) void k_pm_down(const uint32_t *__restrict__ ci, const uint8_t *__restrict__ fi, int hi, int wi,
                                                     uint32_t *__restrict__ co, uint8_t *__restrict__ fo, int ho, int wo) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ho * wo) return;
    const int y = i / wo, x = i - y * wo;
    unsigned s0 = 0, s1 = 0, s2 = 0, n = 0;
    uint8_t f = 0;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int yy = 2 * y + dy, xx = 2 * x + dx;
            if (yy >= hi || xx >= wi) continue;
            const int j = yy * wi + xx;
            const uint8_t fc = fi[j];
            f |= fc;
            if (fc & kKnown) {
                const uint32_t c = ci[j];
                s0 += c & 255; s1 += (c >> 8) & 255; s2 += (c >> 16) & 255; ++n;
            }
        }
    uint32_t c = 0;
    if (n) c = ((s0 + n / 2) / n) | (((s1 + n / 2) / n) << 8) | (((s2 + n / 2) / n) << 16);
    co[i] = c;
    fo[i] = f;
}

// roles of every pixel of every level, and per block the number of valid sources / targets / hole pixels
__global__ __launch_bounds__(kBlock) void k_pm_roles(Levels L, int r, const uint8_t *__restrict__ flags, uint8_t *__restrict__ roles,
                                                      int *__restrict__ blk) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const int l = level_of(L, g);
    const int h = L.h[l], w = L.w[l], i = g - L.off[l];
    uint8_t role = 0;
    if (i < h * w) {
        const uint8_t *F = flags + L.off[l];
        const int y = i / w, x = i - y * w;
        if (!(F[i] & kKnown)) role |= kHole;
        if (y >= r && y < h - r && x >= r && x < w - r) {
            bool bad = false, hole = false;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const uint8_t f = F[i + dy * w + dx];
                    hole |= !(f & kKnown);
                    bad |= !(f & kKnown) || (f & kExcl);
                }
            if (!bad) role |= kValid;
            if (hole) role |= kTarget;
        }
        roles[g] = role;
    }
    __shared__ int cnt[kBlock / 64][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cv = __popcll(__ballot(role & kValid)), ct = __popcll(__ballot(role & kTarget)), ch = __popcll(__ballot(role & kHole));
    if (lane == 0) { cnt[wv][0] = cv; cnt[wv][1] = ct; cnt[wv][2] = ch; }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
        for (int k = 0; k < kBlock / 64; ++k) s += cnt[k][threadIdx.x];
        blk[blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// one block per level: exclusive offsets of the level's blocks (in place) and info[l] = {valid, targets, holes, known}
__global__ __launch_bounds__(kBlock) void k_pm_scan(Levels L, int *__restrict__ blk, int *__restrict__ info) {
    const int l = blockIdx.x;
    const int b0 = L.off[l] / kBlock, nb = (int)(pad256((int64_t)L.h[l] * L.w[l]) / kBlock);
    __shared__ int part[kBlock];
    int carry[3] = {0, 0, 0};
    for (int c0 = 0; c0 < nb; c0 += kBlock) {
        const int b = c0 + threadIdx.x;
        for (int k = 0; k < 3; ++k) {
            const int v = b < nb ? blk[(b0 + b) * 3 + k] : 0;
            part[threadIdx.x] = v;
            __syncthreads();
            for (int s = 1; s < kBlock; s <<= 1) {          // Hillis-Steele inclusive scan
                const int t = threadIdx.x >= s ? part[threadIdx.x - s] : 0;
                __syncthreads();
                part[threadIdx.x] += t;
                __syncthreads();
            }
            if (b < nb) blk[(b0 + b) * 3 + k] = carry[k] + part[threadIdx.x] - v;
            carry[k] += part[kBlock - 1];
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        info[4 * l + 0] = carry[0]; info[4 * l + 1] = carry[1]; info[4 * l + 2] = carry[2];
        info[4 * l + 3] = L.h[l] * L.w[l] - carry[2];
    }
}

// ordered compaction: each block writes its pixels of each role at its offset, in pixel order (wave ballot prefix)
__global__ __launch_bounds__(kBlock) void k_pm_lists(Levels L, const uint8_t *__restrict__ roles, const int *__restrict__ blk,
                                                      int *__restrict__ lv, int *__restrict__ lt, int *__restrict__ lh) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const int l = level_of(L, g);
    const int i = g - L.off[l];
    const uint8_t role = i < L.h[l] * L.w[l] ? roles[g] : 0;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int cnt[3][kBlock / 64];
    int *lists[3] = {lv, lt, lh};
    const uint8_t bits[3] = {kValid, kTarget, kHole};
    const unsigned long long below = (1ull << lane) - 1;
    unsigned long long m[3];
    for (int k = 0; k < 3; ++k) {
        m[k] = __ballot(role & bits[k]);
        if (lane == 0) cnt[k][wv] = __popcll(m[k]);
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        if (!(role & bits[k])) continue;
        int pos = blk[blockIdx.x * 3 + k] + __popcll(m[k] & below);
        for (int v = 0; v < wv; ++v) pos += cnt[k][v];
        lists[k][L.off[l] + pos] = i;
    }
}

// ---- run ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_pm_mean_sum(const uint32_t *__restrict__ col, const uint8_t *__restrict__ flags, int n,
                                                         unsigned long long *__restrict__ sums) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    unsigned v[4] = {0, 0, 0, 0};
    if (i < n && (flags[i] & kKnown)) {
        const uint32_t c = col[i];
        v[0] = c & 255; v[1] = (c >> 8) & 255; v[2] = (c >> 16) & 255; v[3] = 1;
    }
    __shared__ unsigned part[kBlock / 64][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 4; ++k) {
        unsigned s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) part[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
        for (int k = 0; k < kBlock / 64; ++k) s += part[k][threadIdx.x];
        if (s) atomicAdd(sums + threadIdx.x, s);
    }
}

__global__ __launch_bounds__(kBlock) void k_pm_mean_fill(uint32_t *__restrict__ col, const int *__restrict__ holes, int nh,
                                                          const unsigned long long *__restrict__ sums) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nh) return;
    const unsigned long long n = sums[3];
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ++ch) c |= (uint32_t)((sums[ch] + n / 2) / n) << (8 * ch);
    col[holes[k]] = c;
}

// hole pixels of a finer level start from the colour of their parent
__global__ __launch_bounds__(kBlock) void k_pm_upsample(uint32_t *__restrict__ col, int w, const int *__restrict__ holes, int nh,
                                                         const uint32_t *__restrict__ pcol, int pw) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nh) return;
    const int q = holes[k], y = q / w, x = q - y * w;
    col[q] = pcol[(y >> 1) * pw + (x >> 1)];
}

// NNF of each target: 2 s_parent + (t mod 2) when that is a valid source, else a uniform draw from the valid sources
__global__ __launch_bounds__(kBlock) void k_pm_nnf_init(const int *__restrict__ targets, int nt, const int *__restrict__ valid, int nv,
                                                         const uint8_t *__restrict__ roles, int h, int w,
                                                         const uint8_t *__restrict__ proles, const int *__restrict__ pnnf, int pw,
                                                         uint32_t base, int *__restrict__ nnf) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nt) return;
    const int t = targets[k], ty = t / w, tx = t - ty * w;
    if (pnnf) {
        const int pi = (ty >> 1) * pw + (tx >> 1);
        if (proles[pi] & kTarget) {
            const int sp = pnnf[pi], sy = sp / pw, sx = sp - sy * pw;
            const int cy = 2 * sy + (ty & 1), cx = 2 * sx + (tx & 1);
            if (cy < h && cx < w && (roles[cy * w + cx] & kValid)) { nnf[t] = cy * w + cx; return; }
        }
    }
    nnf[t] = valid[hash_px(base, t, 0) % (uint32_t)nv];
}

// SSD of the p x p x 3 windows centred at t and s; returns early (a value >= best) once a row ends at or above best
__device__ __forceinline__ int patch_ssd(const uint32_t *__restrict__ col, int w, int r, int t, int s, int best) {
    const uint32_t *a = col + t - r * w - r, *b = col + s - r * w - r;
    int d = 0;
    for (int dy = 0; dy <= 2 * r; ++dy) {
        for (int dx = 0; dx <= 2 * r; ++dx) {
            const uint32_t u = a[dx], v = b[dx];
            const int e0 = (int)(u & 255) - (int)(v & 255);
            const int e1 = (int)((u >> 8) & 255) - (int)((v >> 8) & 255);
            const int e2 = (int)((u >> 16) & 255) - (int)((v >> 16) & 255);
            d += e0 * e0 + e1 * e1 + e2 * e2;
        }
        if (d >= best) return d;
        a += w; b += w;
    }
    return d;
}

// one Jacobi pass: candidates in the contract's order (current, propagation at 1 and kJump, random search); strictly smaller wins
__global__ __launch_bounds__(kBlock) void k_pm_nnf_pass(const uint32_t *__restrict__ col, const uint8_t *__restrict__ roles, int h,
                                                         int w, int r, const int *__restrict__ targets, int nt,
                                                         const int *__restrict__ nin, int *__restrict__ nout,
                                                         uint32_t *__restrict__ wgt, uint32_t base, uint32_t P) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nt) return;
    const int t = targets[k], ty = t / w, tx = t - ty * w;
    int best = nin[t];
    int by = best / w, bx = best - by * w;
    int bd = patch_ssd(col, w, r, t, best, INT32_MAX);
    auto consider = [&](int cy, int cx) {
        if (cy < 0 || cy >= h || cx < 0 || cx >= w) return;
        const int c = cy * w + cx;
        if (!(roles[c] & kValid)) return;
        const int d = patch_ssd(col, w, r, t, c, bd);
        if (d < bd) { bd = d; by = cy; bx = cx; }
    };
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int s = j ? kJump : 1;
        const int dys[4] = {0, 0, -s, s}, dxs[4] = {-s, s, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ny = ty + dys[e], nx = tx + dxs[e];
            if (ny < 0 || ny >= h || nx < 0 || nx >= w) continue;
            const int n = ny * w + nx;
            if (!(roles[n] & kTarget)) continue;
            const int sn = nin[n], sy = sn / w, sx = sn - sy * w;
            consider(sy - dys[e], sx - dxs[e]);
        }
    }
    uint32_t j = 0;
    for (int R = max(h, w); R >= 1; R >>= 1, ++j) {
        const uint32_t m = 2u * R + 1;
        const int oy = (int)(hash_px(base, t, 2 * j) % m) - R;
        const int ox = (int)(hash_px(base, t, 2 * j + 1) % m) - R;
        consider(by + oy, bx + ox);
    }
    nout[t] = by * w + bx;
    wgt[t] = (uint32_t)(((uint64_t)P << 16) / ((uint64_t)P + (uint64_t)bd));
}

// M-step: each hole pixel takes the weighted mean of the colours every covering target's match puts there (known pixels only)
__global__ __launch_bounds__(kBlock) void k_pm_vote(uint32_t *__restrict__ col, int h, int w, int r, const int *__restrict__ holes,
                                                     int nh, const int *__restrict__ nnf, const uint32_t *__restrict__ wgt) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nh) return;
    const int q = holes[k], qy = q / w, qx = q - qy * w;
    uint64_t sw = 0, s0 = 0, s1 = 0, s2 = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int ty = qy - dy;
        if (ty < r || ty >= h - r) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int tx = qx - dx;
            if (tx < r || tx >= w - r) continue;
            const int t = ty * w + tx;
            const uint64_t wt = wgt[t];
            const uint32_t c = col[nnf[t] + dy * w + dx];
            sw += wt; s0 += wt * (c & 255); s1 += wt * ((c >> 8) & 255); s2 += wt * ((c >> 16) & 255);
        }
    }
    col[q] = (uint32_t)((s0 + sw / 2) / sw) | ((uint32_t)((s1 + sw / 2) / sw) << 8) | ((uint32_t)((s2 + sw / 2) / sw) << 16);
}

__global__ __launch_bounds__(kBlock) void k_pm_output(const uint32_t *__restrict__ col, int n, uint8_t *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = col[i];
    out[3 * i] = c & 255; out[3 * i + 1] = (c >> 8) & 255; out[3 * i + 2] = (c >> 16) & 255;
}

}  // namespace

extern "C" int csm_patchmatch_levels(int H, int W, int p) { return shape_ok(H, W, p) ? make_levels(H, W, p).n : 0; }

extern "C" size_t csm_patchmatch_scratch_bytes(int H, int W, int p) {
    if (!shape_ok(H, W, p)) return 0;
    return layout(make_levels(H, W, p), nullptr).bytes;
}

extern "C" int csm_patchmatch_prepare(const uint8_t *img, const uint8_t *mask, const uint8_t *global_mask, int H, int W, int p,
                                      int *info, void *scratch, void *stream) {
    CSM_REQUIRE(shape_ok(H, W, p));
    CSM_REQUIRE(img && mask && info && scratch);
    const Levels L = make_levels(H, W, p);
    const Scratch S = layout(L, scratch);
    hipStream_t st = (hipStream_t)stream;
    k_pm_init<<<csm::cdiv((int64_t)H * W, kBlock), kBlock, 0, st>>>(img, mask, global_mask, H * W, S.col, S.flags);
    int rc = csm::check_launch("k_pm_init"); if (rc) return rc;
    for (int l = 1; l < L.n; ++l) {
        k_pm_down<<<csm::cdiv((int64_t)L.h[l] * L.w[l], kBlock), kBlock, 0, st>>>(S.col + L.off[l - 1], S.flags + L.off[l - 1], L.h[l - 1],
                                                                               L.w[l - 1], S.col + L.off[l], S.flags + L.off[l], L.h[l], L.w[l]);
        rc = csm::check_launch("k_pm_down"); if (rc) return rc;
    }
    const unsigned nblk = (unsigned)(total_pixels(L) / kBlock);
    k_pm_roles<<<nblk, kBlock, 0, st>>>(L, p / 2, S.flags, S.roles, S.blk);
    rc = csm::check_launch("k_pm_roles"); if (rc) return rc;
    k_pm_scan<<<L.n, kBlock, 0, st>>>(L, S.blk, info);
    rc = csm::check_launch("k_pm_scan"); if (rc) return rc;
    k_pm_lists<<<nblk, kBlock, 0, st>>>(L, S.roles, S.blk, S.lists[0], S.lists[1], S.lists[2]);
    return csm::check_launch("k_pm_lists");
}

extern "C" int csm_patchmatch_run(int H, int W, int p, int levels, const int *info_host, unsigned seed, uint8_t *out, void *scratch,
                                  void *stream) {
    CSM_REQUIRE(shape_ok(H, W, p));
    CSM_REQUIRE(info_host && out && scratch);
    const Levels L = make_levels(H, W, p);
    CSM_REQUIRE(levels >= 1 && levels <= L.n);
    for (int l = 0; l < levels; ++l) CSM_REQUIRE(info_host[4 * l] > 0);     // every scheduled level has a valid source
    const Scratch S = layout(L, scratch);
    hipStream_t st = (hipStream_t)stream;
    const int r = p / 2;
    const uint32_t P = 3u * p * p * 64;
    int rc;
    int cur = 0;                                       // NNF buffer holding the last pass of the level above
    if (info_host[1] > 0) {
        for (int l = levels - 1; l >= 0; --l) {
            const int h = L.h[l], w = L.w[l], o = L.off[l];
            const int nv = info_host[4 * l], nt = info_host[4 * l + 1], nh = info_host[4 * l + 2];
            const int *valid = S.lists[0] + o, *targets = S.lists[1] + o, *holes = S.lists[2] + o;
            uint32_t *col = S.col + o;
            const unsigned gt = csm::cdiv(nt, kBlock), gh = csm::cdiv(nh, kBlock);
            const bool top = l == levels - 1;
            if (top) {
                if (nh > 0) {
                    CSM_HIP(hipMemsetAsync(S.sums, 0, 4 * sizeof(unsigned long long), st));
                    k_pm_mean_sum<<<csm::cdiv((int64_t)h * w, kBlock), kBlock, 0, st>>>(col, S.flags + o, h * w, S.sums);
                    rc = csm::check_launch("k_pm_mean_sum"); if (rc) return rc;
                    k_pm_mean_fill<<<gh, kBlock, 0, st>>>(col, holes, nh, S.sums);
                    rc = csm::check_launch("k_pm_mean_fill"); if (rc) return rc;
                }
            } else if (nh > 0) {
                k_pm_upsample<<<gh, kBlock, 0, st>>>(col, w, holes, nh, S.col + L.off[l + 1], L.w[l + 1]);
                rc = csm::check_launch("k_pm_upsample"); if (rc) return rc;
            }
            if (nt == 0) continue;                     // a coarse level without holes: nothing to search
            const int po = top ? 0 : L.off[l + 1];
            k_pm_nnf_init<<<gt, kBlock, 0, st>>>(targets, nt, valid, nv, S.roles + o, h, w, top ? nullptr : S.roles + po,
                                                 top ? nullptr : S.nnf[cur] + po, top ? 0 : L.w[l + 1],
                                                 hash_base(seed, l, 0, kInitPass), S.nnf[0] + o);
            rc = csm::check_launch("k_pm_nnf_init"); if (rc) return rc;
            cur = 0;
            for (int it = 0; it < em_iters(l); ++it) {
                for (int ps = 0; ps < nnf_passes(l); ++ps) {
                    k_pm_nnf_pass<<<gt, kBlock, 0, st>>>(col, S.roles + o, h, w, r, targets, nt, S.nnf[cur] + o, S.nnf[cur ^ 1] + o,
                                                         S.wgt + o, hash_base(seed, l, it, ps), P);
                    rc = csm::check_launch("k_pm_nnf_pass"); if (rc) return rc;
                    cur ^= 1;
                }
                k_pm_vote<<<gh, kBlock, 0, st>>>(col, h, w, r, holes, nh, S.nnf[cur] + o, S.wgt + o);
                rc = csm::check_launch("k_pm_vote"); if (rc) return rc;
            }
        }
    }
    k_pm_output<<<csm::cdiv((int64_t)H * W, kBlock), kBlock, 0, st>>>(S.col, H * W, out);
    return csm::check_launch("k_pm_output");
}
