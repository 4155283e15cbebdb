// maskrle.hip -- COCO compressed RLE of instance masks on the device, for gfx950: the strings of
// pycocotools.mask.encode(np.asfortranarray(m[..., None] > 0).astype(np.uint8))[0]['counts'] (maskApi.c rleEncode + rleToString),
// which utils/io_utils.py mask2rle stores in the annotation files of AnimeInsSeg.infer(save_annotation=...).
//
// The run-length sequence walks the mask in column-major order (j = x * H + y) starting from the value 0; a transition at j is a
// pixel whose value differs from pixel j - 1 (for y = 0 that is (H - 1, x - 1), for j = 0 the start value 0).  With the transitions
// t_0 < t_1 < ... < t_{T-1}, t_{-1} = 0 and t_T = H * W, count g is t_g - t_{g-1} (g = 0..T) and the string stores
//   d_g = cnts[g] - (g > 2 ? cnts[g-2] : 0)
// in 5-bit groups, low first, 0x20 = "more", offset by 48.  So count g needs t_{g-3}..t_g: its own transition and the last three
// before it, which for long runs lie many columns earlier.
//
// Work unit = one column segment (x, s) of one instance: the column is cut into S <= 8 segments of R rows, and units are ordered
// u = x * S + s, which is the column-major order of their pixels.  A unit's transitions are decided by its own pixels and the one
// pixel before it, so every pass reads the masks directly, one thread per unit (the 64 lanes of a wave read 64 consecutive bytes of
// a row).  What a unit needs from the units before it is the carry {transitions so far, positions of the last three}: it is
// associative, so one block per instance scans it.
//   measure: k_rle_units (carry of each unit alone, pixels set) -> k_rle_carry_scan (exclusive carries, num_counts, area)
//            -> k_rle_unit_chars (characters of the counts each unit ends) -> k_rle_char_scan (unit offsets, string_bytes)
//            -> k_rle_instance_offsets (byte_offset of each instance)
//   write:   k_rle_write (each unit writes its characters at its offset)
// Scratch is n * W * S * 28 bytes; nothing is proportional to the number of counts, and no pass uses atomics (deterministic).
#include "csm_common.h"
#include "csm_bits.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxSegs = 8;      // column segments per column (threads in flight for tall masks; bounds the scratch at O(n * W))
constexpr int kSegRows = 128;    // rows per segment below which a column is not cut further

struct Carry {
    int cnt;                 // transitions
    int a0, a1, a2;          // positions of the last three (a2 newest); those beyond cnt are unused
};

__device__ __forceinline__ Carry load_carry(const int4 *p) { const int4 v = *p; return {v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void store_carry(int4 *p, const Carry &c) { *p = make_int4(c.cnt, c.a0, c.a1, c.a2); }

// the carry of the pixels of A followed by those of B
__device__ __forceinline__ Carry combine(const Carry &A, const Carry &B) {
    Carry r;
    r.cnt = A.cnt + B.cnt;
    if (B.cnt >= 3)       { r.a0 = B.a0; r.a1 = B.a1; r.a2 = B.a2; }
    else if (B.cnt == 2)  { r.a0 = A.a2; r.a1 = B.a1; r.a2 = B.a2; }
    else if (B.cnt == 1)  { r.a0 = A.a1; r.a1 = A.a2; r.a2 = B.a2; }
    else                  { r.a0 = A.a0; r.a1 = A.a1; r.a2 = A.a2; }
    return r;
}

__device__ __forceinline__ void push(Carry &c, int p) { c.a0 = c.a1; c.a1 = c.a2; c.a2 = p; ++c.cnt; }

// d_g of the count that ends at position p (a transition, or H * W for the last count), given the carry before it (g = c.cnt)
__device__ __forceinline__ int64_t rle_delta(const Carry &c, int p) {
    int64_t x = (int64_t)p - (c.cnt >= 1 ? c.a2 : 0);
    if (c.cnt > 2) x -= (int64_t)c.a1 - c.a0;
    return x;
}

// rleToString: characters of one value (1..7 for |x| < 2^34)
__device__ __forceinline__ int rle_chars(int64_t x) {
    int n = 0;
    bool more = true;
    while (more) {
        const int64_t c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++n;
    }
    return n;
}

// writes the characters of x at out[pos..], never at or past end; returns the new pos
__device__ __forceinline__ int64_t rle_emit(int64_t x, char *__restrict__ out, int64_t pos, int64_t end) {
    bool more = true;
    while (more) {
        int64_t c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (pos < end) out[pos] = (char)(c + 48);
        ++pos;
    }
    return pos;
}

struct Unit {
    int x, s, inst, y0, y1;
    int64_t idx;             // index into the per-unit scratch arrays
};

// the unit of this thread (grid: (cdiv(W, 256), S, n)); false past the last column
__device__ __forceinline__ bool unit_of_thread(int W, int S, int R, int H, Unit &u) {
    u.x = blockIdx.x * kBlock + threadIdx.x;
    u.s = blockIdx.y;
    u.inst = blockIdx.z;
    if (u.x >= W) return false;
    u.y0 = u.s * R;
    u.y1 = min(H, u.y0 + R);
    u.idx = ((int64_t)u.inst * W + u.x) * S + u.s;
    return true;
}

// value of the pixel before the unit's first one in column-major order
__device__ __forceinline__ int value_before(const uint8_t *__restrict__ M, int H, int W, const Unit &u) {
    if (u.y0 > 0) return M[(int64_t)(u.y0 - 1) * W + u.x] != 0;
    return u.x > 0 ? M[(int64_t)(H - 1) * W + u.x - 1] != 0 : 0;
}

__global__ __launch_bounds__(kBlock) void k_rle_units(const uint8_t *__restrict__ masks, int H, int W, int S, int R,
                                                       int4 *__restrict__ carry, int *__restrict__ area) {
    Unit u;
    if (!unit_of_thread(W, S, R, H, u)) return;
    const uint8_t *M = masks + (int64_t)u.inst * H * W;
    int prev = value_before(M, H, W, u), set = 0;
    Carry c = {0, 0, 0, 0};
    const int base = u.x * H;
    for (int y = u.y0; y < u.y1; ++y) {
        const int v = M[(int64_t)y * W + u.x] != 0;
        set += v;
        if (v != prev) push(c, base + y);
        prev = v;
    }
    store_carry(carry + u.idx, c);
    area[u.idx] = set;
}

// one block per instance: each thread folds a run of consecutive units, the block scans the runs, then each thread rewrites its
// units with the carry of everything before them.  info[inst] = {num_counts, -, area, -}.
__global__ __launch_bounds__(kBlock) void k_rle_carry_scan(int64_t U, int4 *__restrict__ carry, const int *__restrict__ area,
                                                            int64_t *__restrict__ info) {
    const int inst = blockIdx.x, t = threadIdx.x;
    const int64_t per = (U + kBlock - 1) / kBlock, u0 = min(U, t * per), u1 = min(U, u0 + per);
    int4 *C = carry + (int64_t)inst * U;
    const int *A = area + (int64_t)inst * U;
    Carry agg = {0, 0, 0, 0};
    int64_t set = 0;
    for (int64_t u = u0; u < u1; ++u) { agg = combine(agg, load_carry(C + u)); set += A[u]; }
    __shared__ int4 sc[kBlock];
    __shared__ int64_t sa[kBlock];
    store_carry(sc + t, agg);
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {                // inclusive scan (Hillis-Steele keeps the left-to-right order)
        Carry v = load_carry(sc + t);
        if (t >= d) v = combine(load_carry(sc + t - d), v);
        __syncthreads();
        store_carry(sc + t, v);
        __syncthreads();
    }
    Carry ex = t ? load_carry(sc + t - 1) : Carry{0, 0, 0, 0};
    const int total = sc[kBlock - 1].x;
    int64_t set_total;
    csm_bits::block_exclusive<kBlock>(set, sa, set_total);
    for (int64_t u = u0; u < u1; ++u) {
        const Carry c = load_carry(C + u);
        store_carry(C + u, ex);
        ex = combine(ex, c);
    }
    if (t == 0) {
        info[4 * inst + 0] = (int64_t)total + 1;
        info[4 * inst + 2] = set_total;
    }
}

// characters of the counts each unit ends: one per transition in it, plus the last count in the instance's last unit
__global__ __launch_bounds__(kBlock) void k_rle_unit_chars(const uint8_t *__restrict__ masks, int H, int W, int S, int R,
                                                            const int4 *__restrict__ carry, int64_t *__restrict__ chars) {
    Unit u;
    if (!unit_of_thread(W, S, R, H, u)) return;
    const uint8_t *M = masks + (int64_t)u.inst * H * W;
    int prev = value_before(M, H, W, u);
    Carry c = load_carry(carry + u.idx);
    const int base = u.x * H;
    int64_t n = 0;
    for (int y = u.y0; y < u.y1; ++y) {
        const int v = M[(int64_t)y * W + u.x] != 0;
        if (v != prev) { n += rle_chars(rle_delta(c, base + y)); push(c, base + y); }
        prev = v;
    }
    if (u.x == W - 1 && u.s == S - 1) n += rle_chars(rle_delta(c, H * W));
    chars[u.idx] = n;
}

// one block per instance: unit character counts -> offsets inside the instance's string; info[inst][1] = string_bytes
__global__ __launch_bounds__(kBlock) void k_rle_char_scan(int64_t U, int64_t *__restrict__ chars, int64_t *__restrict__ info) {
    const int inst = blockIdx.x, t = threadIdx.x;
    const int64_t per = (U + kBlock - 1) / kBlock, u0 = min(U, t * per), u1 = min(U, u0 + per);
    int64_t *Ch = chars + (int64_t)inst * U;
    int64_t sum = 0;
    for (int64_t u = u0; u < u1; ++u) sum += Ch[u];
    __shared__ int64_t sh[kBlock];
    int64_t total;
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sh, total);
    for (int64_t u = u0; u < u1; ++u) { const int64_t v = Ch[u]; Ch[u] = ex; ex += v; }
    if (t == 0) info[4 * inst + 1] = total;
}

// one block: info[i][3] = sum of info[k][1] over k < i
__global__ __launch_bounds__(kBlock) void k_rle_instance_offsets(int n, int64_t *__restrict__ info) {
    const int t = threadIdx.x;
    const int per = (n + kBlock - 1) / kBlock, i0 = min(n, t * per), i1 = min(n, i0 + per);
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += info[4 * i + 1];
    __shared__ int64_t sh[kBlock];
    int64_t total;
    int64_t ex = csm_bits::block_exclusive<kBlock>(sum, sh, total);
    for (int i = i0; i < i1; ++i) { info[4 * i + 3] = ex; ex += info[4 * i + 1]; }
}

// each unit writes its characters in [its offset, the next unit's offset): the bound holds even for masks that changed since
// the measure call (the strings are then wrong, but nothing is written outside the instance's own bytes)
__global__ __launch_bounds__(kBlock) void k_rle_write(const uint8_t *__restrict__ masks, int H, int W, int S, int R,
                                                       const int4 *__restrict__ carry, const int64_t *__restrict__ chars,
                                                       const int64_t *__restrict__ info, char *__restrict__ out) {
    Unit u;
    if (!unit_of_thread(W, S, R, H, u)) return;
    const int64_t U = (int64_t)W * S, last = (int64_t)u.inst * U + U - 1;
    char *O = out + info[4 * u.inst + 3];
    int64_t pos = chars[u.idx];
    const int64_t end = u.idx < last ? chars[u.idx + 1] : info[4 * u.inst + 1];
    const uint8_t *M = masks + (int64_t)u.inst * H * W;
    int prev = value_before(M, H, W, u);
    Carry c = load_carry(carry + u.idx);
    const int base = u.x * H;
    for (int y = u.y0; y < u.y1; ++y) {
        const int v = M[(int64_t)y * W + u.x] != 0;
        if (v != prev) { pos = rle_emit(rle_delta(c, base + y), O, pos, end); push(c, base + y); }
        prev = v;
    }
    if (u.idx == last) rle_emit(rle_delta(c, H * W), O, pos, end);
}

// segments per column and rows per segment; every segment is non-empty
void rle_split(int H, int &S, int &R) {
    S = (int)std::min<int64_t>(kMaxSegs, csm::cdiv(H, kSegRows));
    R = (int)csm::cdiv(H, S);
    S = (int)csm::cdiv(H, R);
}

struct RleScratch {
    int64_t *chars;
    int4 *carry;
    int *area;
};

RleScratch rle_scratch(void *scratch, int n, int W, int S) {
    const int64_t units = (int64_t)n * W * S;
    char *p = (char *)scratch;
    RleScratch r;
    r.chars = (int64_t *)p;
    r.carry = (int4 *)(p + units * 8);
    r.area = (int *)(p + units * 24);
    return r;
}

bool rle_shape_ok(int n, int H, int W) { return n >= 0 && H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX; }

}  // namespace

extern "C" size_t csm_mask_rle_scratch_bytes(int n, int H, int W) {
    if (!rle_shape_ok(n, H, W)) return 0;
    int S, R;
    rle_split(H, S, R);
    return (size_t)n * W * S * 28;
}

extern "C" int csm_mask_rle_measure(const uint8_t *masks, int n, int H, int W, int64_t *info, void *scratch, void *stream) {
    CSM_REQUIRE(rle_shape_ok(n, H, W));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(masks && info && scratch && n <= 65535);
    int S, R;
    rle_split(H, S, R);
    const RleScratch sc = rle_scratch(scratch, n, W, S);
    const int64_t U = (int64_t)W * S;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(csm::cdiv(W, kBlock), S, n);
    k_rle_units<<<grid, kBlock, 0, st>>>(masks, H, W, S, R, sc.carry, sc.area);
    int rc = csm::check_launch("k_rle_units"); if (rc) return rc;
    k_rle_carry_scan<<<n, kBlock, 0, st>>>(U, sc.carry, sc.area, info);
    rc = csm::check_launch("k_rle_carry_scan"); if (rc) return rc;
    k_rle_unit_chars<<<grid, kBlock, 0, st>>>(masks, H, W, S, R, sc.carry, sc.chars);
    rc = csm::check_launch("k_rle_unit_chars"); if (rc) return rc;
    k_rle_char_scan<<<n, kBlock, 0, st>>>(U, sc.chars, info);
    rc = csm::check_launch("k_rle_char_scan"); if (rc) return rc;
    k_rle_instance_offsets<<<1, kBlock, 0, st>>>(n, info);
    return csm::check_launch("k_rle_instance_offsets");
}

extern "C" int csm_mask_rle_write(const uint8_t *masks, int n, int H, int W, const int64_t *info, char *out, void *scratch,
                                  void *stream) {
    CSM_REQUIRE(rle_shape_ok(n, H, W));
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(masks && info && out && scratch && n <= 65535);
    int S, R;
    rle_split(H, S, R);
    const RleScratch sc = rle_scratch(scratch, n, W, S);
    k_rle_write<<<dim3(csm::cdiv(W, kBlock), S, n), kBlock, 0, (hipStream_t)stream>>>(masks, H, W, S, R, sc.carry, sc.chars, info, out);
    return csm::check_launch("k_rle_write");
}
