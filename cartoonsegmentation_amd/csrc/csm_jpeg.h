// csm_jpeg.h -- what the JPEG decoders of jpegdec.hip (baseline) and jpegprog.hip (progressive, §4.11) share: the
// file descriptor and the scratch plan, the bit reader, the Huffman tables in LDS, the subsequence machine of the entropy decode
// (k_js_sync_local, k_js_sync_global, k_js_scan, k_js_write and the host loop that runs them, templates over a codec policy that
// each file instantiates with its own), the segmented scan of the DC prediction, and the kernels from the coefficient store to the
// pixels (k_jd_idct, k_jd_colour).  Included by those two files only; everything is local to the including file.
#pragma once
#include "csm_common.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int kSubseq = 32;                  // bytes of entropy data per lane
constexpr int kLanes = 256;                  // lanes (subsequences) per workgroup
constexpr int kHuffSlots = 6;
constexpr int kTableBytes = 2 * 256 + 4 * 18 + 4 * 18 + 256;       // jpegcode.TABLE_BYTES
constexpr int kQuantBytes = 3 * 64 * 2;
constexpr int kFileTableBytes = kHuffSlots * kTableBytes + kQuantBytes;
constexpr int kDescWords = 20;
constexpr int kMaxEntropy = 1 << 28;
constexpr uint64_t kDead = ~0ull;            // state of a lane that met an invalid code

__device__ const uint8_t kNatural[64] = {    // natural (row-major) index of the i-th coefficient of the scan
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JFile {
    // from the caller's descriptor
    int H, W, nc, hs, vs, ri;
    int ent_off, ent_len, tab_off;
    int dcs[3], acs[3];
    int64_t out_off;
    // derived
    int mx, my, bpm, nblk;       // MCUs per row, MCU rows, blocks per MCU, blocks
    int sub0, nsub, nwg;         // first subsequence (of the call), subsequences, workgroups
    uint32_t tabsel;             // per component c: slot of its DC table in bits 8c..8c+3, of its AC table in bits 8c+4..8c+7
    int cw, ch;                  // true size of a chroma plane
    int pw[3], ph[3];            // padded size of each component's plane
    int64_t blk0;                // first block (of the call)
    int64_t plane_off[3];        // byte offset of each plane in the plane region
};

struct Plan {
    std::vector<JFile> files;
    int64_t nsub = 0, blocks = 0, plane_bytes = 0;
    int max_wg = 0, max_blocks = 0;
    int64_t max_pixels = 0;
    // byte offsets of the scratch regions
    int64_t o_files, o_state, o_cnt_n, o_cnt_r, o_off_n, o_off_r, o_flag, o_err, o_coef, o_planes, total;
};

// false: the descriptors are invalid (the error is set)
bool make_plan(const int32_t *desc, int n, int64_t blob_bytes, int64_t out_bytes, bool check_ranges, Plan &p) {
    if (!desc || n < 1 || n > 65535) { csm::set_error("invalid argument: 1 <= n <= 65535 descriptors"); return false; }
    p.files.resize(n);
    for (int i = 0; i < n; ++i) {
        const int32_t *d = desc + (int64_t)i * kDescWords;
        JFile &f = p.files[i];
        f.H = d[0]; f.W = d[1]; f.nc = d[2]; f.hs = d[3]; f.vs = d[4]; f.ri = d[5];
        f.ent_off = d[6]; f.ent_len = d[7]; f.tab_off = d[8];
        for (int c = 0; c < 3; ++c) { f.dcs[c] = d[9 + c]; f.acs[c] = d[12 + c]; }
        f.out_off = (int64_t)d[15] | ((int64_t)d[16] << 31);
        bool ok = f.H >= 1 && f.H <= 65535 && f.W >= 1 && f.W <= 65535 && (f.nc == 1 || f.nc == 3) && f.ri >= 0 && f.ri <= 65535;
        ok = ok && ((f.hs == 1 && f.vs == 1) || (f.nc == 3 && f.hs == 2 && (f.vs == 1 || f.vs == 2)));
        ok = ok && f.ent_off >= 0 && f.ent_len >= 0 && f.ent_len <= kMaxEntropy && f.tab_off >= 0 && (f.tab_off & 3) == 0;
        ok = ok && d[15] >= 0 && d[16] >= 0 && (f.out_off & 3) == 0;
        for (int c = 0; c < 3; ++c) ok = ok && f.dcs[c] >= 0 && f.dcs[c] < kHuffSlots && f.acs[c] >= 0 && f.acs[c] < kHuffSlots;
        if (ok && check_ranges) {
            ok = (int64_t)f.ent_off + f.ent_len <= blob_bytes && (int64_t)f.tab_off + kFileTableBytes <= blob_bytes &&
                 f.out_off + (int64_t)f.H * f.W * 3 <= out_bytes;
        }
        if (!ok) { csm::set_error("invalid argument: descriptor %d of the JPEG decode", i); return false; }
        f.mx = (f.W + 8 * f.hs - 1) / (8 * f.hs);
        f.my = (f.H + 8 * f.vs - 1) / (8 * f.vs);
        f.bpm = f.nc == 1 ? 1 : f.hs * f.vs + 2;
        const int64_t nblk = (int64_t)f.mx * f.my * f.bpm;
        if (nblk * 64 >= INT32_MAX) { csm::set_error("invalid argument: file %d has too many blocks", i); return false; }
        f.nblk = (int)nblk;
        f.nsub = std::max(1, (f.ent_len + kSubseq - 1) / kSubseq);
        f.nwg = (f.nsub + kLanes - 1) / kLanes;
        if (p.nsub + f.nsub >= INT32_MAX) { csm::set_error("invalid argument: too much entropy data in one call"); return false; }
        f.sub0 = (int)p.nsub;
        f.blk0 = p.blocks;
        f.tabsel = 0;
        for (int c = 0; c < 3; ++c) f.tabsel |= (uint32_t)(f.dcs[c] | f.acs[c] << 4) << (8 * c);
        f.cw = (f.W + f.hs - 1) / f.hs;
        f.ch = (f.H + f.vs - 1) / f.vs;
        for (int c = 0; c < 3; ++c) {
            const int h = c == 0 ? f.hs : 1, v = c == 0 ? f.vs : 1;
            f.pw[c] = f.mx * h * 8; f.ph[c] = f.my * v * 8;
            f.plane_off[c] = p.plane_bytes;
            if (c < f.nc) p.plane_bytes += csm::align16((int64_t)f.pw[c] * f.ph[c]);
        }
        p.nsub += f.nsub;
        p.blocks += nblk;
        p.max_wg = std::max(p.max_wg, f.nwg);
        p.max_blocks = std::max(p.max_blocks, f.nblk);
        p.max_pixels = std::max(p.max_pixels, (int64_t)f.H * f.W);
    }
    int64_t o = 0;
    p.o_files = o;   o += csm::align16((int64_t)n * sizeof(JFile));
    p.o_state = o;   o += csm::align16(p.nsub * 8);
    p.o_cnt_n = o;   o += csm::align16(p.nsub * 4);
    p.o_cnt_r = o;   o += csm::align16(p.nsub * 4);
    p.o_off_n = o;   o += csm::align16(p.nsub * 8);
    p.o_off_r = o;   o += csm::align16(p.nsub * 4);
    p.o_flag = o;    o += 16;
    p.o_err = o;     o += csm::align16((int64_t)n * 4);
    p.o_coef = o;    o += csm::align16(p.blocks * 128);
    p.o_planes = o;  o += p.plane_bytes;
    p.total = o;
    return true;
}

// ---- the bit reader ---------------------------------------------------------------------------------------------------------
// MSB-first window of up to 64 bits over the entropy bytes e[0, len) of one file, fed by aligned 32-bit loads where a word holds no
// FF byte and byte by byte elsewhere.  A stuffed FF 00 feeds FF; a marker stops the feed (the bits behind the real ones read as 0).
// hist keeps one bit per fed byte (newest lowest): set where the byte stands for two bytes of the file, so that the file position of
// the next unread bit follows from pos, nb and hist.
struct Reader {
    const uint8_t *e;
    int len;
    uint64_t win;
    int nb;            // real bits in win
    int pos;           // next byte of the file to feed
    uint32_t hist;
    int stop;          // 0, 1: a restart marker (its code at mpos + 1) is next, 2: the data end here
    int mpos;

    __device__ __forceinline__ void open(const uint8_t *data, int n, int byte) {
        e = data; len = n; win = 0; nb = 0; pos = min(byte, n); hist = 0; stop = 0; mpos = 0;
    }
    __device__ __forceinline__ void refill() {
        while (nb <= 32 && !stop) {
            if (pos >= len) { stop = 2; break; }
            if ((((uintptr_t)(e + pos)) & 3) == 0 && pos + 4 <= len) {
                const uint32_t w = *(const uint32_t *)(e + pos);
                const uint32_t x = ~w;
                if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {                 // no FF byte in the word
                    win |= (uint64_t)__builtin_bswap32(w) << (32 - nb);
                    nb += 32; pos += 4; hist <<= 4;
                    continue;
                }
            }
            const uint32_t v = e[pos];
            if (v != 0xFFu) { win |= (uint64_t)v << (56 - nb); nb += 8; pos += 1; hist <<= 1; continue; }
            int j = pos + 1;
            while (j < len && e[j] == 0xFFu) ++j;                                   // fill bytes
            const uint32_t v2 = j < len ? e[j] : 0xD9u;
            if (v2 == 0 && j == pos + 1) { win |= (uint64_t)0xFFu << (56 - nb); nb += 8; pos += 2; hist = (hist << 1) | 1u; }
            else { stop = (v2 >= 0xD0u && v2 <= 0xD7u) ? 1 : 2; mpos = j - 1; }
        }
    }
    __device__ __forceinline__ void skip(int n) { win <<= n; nb -= n; }
    // the marker is taken: the feed goes on behind it
    __device__ __forceinline__ void cross() { pos = min(mpos + 2, len); win = 0; nb = 0; hist = 0; stop = 0; }
    // bit position (in the file's entropy bytes) of the next unread bit
    __device__ __forceinline__ uint32_t bitpos() const {
        const int k = (nb + 7) >> 3;
        const int first = pos - k - __popc(hist & ((1u << k) - 1u));
        return (uint32_t)first * 8u + (uint32_t)(8 * k - nb);
    }
    // only 1-bits (or nothing) are left in front of a marker or the end
    __device__ __forceinline__ bool at_marker() const {
        return stop && nb < 8 && (nb == 0 || (win >> (64 - nb)) == ((1ull << nb) - 1ull));
    }
};

template <int N> struct HuffTables {            // N decode tables (jpegcode.TABLE_BYTES each) in LDS
    uint32_t w[N * kTableBytes / 4];
    __device__ __forceinline__ const uint16_t *lut(int s) const { return (const uint16_t *)((const uint8_t *)w + s * kTableBytes); }
    __device__ __forceinline__ const int *maxcode(int s) const { return (const int *)((const uint8_t *)w + s * kTableBytes + 512); }
    __device__ __forceinline__ const int *valoff(int s) const { return (const int *)((const uint8_t *)w + s * kTableBytes + 584); }
    __device__ __forceinline__ const uint8_t *vals(int s) const { return (const uint8_t *)w + s * kTableBytes + 656; }
};

// the first n (<= N) tables from src (4-byte aligned), by the whole workgroup
template <int N> __device__ __forceinline__ void load_tables(HuffTables<N> &T, const uint8_t *src, int n) {
    for (int i = threadIdx.x; i < n * (kTableBytes / 4); i += blockDim.x) T.w[i] = ((const uint32_t *)src)[i];
}

// the code at the top of v (the next 32 bits) in table `slot`: false for an invalid code
template <int N> __device__ __forceinline__ bool huff_decode(const HuffTables<N> &T, int slot, uint32_t v, int &ln, int &sym) {
    const uint32_t e = T.lut(slot)[v >> 24];
    if (e) { ln = (int)(e >> 8); sym = (int)(e & 255u); return true; }
    const int *mc = T.maxcode(slot);
    const int code16 = (int)(v >> 16);
    int c = 0;
    for (ln = 9; ln <= 16; ++ln) { c = code16 >> (16 - ln); if (c <= mc[ln]) break; }
    if (ln > 16) return false;
    sym = T.vals(slot)[(T.valoff(slot)[ln] + c) & 255];
    return true;
}

// ---- the subsequence machine --------------------------------------------------------------------------------------------------
// The self-synchronising decode of Weissenberger and Schmidt (ICPP 2018) over work items (a baseline file, a progressive first scan)
// whose entropy bytes are cut into subsequences of kSubseq bytes, a lane to each, kLanes of them to a workgroup.  A lane's state is
// (bit position, b, z); it counts the coefficient slots and the restart markers it passes.  What a codec adds is a policy P:
//
//   using Tables = HuffTables<n>;  struct Args { ... };             what the kernels are handed to find the work items
//   P(const Args &, int item)                                       work item `item` of the launch
//   seq()                                                           the descriptor that holds ent_off, ent_len, sub0, nsub, nwg
//   load(T, blob)                                                   the item's tables, by the whole workgroup
//   table(b, z)                                                     table slot of the next symbol
//   symbol(sym, z, y)                                               fills y for Huffman symbol `sym`; false: invalid in this state
//   advance(y, bits, b, z)                                          the slots the symbol takes (bits: its y.extra bits); moves (b, z) on
//   clamp(b, z)                                                     brings a state read from memory into range
//   store(coef, at, val)                                            coefficient `val` at slot `at` of the item (bounds checked)
//   interval_slots(), total_slots(), err_index(item)                slots of a restart interval, of the item; its word of err
struct Symbol {
    int adv;             // slots it takes where that is known before its extra bits are read
    int size;            // bits of its coefficient's value; 0: no coefficient
    int extra;           // raw bits behind the code
};

struct Sink {            // what the coefficient stores of the write pass need
    int16_t *coef;
    int64_t slot;        // slot of the current state
    int64_t per_marker;  // slots of a restart interval
    int marks_before;
};

__device__ __forceinline__ uint64_t pack_state(uint32_t p, int b, int z) { return ((uint64_t)p << 16) | ((uint64_t)b << 8) | (uint64_t)z; }

// Decodes symbols from (rd, b, z) while the next symbol begins before bit `limit` of the item's entropy bytes.  Returns the packed
// end state, kDead after an invalid code.  n_slots / n_mark count the coefficient slots and the restart markers passed.
template <bool EMIT, class P>
__device__ uint64_t subseq_run(const P &w, const typename P::Tables &T, Reader &rd, int &b, int &z, uint32_t limit, int &n_slots,
                               int &n_mark, Sink &sink) {
    for (;;) {
        rd.refill();
        bool marker = rd.at_marker();
        Symbol y{};
        int total = 0;
        uint32_t v = 0;
        if (!marker) {
            if (rd.bitpos() >= limit) return pack_state(rd.bitpos(), b, z);
            v = (uint32_t)(rd.win >> 32);
            int ln, sym;
            if (!huff_decode(T, w.table(b, z), v, ln, sym) || !w.symbol(sym, z, y)) return kDead;
            total = ln + y.extra;                // at most 16 + 15 bits
            marker = total > rd.nb;              // the symbol runs into a marker or the end: not a symbol
        }
        if (marker) {
            if (rd.stop != 1) { b = 0; z = 0; return pack_state((uint32_t)w.seq().ent_len * 8u, 0, 0); }
            rd.cross();
            b = 0; z = 0;
            ++n_mark;
            if constexpr (EMIT) sink.slot = (int64_t)(sink.marks_before + n_mark) * sink.per_marker;
            continue;
        }
        const int bits = y.extra ? (int)((v >> (32 - total)) & ((1u << y.extra) - 1u)) : 0;
        const int adv = w.advance(y, bits, b, z);
        if constexpr (EMIT) {
            if (y.size) {
                int val = bits;
                if (val < (1 << (y.size - 1))) val -= (1 << y.size) - 1;
                w.store(sink.coef, sink.slot + adv - 1, val);
            }
            sink.slot += adv;
        }
        rd.skip(total);
        n_slots += adv;
    }
}

// a reader at the packed state st (not kDead) of the item
template <class P> __device__ __forceinline__ void open_at(const P &w, Reader &rd, const uint8_t *ent, uint64_t st, int &b, int &z) {
    const uint32_t p = (uint32_t)(st >> 16);
    b = (int)((st >> 8) & 255u); z = (int)(st & 255u);
    w.clamp(b, z);
    rd.open(ent, w.seq().ent_len, (int)min(p >> 3, (uint32_t)w.seq().ent_len));
    rd.refill();
    const int off = (int)(p & 7u);
    if (off < rd.nb) rd.skip(off);
}

// grid (workgroups of the largest item, items); lane = one subsequence.  Every lane decodes its own subsequence from a cold state,
// then goes on into its successors from its own end state, through LDS, until its end state equals the one recorded there or the
// workgroup ends.
template <class P>
__global__ __launch_bounds__(kLanes) void k_js_sync_local(const uint8_t *__restrict__ blob, const typename P::Args a,
                                                           uint64_t *__restrict__ state, int *__restrict__ cnt_n, int *__restrict__ cnt_r) {
    __shared__ typename P::Tables T;
    __shared__ uint64_t sState[kLanes];
    __shared__ int sN[kLanes], sR[kLanes];
    const P w(a, blockIdx.y);
    const auto &q = w.seq();
    if ((int)blockIdx.x >= q.nwg) return;
    const int t = threadIdx.x, j = blockIdx.x * kLanes + t;
    const bool valid = j < q.nsub;
    const uint8_t *ent = blob + q.ent_off;
    w.load(T, blob);
    __syncthreads();
    Reader rd;
    Sink none{};
    int b = 0, z = 0;
    uint64_t cur = kDead;
    if (valid) {
        // cold: b = z = 0 (the first block of a restart unit, its first coefficient).  On the 00 of a stuffed pair or on the code of
        // a marker, start behind it.
        int start = j * kSubseq;
        if (start > 0 && start < q.ent_len && ent[start - 1] == 0xFFu && (ent[start] == 0 || (ent[start] >= 0xD0u && ent[start] <= 0xD7u))) ++start;
        rd.open(ent, q.ent_len, start);
        int n = 0, r = 0;
        cur = subseq_run<false>(w, T, rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), n, r, none);
        sN[t] = n; sR[t] = r;
    }
    sState[t] = cur;
    bool active = valid && cur != kDead;
    for (int step = 1; step < kLanes; ++step) {
        __syncthreads();
        const int tj = t + step;
        const bool go = active && tj < kLanes && j + step < q.nsub;
        if (!go) active = false;
        if (go) {
            int n = 0, r = 0;
            const uint64_t ns = subseq_run<false>(w, T, rd, b, z, (uint32_t)(j + step + 1) * (kSubseq * 8u), n, r, none);
            const uint64_t old = sState[tj];
            sState[tj] = ns; sN[tj] = n; sR[tj] = r;
            if (ns == kDead || ns == old) active = false;
        }
        if (!__syncthreads_or(active)) break;
    }
    __syncthreads();
    if (valid) {
        state[q.sub0 + j] = sState[t];
        cnt_n[q.sub0 + j] = sN[t];
        cnt_r[q.sub0 + j] = sR[t];
    }
}

// grid (workgroups of the largest item, items), one wave; lane 0 carries the end state of the workgroup before this one into its own
// subsequences until it meets the recorded state
template <class P>
__global__ __launch_bounds__(64) void k_js_sync_global(const uint8_t *__restrict__ blob, const typename P::Args a, uint64_t *state,
                                                        int *__restrict__ cnt_n, int *__restrict__ cnt_r, int *__restrict__ flag) {
    __shared__ typename P::Tables T;
    const P w(a, blockIdx.y);
    const auto &q = w.seq();
    if (blockIdx.x == 0 || (int)blockIdx.x >= q.nwg) return;
    w.load(T, blob);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int j0 = blockIdx.x * kLanes, j1 = min(j0 + kLanes, q.nsub);
    // the state of the workgroup before this one may be rewritten while it is read here: either value is a state, and a rewrite
    // raises the flag, so that this workgroup reads it again in the next launch
    uint64_t st = __hip_atomic_load(state + q.sub0 + j0 - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st == kDead) return;
    Reader rd;
    Sink none{};
    int b, z;
    open_at(w, rd, blob + q.ent_off, st, b, z);
    for (int j = j0; j < j1; ++j) {
        int n = 0, r = 0;
        const uint64_t ns = subseq_run<false>(w, T, rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), n, r, none);
        const uint64_t old = state[q.sub0 + j];
        cnt_n[q.sub0 + j] = n;
        cnt_r[q.sub0 + j] = r;
        if (ns == old) break;
        __hip_atomic_store(state + q.sub0 + j, ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = 1;
        if (ns == kDead) break;
    }
}

template <typename T> __device__ T block_exclusive(T v, T *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {
        const T w = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += w;
        __syncthreads();
    }
    const T ex = t ? sh[t - 1] : 0;
    __syncthreads();
    return ex;
}

// one workgroup per item: off_n / off_r = exclusive sums of cnt_n / cnt_r over the item's subsequences, the output position of each
template <class P>
__global__ __launch_bounds__(kLanes) void k_js_scan(const typename P::Args a, const int *__restrict__ cnt_n, const int *__restrict__ cnt_r,
                                                     int64_t *__restrict__ off_n, int *__restrict__ off_r) {
    __shared__ int64_t sh[kLanes];
    const P w(a, blockIdx.x);
    const auto &q = w.seq();
    const int t = threadIdx.x;
    const int per = (q.nsub + kLanes - 1) / kLanes, j0 = min(q.nsub, t * per), j1 = min(q.nsub, j0 + per);
    int64_t sn = 0, sr = 0;
    for (int j = j0; j < j1; ++j) { sn += cnt_n[q.sub0 + j]; sr += cnt_r[q.sub0 + j]; }
    int64_t en = block_exclusive(sn, sh);
    int64_t er = block_exclusive(sr, sh);
    for (int j = j0; j < j1; ++j) {
        off_n[q.sub0 + j] = en; off_r[q.sub0 + j] = (int)min(er, (int64_t)INT32_MAX);
        en += cnt_n[q.sub0 + j]; er += cnt_r[q.sub0 + j];
    }
}

// grid as k_js_sync_local.  Every lane decodes its subsequence once more from its entry state and stores the coefficients (the
// buffer is zeroed before).  err bits: 1 an invalid code or a subsequence without a state, 2 the data do not hold the item's blocks
// exactly
template <class P>
__global__ __launch_bounds__(kLanes) void k_js_write(const uint8_t *__restrict__ blob, const typename P::Args a,
                                                      const uint64_t *__restrict__ state, const int *__restrict__ cnt_n,
                                                      const int64_t *__restrict__ off_n, const int *__restrict__ off_r,
                                                      int16_t *__restrict__ coef, int *__restrict__ err) {
    __shared__ typename P::Tables T;
    const P w(a, blockIdx.y);
    const auto &q = w.seq();
    if ((int)blockIdx.x >= q.nwg) return;
    w.load(T, blob);
    __syncthreads();
    const int j = blockIdx.x * kLanes + threadIdx.x;
    if (j >= q.nsub) return;
    int *e = err + w.err_index(blockIdx.y);
    const uint64_t st = j == 0 ? pack_state(0, 0, 0) : state[q.sub0 + j - 1];
    if (st == kDead) { atomicOr(e, 1); return; }
    Reader rd;
    int b, z;
    open_at(w, rd, blob + q.ent_off, st, b, z);
    Sink sink{coef, off_n[q.sub0 + j], w.interval_slots(), off_r[q.sub0 + j]};
    int n = 0, r = 0;
    const uint64_t ns = subseq_run<true>(w, T, rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), n, r, sink);
    if (ns == kDead) atomicOr(e, 1);
    if (j == q.nsub - 1 && off_n[q.sub0 + j] + cnt_n[q.sub0 + j] != w.total_slots()) atomicOr(e, 2);
}

// the scratch regions of the machine: Plan and PPlan lay them out under the same names
struct Subseq {
    uint64_t *state;
    int *cnt_n, *cnt_r;
    int64_t *off_n;
    int *off_r, *flag;
};

template <class L> Subseq subseq_regions(char *S, const L &p) {
    return {(uint64_t *)(S + p.o_state), (int *)(S + p.o_cnt_n), (int *)(S + p.o_cnt_r), (int64_t *)(S + p.o_off_n),
            (int *)(S + p.o_off_r), (int *)(S + p.o_flag)};
}

// The machine over `items` work items that hold nsub subsequences together, the largest max_wg workgroups: k_js_sync_local,
// k_js_sync_global relaunched until the flag stays clear (the host reads the 4-byte flag: one stream synchronise per pass; after more
// passes than there are subsequences it gives up), k_js_scan, k_js_write.  `passes` counts the passes of the whole call: the caller
// has cleared the flag before the first of them.
template <class P>
int subseq_decode(const uint8_t *blob, const typename P::Args &a, int items, int max_wg, int64_t nsub, const Subseq &q, int16_t *coef,
                  int *err, int &passes, hipStream_t st) {
    const dim3 grid((unsigned)max_wg, (unsigned)items);
    k_js_sync_local<P><<<grid, kLanes, 0, st>>>(blob, a, q.state, q.cnt_n, q.cnt_r);
    int rc = csm::check_launch("k_js_sync_local"); if (rc) return rc;
    if (max_wg > 1) {
        for (int own = 0;; ++own) {
            if (own > nsub) {
                (void)hipStreamSynchronize(st);
                csm::set_error("jpeg decode: the subsequence states did not settle in %d passes", own);
                return CSM_ERR_DATA;
            }
            int changed = 0;
            if (passes) CSM_HIP(hipMemsetAsync(q.flag, 0, 4, st));
            k_js_sync_global<P><<<grid, 64, 0, st>>>(blob, a, q.state, q.cnt_n, q.cnt_r, q.flag);
            rc = csm::check_launch("k_js_sync_global"); if (rc) return rc;
            CSM_HIP(hipMemcpyAsync(&changed, q.flag, 4, hipMemcpyDeviceToHost, st));
            CSM_HIP(hipStreamSynchronize(st));
            ++passes;
            if (!changed) break;
        }
    }
    k_js_scan<P><<<items, kLanes, 0, st>>>(a, q.cnt_n, q.cnt_r, q.off_n, q.off_r);
    rc = csm::check_launch("k_js_scan"); if (rc) return rc;
    k_js_write<P><<<grid, kLanes, 0, st>>>(blob, a, q.state, q.cnt_n, q.off_n, q.off_r, coef, err);
    return csm::check_launch("k_js_write");
}

// ---- DC prediction ------------------------------------------------------------------------------------------------------------
// By a whole workgroup of kLanes: the DC differences at C[addr(k)], k in [0, total) in the scan order of one component, become
// values << al; the sum restarts where resets(k).  A thread sums a run of consecutive blocks; the runs are joined by a segmented scan.
template <class Addr, class Resets> __device__ __forceinline__ void dc_predict(int16_t *C, int total, int al, Addr addr, Resets resets) {
    __shared__ int sSum[kLanes];
    __shared__ int sFlag[kLanes];
    const int t = threadIdx.x;
    const int per = (total + kLanes - 1) / kLanes, k0 = min(total, t * per), k1 = min(total, k0 + per);
    int sum = 0, flag = 0;
    for (int k = k0; k < k1; ++k) {
        if (resets(k)) { sum = 0; flag = 1; }
        sum += C[addr(k)];
    }
    sSum[t] = sum; sFlag[t] = flag;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {           // inclusive segmented scan: (a, fa) . (b, fb) = (fb ? b : a + b, fa | fb)
        int s = sSum[t], fl = sFlag[t];
        if (t >= d) { if (!fl) s += sSum[t - d]; fl |= sFlag[t - d]; }
        __syncthreads();
        sSum[t] = s; sFlag[t] = fl;
        __syncthreads();
    }
    int run = t ? sSum[t - 1] : 0;
    for (int k = k0; k < k1; ++k) {
        if (resets(k)) run = 0;
        const int64_t at = addr(k);
        run += C[at];
        C[at] = (int16_t)(run * (1 << al));
    }
}

// ---- inverse DCT ------------------------------------------------------------------------------------------------------------
// one pass of the Loeffler-Ligtenberg-Moschytz inverse DCT with 13-bit constants on i[0..7] -> o[0..7], descaled by `shift` bits
__device__ __forceinline__ void idct_pass(const int *i, int *o, int shift) {
    int z1 = (i[2] + i[6]) * 4433;
    const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const int t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o0 = i[7], o1 = i[5], o2 = i[3], o3 = i[1];
    z1 = o0 + o3;
    int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    const int r = 1 << (shift - 1);
    o[0] = (t10 + o3 + r) >> shift; o[7] = (t10 - o3 + r) >> shift;
    o[1] = (t11 + o2 + r) >> shift; o[6] = (t11 - o2 + r) >> shift;
    o[2] = (t12 + o1 + r) >> shift; o[5] = (t12 - o1 + r) >> shift;
    o[3] = (t13 + o0 + r) >> shift; o[4] = (t13 - o0 + r) >> shift;
}

constexpr int kIdctBlocks = 32;              // 8x8 blocks per workgroup: eight lanes each
constexpr int kIdctStride = 72;              // words per block in LDS

// grid (groups of 32 blocks of the largest file, files).  Lane c of a block dequantises and transforms column c, the block goes
// through LDS, lane r transforms row r and stores its eight samples.
__global__ __launch_bounds__(kLanes) void k_jd_idct(const uint8_t *__restrict__ blob, const JFile *__restrict__ files,
                                                     const int16_t *__restrict__ coef, uint8_t *__restrict__ planes) {
    __shared__ int sW[kIdctBlocks * kIdctStride];
    const JFile f = files[blockIdx.y];
    if ((int64_t)blockIdx.x * kIdctBlocks >= f.nblk) return;
    const int t = threadIdx.x, lb = t >> 3, l = t & 7;
    const int bi = blockIdx.x * kIdctBlocks + lb;
    const bool live = bi < f.nblk;
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs;
    const int m = bi / f.bpm, sb = bi - m * f.bpm;
    const int comp = sb < ysub ? 0 : sb - ysub + 1;
    if (live) {
        const uint16_t *Q = (const uint16_t *)(blob + f.tab_off + kHuffSlots * kTableBytes) + comp * 64;
        const int16_t *C = coef + (f.blk0 + bi) * 64;
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int)C[r * 8 + l] * (int)Q[r * 8 + l];
        idct_pass(in, out, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) sW[lb * kIdctStride + r * 8 + l] = out[r];
    }
    __syncthreads();
    if (live) {
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = sW[lb * kIdctStride + l * 8 + k];
        idct_pass(in, out, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(255, max(0, out[k] + 128)) << (8 * k);
            hi |= (uint32_t)min(255, max(0, out[k + 4] + 128)) << (8 * k);
        }
        const int h = comp == 0 ? f.hs : 1, v = comp == 0 ? f.vs : 1;
        const int sv = comp == 0 ? sb / f.hs : 0, sh = comp == 0 ? sb - sv * f.hs : 0;
        const int by = (m / f.mx) * v + sv, bx = (m % f.mx) * h + sh;
        const int64_t poff = comp == 0 ? f.plane_off[0] : comp == 1 ? f.plane_off[1] : f.plane_off[2];
        const int pw = comp == 0 ? f.pw[0] : f.pw[1];
        uint8_t *P = planes + poff + ((int64_t)by * 8 + l) * pw + bx * 8;      // 8-byte aligned
        *(uint2 *)P = make_uint2(lo, hi);
    }
}

// ---- upsampling and colour ----------------------------------------------------------------------------------------------------
// the chroma sample of plane P at pixel (y, x): the triangle filter over the plane's true size cw x ch, edges replicated
__device__ __forceinline__ int chroma_at(const uint8_t *__restrict__ P, const JFile &f, int y, int x) {
    const int pw = f.pw[1];
    if (f.hs == 1) return P[(int64_t)y * pw + x];
    const int i = x >> 1, odd = x & 1;
    const int in = odd ? min(i + 1, f.cw - 1) : max(i - 1, 0);
    if (f.vs == 1) {
        const uint8_t *R = P + (int64_t)y * pw;
        return (3 * R[i] + R[in] + 1 + odd) >> 2;
    }
    const int j = y >> 1, jf = (y & 1) ? min(j + 1, f.ch - 1) : max(j - 1, 0);
    const uint8_t *N = P + (int64_t)j * pw, *F = P + (int64_t)jf * pw;
    const int t = 3 * N[i] + F[i], tn = 3 * N[in] + F[in];
    return (3 * t + tn + 8 - odd) >> 4;
}

__device__ __forceinline__ uint32_t bgr_at(const uint8_t *__restrict__ planes, const JFile &f, int64_t pix) {
    const int y = (int)(pix / f.W), x = (int)(pix - (int64_t)y * f.W);
    const int Y = planes[f.plane_off[0] + (int64_t)y * f.pw[0] + x];
    if (f.nc == 1) return (uint32_t)Y * 0x010101u;
    const int cb = chroma_at(planes + f.plane_off[1], f, y, x) - 128, cr = chroma_at(planes + f.plane_off[2], f, y, x) - 128;
    const int R = min(255, max(0, Y + ((91881 * cr + 32768) >> 16)));
    const int B = min(255, max(0, Y + ((116130 * cb + 32768) >> 16)));
    const int G = min(255, max(0, Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)));
    return (uint32_t)B | (uint32_t)G << 8 | (uint32_t)R << 16;
}

// grid (groups of 4 * kLanes pixels of the largest file, files); a thread converts four consecutive pixels of the flat image and
// stores their 12 bytes as three words (the image starts on a 4-byte boundary); the last thread of a file stores bytes
__global__ __launch_bounds__(kLanes) void k_jd_colour(const JFile *__restrict__ files, const uint8_t *__restrict__ planes,
                                                       uint8_t *__restrict__ out) {
    const JFile f = files[blockIdx.y];
    const int64_t npix = (int64_t)f.H * f.W;
    const int64_t p0 = ((int64_t)blockIdx.x * kLanes + threadIdx.x) * 4;
    if (p0 >= npix) return;
    uint8_t *O = out + f.out_off + p0 * 3;
    if (p0 + 4 <= npix) {
        const uint32_t a = bgr_at(planes, f, p0), b = bgr_at(planes, f, p0 + 1), c = bgr_at(planes, f, p0 + 2), d = bgr_at(planes, f, p0 + 3);
        uint32_t *O4 = (uint32_t *)O;
        O4[0] = a | b << 24;
        O4[1] = b >> 8 | c << 16;
        O4[2] = c >> 16 | d << 8;
    } else {
        for (int64_t p = p0; p < npix; ++p) {
            const uint32_t a = bgr_at(planes, f, p);
            O[0] = (uint8_t)a; O[1] = (uint8_t)(a >> 8); O[2] = (uint8_t)(a >> 16);
            O += 3;
        }
    }
}

}  // namespace
