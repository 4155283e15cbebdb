// jpegdec.hip -- baseline JPEG files (ITU T.81 SOF0 / SOF1, Huffman, one interleaved scan; grey, 4:4:4, 4:2:2, 4:2:0) to uint8 BGR
// on the device, for gfx950.  The contract is fixed to the byte and restated in numpy in
// tests/jpegdec_restatement.py; the host side (marker parser, table builder) is cartoonsegmentation_amd/jpegcode.py.
//
// Entropy decode: files from the outside world carry no restart markers, so the segment is decoded in parallel by the
// self-synchronising subsequence decode of Weissenberger and Schmidt (ICPP 2018).  The entropy bytes of every file are cut into
// subsequences of kSubseq bytes; one lane owns one.  A lane's state is (bit position, block of the MCU, zigzag index) and it counts
// the coefficient slots and the restart markers it passes.
//
//   k_jd_sync_local   every lane decodes its own subsequence from a cold state, then goes on into its successors from its own end
//                     state, through LDS, until its end state equals the one recorded there or the workgroup ends
//   k_jd_sync_global  (relaunched until a device flag reports no change; the host reads the 4-byte flag) one lane per workgroup
//                     carries the end state of the workgroup before it into its own subsequences until it meets the recorded state
//   k_jd_scan         exclusive scan of the slot and marker counts per file: the output position of every subsequence
//   k_jd_write        decodes every subsequence once more from its entry state; int16 coefficients in natural order at their
//                     block (the buffer is zeroed before), DC still as a difference
//   k_jd_dc           segmented scan per component (restarting at every restart interval): DC differences -> values
//   k_jd_idct         dequantisation and the two passes of the 13-bit integer inverse DCT -> the sample planes
//   k_jd_colour       triangle chroma upsampling, colour conversion, BGR stores
//
// No kernel waits on another workgroup and there is no spin loop on memory.  FF 00 stuffing and RSTn markers are handled in line.
// Every read is clamped to the file's entropy range and every coefficient store to the file's block count, whatever the data.
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

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

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
            if (c < f.nc) p.plane_bytes += align16((int64_t)f.pw[c] * f.ph[c]);
        }
        p.nsub += f.nsub;
        p.blocks += nblk;
        p.max_wg = std::max(p.max_wg, f.nwg);
        p.max_blocks = std::max(p.max_blocks, f.nblk);
        p.max_pixels = std::max(p.max_pixels, (int64_t)f.H * f.W);
    }
    int64_t o = 0;
    p.o_files = o;   o += align16((int64_t)n * sizeof(JFile));
    p.o_state = o;   o += align16(p.nsub * 8);
    p.o_cnt_n = o;   o += align16(p.nsub * 4);
    p.o_cnt_r = o;   o += align16(p.nsub * 4);
    p.o_off_n = o;   o += align16(p.nsub * 8);
    p.o_off_r = o;   o += align16(p.nsub * 4);
    p.o_flag = o;    o += 16;
    p.o_err = o;     o += align16((int64_t)n * 4);
    p.o_coef = o;    o += align16(p.blocks * 128);
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

struct Tables {                 // of one file, in LDS: jpegcode.file_tables without the quantisation tables
    uint32_t w[kHuffSlots * kTableBytes / 4];
    __device__ __forceinline__ const uint16_t *lut(int s) const { return (const uint16_t *)((const uint8_t *)w + s * kTableBytes); }
    __device__ __forceinline__ const int *maxcode(int s) const { return (const int *)((const uint8_t *)w + s * kTableBytes + 512); }
    __device__ __forceinline__ const int *valoff(int s) const { return (const int *)((const uint8_t *)w + s * kTableBytes + 584); }
    __device__ __forceinline__ const uint8_t *vals(int s) const { return (const uint8_t *)w + s * kTableBytes + 656; }
};

__device__ __forceinline__ void load_tables(Tables &T, const uint8_t *blob, const JFile &f) {
    const uint32_t *src = (const uint32_t *)(blob + f.tab_off);
    for (int i = threadIdx.x; i < kHuffSlots * kTableBytes / 4; i += blockDim.x) T.w[i] = src[i];
}

__device__ __forceinline__ uint64_t pack_state(uint32_t p, int b, int z) { return ((uint64_t)p << 16) | ((uint64_t)b << 8) | (uint64_t)z; }

// what the coefficient stores of the write pass need
struct Sink {
    int16_t *coef;       // the file's blocks
    int64_t slots;       // 64 * blocks of the file
    int64_t slot;        // slot of the current state
    int64_t per_marker;  // slots of a restart interval
    int marks_before;
};

// Decodes symbols from (rd, b, z) while the next symbol begins before bit `limit` of the file's entropy bytes.  Returns the packed
// end state, kDead after an invalid code.  n_slots / n_mark count the coefficient slots and the restart markers passed.
template <bool EMIT>
__device__ uint64_t jd_run(Reader &rd, int &b, int &z, uint32_t limit, const JFile &f, const Tables &T, int &n_slots, int &n_mark,
                           Sink &sink) {
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs;
    for (;;) {
        rd.refill();
        bool marker = rd.at_marker();
        int adv = 0, s = 0, total = 0;
        uint32_t v = 0;
        if (!marker) {
            if (rd.bitpos() >= limit) return pack_state(rd.bitpos(), b, z);
            v = (uint32_t)(rd.win >> 32);
            const int comp = b < ysub ? 0 : b - ysub + 1;
            const int slot = (int)(f.tabsel >> (8 * comp + (z == 0 ? 0 : 4))) & 15;
            const uint32_t e = T.lut(slot)[v >> 24];
            int ln, sym;
            if (e) { ln = (int)(e >> 8); sym = (int)(e & 255u); }
            else {
                const int *mc = T.maxcode(slot);
                const int code16 = (int)(v >> 16);
                int c = 0;
                for (ln = 9; ln <= 16; ++ln) { c = code16 >> (16 - ln); if (c <= mc[ln]) break; }
                if (ln > 16) return kDead;
                sym = T.vals(slot)[(T.valoff(slot)[ln] + c) & 255];
            }
            if (z == 0) {
                s = sym; adv = 1;
                if (s > 11) return kDead;
            } else {
                const int run = sym >> 4;
                s = sym & 15;
                if (s == 0) {
                    if (run == 15) adv = 16;
                    else if (run == 0) adv = 64 - z;
                    else return kDead;
                } else {
                    if (s > 10) return kDead;
                    adv = run + 1;
                }
                if (z + adv > 64) return kDead;
            }
            total = ln + s;
            marker = total > rd.nb;              // the symbol runs into a marker or the end: not a symbol
        }
        if (marker) {
            if (rd.stop != 1) { b = 0; z = 0; return pack_state((uint32_t)f.ent_len * 8u, 0, 0); }
            rd.cross();
            b = 0; z = 0;
            ++n_mark;
            if constexpr (EMIT) sink.slot = (int64_t)(sink.marks_before + n_mark) * sink.per_marker;
            continue;
        }
        if constexpr (EMIT) {
            if (s) {
                int val = (int)((v >> (32 - total)) & ((1u << s) - 1u));
                if (val < (1 << (s - 1))) val -= (1 << s) - 1;
                const int64_t at = sink.slot + adv - 1;
                if (at >= 0 && at < sink.slots) sink.coef[(at & ~(int64_t)63) + kNatural[at & 63]] = (int16_t)val;
            }
            sink.slot += adv;
        }
        rd.skip(total);
        z += adv;
        n_slots += adv;
        if (z == 64) { z = 0; b = b + 1 < f.bpm ? b + 1 : 0; }
    }
}

// a reader at the packed state st (not kDead) of the file
__device__ __forceinline__ void open_at(Reader &rd, const uint8_t *ent, const JFile &f, uint64_t st, int &b, int &z) {
    const uint32_t p = (uint32_t)(st >> 16);
    b = (int)((st >> 8) & 255u); z = (int)(st & 255u);
    if (b >= f.bpm) b = 0;
    if (z > 63) z = 0;
    rd.open(ent, f.ent_len, (int)min(p >> 3, (uint32_t)f.ent_len));
    rd.refill();
    const int off = (int)(p & 7u);
    if (off < rd.nb) rd.skip(off);
}

__device__ __forceinline__ bool same_state(uint64_t a, uint64_t b) { return a == b && a != kDead; }

// ---- synchronisation --------------------------------------------------------------------------------------------------------
// grid (workgroups of the largest file, files); lane = one subsequence
__global__ __launch_bounds__(kLanes) void k_jd_sync_local(const uint8_t *__restrict__ blob, const JFile *__restrict__ files,
                                                           uint64_t *__restrict__ state, int *__restrict__ cnt_n, int *__restrict__ cnt_r) {
    __shared__ Tables T;
    __shared__ uint64_t sState[kLanes];
    __shared__ int sN[kLanes], sR[kLanes];
    const JFile f = files[blockIdx.y];
    if ((int)blockIdx.x >= f.nwg) return;
    const int t = threadIdx.x, j = blockIdx.x * kLanes + t;
    const bool valid = j < f.nsub;
    const uint8_t *ent = blob + f.ent_off;
    load_tables(T, blob, f);
    __syncthreads();
    Reader rd;
    Sink none{};
    int b = 0, z = 0;
    uint64_t cur = kDead;
    if (valid) {
        // cold: block 0 of an MCU, zigzag index 0.  On the 00 of a stuffed pair or on the code of a marker, start behind it.
        int start = j * kSubseq;
        if (start > 0 && start < f.ent_len && ent[start - 1] == 0xFFu && (ent[start] == 0 || (ent[start] >= 0xD0u && ent[start] <= 0xD7u))) ++start;
        rd.open(ent, f.ent_len, start);
        int n = 0, r = 0;
        cur = jd_run<false>(rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), f, T, n, r, none);
        sN[t] = n; sR[t] = r;
    }
    sState[t] = cur;
    bool active = valid && cur != kDead;
    for (int step = 1; step < kLanes; ++step) {
        __syncthreads();
        const int tj = t + step;
        const bool go = active && tj < kLanes && j + step < f.nsub;
        if (!go) active = false;
        if (go) {
            int n = 0, r = 0;
            const uint64_t ns = jd_run<false>(rd, b, z, (uint32_t)(j + step + 1) * (kSubseq * 8u), f, T, n, r, none);
            const uint64_t old = sState[tj];
            sState[tj] = ns; sN[tj] = n; sR[tj] = r;
            if (ns == kDead || ns == old) active = false;
        }
        if (!__syncthreads_or(active)) break;
    }
    __syncthreads();
    if (valid) {
        state[f.sub0 + j] = sState[t];
        cnt_n[f.sub0 + j] = sN[t];
        cnt_r[f.sub0 + j] = sR[t];
    }
}

// grid (workgroups of the largest file, files), one wave; lane 0 carries the state across the workgroup's first boundary
__global__ __launch_bounds__(64) void k_jd_sync_global(const uint8_t *__restrict__ blob, const JFile *__restrict__ files, uint64_t *state,
                                                        int *__restrict__ cnt_n, int *__restrict__ cnt_r, int *__restrict__ flag) {
    __shared__ Tables T;
    const JFile f = files[blockIdx.y];
    if (blockIdx.x == 0 || (int)blockIdx.x >= f.nwg) return;
    load_tables(T, blob, f);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int j0 = blockIdx.x * kLanes, j1 = min(j0 + kLanes, f.nsub);
    // the state of the workgroup before this one may be rewritten while it is read here: either value is a state, and a rewrite
    // raises the flag, so that this workgroup reads it again in the next launch
    uint64_t st = __hip_atomic_load(state + f.sub0 + j0 - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st == kDead) return;
    Reader rd;
    Sink none{};
    int b, z;
    open_at(rd, blob + f.ent_off, f, st, b, z);
    for (int j = j0; j < j1; ++j) {
        int n = 0, r = 0;
        const uint64_t ns = jd_run<false>(rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), f, T, n, r, none);
        const uint64_t old = state[f.sub0 + j];
        cnt_n[f.sub0 + j] = n;
        cnt_r[f.sub0 + j] = r;
        if (ns == old) break;
        __hip_atomic_store(state + f.sub0 + j, ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = 1;
        if (ns == kDead) break;
    }
}

// ---- output positions -------------------------------------------------------------------------------------------------------
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

// one workgroup per file: off_n / off_r = exclusive sums of cnt_n / cnt_r over the file's subsequences
__global__ __launch_bounds__(kLanes) void k_jd_scan(const JFile *__restrict__ files, const int *__restrict__ cnt_n, const int *__restrict__ cnt_r,
                                                     int64_t *__restrict__ off_n, int *__restrict__ off_r) {
    __shared__ int64_t sh[kLanes];
    const JFile f = files[blockIdx.x];
    const int t = threadIdx.x;
    const int per = (f.nsub + kLanes - 1) / kLanes, j0 = min(f.nsub, t * per), j1 = min(f.nsub, j0 + per);
    int64_t sn = 0, sr = 0;
    for (int j = j0; j < j1; ++j) { sn += cnt_n[f.sub0 + j]; sr += cnt_r[f.sub0 + j]; }
    int64_t en = block_exclusive(sn, sh);
    int64_t er = block_exclusive(sr, sh);
    for (int j = j0; j < j1; ++j) {
        off_n[f.sub0 + j] = en; off_r[f.sub0 + j] = (int)min(er, (int64_t)INT32_MAX);
        en += cnt_n[f.sub0 + j]; er += cnt_r[f.sub0 + j];
    }
}

// ---- write pass -------------------------------------------------------------------------------------------------------------
// err bits: 1 an invalid code or a subsequence without a state, 2 the data do not hold the file's blocks exactly
__global__ __launch_bounds__(kLanes) void k_jd_write(const uint8_t *__restrict__ blob, const JFile *__restrict__ files,
                                                      const uint64_t *__restrict__ state, const int *__restrict__ cnt_n,
                                                      const int64_t *__restrict__ off_n, const int *__restrict__ off_r,
                                                      int16_t *__restrict__ coef, int *__restrict__ err) {
    __shared__ Tables T;
    const JFile f = files[blockIdx.y];
    if ((int)blockIdx.x >= f.nwg) return;
    load_tables(T, blob, f);
    __syncthreads();
    const int j = blockIdx.x * kLanes + threadIdx.x;
    if (j >= f.nsub) return;
    const uint64_t st = j == 0 ? pack_state(0, 0, 0) : state[f.sub0 + j - 1];
    if (st == kDead) { atomicOr(err + blockIdx.y, 1); return; }
    Reader rd;
    int b, z;
    open_at(rd, blob + f.ent_off, f, st, b, z);
    Sink sink;
    sink.coef = coef + f.blk0 * 64;
    sink.slots = (int64_t)f.nblk * 64;
    sink.slot = off_n[f.sub0 + j];
    sink.per_marker = (int64_t)f.ri * f.bpm * 64;
    sink.marks_before = off_r[f.sub0 + j];
    int n = 0, r = 0;
    const uint64_t ns = jd_run<true>(rd, b, z, (uint32_t)(j + 1) * (kSubseq * 8u), f, T, n, r, sink);
    if (ns == kDead) atomicOr(err + blockIdx.y, 1);
    if (j == f.nsub - 1 && off_n[f.sub0 + j] + cnt_n[f.sub0 + j] != sink.slots) atomicOr(err + blockIdx.y, 2);
}

// ---- DC prediction ----------------------------------------------------------------------------------------------------------
// grid (components, files): the DC differences of one component in scan order become values; the sum restarts at every restart
// interval.  A thread sums a run of consecutive blocks; the runs are joined by a segmented scan over the workgroup.
__global__ __launch_bounds__(kLanes) void k_jd_dc(const JFile *__restrict__ files, int16_t *__restrict__ coef) {
    __shared__ int sSum[kLanes];
    __shared__ int sFlag[kLanes];
    const JFile f = files[blockIdx.y];
    const int c = blockIdx.x, t = threadIdx.x;
    if (c >= f.nc) return;
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs;
    const int nbc = c == 0 ? ysub : 1, first = c == 0 ? 0 : ysub + c - 1;
    const int mcus = f.mx * f.my;
    const int total = mcus * nbc;
    int16_t *C = coef + f.blk0 * 64;
    const int per = (total + kLanes - 1) / kLanes, k0 = min(total, t * per), k1 = min(total, k0 + per);
    auto addr = [&](int k) { const int m = k / nbc, sb = k - m * nbc; return ((int64_t)m * f.bpm + first + sb) * 64; };
    auto resets = [&](int k) { const int m = k / nbc; return f.ri > 0 && k - m * nbc == 0 && m % f.ri == 0; };
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
        run += C[addr(k)];
        C[addr(k)] = (int16_t)run;
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

extern "C" int csm_jpeg_decode_subseq_bytes(void) { return kSubseq; }

extern "C" int csm_jpeg_decode_desc_words(void) { return kDescWords; }

extern "C" size_t csm_jpeg_decode_scratch_bytes(const int32_t *desc_host, int n) {
    Plan p;
    if (!make_plan(desc_host, n, 0, 0, false, p)) return 0;
    return (size_t)p.total;
}

extern "C" int csm_jpeg_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                               void *scratch, int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && out && scratch && blob_bytes > 0 && out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    Plan p;
    if (!make_plan(desc_host, n, blob_bytes, out_bytes, true, p)) return CSM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *S = (char *)scratch;
    JFile *files = (JFile *)(S + p.o_files);
    uint64_t *state = (uint64_t *)(S + p.o_state);
    int *cnt_n = (int *)(S + p.o_cnt_n), *cnt_r = (int *)(S + p.o_cnt_r), *off_r = (int *)(S + p.o_off_r);
    int64_t *off_n = (int64_t *)(S + p.o_off_n);
    int *flag = (int *)(S + p.o_flag), *err = (int *)(S + p.o_err);
    int16_t *coef = (int16_t *)(S + p.o_coef);
    uint8_t *planes = (uint8_t *)(S + p.o_planes);
    // the descriptors live in p until this call returns, and it returns only after the stream has drained (below)
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(JFile), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemsetAsync(flag, 0, (size_t)(p.o_coef - p.o_flag) + (size_t)align16(p.blocks * 128), st));       // flag, err, coefficients
    const dim3 sub_grid((unsigned)p.max_wg, (unsigned)n);
    k_jd_sync_local<<<sub_grid, kLanes, 0, st>>>(blob, files, state, cnt_n, cnt_r);
    int rc = csm::check_launch("k_jd_sync_local"); if (rc) return rc;
    int passes = 0;
    if (p.max_wg > 1) {
        for (;;) {
            if (passes > p.nsub) {
                (void)hipStreamSynchronize(st);
                csm::set_error("jpeg decode: the subsequence states did not settle in %d passes", passes);
                return CSM_ERR_DATA;
            }
            int changed = 0;
            if (passes) CSM_HIP(hipMemsetAsync(flag, 0, 4, st));
            k_jd_sync_global<<<sub_grid, 64, 0, st>>>(blob, files, state, cnt_n, cnt_r, flag);
            rc = csm::check_launch("k_jd_sync_global"); if (rc) return rc;
            CSM_HIP(hipMemcpyAsync(&changed, flag, 4, hipMemcpyDeviceToHost, st));
            CSM_HIP(hipStreamSynchronize(st));
            ++passes;
            if (!changed) break;
        }
    }
    k_jd_scan<<<n, kLanes, 0, st>>>(files, cnt_n, cnt_r, off_n, off_r);
    rc = csm::check_launch("k_jd_scan"); if (rc) return rc;
    k_jd_write<<<sub_grid, kLanes, 0, st>>>(blob, files, state, cnt_n, off_n, off_r, coef, err);
    rc = csm::check_launch("k_jd_write"); if (rc) return rc;
    k_jd_dc<<<dim3(3, (unsigned)n), kLanes, 0, st>>>(files, coef);
    rc = csm::check_launch("k_jd_dc"); if (rc) return rc;
    k_jd_idct<<<dim3(csm::cdiv(p.max_blocks, kIdctBlocks), (unsigned)n), kLanes, 0, st>>>(blob, files, coef, planes);
    rc = csm::check_launch("k_jd_idct"); if (rc) return rc;
    k_jd_colour<<<dim3(csm::cdiv(p.max_pixels, 4 * kLanes), (unsigned)n), kLanes, 0, st>>>(files, planes, out);
    rc = csm::check_launch("k_jd_colour"); if (rc) return rc;
    std::vector<int> err_host(n);
    CSM_HIP(hipMemcpyAsync(err_host.data(), err, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    if (info_host) info_host[0] = passes;
    for (int i = 0; i < n; ++i) {
        if (err_host[i]) {
            csm::set_error("jpeg decode: file %d of the call has corrupt entropy data (%s)", i,
                           (err_host[i] & 1) ? "an invalid Huffman code" : "the data do not hold the frame's blocks");
            return CSM_ERR_DATA;
        }
    }
    return CSM_OK;
}
