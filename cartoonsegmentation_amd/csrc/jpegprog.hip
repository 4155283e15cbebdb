// jpegprog.hip -- progressive JPEG files (ITU T.81 SOF2, Huffman; spectral selection and successive approximation; grey, 4:4:4,
// 4:2:2, 4:2:0) to uint8 BGR on the device, for gfx950.  The contract is DESIGN.md §4.11; the coefficient decode is restated in
// tests/jpegprog_restatement.py, the host side (marker parser, scan script checks, table builder) is
// cartoonsegmentation_amd/jpegcode.py.  The coefficient store is the baseline decoder's (int16 [blocks][64], natural order,
// MCU-interleaved block order, zeroed first) and the pixels come from the same k_jd_idct and k_jd_colour (csm_jpeg.h).
//
// A work item is a (file, scan) pair.  The host orders the scans by dependency level (the scans of one level write disjoint
// coefficients) and launches one group of kernels per level over all files of the call.
//
//   first scans (ah = 0): the subsequence machine of csm_jpeg.h under the policy `FirstScan` below; a lane's state is (bit position,
//   block of the restart unit) in a DC scan and (bit position, k - ss) in an AC scan.  An EOBn symbol takes the rest of its block
//   and `run` whole bands of slots at once: the run uses no further bits and is no part of the state, so the scan still
//   synchronises by itself.
//     k_js_sync_local<FirstScan>, k_js_sync_global<FirstScan> (relaunched by the host until a device flag stays clear),
//     k_js_scan<FirstScan>, k_js_write<FirstScan>
//     k_pj_dc       DC first scans: differences -> values per component (restarting at every restart interval), then << al
//   refinements (ah = al + 1): the correction bits between two symbols of an AC refinement depend on the block's history, so a
//   lane that does not know its block can never find it: one lane decodes one restart interval of one scan, serially.
//     k_pj_mask     every block of an AC refinement scan -> the 64-bit mask of its band's non-zero coefficients
//     k_pj_refine   one wave per restart interval of a scan (the host lists where they begin), decoding on its lane 0; steps by
//                   symbols: the (r + 1)-th clear bit of the mask at or after k is the symbol's target, the set bits up to it are
//                   its correction bits.  It reads no coefficient and writes none: per block three 64-bit masks (corrections
//                   set, new coefficients, their signs); a DC refinement is one bit per block, written 32 to a word.
//     k_pj_apply    a lane per block applies those records to the coefficients
//
// No kernel waits on another workgroup and there is no spin loop on memory.  Every read is clamped to the scan's entropy range
// (Reader), every block index is checked against the scan's block count, every loop is bounded by a block count or an entropy
// length known before launch.
#include "csm_jpeg.h"

namespace {

constexpr int kScanWords = 16;
constexpr int kScanTables = 3;               // decode tables of one scan at the most: a DC table per component

struct PScan {
    // from the caller's descriptor
    int file, ns, comp, ss, se, ah, al, ent_off, ent_len, ri, tab_off, level;
    // derived
    int L;                       // coefficients of the band
    int bw, bh;                  // block grid of a one-component scan (the component's true size)
    int nblk;                    // blocks of the scan
    int bpu;                     // blocks per restart unit: an MCU's in a scan of all components, else 1
    int ntab;
    int sub0, nsub, nwg;         // first subsequence (of the call), subsequences, workgroups: first scans
    int64_t mask0;               // first 64-bit word (of the call) of the scan's records: refinements
    int nint, iv_off;            // restart intervals; refinements: offset in the blob of int32 [nint], the byte where each one begins
};

struct PPlan {
    std::vector<PScan> scans;    // ordered by (level, refinement)
    int64_t nsub = 0, masks = 0;
    int64_t o_scans, o_state, o_cnt_n, o_cnt_r, o_off_n, o_off_r, o_mask, o_flag, total;
};

// false: the descriptors are invalid (the error is set)
bool make_scan_plan(const Plan &p, const int32_t *sdesc, int n_scans, int64_t blob_bytes, bool check_ranges, PPlan &q) {
    const int n = (int)p.files.size();
    if (!sdesc || n_scans < 1 || n_scans > 64 * n) { csm::set_error("invalid argument: 1 <= n_scans <= 64 n scan descriptors"); return false; }
    q.scans.resize(n_scans);
    for (int i = 0; i < n_scans; ++i) {
        const int32_t *d = sdesc + (int64_t)i * kScanWords;
        PScan &s = q.scans[i];
        s.file = d[0]; s.ns = d[1]; s.comp = d[2]; s.ss = d[3]; s.se = d[4]; s.ah = d[5]; s.al = d[6];
        s.ent_off = d[7]; s.ent_len = d[8]; s.ri = d[9]; s.tab_off = d[10]; s.level = d[11]; s.iv_off = d[12];
        bool ok = s.file >= 0 && s.file < n;
        if (ok) {
            const JFile &f = p.files[s.file];
            ok = (s.ns == 1 || s.ns == f.nc) && s.comp >= 0 && s.comp + s.ns <= f.nc;
            ok = ok && s.ss >= 0 && s.ss <= s.se && s.se <= 63 && (s.ss > 0 ? s.ns == 1 : s.se == 0);
            ok = ok && s.al >= 0 && s.al <= 13 && (s.ah == 0 || s.ah == s.al + 1);
            ok = ok && s.ent_off >= 0 && s.ent_len >= 0 && s.ent_len <= kMaxEntropy && s.ri >= 0 && s.ri <= 65535;
            ok = ok && s.tab_off >= 0 && (s.tab_off & 3) == 0 && s.level >= 0 && s.level < 64;
            s.ntab = s.ss > 0 ? 1 : s.ah ? 0 : s.ns;
            if (ok && check_ranges)
                ok = (int64_t)s.ent_off + s.ent_len <= blob_bytes && (int64_t)s.tab_off + (int64_t)s.ntab * kTableBytes <= blob_bytes;
        }
        if (!ok) { csm::set_error("invalid argument: scan descriptor %d of the progressive JPEG decode", i); return false; }
        const JFile &f = p.files[s.file];
        s.L = s.se - s.ss + 1;
        if (s.ns > 1) { s.bw = s.bh = 0; s.nblk = f.nblk; s.bpu = f.bpm; }
        else {
            const int h = s.comp == 0 ? f.hs : 1, v = s.comp == 0 ? f.vs : 1;
            s.bw = ((f.W * h + f.hs - 1) / f.hs + 7) / 8;
            s.bh = ((f.H * v + f.vs - 1) / f.vs + 7) / 8;
            s.nblk = s.bw * s.bh;
            s.bpu = 1;
        }
        s.sub0 = 0; s.nsub = 0; s.nwg = 0; s.mask0 = 0;
        const int per = s.ri * s.bpu;
        s.nint = per > 0 ? std::max(1, (s.nblk + per - 1) / per) : 1;
        if (s.ah == 0 || s.nint == 1) s.iv_off = 0;
        else if (s.iv_off < 0 || (s.iv_off & 3) || (check_ranges && (int64_t)s.iv_off + (int64_t)s.nint * 4 > blob_bytes)) {
            csm::set_error("invalid argument: scan descriptor %d of the progressive JPEG decode (restart interval table)", i);
            return false;
        }
    }
    std::stable_sort(q.scans.begin(), q.scans.end(), [](const PScan &a, const PScan &b) {
        return a.level != b.level ? a.level < b.level : (a.ah != 0) < (b.ah != 0);
    });
    for (PScan &s : q.scans) {
        if (s.ah == 0) {
            s.nsub = std::max(1, (s.ent_len + kSubseq - 1) / kSubseq);
            s.nwg = (s.nsub + kLanes - 1) / kLanes;
            if (q.nsub + s.nsub >= INT32_MAX) { csm::set_error("invalid argument: too much entropy data in one call"); return false; }
            s.sub0 = (int)q.nsub;
            q.nsub += s.nsub;
        } else {
            // 64-bit words of the scan's records: four per block of an AC refinement, the bit words of a DC refinement
            const int per = s.nint > 1 ? s.ri * s.bpu : s.nblk;
            s.mask0 = q.masks;
            q.masks += s.ss > 0 ? (int64_t)s.nblk * 4 : ((int64_t)s.nint * ((per + 31) / 32) + 1) / 2;
        }
    }
    int64_t o = p.total;
    q.o_scans = o;  o += csm::align16((int64_t)n_scans * sizeof(PScan));
    q.o_state = o;  o += csm::align16(q.nsub * 8);
    q.o_cnt_n = o;  o += csm::align16(q.nsub * 4);
    q.o_cnt_r = o;  o += csm::align16(q.nsub * 4);
    q.o_off_n = o;  o += csm::align16(q.nsub * 8);
    q.o_off_r = o;  o += csm::align16(q.nsub * 4);
    q.o_mask = o;   o += csm::align16(q.masks * 8);
    q.o_flag = o;   o += 16;
    q.total = o;
    return true;
}

using ScanTables = HuffTables<kScanTables>;     // of one scan, in LDS: jpegcode.scan_tables

// store index (MCU-interleaved order of the file) of block i (< s.nblk) of the scan
__device__ __forceinline__ int store_index(const JFile &f, const PScan &s, int i) {
    if (s.ns > 1) return i;
    const int c = s.comp, h = c == 0 ? f.hs : 1, v = c == 0 ? f.vs : 1;
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs, first = c == 0 ? 0 : ysub + c - 1;
    const int by = i / s.bw, bx = i - by * s.bw;
    return ((by / v) * f.mx + bx / h) * f.bpm + first + (by % v) * h + (bx % h);
}

// ---- first scans ------------------------------------------------------------------------------------------------------------------
// The machine's policy for a first scan.  DC scan: b = block of the restart unit, one symbol (its size) and one slot per block.  AC
// scan: z = k - ss; a slot is one coefficient of the band of one block, blocks in scan order; a symbol (run, size) takes run + 1
// slots, ZRL 16, EOBn the rest of its block and (1 << n) - 1 + its n extra bits further bands.
struct FirstScan {
    using Tables = ScanTables;
    struct Args { const JFile *files; const PScan *scans; };       // scans: the first scans of the level
    const PScan s;
    const JFile f;
    __device__ FirstScan(const Args &a, int item) : s(a.scans[item]), f(a.files[s.file]) {}
    __device__ const PScan &seq() const { return s; }
    __device__ void load(Tables &T, const uint8_t *blob) const { load_tables(T, blob + s.tab_off, s.ntab); }
    __device__ int table(int b, int) const { return s.ss == 0 && s.ns > 1 ? (b < s.bpu - 2 ? 0 : b - (s.bpu - 3)) : 0; }
    __device__ bool symbol(int sym, int z, Symbol &y) const {
        if (s.ss == 0) { y.size = y.extra = sym; y.adv = 1; return sym <= 11; }
        const int run = sym >> 4;
        y.size = y.extra = sym & 15;
        if (y.size == 0) {
            if (run == 15) y.adv = 16;
            else { y.adv = 0; y.extra = run; }          // EOBn: what it takes follows from its extra bits (advance)
        } else {
            if (y.size > 10) return false;
            y.adv = run + 1;
        }
        return z + y.adv <= s.L;
    }
    __device__ int advance(const Symbol &y, int bits, int &b, int &z) const {
        if (s.ss == 0) { b = b + 1 < s.bpu ? b + 1 : 0; return 1; }
        const int adv = y.adv ? y.adv : (s.L - z) + ((1 << y.extra) - 1 + bits) * s.L;          // at most 32767 * 63 + 63
        z += adv;
        if (!y.adv || z >= s.L) z = 0;
        return adv;
    }
    __device__ void clamp(int &b, int &z) const {
        if (b >= s.bpu || s.ss > 0) b = 0;
        if (z >= s.L) z = 0;
    }
    __device__ void store(int16_t *coef, int64_t at, int val) const {
        const int64_t blk = at / s.L;
        if (at < 0 || blk >= s.nblk) return;
        const int k = s.ss + (int)(at - blk * s.L);
        // a DC difference is stored as it is: k_pj_dc sums and shifts
        coef[(f.blk0 + store_index(f, s, (int)blk)) * 64 + kNatural[k]] = (int16_t)(s.ss == 0 ? val : val * (1 << s.al));
    }
    __device__ int64_t interval_slots() const { return (int64_t)s.ri * s.bpu * s.L; }
    __device__ int64_t total_slots() const { return (int64_t)s.nblk * s.L; }
    __device__ int err_index(int) const { return s.file; }
};

// grid (components, first scans of the level): the DC differences of one component in scan order become values, << al; the sum
// restarts at every restart interval
__global__ __launch_bounds__(kLanes) void k_pj_dc(const JFile *__restrict__ files, const PScan *__restrict__ scans, int16_t *__restrict__ coef) {
    const PScan s = scans[blockIdx.y];
    if (s.ss != 0 || (int)blockIdx.x >= s.ns) return;
    const JFile f = files[s.file];
    const bool inter = s.ns > 1;
    const int c = inter ? (int)blockIdx.x : s.comp;
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs;
    const int nbc = inter && c == 0 ? ysub : 1, first = c == 0 ? 0 : ysub + c - 1;
    const int every = s.ri * nbc;                       // blocks of this component in a restart interval
    dc_predict(coef + f.blk0 * 64, inter ? f.mx * f.my * nbc : s.nblk, s.al,
               [&](int k) -> int64_t {
                   if (!inter) return (int64_t)store_index(f, s, k) * 64;
                   const int m = k / nbc, sb = k - m * nbc;
                   return ((int64_t)m * f.bpm + first + sb) * 64;
               },
               [&](int k) { return every > 0 && k % every == 0; });
}


// ---- refinements ------------------------------------------------------------------------------------------------------------------
// The serial decode never touches a coefficient: per block of an AC refinement it reads one 64-bit history mask and writes three
// (the coefficients whose correction bit is set, the new coefficients, the signs of the new ones); a DC refinement writes its bits
// as 32-bit words.  Kernels with a lane per block make the masks before (k_pj_mask) and apply the records after (k_pj_apply).
constexpr int kRecWords = 4;                 // 64-bit words per block of an AC refinement: history, corrections, new, signs

// words of 32 DC refinement bits per restart interval
__device__ __forceinline__ int dc_words(const PScan &s) { return ((s.nint > 1 ? s.ri * s.bpu : s.nblk) + 31) / 32; }

// grid (groups of kLanes blocks of the largest scan, refinement scans of the level): bit k of a block's mask = coefficient k (zigzag
// order) of the band is non-zero
__global__ __launch_bounds__(kLanes) void k_pj_mask(const JFile *__restrict__ files, const PScan *__restrict__ scans,
                                                     const int16_t *__restrict__ coef, uint64_t *__restrict__ rec) {
    const PScan s = scans[blockIdx.y];
    if (s.ss == 0) return;
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= s.nblk) return;
    const JFile f = files[s.file];
    const int16_t *C = coef + (f.blk0 + store_index(f, s, i)) * 64;
    uint64_t m = 0;
    for (int k = s.ss; k <= s.se; ++k) m |= (uint64_t)(C[kNatural[k]] != 0) << k;
    rec[s.mask0 + (int64_t)i * kRecWords] = m;
}

// the next n (<= 32) bits; false when the interval holds fewer
__device__ __forceinline__ bool take_bits(Reader &rd, int n, uint32_t &out) {
    rd.refill();
    if (rd.nb < n) return false;
    out = n ? (uint32_t)(rd.win >> (64 - n)) : 0u;
    rd.skip(n);
    return true;
}

// reads the correction bits of the coefficients in m (bits of the block's history mask), in ascending order of k, and sets in `set`
// the coefficients whose bit is 1.  false when the data end.
__device__ __forceinline__ bool corrections(Reader &rd, uint64_t m, uint64_t &set) {
    while (m) {
        const int n = min(__popcll(m), 32);
        uint32_t word;
        if (!take_bits(rd, n, word)) return false;
        for (int i = n - 1; i >= 0; --i) {
            const uint64_t low = m & (0ull - m);
            m ^= low;
            if ((word >> i) & 1u) set |= low;
        }
    }
    return true;
}

// keeps a load whose only purpose is to bring a cache line to this compute unit
__device__ __forceinline__ void touch(const void *p) {
    const uint32_t v = *(const volatile uint8_t *)p;
    asm volatile("" ::"v"(v));
}

// grid (workgroups per scan, refinement scans of the level); a WAVE decodes one restart interval of the scan at a time, serially on
// its lane 0: the interval starts at the byte offset that the host found behind its restart marker (int32 table in the blob; whatever
// it holds, the reader stays inside the scan's bytes and the block indices follow from the interval's number alone).  Before every
// 64 blocks the whole wave touches the cache lines that lane 0 is about to read (the next 8 KB of entropy data, the history masks),
// so that its dependent loads hit the compute unit's cache; the result does not depend on it.
__global__ __launch_bounds__(kLanes) void k_pj_refine(const uint8_t *__restrict__ blob, const JFile *__restrict__ files,
                                                       const PScan *__restrict__ scans, uint64_t *__restrict__ rec_all,
                                                       int *__restrict__ err) {
    __shared__ ScanTables T;
    const PScan s = scans[blockIdx.y];
    load_tables(T, blob + s.tab_off, s.ntab);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = blockIdx.x * (kLanes / 64) + (threadIdx.x >> 6), waves = gridDim.x * (kLanes / 64);
    const int per = s.nint > 1 ? s.ri * s.bpu : s.nblk;             // blocks of a restart interval
    const int *starts = (const int *)(blob + s.iv_off);
    const uint8_t *ent = blob + s.ent_off;
    uint64_t *rec = rec_all + s.mask0;
    const uint64_t band = (s.se == 63 ? ~0ull : (1ull << (s.se + 1)) - 1ull) & ~((1ull << s.ss) - 1ull);
    const int wpi = dc_words(s);
    int bad = 0;
    for (int iv = wave; iv < s.nint && !bad; iv += waves) {         // uniform over the wave
        const int i0 = iv * per, i1 = min(s.nblk, i0 + per);
        Reader rd;
        rd.open(ent, s.ent_len, iv == 0 ? 0 : max(0, starts[iv]));
        int eobrun = 0;
        for (int g = i0; g < i1 && !bad; g += 64) {
            const int g1 = min(i1, g + 64);
            if (s.ent_len > 0) touch(ent + min((int64_t)__shfl(rd.pos, 0) + lane * 128, (int64_t)s.ent_len - 1));
            if (s.ss > 0 && g + lane * 4 < g1) touch(rec + (int64_t)(g + lane * 4) * kRecWords);
            if (lane == 0) {
                if (s.ss == 0) {
                    // DC: one bit per block, 32 blocks to a word, the first block in bit 31
                    for (int i = g; i < g1;) {
                        const int n = min(32, g1 - i);
                        uint32_t word;
                        if (!take_bits(rd, n, word)) { bad = 2; break; }
                        ((uint32_t *)rec)[(int64_t)iv * wpi + ((i - i0) >> 5)] = word << (32 - n);
                        i += n;
                    }
                } else {
                    for (int i = g; i < g1 && !bad; ++i) {
                        const uint64_t hist = rec[(int64_t)i * kRecWords] & band;
                        uint64_t corr = 0, fresh = 0, sign = 0;
                        int k = s.ss;
                        if (eobrun == 0) {
                            while (k <= s.se) {
                                rd.refill();
                                const uint32_t v = (uint32_t)(rd.win >> 32);
                                int ln, sym;
                                if (!huff_decode(T, 0, v, ln, sym)) { bad = 1; break; }
                                const int r = sym >> 4, sz = sym & 15;
                                if (sz > 1) { bad = 4; break; }
                                const int extra = sz ? 1 : r < 15 ? r : 0, total = ln + extra;
                                if (total > rd.nb) { bad = 2; break; }
                                const int bits = extra ? (int)((v >> (32 - total)) & ((1u << extra) - 1u)) : 0;
                                rd.skip(total);
                                if (sz == 0 && r < 15) { eobrun = (1 << r) + bits; break; }        // this block included
                                // the (r + 1)-th coefficient without history at or after k
                                uint64_t free = ~hist & band & ~((1ull << k) - 1ull);
                                for (int q = 0; q < r; ++q) free &= free - 1;
                                const int target = free ? __ffsll((long long)free) - 1 : 64;
                                const uint64_t upto = target >= 63 ? ~0ull : (1ull << (target + 1)) - 1ull;
                                if (!corrections(rd, hist & upto & ~((1ull << k) - 1ull), corr)) { bad = 2; break; }
                                if (target > s.se) {
                                    if (sz) bad = 4;                                                // a coefficient placed past the band
                                    k = s.se + 1;
                                    break;
                                }
                                if (sz) { fresh |= 1ull << target; if (bits) sign |= 1ull << target; }
                                k = target + 1;
                            }
                        }
                        if (!bad && eobrun > 0) {
                            if (k <= s.se && !corrections(rd, hist & ~((1ull << k) - 1ull), corr)) bad = 2;
                            --eobrun;
                        }
                        rec[(int64_t)i * kRecWords + 1] = corr;
                        rec[(int64_t)i * kRecWords + 2] = fresh;
                        rec[(int64_t)i * kRecWords + 3] = sign;
                    }
                }
                if (!bad && g1 == i1) {                 // fewer than 8 bits are left in front of the next marker, or of the end
                    rd.refill();
                    if (rd.stop != (iv == s.nint - 1 ? 2 : 1) || rd.nb >= 8) bad = 2;
                }
            }
            bad = __shfl(bad, 0);
        }
    }
    if (bad && lane == 0) atomicOr(err + s.file, bad);
}

// grid (groups of kLanes blocks of the largest scan, refinement scans of the level): a lane applies the record of one block.  AC: a
// set correction bit moves the coefficient by 1 << al away from zero (unless that bit of it is set already: it never is after the
// scans before), a new coefficient is +- 1 << al.  DC: the bit is ORed in at 1 << al, in two's complement.
__global__ __launch_bounds__(kLanes) void k_pj_apply(const JFile *__restrict__ files, const PScan *__restrict__ scans,
                                                      const uint64_t *__restrict__ rec_all, int16_t *__restrict__ coef) {
    const PScan s = scans[blockIdx.y];
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= s.nblk) return;
    const JFile f = files[s.file];
    int16_t *C = coef + (f.blk0 + store_index(f, s, i)) * 64;
    const uint64_t *rec = rec_all + s.mask0;
    const int p1 = 1 << s.al;
    if (s.ss == 0) {
        const int per = s.nint > 1 ? s.ri * s.bpu : s.nblk;
        const int iv = i / per, j = i - iv * per;
        const uint32_t word = ((const uint32_t *)rec)[(int64_t)iv * dc_words(s) + (j >> 5)];
        if ((word >> (31 - (j & 31))) & 1u) C[0] |= (int16_t)p1;
        return;
    }
    uint64_t corr = rec[(int64_t)i * kRecWords + 1], fresh = rec[(int64_t)i * kRecWords + 2];
    const uint64_t sign = rec[(int64_t)i * kRecWords + 3];
    const uint64_t band = (s.se == 63 ? ~0ull : (1ull << (s.se + 1)) - 1ull) & ~((1ull << s.ss) - 1ull);
    corr &= band; fresh &= band;
    while (corr) {
        const int k = __ffsll((long long)corr) - 1;
        corr &= corr - 1;
        const int c = C[kNatural[k]], a = c < 0 ? -c : c;
        if ((a & p1) == 0) C[kNatural[k]] = (int16_t)(c >= 0 ? c + p1 : c - p1);
    }
    while (fresh) {
        const int k = __ffsll((long long)fresh) - 1;
        fresh &= fresh - 1;
        C[kNatural[k]] = (int16_t)((sign >> k) & 1u ? p1 : -p1);
    }
}

}  // namespace

extern "C" int csm_jpeg_decode_scan_desc_words(void) { return kScanWords; }

extern "C" size_t csm_jpeg_decode_progressive_scratch_bytes(const int32_t *desc_host, int n, const int32_t *scan_desc_host, int n_scans) {
    Plan p;
    PPlan q;
    if (!make_plan(desc_host, n, 0, 0, false, p)) return 0;
    if (!make_scan_plan(p, scan_desc_host, n_scans, 0, false, q)) return 0;
    return (size_t)q.total;
}

extern "C" int csm_jpeg_decode_progressive(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n,
                                           const int32_t *scan_desc_host, int n_scans, uint8_t *out, int64_t out_bytes, void *scratch,
                                           int *info_host, void *stream) {
    if (n == 0) return CSM_OK;
    CSM_REQUIRE(blob && desc_host && scan_desc_host && out && scratch && blob_bytes > 0 && out_bytes > 0);
    CSM_REQUIRE(((uintptr_t)blob & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
    Plan p;
    PPlan q;
    if (!make_plan(desc_host, n, blob_bytes, out_bytes, true, p)) return CSM_ERR_ARG;
    if (!make_scan_plan(p, scan_desc_host, n_scans, blob_bytes, true, q)) return CSM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *S = (char *)scratch;
    JFile *files = (JFile *)(S + p.o_files);
    int *err = (int *)(S + p.o_err);
    int16_t *coef = (int16_t *)(S + p.o_coef);
    uint8_t *planes = (uint8_t *)(S + p.o_planes);
    PScan *scans = (PScan *)(S + q.o_scans);
    const Subseq sub = subseq_regions(S, q);
    uint64_t *mask = (uint64_t *)(S + q.o_mask);
    // the descriptors live in p and q until this call returns, and it returns only after the stream has drained (below)
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(JFile), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemcpyAsync(scans, q.scans.data(), (size_t)n_scans * sizeof(PScan), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemsetAsync(S + p.o_flag, 0, (size_t)(p.o_coef - p.o_flag) + (size_t)csm::align16(p.blocks * 128), st));   // flag, err, coefficients
    CSM_HIP(hipMemsetAsync(sub.flag, 0, 16, st));
    int passes = 0, levels = 0, rc;
    int i = 0;
    while (i < n_scans) {
        // [i, m): the first scans of this level, [m, e): its refinements
        int m = i, e;
        while (m < n_scans && q.scans[m].level == q.scans[i].level && q.scans[m].ah == 0) ++m;
        e = m;
        while (e < n_scans && q.scans[e].level == q.scans[i].level) ++e;
        ++levels;
        if (m - i > 65535 || e - m > 65535) { csm::set_error("invalid argument: more than 65535 scans in one level"); return CSM_ERR_ARG; }
        if (m > i) {
            int max_wg = 0, level_sub = 0;
            for (int k = i; k < m; ++k) { max_wg = std::max(max_wg, q.scans[k].nwg); level_sub += q.scans[k].nsub; }
            rc = subseq_decode<FirstScan>(blob, {files, scans + i}, m - i, max_wg, level_sub, sub, coef, err, passes, st); if (rc) return rc;
            k_pj_dc<<<dim3(3, (unsigned)(m - i)), kLanes, 0, st>>>(files, scans + i, coef);
            rc = csm::check_launch("k_pj_dc"); if (rc) return rc;
        }
        if (e > m) {
            int max_ac = 0, max_blk = 0, max_int = 1;
            for (int k = m; k < e; ++k) {
                if (q.scans[k].ss > 0) max_ac = std::max(max_ac, q.scans[k].nblk);
                max_blk = std::max(max_blk, q.scans[k].nblk);
                max_int = std::max(max_int, q.scans[k].nint);
            }
            if (max_ac) {
                k_pj_mask<<<dim3(csm::cdiv(max_ac, kLanes), (unsigned)(e - m)), kLanes, 0, st>>>(files, scans + m, coef, mask);
                rc = csm::check_launch("k_pj_mask"); if (rc) return rc;
            }
            // four waves to a workgroup, a restart interval to a wave at a time, at most 64 workgroups per scan
            k_pj_refine<<<dim3(std::min(64u, csm::cdiv(max_int, kLanes / 64)), (unsigned)(e - m)), kLanes, 0, st>>>(blob, files, scans + m, mask, err);
            rc = csm::check_launch("k_pj_refine"); if (rc) return rc;
            k_pj_apply<<<dim3(csm::cdiv(max_blk, kLanes), (unsigned)(e - m)), kLanes, 0, st>>>(files, scans + m, mask, coef);
            rc = csm::check_launch("k_pj_apply"); if (rc) return rc;
        }
        i = e;
    }
    k_jd_idct<<<dim3(csm::cdiv(p.max_blocks, kIdctBlocks), (unsigned)n), kLanes, 0, st>>>(blob, files, coef, planes);
    rc = csm::check_launch("k_jd_idct"); if (rc) return rc;
    k_jd_colour<<<dim3(csm::cdiv(p.max_pixels, 4 * kLanes), (unsigned)n), kLanes, 0, st>>>(files, planes, out);
    rc = csm::check_launch("k_jd_colour"); if (rc) return rc;
    std::vector<int> err_host(n);
    CSM_HIP(hipMemcpyAsync(err_host.data(), err, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    if (info_host) { info_host[0] = passes; info_host[1] = levels; info_host[2] = 0; info_host[3] = 0; }
    for (int k = 0; k < n; ++k) {
        if (err_host[k]) {
            csm::set_error("jpeg decode: file %d of the call has corrupt entropy data (%s)", k,
                           (err_host[k] & 1) ? "an invalid Huffman code" : (err_host[k] & 4) ? "an invalid refinement symbol"
                                                                           : "the data do not hold a scan's blocks");
            return CSM_ERR_DATA;
        }
    }
    return CSM_OK;
}
