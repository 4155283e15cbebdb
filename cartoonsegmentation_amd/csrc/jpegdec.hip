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
#include "csm_jpeg.h"

namespace {

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
    CSM_HIP(hipMemsetAsync(flag, 0, (size_t)(p.o_coef - p.o_flag) + (size_t)csm::align16(p.blocks * 128), st));       // flag, err, coefficients
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
