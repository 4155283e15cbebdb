// jpegdec.hip -- baseline JPEG files (ITU T.81 SOF0 / SOF1, Huffman, one interleaved scan; grey, 4:4:4, 4:2:2, 4:2:0) to uint8 BGR
// on the device, for gfx950.  The contract is fixed to the byte and restated in numpy in
// tests/jpegdec_restatement.py; the host side (marker parser, table builder) is cartoonsegmentation_amd/jpegcode.py.
//
// Entropy decode: files from the outside world carry no restart markers, so the segment is decoded in parallel by the
// self-synchronising subsequence decode of Weissenberger and Schmidt (ICPP 2018): the machine of csm_jpeg.h under the policy
// `Baseline` below.  The entropy bytes of every file are cut into subsequences of kSubseq bytes; one lane owns one.  A lane's state
// is (bit position, block of the MCU, zigzag index) and it counts the coefficient slots and the restart markers it passes.
//
//   k_js_sync_local<Baseline>   every lane decodes its own subsequence from a cold state, then goes on into its successors from its
//                               own end state, through LDS, until its end state equals the one recorded there or the workgroup ends
//   k_js_sync_global<Baseline>  (relaunched until a device flag reports no change; the host reads the 4-byte flag) one lane per
//                               workgroup carries the end state of the workgroup before it into its own subsequences until it meets
//                               the recorded state
//   k_js_scan<Baseline>         exclusive scan of the slot and marker counts per file: the output position of every subsequence
//   k_js_write<Baseline>        decodes every subsequence once more from its entry state; int16 coefficients in natural order at
//                               their block (the buffer is zeroed before), DC still as a difference
//   k_jd_dc                     segmented scan per component (restarting at every restart interval): DC differences -> values
//   k_jd_idct                   dequantisation and the two passes of the 13-bit integer inverse DCT -> the sample planes
//   k_jd_colour                 triangle chroma upsampling, colour conversion, BGR stores
//
// No kernel waits on another workgroup and there is no spin loop on memory.  FF 00 stuffing and RSTn markers are handled in line.
// Every read is clamped to the file's entropy range and every coefficient store to the file's block count, whatever the data.
#include "csm_jpeg.h"

namespace {

// The machine's policy for a baseline file: b = block of the MCU, z = zigzag index, a slot = one coefficient of one block in scan
// order.  A DC symbol is its size; an AC symbol (run, size) takes run + 1 slots, ZRL 16, EOB the rest of the block.
struct Baseline {
    using Tables = HuffTables<kHuffSlots>;          // jpegcode.file_tables without the quantisation tables
    struct Args { const JFile *files; };
    const JFile f;
    const int ysub;
    __device__ Baseline(const Args &a, int item) : f(a.files[item]), ysub(f.nc == 1 ? 1 : f.hs * f.vs) {}
    __device__ const JFile &seq() const { return f; }
    __device__ void load(Tables &T, const uint8_t *blob) const { load_tables(T, blob + f.tab_off, kHuffSlots); }
    __device__ int table(int b, int z) const {
        const int comp = b < ysub ? 0 : b - ysub + 1;
        return (int)(f.tabsel >> (8 * comp + (z == 0 ? 0 : 4))) & 15;
    }
    __device__ bool symbol(int sym, int z, Symbol &y) const {
        if (z == 0) { y.size = y.extra = sym; y.adv = 1; return sym <= 11; }
        const int run = sym >> 4;
        y.size = y.extra = sym & 15;
        if (y.size == 0) {
            if (run == 15) y.adv = 16;
            else if (run == 0) y.adv = 64 - z;
            else return false;
        } else {
            if (y.size > 10) return false;
            y.adv = run + 1;
        }
        return z + y.adv <= 64;
    }
    __device__ int advance(const Symbol &y, int, int &b, int &z) const {
        z += y.adv;
        if (z == 64) { z = 0; b = b + 1 < f.bpm ? b + 1 : 0; }
        return y.adv;
    }
    __device__ void clamp(int &b, int &z) const {
        if (b >= f.bpm) b = 0;
        if (z > 63) z = 0;
    }
    __device__ void store(int16_t *coef, int64_t at, int val) const {
        if (at >= 0 && at < total_slots()) coef[f.blk0 * 64 + (at & ~(int64_t)63) + kNatural[at & 63]] = (int16_t)val;
    }
    __device__ int64_t interval_slots() const { return (int64_t)f.ri * f.bpm * 64; }
    __device__ int64_t total_slots() const { return (int64_t)f.nblk * 64; }
    __device__ int err_index(int item) const { return item; }
};

// grid (components, files): the DC differences of one component in scan order become values; the sum restarts at every restart
// interval
__global__ __launch_bounds__(kLanes) void k_jd_dc(const JFile *__restrict__ files, int16_t *__restrict__ coef) {
    const JFile f = files[blockIdx.y];
    const int c = blockIdx.x;
    if (c >= f.nc) return;
    const int ysub = f.nc == 1 ? 1 : f.hs * f.vs;
    const int nbc = c == 0 ? ysub : 1, first = c == 0 ? 0 : ysub + c - 1;
    dc_predict(coef + f.blk0 * 64, f.mx * f.my * nbc, 0,
               [&](int k) { const int m = k / nbc, sb = k - m * nbc; return ((int64_t)m * f.bpm + first + sb) * 64; },
               [&](int k) { const int m = k / nbc; return f.ri > 0 && k - m * nbc == 0 && m % f.ri == 0; });
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
    const Subseq sub = subseq_regions(S, p);
    int *err = (int *)(S + p.o_err);
    int16_t *coef = (int16_t *)(S + p.o_coef);
    uint8_t *planes = (uint8_t *)(S + p.o_planes);
    // the descriptors live in p until this call returns, and it returns only after the stream has drained (below)
    CSM_HIP(hipMemcpyAsync(files, p.files.data(), (size_t)n * sizeof(JFile), hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemsetAsync(sub.flag, 0, (size_t)(p.o_coef - p.o_flag) + (size_t)csm::align16(p.blocks * 128), st));   // flag, err, coefficients
    int passes = 0;
    int rc = subseq_decode<Baseline>(blob, {files}, n, p.max_wg, p.nsub, sub, coef, err, passes, st); if (rc) return rc;
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
