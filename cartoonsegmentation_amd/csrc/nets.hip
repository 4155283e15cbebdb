// nets.hip -- layer-program executor for the dense nets of the hot path (ISNet refine, LeReS depth,
// RTMDet-Ins) on gfx950.  C ABI: csm_run_program (include/csm355.h).
//
// Design (CDNA4-first, not a cuDNN call sequence):
//   * activations NHWC fp32; a tensor view = (base, channels, channel pitch) so torch.cat is free;
//   * every dense / grouped convolution is ONE implicit-GEMM kernel on the exact-fp32 matrix pipe
//     (v_mfma_f32_32x32x2_f32, 157 TF/s peak): M = output pixels, N = output channels,
//     K = taps x input channels.  256-thread blocks = 4 waves in a WM x WN grid, each wave owns
//     32 x (32*TN) outputs.  K is consumed in chunks of 32 channels of one tap: the A tile
//     (BM pixels x 128 B, fully coalesced because NHWC keeps a pixel's channels contiguous) and the
//     pre-packed weight tile (BN x 128 B) are register-staged into LDS (row pitch 36 floats =>
//     conflict-free ds_read_b128) and double buffered, one barrier per chunk.
//   * global loads run two K-chunks ahead of the MFMAs in two register sets; they are unconditional with a fixed
//     count per step so that hipcc emits counted s_waitcnt vmcnt(N) instead of draining the queue.
//   * folded-BN bias initialises the accumulator; activation / residual are fused in the epilogue.
//   * grouped 3x3 (ResNeXt, 32 groups) runs on the same kernel as block-diagonal 32-channel
//     super-groups (zero-padded weights): fmaf(x, 0, acc) is exact, so numerics are unchanged.
//   * blockIdx -> tile mapping is XCD-aware: the 8 XCDs each get a contiguous range of M tiles so
//     that the 3x3 halo re-reads of neighbouring tiles hit the same 4 MiB L2.
// Numerical contract: see include/csm355.h (one fmaf chain per output, fixed K order).
//
// This file is the host side: the executor (run_ops), the table of tile configurations, the tile autotuner and its cache.  The kernels
// live in conv_mfma.hip (k_conv_mfma), conv_dma.hip (k_conv_dma, k_conv_dma_p), conv_patch.hip (k_conv_patch, k_conv_patch_p, k_conv_ws)
// and netops.hip (stem / narrow convolutions and every layer kernel that is not an implicit GEMM); csm_convcfg.h is what they share.
#include "csm_common.h"
#include "csm_convcfg.h"
#include "csm_tokens.h"
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>
#include <algorithm>
#include <utility>

using namespace csmconv;

int csmconv::g_ngroup_enable = 1;

// ---- the table of tile configurations: the rows of the family files, indexed by id ----------------------------------------------
// A missing or doubly defined id would send a tuned layer to the wrong kernel: checked once, at first use, and fatal.
static const ConvCfg &cfg_row(int id) {
    static const ConvCfg *table[CFG_COUNT];
    static const bool checked = [] {
        for (const std::span<const ConvCfg> rows : {conv_cfgs_mfma(), conv_cfgs_dma(), conv_cfgs_patch(), conv_cfgs_narrow()})
            for (const ConvCfg &r : rows) {
                if (r.id < 0 || r.id >= CFG_COUNT || table[r.id]) { fprintf(stderr, "csm355: conv tile configuration %d (%s) is out of range or defined twice\n", r.id, r.name); abort(); }
                table[r.id] = &r;
            }
        for (int id = 0; id < CFG_COUNT; ++id)
            if (!table[id]) { fprintf(stderr, "csm355: conv tile configuration %d has no table row\n", id); abort(); }
        return true;
    }();
    (void)checked;
    return *table[id];
}

// The candidates csm_conv_autotune times, in this order (the _s3 / _s4 tiles measured slower everywhere and the two alias ids are not timed)
static const int kTuneOrder[] = {CFG_64x64, CFG_128x32, CFG_64x16, CFG_D64x64, CFG_D128x64, CFG_D64x128, CFG_D128x128,
                                 CFG_D128x128_8w, CFG_D256x128_8w, CFG_D128x32, CFG_NARROW, CFG_D96x128, CFG_D160x128,
                                 CFG_D224x128, CFG_D192x128, CFG_P64x64, CFG_P128x64, CFG_P64x128, CFG_P128x128, CFG_P256x128,
                                 CFG_P128x32, CFG_P64x64_w8, CFG_P128x128_w8, CFG_P128x32_w8, CFG_P128x128_8w,
                                 CFG_Q64x64, CFG_Q128x64, CFG_Q64x128, CFG_Q128x128_8w, CFG_Q128x32,
                                 CFG_R128x32, CFG_R64x64, CFG_R128x64, CFG_R128x128_8w, CFG_R64x128, CFG_R128x128_8w_o4,
                                 CFG_W256x32, CFG_W256x64};

// ---- tile selection ---------------------------------------------------------------------------------------
// Measured on the three nets (tools/conv_bench.py --sweep, profiles/): occupancy beats register-tile reuse in this
// two-stage pipeline, so the default is the 64x64 tile (4 blocks = 16 waves per CU); narrow outputs get narrow tiles.
static int g_force_cfg = -1;
static int g_force_serial = -1;    // tests: -1 = rule / tuned, 0 = parallel split-K, 1 = serial split-K
static int g_tune_split = 1;       // tuner: consider mixed-tile launches (csm_debug_conv_tuner_options)
static int g_dbg = 0;
constexpr int kTileSerial = 64;
constexpr int kTileSplit = 128;    // csm_op.tile bit 7: mixed-tile launch (big tiles for whole rounds + 64 x 64 tiles for the rest)

static void read_force_env() {
    static bool env_read = false;
    if (env_read) return;      // tuning aid: CSM_FORCE_CONV_CFG=<n> forces one tile configuration for every eligible conv
    env_read = true;
    const char *e = getenv("CSM_FORCE_CONV_CFG");
    if (e && *e) g_force_cfg = atoi(e);
}

// Default rule when an op carries no tuned tile (csm_op.tile == 0): the LDS-DMA kernel with the 64x64 tile wins or ties on
// every layer of the three nets at batch 1 (profiles/r01_conv_sweep.txt); narrow outputs get narrow tiles.
static int choose_cfg(const ConvArgs &a, int N) {
    read_force_env();
    if (g_force_cfg >= 0 && g_force_cfg < CFG_COUNT) return g_force_cfg;
    if (N <= 16) return CFG_64x16;      // (k_conv_narrow is an autotune candidate only: it wins on some cout = 1 layers, loses on others)
    if (N <= 32) return dma_eligible(a) ? CFG_D128x32 : CFG_128x32;
    return CFG_D64x64;
}

// What is launched for a layer whose tuned / forced / default configuration is `cfg`: a family that cannot run the layer hands it to the
// nearest one that can.  Pure: depends on the row's family and the argument block only.
static int resolve_cfg(int cfg, const ConvArgs &a) {
    if (cfg_row(cfg).family == FAM_WS && !(patch_eligible(a) && ws_fits(a, cfg_row(cfg).bn))) cfg = CFG_R64x64;
    if (fam_needs_patch(cfg_row(cfg).family) && !patch_eligible(a)) cfg = CFG_D64x64;
    if (cfg_row(cfg).family == FAM_NARROW && !narrow_eligible(a)) cfg = CFG_64x16;
    if (fam_uses_dma(cfg_row(cfg).family) && !dma_eligible(a)) cfg = a.cout_g <= 16 ? CFG_64x16 : (a.cout_g <= 32 ? CFG_128x32 : CFG_64x64);
    return cfg;
}

// The argument block of a CONV op, but for the split-K scratch (ConvArgs::partial) and the launch-form fields (serial, split)
static ConvArgs conv_args(const csm_op &op, const View &in, const View &out, const View &in1, const float *weights) {
    ConvArgs a{};
    a.in = in; a.out = out; a.res = in1;
    a.w = weights + op.w_off; a.bias = op.b_off >= 0 ? weights + op.b_off : nullptr;
    a.slope = op.aux_off >= 0 ? weights + op.aux_off : nullptr;
    a.kh = op.kh; a.kw = op.kw; a.stride = op.stride; a.pad = op.pad; a.dil = op.dil;
    a.groups = op.groups; a.cin_g = op.cin_g; a.cout_g = op.cout_g; a.npad = (op.cout_g + 31) / 32 * 32;
    a.act = op.act; a.res_mode = op.in1 >= 0 ? op.res_mode : 0;
    a.M = out.n * out.h * out.w; a.ncb = (op.cin_g + 31) / 32;
    set_fast_div((unsigned)(out.h * out.w), a.dv_hw_mul, a.dv_hw_shr); set_fast_div((unsigned)out.w, a.dv_w_mul, a.dv_w_shr);
    a.ksplit = op.ksplit > 1 ? op.ksplit : 1; a.partial = nullptr;
    a.dbg = g_dbg;
    return a;
}

static View view_at(float *base, const csm_tensor_desc &t) { return View{base + t.offset, t.n, t.h, t.w, t.c, t.ld}; }

static int make_view(const csm_tensor_desc *tensors, int n_tensors, int id, float *workspace, void *const *ext,
                     int n_ext, View &v) {
    if (id < 0 || id >= n_tensors) { csm::set_error("tensor id %d out of range", id); return CSM_ERR_ARG; }
    const csm_tensor_desc &t = tensors[id];
    float *base;
    if (t.ext >= 0) {
        if (t.ext >= n_ext || !ext[t.ext]) { csm::set_error("ext slot %d missing", t.ext); return CSM_ERR_ARG; }
        base = (float *)ext[t.ext];
    } else base = workspace;
    v = view_at(base, t);
    return CSM_OK;
}

static int run_ops(const csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors, const float *weights,
                   float *workspace, void *const *ext, int n_ext, hipStream_t st, hipEvent_t *ev) {
    if (ev) CSM_HIP(hipEventRecord(ev[0], st));
    for (int i = 0; i < n_ops; ++i) {
        const csm_op &op = ops[i];
        View in{}, in1{}, out{};
        int rc = make_view(tensors, n_tensors, op.in0, workspace, ext, n_ext, in); if (rc) return rc;
        rc = make_view(tensors, n_tensors, op.out, workspace, ext, n_ext, out); if (rc) return rc;
        if (op.in1 >= 0) { rc = make_view(tensors, n_tensors, op.in1, workspace, ext, n_ext, in1); if (rc) return rc; }
        switch (op.kind) {
            case CSM_OP_CONV: {
                ConvArgs a = conv_args(op, in, out, in1, weights);
                if (a.ksplit > 1) {
                    View sc{};
                    if (op.groups != 1) { csm::set_error("op %d: ksplit needs groups == 1", i); return CSM_ERR_ARG; }
                    rc = make_view(tensors, n_tensors, op.scratch, workspace, ext, n_ext, sc); if (rc) return rc;
                    a.partial = sc.p;
                }
                if ((in.ld & 3) || (op.cin_g & 3) || (((uintptr_t)in.p) & 15)) {
                    csm::set_error("op %d: conv input must be 16-byte aligned with channels %% 4 == 0", i); return CSM_ERR_ARG;
                }
                if (op.flags & CSM_CONV_FLAG_WINOGRAD) {      // Winograd F(2x2, 3x3): its own arithmetic (part of the lowering's contract), its own kernel
                    if (!wino_eligible(a)) { csm::set_error("op %d: Winograd flag on an ineligible convolution (3x3 / stride 1 / pad 1 / dense / cin %% 32 / cout %% 64 / ksplit 1)", i); return CSM_ERR_ARG; }
                    rc = launch_conv_wino(a, st);
                    if (rc) return rc;
                    break;
                }
                if (op.flags & CSM_CONV_FLAG_WINOGRAD4) {     // Winograd F(4x4, 3x3): the same layer class, 36 instead of 64 products per 4x4 outputs (wino4.hip)
                    if (op.scratch >= 0) {                    // optional scratch of the row-split execution forms (small launches): speed only
                        View sc{};
                        rc = make_view(tensors, n_tensors, op.scratch, workspace, ext, n_ext, sc); if (rc) return rc;
                        if ((int64_t)sc.n * sc.h * sc.w * sc.c < wino4_scratch_floats(out.n, out.h, out.w, op.cout_g) || sc.ld != sc.c || (((uintptr_t)sc.p) & 15)) {
                            csm::set_error("op %d: Winograd F(4x4) scratch tensor too small or not contiguous", i); return CSM_ERR_ARG;
                        }
                        a.partial = sc.p;
                    }
                    if (!wino4_eligible(a)) { csm::set_error("op %d: Winograd F(4x4) flag on an ineligible convolution (3x3 / stride 1 / pad 1 / dense / cin %% 32 / cout %% 64 / ksplit 1)", i); return CSM_ERR_ARG; }
                    rc = launch_conv_wino4(a, st);
                    if (rc) return rc;
                    break;
                }
                if (op.flags & CSM_CONV_FLAG_GROUPED) {       // narrow groups on the vector pipe: the direct chain, its own weight image (grouped.hip)
                    if (!grouped_eligible(a)) { csm::set_error("op %d: grouped-conv flag on an ineligible convolution (3x3 / stride 1 / pad 1 / cin_g == cout_g in {8, 16, 32} / channels %% 32 / ksplit 1)", i); return CSM_ERR_ARG; }
                    rc = launch_conv_grouped(a, st);
                    if (rc) return rc;
                    break;
                }
                if (op.flags & 2) {      // stem: (tap, channel)-packed K (weights packed by the host for exactly this kernel)
                    if (op.groups != 1 || op.cin_g != 4 || a.ksplit != 1) { csm::set_error("op %d: stem flag needs groups 1, cin 4, ksplit 1", i); return CSM_ERR_ARG; }
                    rc = launch_conv_stem(a, st);
                    if (rc) return rc;
                    break;
                }
                // csm_op.tile = 1 + configuration (+ kTileSerial: split-K runs walked by one block).  Untuned ops: serial once the
                // batch supplies enough output tiles by itself (speed only: both executions give the same bits)
                const int tcfg = op.tile & (kTileSerial - 1);
                a.split = (op.tile & kTileSplit) != 0 && g_force_cfg < 0;
                const bool tuned = tcfg > 0 && tcfg <= CFG_COUNT && g_force_cfg < 0;
                a.serial = a.ksplit > 1 && (g_force_serial >= 0 ? g_force_serial != 0 : tuned ? (op.tile & kTileSerial) != 0
                                            : (int64_t)((a.M + 63) / 64) * ((op.cout_g + 63) / 64) >= 512);
                int cfg = tuned ? tcfg - 1 : choose_cfg(a, op.cout_g);
                rc = cfg_row(resolve_cfg(cfg, a)).launch(a, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_LAYERNORM: {
                if (op.w_off < 0 || op.b_off < 0 || op.aux_off < 0 || in.c != out.c) { csm::set_error("op %d: layernorm operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_layernorm(in.p, in.ld, out.p, out.ld, (int64_t)in.n * in.h * in.w, in.c, weights + op.w_off, weights + op.b_off,
                                           weights + op.aux_off /* {eps}, read on the device */, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_ATTENTION: {
                const int heads = op.groups, d = op.cin_g;
                if (heads < 1 || in.c != 3 * heads * d || out.c != heads * d || in.w != 1 || out.h != in.h) { csm::set_error("op %d: attention operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_attention(in.p, in.ld, out.p, out.ld, in.n, in.h, heads, d, op.aux_off >= 0 ? weights + op.aux_off : nullptr, op.kh, op.kw, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_ATTENTION_RELPOS: {
                const int heads = op.groups, d = op.cin_g;
                if (heads < 1 || in.c != 3 * heads * d || out.c != heads * d || out.n != in.n || out.h * out.w != in.h * in.w || op.aux_off < 0) { csm::set_error("op %d: attention_relpos operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_attention_relpos(in.p, in.ld, out.p, out.ld, in.n, in.h * in.w, heads, d, weights + op.aux_off, op.kh, op.kw, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_CROSS_ATTENTION: {
                const int heads = op.groups, d = op.cin_g;
                if (heads < 1 || op.in1 < 0 || in.c != heads * d || in1.c != 2 * heads * d || out.c != heads * d || in1.n != in.n || out.n != in.n || out.h * out.w != in.h * in.w) { csm::set_error("op %d: cross_attention operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_cross_attention(in.p, in.ld, in1.p, in1.ld, out.p, out.ld, in.n, in.h * in.w, in1.h * in1.w, heads, d, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_CHANNEL_DOT: {
                if (op.in1 < 0 || in1.c != in.c || in1.n != in.n || in1.h * in1.w != 1 || out.n != in.n || out.h != in.h || out.w != in.w) { csm::set_error("op %d: channel_dot operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_channel_dot(in.p, in.ld, in1.p, in1.ld, out.p, out.ld, in.n, (int64_t)in.h * in.w, in.c, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_TOKENS: {
                const int mode = op.flags;
                if (mode == 3 || mode == 4) {          // window partition / un-partition (sam.hip); kh = window size
                    const View &map = mode == 3 ? in : out, &win = mode == 3 ? out : in;
                    const int ws = op.kh, wy = ws > 0 ? (map.h + ws - 1) / ws : 0, wx = ws > 0 ? (map.w + ws - 1) / ws : 0;
                    if (ws < 1 || in.c != out.c || win.n != map.n * wy * wx || win.h * win.w != ws * ws ||
                        (mode == 4 && op.in1 >= 0 && (in1.n != out.n || in1.h != out.h || in1.w != out.w || in1.c != out.c)) || (mode == 3 && op.in1 >= 0)) {
                        csm::set_error("op %d: tokens operands (mode %d)", i, mode); return CSM_ERR_ARG;
                    }
                    rc = csm::launch_window(mode == 4, in.p, in.ld, op.in1 >= 0 ? in1.p : nullptr, op.in1 >= 0 ? in1.ld : 0, out.p, out.ld, map.n, map.h, map.w, ws, in.c, st);
                    if (rc) return rc;
                    break;
                }
                if (mode == 5 || mode == 6) {          // broadcast add (sam.hip)
                    const int64_t np = (int64_t)out.h * out.w;
                    if (in.c != out.c || (int64_t)in.h * in.w != np || (op.in1 >= 0 && (in1.c != out.c || (int64_t)in1.h * in1.w != np)) || (mode == 6 && op.aux_off < 0)) {
                        csm::set_error("op %d: tokens operands (mode %d)", i, mode); return CSM_ERR_ARG;
                    }
                    rc = csm::launch_bcast_add(in.p, in.ld, in.n, op.in1 >= 0 ? in1.p : nullptr, op.in1 >= 0 ? in1.ld : 0, op.in1 >= 0 ? in1.n : 1, out.p, out.ld, out.n, np,
                                               out.c, op.aux_off >= 0 ? weights + op.aux_off : nullptr, mode == 6, st);
                    if (rc) return rc;
                    break;
                }
                const int np = mode == 0 ? in.h * in.w : out.h * out.w;
                const bool ok = mode == 0 ? (out.h == np + 1 && out.w == 1 && out.c == in.c && op.aux_off >= 0)
                                          : (in.h == np + 1 && in.w == 1 && out.c == (mode == 1 ? 2 : 1) * in.c);
                if (!ok || in.n != out.n) { csm::set_error("op %d: tokens operands (mode %d)", i, mode); return CSM_ERR_ARG; }
                rc = csm::launch_tokens(mode, in.p, in.ld, out.p, out.ld, in.n, np, in.c, op.aux_off >= 0 ? weights + op.aux_off : nullptr, st);
                if (rc) return rc;
                break;
            }
            case CSM_OP_DEPTH_TO_SPACE: {
                const int k = op.stride;
                if (k < 1 || out.h != in.h * k || out.w != in.w * k || in.c != k * k * out.c) { csm::set_error("op %d: depth_to_space operands", i); return CSM_ERR_ARG; }
                rc = csm::launch_depth_to_space(in.p, in.ld, out.p, out.ld, in.n, in.h, in.w, k, out.c, st);
                if (rc) return rc;
                break;
            }
            default:                                  // every other layer kernel (netops.hip); an unknown kind is its error
                rc = launch_netop(op, i, in, in1, out, weights, st);
                if (rc) return rc;
                break;
        }
        rc = csm::check_launch("program op");
        if (rc) { csm::set_error("op %d (kind %d) launch failed", i, op.kind); return rc; }
        if (ev) CSM_HIP(hipEventRecord(ev[i + 1], st));
    }
    return CSM_OK;
}

extern "C" int csm_run_program(const csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors,
                               const float *weights, float *workspace, void *const *ext, int n_ext, void *stream) {
    CSM_REQUIRE(ops && tensors && n_ops >= 0 && n_tensors > 0);
    return run_ops(ops, n_ops, tensors, n_tensors, weights, workspace, ext, n_ext, (hipStream_t)stream, nullptr);
}

// HIP events released on every exit path (the CSM_HIP early returns inside the timing loops used to leak them)
struct EventSet {
    std::vector<hipEvent_t> ev;
    bool ok = true;
    explicit EventSet(size_t n) {
        ev.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            hipEvent_t e;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) { csm::set_error("hipEventCreate: %s", hipGetErrorString(r)); ok = false; return; }
            ev.push_back(e);
        }
    }
    ~EventSet() { for (auto e : ev) (void)hipEventDestroy(e); }
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
};

// Same as csm_run_program, but brackets every op with HIP events on `stream`, synchronises the stream and returns
// the per-op durations (ms) in op_ms[n_ops].  Measurement aid for bench.py's roofline (not graph-capturable).
extern "C" int csm_run_program_profile(const csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors,
                                       const float *weights, float *workspace, void *const *ext, int n_ext, void *stream,
                                       float *op_ms) {
    CSM_REQUIRE(ops && tensors && op_ms && n_ops >= 0 && n_tensors > 0);
    hipStream_t st = (hipStream_t)stream;
    EventSet evs(n_ops + 1);
    if (!evs.ok) return CSM_ERR_HIP;
    int rc = run_ops(ops, n_ops, tensors, n_tensors, weights, workspace, ext, n_ext, st, evs.ev.data());
    if (rc == CSM_OK) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { csm::set_error("profile sync: %s", hipGetErrorString(e)); rc = CSM_ERR_HIP; }
        else for (int i = 0; i < n_ops; ++i) (void)hipEventElapsedTime(&op_ms[i], evs.ev[i], evs.ev[i + 1]);
    }
    return rc;
}

// layer signature -> tuned tile; process-global, shared by every program and (through the mutex) by host threads that drive
// different GPUs / streams
static std::map<std::array<int, 16>, int> g_tile_cache;
static std::mutex g_tile_mutex;

extern "C" int csm_conv_autotune(csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors, const float *weights,
                                 float *workspace, void *const *ext, int n_ext, void *stream, int reps) {
    CSM_REQUIRE(ops && tensors && n_ops >= 0 && n_tensors > 0);
    read_force_env();
    if (g_force_cfg >= 0) return 0;
    if (reps < 1) reps = 3;
    hipStream_t st = (hipStream_t)stream;
    EventSet evs(2);
    if (!evs.ok) return -CSM_ERR_HIP;
    hipEvent_t *ev = evs.ev.data();
    int tuned = 0, rc = CSM_OK;
    for (int i = 0; i < n_ops && rc == CSM_OK; ++i) {
        csm_op &op = ops[i];
        if (op.kind != CSM_OP_CONV || (op.flags & (CSM_CONV_FLAG_STEM | CSM_CONV_FLAG_WINOGRAD | CSM_CONV_FLAG_WINOGRAD4 | CSM_CONV_FLAG_GROUPED))) continue;          // stems, Winograd and vector-pipe grouped layers have one dedicated kernel
        const int npad = (op.cout_g + 31) / 32 * 32;
        // identical layers (same shapes / strides / split) share one measurement, also across programs
        View vin{}, vout{};
        rc = make_view(tensors, n_tensors, op.in0, workspace, ext, n_ext, vin); if (rc) break;
        rc = make_view(tensors, n_tensors, op.out, workspace, ext, n_ext, vout); if (rc) break;
        const std::array<int, 16> key = {vin.n, vin.h, vin.w, vin.ld, vout.h, vout.w, vout.ld, op.kh, op.kw, op.stride, op.dil,
                                         op.groups, op.cin_g, op.cout_g, op.ksplit, op.pad};
        {
            std::lock_guard<std::mutex> lk(g_tile_mutex);
            auto hit = g_tile_cache.find(key);
            if (hit != g_tile_cache.end()) { op.tile = hit->second; ++tuned; continue; }
        }
        // one timed run of `op` with the tile in op.tile: min over `n` repetitions after one warm-up (which also sets the LDS attribute)
        auto time_tile = [&](int n, float &tmin) -> int {
            tmin = 1e30f;
            for (int r = 0; r <= n; ++r) {
                hipError_t he = hipEventRecord(ev[0], st);
                int rc2 = CSM_OK;
                if (he == hipSuccess) rc2 = run_ops(&op, 1, tensors, n_tensors, weights, workspace, ext, n_ext, st, nullptr);
                if (rc2) return rc2;
                if (he == hipSuccess) he = hipEventRecord(ev[1], st);
                if (he == hipSuccess) he = hipEventSynchronize(ev[1]);
                if (he != hipSuccess) { csm::set_error("conv_autotune timing: %s", hipGetErrorString(he)); return CSM_ERR_HIP; }
                float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
                if (r > 0 && ms < tmin) tmin = ms;
            }
            return CSM_OK;
        };
        float best = 1e30f; int best_cfg = -1;
        std::vector<std::pair<float, int>> timed;
        // warm-up: the first candidates of a layer used to be timed on a GPU that had just idled (clock ramp, cold L2 / Infinity Cache) and
        // measured 3-5 % slower than the same kernel a few milliseconds later -- enough to lose against a slower tile timed afterwards
        {
            op.tile = 0;
            float tw = 0.f;
            for (int w = 0; w < 4 && tw < 4.0f && rc == CSM_OK; ++w) { float t1; rc = time_tile(4, t1); tw += 5.0f * t1; }
            if (rc) break;
        }
        const bool is_patch_layer = op.kh == 3 && op.kw == 3 && op.stride == 1 && op.dil == 1;
        for (const int cand : kTuneOrder) {
            const int fam = cfg_row(cand).family, bn = cfg_row(cand).bn;
            if (bn >= 2 * npad && bn > 32) continue;      // tile much wider than the output: never wins
            if (fam_needs_patch(fam) && !is_patch_layer) continue;
            if (fam == FAM_WS &&
                (op.ksplit > 1 || (op.cin_g & 31) || (size_t)kWsPatchBytes + (size_t)9 * ((op.cin_g + 31) / 32) * bn * 128 > (size_t)160 * 1024 ||
                 op.groups * ((op.cout_g + bn - 1) / bn) > 64)) continue;
            if (fam == FAM_NARROW && (op.cout_g > 4 || op.groups != 1 || op.ksplit > 1)) continue;
            if (bn == 16 && op.cout_g > 16) continue;
            if (bn == 32 && op.cout_g > 64 && (op.cout_g % 64) != 32) continue;   // (96, 160 ... outputs: 32-wide tiles waste no MFMA columns)
            for (int ser = 0; ser <= (op.ksplit > 1 ? 1 : 0) && rc == CSM_OK; ++ser) {     // split-K layers: both executions
                if (fam_persistent(fam) && op.ksplit > 1 && !ser) continue;                    // (the persistent kernels walk split K serially only)
                const bool dfam = fam == FAM_DMA && cand != CFG_D64x64;                        // (the mixed launch's small tile IS D64x64)
                for (int sp = 0; sp <= ((dfam && g_tune_split && (op.ksplit <= 1 || ser)) ? 1 : 0) && rc == CSM_OK; ++sp) {   // mixed-tile launch
                    op.tile = cand + 1 + (ser ? kTileSerial : 0) + (sp ? kTileSplit : 0);
                    float tmin;
                    rc = time_tile(reps, tmin);
                    if (rc) break;
                    timed.emplace_back(tmin, op.tile - 1);
                }
            }
            if (rc) break;
        }
        if (rc) break;
        // the three fastest are within a few percent of each other on many layers and one sample of three is noisy: time them again
        // (twice the repetitions, minimum of both rounds) before choosing
        std::sort(timed.begin(), timed.end());
        static const int retime = getenv("CSM_TUNE_RETIME") ? atoi(getenv("CSM_TUNE_RETIME")) : 1;
        if (!retime && !timed.empty()) { best = timed[0].first; best_cfg = timed[0].second; }
        // the finalists (five fastest) are timed again in three INTERLEAVED rounds (a b c d e a b c d e ...), so that a drift of the clock
        // or of the cache state hits all of them alike; the minimum over all of a candidate's samples decides
        const size_t nfin = std::min<size_t>(timed.size(), 5);
        for (int round = 0; retime && round < 3 && rc == CSM_OK; ++round)
            for (size_t k = 0; k < nfin && rc == CSM_OK; ++k) {
                op.tile = timed[k].second + 1;
                float tmin;
                rc = time_tile(reps, tmin);
                if (rc) break;
                if (tmin < timed[k].first) timed[k].first = tmin;
            }
        for (size_t k = 0; retime && k < nfin; ++k)
            if (timed[k].first < best) { best = timed[k].first; best_cfg = timed[k].second; }
        if (rc) break;
        op.tile = best_cfg >= 0 ? best_cfg + 1 : 0;
        { std::lock_guard<std::mutex> lk(g_tile_mutex); g_tile_cache[key] = op.tile; }
        ++tuned;
    }
    return rc == CSM_OK ? tuned : -rc;
}

// Tuned tiles as a text file (one line per layer signature: 16 integers + tile) so that a later process can skip the
// measurement: load merges into the in-memory table that csm_conv_autotune consults first.
extern "C" int csm_conv_tile_cache_save(const char *path) {
    CSM_REQUIRE(path);
    FILE *f = fopen(path, "w");
    if (!f) { csm::set_error("cannot write %s", path); return CSM_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g_tile_mutex);
    for (const auto &kv : g_tile_cache) {
        for (int v : kv.first) fprintf(f, "%d ", v);
        fprintf(f, "%d\n", kv.second);
    }
    fclose(f);
    return CSM_OK;
}

extern "C" int csm_conv_tile_cache_load(const char *path) {
    CSM_REQUIRE(path);
    FILE *f = fopen(path, "r");
    if (!f) return 0;                       // no file yet: nothing cached
    int n = 0;
    for (;;) {
        std::array<int, 16> key; int tile = 0; bool ok = true;
        for (int &v : key) ok = ok && fscanf(f, "%d", &v) == 1;
        if (!ok || fscanf(f, "%d", &tile) != 1) break;
        if (tile >= 0 && (tile & (kTileSerial - 1)) <= CFG_COUNT && tile < 2 * kTileSplit) { std::lock_guard<std::mutex> lk(g_tile_mutex); g_tile_cache[key] = tile; ++n; }
    }
    fclose(f);
    return n;
}

// debug / tuning knob: low byte = forced conv tile configuration (-1 = built-in rule), bits 8.. = phase-ablation flags
// (ConvArgs::dbg).  Not part of the stable ABI.
extern "C" int csm_debug_force_conv_cfg(int cfg) {
    if (cfg >= 0) { g_force_cfg = cfg & 0xff; g_dbg = cfg >> 8; } else { g_force_cfg = -1; g_dbg = 0; }
    return CSM_OK;
}

// measurement aid: which launch forms the autotuner may choose from (bit 0: mixed-tile launches); default all
extern "C" int csm_debug_conv_tuner_options(int options) {
    g_tune_split = options & 1;
    g_ngroup_enable = (options & 2) ? 0 : 1;          // bit 1: N-grouped tile order off
    return CSM_OK;
}

// tests: force how split-K layers are executed (-1 = tuned / rule, 0 = S blocks + reduce kernel, 1 = one block walks the runs)
extern "C" int csm_debug_force_splitk_serial(int mode) {
    g_force_serial = mode < 0 ? -1 : (mode ? 1 : 0);
    return CSM_OK;
}

// ---- the configuration table for tests and tools (host only; not part of the stable ABI) ----------------------------------------
extern "C" int csm_debug_conv_cfg_count(void) { return CFG_COUNT; }

extern "C" int csm_debug_conv_cfg_info(int cfg, csm_conv_cfg_desc *info) {
    CSM_REQUIRE(info);
    if (cfg < 0 || cfg >= CFG_COUNT) { csm::set_error("conv tile configuration %d out of range (0 .. %d)", cfg, CFG_COUNT - 1); return CSM_ERR_ARG; }
    static const char *const fam_names[FAM_COUNT] = {"MFMA", "DMA", "PATCH", "DMA_P", "PATCH_P", "WS", "NARROW"};
    const ConvCfg &r = cfg_row(cfg);
    info->id = r.id; info->bn = r.bn; info->name = r.name; info->family = fam_names[r.family];
    info->tune_pos = -1;
    for (size_t k = 0; k < sizeof(kTuneOrder) / sizeof(int); ++k)
        if (kTuneOrder[k] == cfg) info->tune_pos = (int)k;
    return CSM_OK;
}

// The id run_ops would launch for `op` with configuration `cfg` on these two tensors; the views sit at their offsets from a null base
// (weights too), so alignment follows the offsets alone.  Returns the id, or a negative status.
extern "C" int csm_debug_conv_resolve_cfg(int cfg, const csm_op *op, const csm_tensor_desc *in_desc, const csm_tensor_desc *out_desc) {
    if (!op || !in_desc || !out_desc || cfg < 0 || cfg >= CFG_COUNT) { csm::set_error("conv_resolve_cfg: bad argument"); return -CSM_ERR_ARG; }
    return resolve_cfg(cfg, conv_args(*op, view_at(nullptr, *in_desc), view_at(nullptr, *out_desc), View{}, nullptr));
}
