/*
 * csm355.h -- C ABI of libcsm355.so: the MI355X (gfx950) hot path of CartoonSegmentation.
 *
 * Drop-in boundary: the reference has no plugin ABI for this path; its
 * operator boundary is utils/cupy_utils.py::launch_kernel(name, src)(grid, block,
 * args=[int32 n, raw device pointers...]) (utils/cupy_utils.py:7-13) -- caller-owned,
 * pre-allocated torch buffers, raw pointers, nothing returned.  This header keeps that
 * convention: plain pointers + sizes, caller-allocated outputs, an explicit HIP stream,
 * int status (0 = ok; message via csm_last_error()).  No torch types.
 *
 * All tensors are contiguous fp32 unless stated; layouts are the reference's
 * (NCHW / [B,C,N]).  Every function is asynchronous on `stream` (a hipStream_t cast
 * to void*; NULL = the null stream) and re-entrant per stream.
 *
 * Reference citations are relative to /root/reference.
 */
#ifndef CSM355_H
#define CSM355_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CSM_OK 0
#define CSM_ERR_ARG 1
#define CSM_ERR_HIP 2
#define CSM_ERR_NAN 3
#define CSM_ERR_DATA 4   /* corrupt input data (csm_jpeg_decode, csm_png_decode, csm_webp_decode) */

/* thread-local message of the last non-zero status */
const char *csm_last_error(void);
/* library/ABI version (major*1000 + minor) and build info string */
int csm_version(void);
const char *csm_build_info(void);

/* ------------------------------------------------------------------------------------
 * Ken Burns warp operators
 * ---------------------------------------------------------------------------------- */

/* kernel_pointrender_updateZee   anime_3dkenburns/models/utils.py:63-149
 * pts [B,3,N]; zee [B,1,H,W] must hold 1e6 on entry (models/utils.py:59). */
int csm_pointrender_update_zee(const float *pts, int B, int64_t N, int H, int W, double focal,
                               double baseline, float *zee, void *stream);

/* kernel_pointrender_updateDegrid   models/utils.py:152-212
 * Deterministic (Jacobi) form: reads zee_in, writes zee_out (must not alias). */
int csm_pointrender_degrid(const float *zee_in, float *zee_out, int B, int H, int W, void *stream);

/* kernel_pointrender_updateOutput   models/utils.py:215-313
 * data [B,C,N] WITHOUT the ones channel; accum [B,C+1,H,W] must be zero on entry;
 * channel C of accum receives the bilinear weight itself (the reference's appended
 * ones channel, models/utils.py:57). */
int csm_pointrender_update_output(const float *pts, const float *data, const float *zee, int B, int C,
                                  int64_t N, int H, int W, double focal, double baseline, float *accum,
                                  void *stream);

/* render_pointcloud   models/utils.py:56-315  (fill + 3 kernels + divide)
 * scratch: zee_scratch 2*B*H*W floats, accum_scratch B*(C+1)*H*W floats.
 * outputs: render [B,C,H,W], existing [B,1,H,W]. */
int csm_render_pointcloud(const float *pts, const float *data, int B, int C, int64_t N, int W, int H,
                          double focal, double baseline, float *zee_scratch, float *accum_scratch,
                          float *render, float *existing, void *stream);

/* The same operator for ONE cloud (B = 1) and any channel count on the destination-tile path (warptile.hip): binning, per-tile
 * z-buffer / degrid / z-test in LDS, the channels splatted in groups of 8 through 64-bit fixed-point LDS accumulators (|data| < 2^30):
 * deterministic sums, ~4x faster than the L2 float atomics at the 68 channels Inpaint.forward splats (pointcloud_inpainting.py:135).
 * scratch: csm_warp_tile_scratch_bytes(H, W, N) bytes (a csm_warp_frame_tiled scratch serves) whose first csm_warp_tile_header_bytes(H, W)
 * are zeroed once by the caller. */
int csm_render_pointcloud_tiled(const float *pts, const float *data, int C, int64_t N, int W, int H, double focal, double baseline,
                                void *scratch, float *render, float *existing, void *stream);

/* fill_disocclusion   anime_3dkenburns/common.py:145-248
 * in [B,C,H,W], depth [B,1,H,W] -> out [B,C,H,W] (out is fully written; no pre-clone needed).
 * scratch: csm_fill_disocclusion_scratch_bytes(B,H,W) bytes of device memory (hole list + valid map). */
size_t csm_fill_disocclusion_scratch_bytes(int B, int H, int W);
int csm_fill_disocclusion(const float *in, const float *depth, float *out, int B, int C, int H, int W,
                          void *scratch, void *stream);

/* spatial_filter(x,'laplacian')   models/utils.py:12-24 ; x,out [BC,H,W] */
int csm_spatial_filter_laplacian(const float *in, float *out, int BC, int H, int W, void *stream);

/* spatial_filter(x,'median-5')   models/utils.py:32-36 (reflect pad, lower median of 25) ; x,out [BC,H,W]
 * A window that contains a NaN yields NaN (torch.median's rule); the same holds for median-3. */
int csm_spatial_filter_median5(const float *in, float *out, int BC, int H, int W, void *stream);

/* spatial_filter(x,'median-3')   models/utils.py:26-30 (reflect pad 1, lower median of 9) ; x,out [BC,H,W] */
int csm_spatial_filter_median3(const float *in, float *out, int BC, int H, int W, void *stream);

/* depth_to_points   models/utils.py:43-50 ; depth [B,1,H,W] -> pts [B,3,H,W] */
int csm_depth_to_points(const float *depth, float *pts, int B, int H, int W, double focal, void *stream);

/* kenburns_effect.py:928-933 fused: normalised disparity [1,1,H,W] (already /max*baseline) ->
 * depth = (1/(disp+eps))*focal*baseline, valid, points (depth*valid), unaltered points.  disp_max -> ONE float in device
 * memory holding max(disparity) (a device pointer so the caller needs no host sync);
 * eps = 1e-5 at kenburns_effect.py:929, 1e-7 at :458 and pointcloud_inpainting.py:117. */
int csm_disparity_to_points(const float *disp, const float *disp_max, int H, int W, double focal, double baseline, float eps,
                            float *depth, float *valid, float *pts, float *unaltered, void *stream);

/* tensor part of process_shift   common.py:74-81 ; shift = float32(sx,sy,sz) */
int csm_process_shift(const float *pts, float *out, int B, int64_t N, float sx, float sy, float sz,
                      void *stream);

/* One output frame of KenBurnsPipeline.process_kenburns (kenburns_effect.py:1027-1040), fused:
 * process_shift -> render_pointcloud(cat[rgb, depth]) -> fill_disocclusion(render,
 * render[3]*(existing>0)) -> uint8 HWC frame.
 * pts [1,3,N], rgb [1,3,N], depth [1,1,N]; scratch >= csm_warp_frame_scratch_floats(H,W) floats.
 * outputs: render_filled [1,4,H,W] (may be NULL), frame_u8 [H,W,3]. */
size_t csm_warp_frame_scratch_floats(int H, int W);
int csm_warp_frame(const float *pts, const float *rgb, const float *depth, int64_t N, int H, int W,
                   double focal, double baseline, float sx, float sy, float sz, float *scratch,
                   float *render_filled, uint8_t *frame_u8, void *stream);

/* The same frame as csm_warp_frame with the splat done per destination tile in LDS (warptile.hip): points are binned by the
 * 32 x 16 tile(s) their footprint touches (integer atomics only), then one block per tile builds the z-buffer window, degrids,
 * z-tests, accumulates into 64-bit fixed-point LDS accumulators (integer atomics: order free, a frame is bit-reproducible),
 * normalises and writes the uint8 frame; holes are filled from row / column validity bitmaps.  Same decisions (z-buffer, coverage,
 * fill sources) as csm_warp_frame; colours within 2^-20 absolute of the exact sum that every fp32 summation order approximates
 * (the reference's own order is unspecified).
 * csm_warp_tile_supported(H, W): 1 when the frame has at most 8192 tiles (up to ~2048 x 2048); larger frames use csm_warp_frame.
 * scratch: csm_warp_tile_scratch_bytes(H, W, N) bytes, 16-B aligned; its first csm_warp_tile_header_bytes(H, W) bytes must be
 * ZERO before the first call (hipMemset once after allocation) -- every call leaves them re-armed for the next frame. */
size_t csm_warp_tile_scratch_bytes(int H, int W, int64_t N);
size_t csm_warp_tile_header_bytes(int H, int W);
int csm_warp_tile_supported(int H, int W);
int csm_warp_frame_tiled(const float *pts, const float *rgb, const float *depth, int64_t N, int H, int W, double focal,
                         double baseline, float sx, float sy, float sz, void *scratch, float *render_filled, uint8_t *frame_u8,
                         void *stream);

/* K frames of ONE cloud under K camera shifts (the frame loop of KenBurnsPipeline.process_kenburns, kenburns_effect.py:1027-1040) in one
 * asynchronous call on `stream`: the frames are dealt round-robin onto `lanes` (1..3) internal streams (lanes = 1: `stream` itself) with one scratch
 * each, forked from and joined to `stream` by events, so that frame k + 1's binning and frame k - 1's hole fill run under frame k's
 * render.  Every frame is bit-identical to csm_warp_frame_tiled with the same arguments.
 * shifts_host: K x (sx, sy, sz) HOST floats (read before the call returns); scratch: csm_warp_frames_scratch_bytes(H, W, N, lanes) device
 * bytes = `lanes` consecutive csm_warp_frame_tiled scratches (each rounded up to 256 B), every one with its header zeroed once by the
 * caller -- hipMemset the whole buffer once; frames_u8 [K][H][W][3]; render_filled NULL or [K][4][H][W]. */
size_t csm_warp_frames_scratch_bytes(int H, int W, int64_t N, int lanes);
int csm_warp_frames_tiled(const float *pts, const float *rgb, const float *depth, int64_t N, int H, int W, double focal, double baseline,
                          const float *shifts_host, int K, int lanes, void *scratch, float *render_filled, uint8_t *frames_u8, void *stream);

/* Coverage search of process_autozoom   anime_3dkenburns/common.py:86-142, batched.
 * For each of K candidate camera shifts (sx_k, sy_k, shift_z) -- the float32 tenShift of process_shift (common.py:74) --
 * counts[k] = number of pixels with tenExisting > 0 after process_shift + render_pointcloud of pts [1,3,N]
 * (the `(tenExisting > 0.0).float().sum()` of common.py:126), without rendering any colour: z-buffer, degrid (Jacobi form) and
 * the z-test only.  Candidates are processed `chunk` (<= csm_autozoom_max_chunk()) at a time, each with its own z-buffer plane.
 * shifts_xy: HOST pointer to K x {sx, sy}; counts: DEVICE int32 [K] (zeroed by the call; read them once after the stream
 * is synchronised); scratch: csm_autozoom_scratch_floats(H, W, chunk) device floats. */
int csm_autozoom_max_chunk(void);
size_t csm_autozoom_scratch_floats(int H, int W, int chunk);
int csm_autozoom_coverage(const float *pts, int64_t N, int H, int W, double focal, double baseline, const float *shifts_xy,
                          float shift_z, int K, int chunk, float *scratch, int *counts, void *stream);

/* The same counts through the BAND path (autozoom.hip): candidates are grouped by their y shift (host side, exact float
 * equality), the points of a group are binned once by destination row band, and one block per (band, group) evaluates all the
 * group's candidates with the band's z-buffer in LDS -- no per-candidate HBM planes.  Same arithmetic, same counts.
 * counts: DEVICE int32 [K]; overflow: DEVICE int32 [1], set non-zero when a band segment was too small for this cloud -- the
 * counts are then INVALID and the caller re-runs csm_autozoom_coverage (read it together with the counts, one transfer).
 * csm_autozoom_band_supported: 0 for frames too wide for the LDS band (then only csm_autozoom_coverage applies).
 * scratch: csm_autozoom_band_scratch_bytes(H, W, N) device bytes, 16-B aligned (no initialisation needed). */
int csm_autozoom_band_supported(int H, int W);
size_t csm_autozoom_band_scratch_bytes(int H, int W, int64_t N);
int csm_autozoom_coverage_bands(const float *pts, int64_t N, int H, int W, double focal, double baseline, const float *shifts_xy,
                                float shift_z, int K, void *scratch, int *counts, int *overflow, void *stream);

/* ------------------------------------------------------------------------------------
 * Dense networks: a flat "layer program" executed on one stream (no allocation, graph-capturable)
 *
 * The reference runs these nets through torch nn.Modules (cuDNN); the replacement boundary is the
 * module call: animeinsseg/models/animeseg_refine/isnet.py:578 (ISNetDIS.forward),
 * depth_modules/leres/leres/multi_depth_model_woauxi.py:30 (RelDepthModel), mmdet RTMDet
 * (call site animeinsseg/__init__.py:450).  The host (Python, cartoonsegmentation_amd/program.py)
 * lowers a net into csm_op records + one packed fp32 weight buffer (BN folded); this library
 * executes them with hand-written gfx950 kernels.  Activations are NHWC fp32 inside a caller-
 * provided workspace; a tensor may be a channel slice of a wider buffer (ld = channel pitch), which
 * is how torch.cat is realised without copies.
 *
 * Numerical contract (so the CPU oracle can be bit-exact): every convolution output is ONE fp32
 * fmaf chain  acc = bias; for each aligned block of 32 input channels (outer); for tap (kh,kw) row-major; for each
 * aligned sub-block of 8 channels, channel order 0,4,1,5,2,6,3,7 (the v_mfma_f32_32x32x2_f32 lane order):
 * acc = fmaf(x, w, acc)
 * -- or `ksplit` such chains over consecutive K runs, summed in order (see csm_op.ksplit; the host picks
 * ksplit > 1 for small feature maps so that all 256 CUs get work at batch 1).  ksplit follows the PER-SAMPLE shape only, so
 * a batch-n program computes, for every sample, the bits of the batch-1 program.  How the runs are executed (S blocks +
 * a reduce kernel, or one block that walks the runs and adds them in registers) is a speed choice with identical results.
 * Epilogue order: (+residual if res_mode==1) -> activation -> (+residual if res_mode==2).
 * SiLU/sigmoid use the polynomial expf documented in DESIGN.md.
 * ---------------------------------------------------------------------------------- */
enum csm_op_kind {
    CSM_OP_CONV = 1,        /* dense or grouped conv on fp32 MFMA (implicit GEMM) */
    CSM_OP_DWCONV = 2,      /* depthwise conv, direct */
    CSM_OP_MAXPOOL = 3,     /* p: k, stride, pad (ceil_mode is implied by the output size) */
    CSM_OP_BILINEAR = 4,    /* p[0]=align_corners; output size from the out tensor */
    CSM_OP_NEAREST = 5,     /* nearest upsample, integer factor from sizes */
    CSM_OP_ADD = 6,         /* out = act(in0 + in1) */
    CSM_OP_GAVGPOOL = 7,    /* global average pool -> [n,1,1,c] */
    CSM_OP_SCALE = 8,       /* out = in0 * in1[n,0,0,c] */
    CSM_OP_NCHW_TO_NHWC = 9,/* in0 = ext NCHW tensor (c real channels) -> NHWC padded to out.c (zeros) */
    CSM_OP_NHWC_TO_NCHW = 10,
    CSM_OP_ACT = 11,        /* out = act(in0) */
    CSM_OP_COPY = 12,       /* out = in0 (slice copy) */
    /* ZoeDepth metric-bins head (depth_modules/zoedepth/models/layers/attractor.py, dist_layers.py) */
    CSM_OP_ATTRACTOR = 13,  /* in0 = attractor points A [n,h,w,na], in1 = bin centers b [n,h,w,nb] -> out = b + agg_i dist(A_i - b):
                               dist = dx / (1 + alpha dx^2) (flags bit 0 = 0, "inv") or exp(-alpha dx^2) dx (bit 0 = 1, "exp");
                               agg = sum over i in order, / na when flags bit 1 (kind "mean"); aux_off -> {alpha}  (gamma = 2) */
    CSM_OP_LOGBINOM = 14,   /* in0 = pt [n,h,w,4] (softplus'ed p0,p1,t0,t1), in1 = bin centers [n,h,w,nb] -> out [n,h,w,1] =
                               sum_k softmax_k(logbinomial_k(p) / t) * centers_k  (ConditionalLogBinomial.forward tail + the
                               weighted sum of zoedepth_v1.py:199); aux_off -> {p_eps, min_temp, max_temp, lb[0..nb)} with
                               lb[k] = log_binom(nb-1, k) tabulated by the host */
    /* MiDaS DPT-BEiT core of ZoeDepth (timm 0.6.x beit_large_patch16_384 + MiDaS 3.1 dpt_depth.py / backbones/beit.py; the reference
     * fetches it with torch.hub, depth_modules/zoedepth/models/base_models/midas.py:341).  A token sequence [B, N, C] is the NHWC tensor
     * n = B, h = N, w = 1, c = C, so every nn.Linear is a 1x1 CSM_OP_CONV (exact fmaf chains, as above).  The ops below hold reductions
     * over channels / keys: their order is implementation-defined and parity with the oracle is tolerance-level (1e-5 relative), not
     * bit-exact. */
    CSM_OP_LAYERNORM = 15,  /* out[p, :] = (in0[p, :] - mean) * rsqrt(var + eps) * gamma + beta over the c channels of every pixel p
                               (biased variance); w_off -> gamma[c], b_off -> beta[c], aux_off -> {eps} */
    CSM_OP_ATTENTION = 16,  /* multi-head self-attention core.  in0 = qkv [n, N, 1, 3 * heads * d] (channels: q | k | v, each head-major;
                               q already carries the 1/sqrt(d) scale), out = [n, N, 1, heads * d]; groups = heads, cin_g = d.
                               out[i, h, :] = sum_j softmax_j(q_i . k_j + bias_h(i, j)) v_j.  BEiT's relative position bias: token 0 is the
                               class token, token 1 + y * kw + x the patch (y, x) of the kh x kw grid (N = kh * kw + 1); aux_off ->
                               table [(2 kh - 1) * (2 kw - 1) + 3][heads]: bias_h(i, j) = table[(yi - yj + kh - 1) * (2 kw - 1) + (xi - xj +
                               kw - 1)][h] between patches, rows T-3 / T-2 / T-1 for cls->patch / patch->cls / cls->cls (timm
                               gen_relative_position_index), stored HEAD-MAJOR ([heads][T]) in the device weight buffer; aux_off < 0:
                               no bias.  Keys are streamed with a running max / sum: any sequence length */
    CSM_OP_TOKENS = 17,     /* token plumbing, mode = flags: 0 "assemble" in0 = patch embedding [n, gh, gw, c] -> out [n, gh*gw + 1, 1, c],
                               row 0 = class token (aux_off -> c floats); 1 "readout project input" in0 = tokens [n, N, 1, c] ->
                               out [n, kh, kw, 2c] = (token 1 + i | class token) (MiDaS ProjectReadout's concat); 2 "readout ignore"
                               -> out [n, kh, kw, c] = token 1 + i (MiDaS Slice) */
    CSM_OP_DEPTH_TO_SPACE = 18, /* out[n, y*k + ky, x*k + kx, c] = in0[n, y, x, (ky*k + kx) * out.c + c], k = stride: the scatter half of a
                               ConvTranspose2d(kernel = stride = k) whose GEMM half is a 1x1 CSM_OP_CONV to k*k*cout channels */
    /* Segment Anything (segment_anything's ImageEncoderViT / PromptEncoder / MaskDecoder, boxes only; csrc/sam.hip).  Same
     * tolerance-level status as the three transformer ops above.  CSM_OP_TOKENS gains the modes
     *   3 "window partition": in0 [n, gh, gw, c] -> out [n * wy * wx, kh * kh, 1, c], wy = ceil(gh / kh), wx = ceil(gw / kh): window
     *     (b, iy, ix) is sample (b * wy + iy) * wx + ix, its token ty * kh + tx the pixel (iy kh + ty, ix kh + tx), ZEROS beyond the map;
     *   4 "window un-partition": the inverse, padding dropped: out [n, gh, gw, c] = in0 [n * wy * wx, kh * kh, 1, c] (+ in1 [n, gh, gw, c]);
     *   5 / 6 "broadcast add": out[b, p, :] = in0[b % in0.n, p, :] (+ in1[b % in1.n, p, :]) (+ aux); in0.n and in1.n are 1 or out.n;
     *     aux_off -> c floats (mode 5, optional) or h * w * c floats, one vector per position (mode 6). */
    CSM_OP_ATTENTION_RELPOS = 19, /* self-attention with the decomposed relative position bias.  in0 = qkv [n, ., ., 3 * heads * d] with
                               N = h * w = kh * kw tokens, token y * kw + x = grid position (y, x) (q | k | v head-major, q carrying
                               1/sqrt(d)); out [n, ., ., heads * d]; groups = heads, cin_g = d in {32, 64, 80, 128}.
                               out[i, h, :] = sum_j softmax_j(q_i . k_j + q_i . R[yi - yj + kh - 1] + q_i . R[2 kh - 1 + xi - xj + kw - 1]) v_j
                               aux_off -> R [(2 kh - 1) + (2 kw - 1)][d]: the height table, then the width table, shared by the heads and
                               multiplied by sqrt(d) by the host (the q of the product is the scaled one) */
    CSM_OP_CROSS_ATTENTION = 20,  /* in0 = q [n, Nq tokens, heads * d] (scaled), in1 = [n, Nk tokens, 2 * heads * d] (k | v, head-major)
                               -> out [n, Nq, heads * d] = softmax_j(q_i . k_j) v_j per head; groups = heads, cin_g = d in
                               {2, 4, 8, 16, 32, 64}; any Nq, Nk (token count = h * w) */
    CSM_OP_CHANNEL_DOT = 21       /* out[n, y, x, 0] = sum_c in0[n, y, x, c] * in1[n, 0, 0, c], ascending c, one fmaf chain from 0 */
};
enum csm_act { CSM_ACT_NONE = 0, CSM_ACT_RELU = 1, CSM_ACT_SILU = 2, CSM_ACT_PRELU = 3, CSM_ACT_HSIGMOID = 4,
               CSM_ACT_SIGMOID = 5, CSM_ACT_SOFTPLUS = 6 /* torch.nn.Softplus(): x > 20 ? x : log(1 + exp(x)) */,
               CSM_ACT_GELU = 7 /* torch.nn.GELU(): 0.5 x (1 + erf(x / sqrt 2)) */ };

typedef struct csm_tensor_desc {
    int64_t offset;      /* floats from the workspace base (ext < 0) or from ext pointer slot `ext` */
    int32_t ext;         /* -1: workspace; >=0: index into the ext pointer table of csm_run_program */
    int32_t n, h, w, c;  /* logical NHWC shape (c = channels of this view) */
    int32_t ld;          /* channel pitch in floats (>= c); NCHW ext tensors: ld is ignored */
} csm_tensor_desc;

/* Winograd contract (csm_op.flags & CSM_CONV_FLAG_WINOGRAD; restated in oracle/nets_oracle.c::orc_conv_wino, executed by
 * csrc/wino.hip::k_conv_wino): F(2x2, 3x3) with the transform matrices of Lavin & Gray (0, +-1, +-1/2 only).
 *   U[f = 4i + j][co][c] = fp32(G g G^T) evaluated in double, rows first: r0 = g0, r1 = ((g0 + g1) + g2) / 2, r2 = ((g0 - g1) + g2) / 2,
 *                          r3 = g2, then the same over the columns;
 *   V = B^T d B on the 4 x 4 input window d (origin (2 ty - 1, 2 tx - 1), zeros outside): t0 = d0 - d2, t1 = d1 + d2, t2 = d2 - d1,
 *                          t3 = d1 - d3 over the row index first, then over the column index -- one fp32 operation per value;
 *   M[f] = one fmaf chain per (f, tile, co) over the input channels from 0.0f, channel order of the direct contract;
 *   Y = A^T M A over j first: s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3, then over i; y = Y + bias; residual / activation as usual.
 * Packed device weights (cout tile of 64, 32-channel block cb, 8-channel step q): [co / 64][cb][q][f][h][co % 64][4] with channel
 * c = 32 cb + 8 q + 4 h + e at element e -- exactly the LDS image of one pipeline step (32 KB), moved by a linear LDS-DMA copy. */
/* Winograd F(4x4, 3x3) contract (csm_op.flags & CSM_CONV_FLAG_WINOGRAD4; restated in oracle/nets_oracle.c::orc_conv_wino4, executed by
 * csrc/wino4.hip::k_conv_wino4): Lavin & Gray's matrices for the points 0, +-1, +-2, inf -- 36 products per 4x4 output tile and channel
 * pair (F(2x2): 64, direct: 144).  Same layer class as F(2x2); which of the two a layer takes is the lowering's per-sample rule.
 *   U[f = 6i + j][co][c] = fp32(G g G^T) in double, rows first: r0 = g0 * 0.25, r1 = -((g0 + g1) + g2) / 6, r2 = -((g0 - g1) + g2) / 6,
 *                          r3 = ((g0 + 2 g1) + 4 g2) / 24, r4 = ((g0 - 2 g1) + 4 g2) / 24, r5 = g2 (IEEE double division), then the columns;
 *   V = B^T d B on the 6 x 6 window d (origin (4 ty - 1, 4 tx - 1), zeros outside), 1-D transform in fp32 with fmaf where written:
 *                          t0 = fmaf(4, d0, fmaf(-5, d2, d4)), t5 = fmaf(4, d1, fmaf(-5, d3, d5)),
 *                          a = fmaf(-4, d2, d4), b = fmaf(-4, d1, d3), t1 = a + b, t2 = a - b,
 *                          c = d4 - d2, e = d3 - d1, t3 = fmaf(2, e, c), t4 = fmaf(-2, e, c)   -- row index first, then column index;
 *   M[f] = one fmaf chain per (f, tile, co) over the input channels from 0.0f, channel order of the direct contract;
 *   Y = A^T M A over j first, then i, 1-D transform p = m1 + m2, q = m1 - m2, r = m3 + m4, t = m3 - m4,
 *                          s0 = (m0 + p) + r, s1 = fmaf(2, t, q), s2 = fmaf(4, r, p), s3 = fmaf(8, t, q) + m5;
 *   y = Y + bias; residual / activation as usual.  Output pixel (4 ty + a, 4 tx + b).
 * Packed device weights (cout tile of 64, step s = 4 input channels: 8-block s >> 1, half s & 1):
 *   [co / 64][s][wave = 6 nh + i][piece p][lh][li][jj][t] = U[6 i + 2 p + jj][64 (co / 64) + 32 nh + li][8 (s >> 1) + 4 lh + 2 (s & 1) + t]
 *   -- 36 KB per (cout tile, step); a wave's 3 KB are its three LDS-DMA pieces, lane 32 lh + li reads its four values as one 16-B word. */
#define CSM_CONV_FLAG_STEM 2
#define CSM_CONV_FLAG_WINOGRAD 4
#define CSM_CONV_FLAG_WINOGRAD4 8
/* Narrow grouped 3x3 convolutions on the vector pipe (csm_op.flags & CSM_CONV_FLAG_GROUPED; csrc/grouped.hip::k_conv_grouped): the DIRECT
 * arithmetic above, unchanged (same fmaf chain, same bits as the block-diagonal matrix-pipe form) -- the flag only says which weight image
 * the op carries.  3x3, stride 1, dilation 1, pad 1, cin_g == cout_g in {8, 16, 32}, channels % 32 == 0, ksplit 1; groups / cin_g /
 * cout_g are the REAL groups (not super-groups).  Packed device weights, one 32-float half unit per (tap, 8-channel block kb, half h):
 *   [group][octet][tap = 3 ky + kx][kb][h][chain position i][t] = w[group cin_g + 8 octet + 4 h + t][8 kb + 4 (i & 1) + (i >> 1)][ky][kx] */
#define CSM_CONV_FLAG_GROUPED 16

typedef struct csm_op {
    int32_t kind;
    int32_t in0, in1, out;   /* tensor ids; in1 = residual / second operand, -1 if none */
    int32_t kh, kw, stride, pad, dil;
    int32_t groups;          /* CONV: number of super-groups (1 = dense); each maps cin_g -> cout_g channels */
    int32_t cin_g, cout_g;
    int32_t act, res_mode;   /* res_mode: 0 none, 1 add before act, 2 add after act.  CONV: the residual view (in1) may BE the output
                                view (same buffer, same channel offset: an in-place add -- every kernel reads exactly the residual
                                elements it writes, ahead of its stores); ANY OTHER overlap of the two views is not allowed: the
                                residual values of a pixel are read before, after or while other blocks store theirs */
    int64_t w_off, b_off, aux_off;   /* float offsets into the weight buffer (aux = PReLU slopes); -1 = none */
    int32_t flags;           /* BILINEAR: bit 0 = align_corners.  CONV: bit 1 = stem (cin padded to 4): weights are packed with K =
                                (tap, channel), 8 taps x 4 channels per 32-wide chunk, for k_conv_stem; the chain is unchanged.
                                CONV bit 2 (CSM_CONV_FLAG_WINOGRAD): exact-fp32 Winograd F(2x2, 3x3) arithmetic (3x3, stride 1, dilation
                                1, pad 1, dense, cin % 32 == 0, cout % 64 == 0, ksplit 1): weights are the transformed panels
                                U = G g G^T packed for k_conv_wino; part of the NUMERICAL contract (set by the lowering from the layer's
                                per-sample shape, never by the tuner) -- see "Winograd contract" below.
                                CONV bit 3 (CSM_CONV_FLAG_WINOGRAD4): the same layer class in the F(4x4, 3x3) arithmetic (weights = its own
                                36-frequency panels packed for k_conv_wino4); bits 2 and 3 are exclusive.
                                CONV bit 4 (CSM_CONV_FLAG_GROUPED): narrow groups on the vector pipe -- direct arithmetic, its own
                                weight image, REAL groups in groups / cin_g / cout_g (see above) */
    int32_t ksplit;          /* CONV: K is cut into `ksplit` runs of (32-channel block, tap) chunks (block-major), run s = chunks
                                [s*T/ksplit, (s+1)*T/ksplit); each run is its own fmaf chain (run 0 starts at the bias,
                                the others at 0) and the runs are added in order ((p0+p1)+p2)...  1 = single chain */
    int32_t scratch;         /* tensor id of the [n,h,w,ksplit*cout] partial-sum buffer when ksplit > 1, else -1.  CONV with
                                CSM_CONV_FLAG_WINOGRAD4: optional (-1 = none) contiguous tensor of >= n * ceil(h/4) * ceil(w/4) * 24 * cout
                                floats; with it the library may run launches of few block tiles in a row-split execution form of
                                the same arithmetic (speed only: same bits) */
    int32_t tile;            /* CONV: 0 = built-in tile rule; low 6 bits k > 0 = tile configuration k-1 (an id of the table in
                                csrc/csm_convcfg.h, listed by csm_debug_conv_cfg_info), bit 6 (64) = split-K runs
                                walked serially by one block instead of ksplit blocks + reduce, bit 7 (128) = mixed-tile launch (the
                                configuration's tiles cover whole rounds of the grid, 64 x 64 tiles the remaining rows).  Speed only:
                                every configuration and every launch form produces the same bits; filled in by csm_conv_autotune */
} csm_op;

/* Measure every eligible tile configuration of every CONV op on the device (HIP events on `stream`, `reps` timed launches
 * each, minimum taken) and store the fastest in ops[i].tile.  Results are unchanged by construction (same fmaf chains);
 * the workspace contents are clobbered.  Returns the number of ops tuned (>= 0) or a negative status. */
int csm_conv_autotune(csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors, const float *weights,
                      float *workspace, void *const *ext, int n_ext, void *stream, int reps);

/* Persist / restore the tuned tiles (text file: layer signature -> tile).  load returns the number of entries merged (0 if the
 * file does not exist); csm_conv_autotune consults the table before measuring. */
int csm_conv_tile_cache_save(const char *path);
int csm_conv_tile_cache_load(const char *path);

/* Execute ops[0..n_ops) in order on `stream`.  `weights` and `workspace` are device pointers;
 * ext[i] are device pointers of external (caller-owned) tensors. */
int csm_run_program(const csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors,
                    const float *weights, float *workspace, void *const *ext, int n_ext, void *stream);
/* Tuning aid (not stable ABI): force the conv tile configuration index, -1 = built-in cost model. */
int csm_debug_force_conv_cfg(int cfg);
/* Test aid (not stable ABI): how ksplit > 1 layers are executed: -1 = tuned / built-in rule, 0 = parallel, 1 = serial. */
int csm_debug_force_splitk_serial(int mode);
/* Measurement aid (not stable ABI): bit 0 = the autotuner may choose mixed-tile launches (default on); bit 1 = N-grouped tile order
 * (layers whose weights exceed an XCD's L2) OFF (default on).  Speed only. */
int csm_debug_conv_tuner_options(int options);
/* Test / tooling aid (not stable ABI, host only: no device is touched): the table of conv tile configurations.  csm_debug_conv_cfg_info
 * fills `info` for id cfg in [0, csm_debug_conv_cfg_count()) -- the strings are static -- and returns CSM_ERR_ARG for any other id.
 * csm_debug_conv_resolve_cfg: the id csm_run_program would launch for CONV `op` (not a stem / Winograd / grouped one) carrying
 * configuration `cfg`, with the input and output views at their offsets from a NULL base (alignment follows the offsets; the weights
 * likewise): a configuration whose kernel family cannot run the layer falls back.  Returns the id, or a negative status. */
typedef struct csm_conv_cfg_desc {
    int32_t id;
    int32_t bn;              /* output channels per tile */
    int32_t tune_pos;        /* position in csm_conv_autotune's candidate order; -1 = never timed */
    const char *name;        /* e.g. "D128x64" */
    const char *family;      /* kernel family: "MFMA", "DMA", "PATCH", "DMA_P", "PATCH_P", "WS" or "NARROW" */
} csm_conv_cfg_desc;
int csm_debug_conv_cfg_count(void);
int csm_debug_conv_cfg_info(int cfg, csm_conv_cfg_desc *info);
int csm_debug_conv_resolve_cfg(int cfg, const csm_op *op, const csm_tensor_desc *in_desc, const csm_tensor_desc *out_desc);
/* Test aid (not stable ABI): bit 0 = CSM_OP_ATTENTION gathers the relative position bias from the table in global memory even when the
 * tile pair's window of the table fits the LDS budget (the path token grids wider than ~340 take).  Same results at the op's tolerance. */
int csm_debug_attention_options(int options);
/* Measurement aid: same execution, each op bracketed by HIP events on `stream`; synchronises and returns ms per op. */
int csm_run_program_profile(const csm_op *ops, int n_ops, const csm_tensor_desc *tensors, int n_tensors,
                            const float *weights, float *workspace, void *const *ext, int n_ext, void *stream,
                            float *op_ms);

/* ------------------------------------------------------------------------------------
 * Segment Anything glue (segment_anything's SamPredictor / ResizeLongestSide / Sam.preprocess / Sam.postprocess_masks; csrc/sam.hip)
 * ---------------------------------------------------------------------------------- */
/* bgr: DEVICE uint8 [H, W, 3] -> out: DEVICE float NCHW [3, S, S] = RGB, bilinear (align_corners = False, no antialiasing) to nh x nw,
 * (v - mean) / std with mean (123.675, 116.28, 103.53) and std (58.395, 57.12, 57.375), zeros beyond (nh, nw).  (segment_anything resizes
 * the uint8 image through PIL instead: a deliberate, documented difference.) */
int csm_sam_preprocess(const uint8_t *bgr, int H, int W, int S, int nh, int nw, float *out, void *stream);
/* logits: DEVICE float [n, L, L] -> masks: DEVICE uint8 (0 / 1) [n, H, W]: bilinear to S x S, crop to [nh, nw], bilinear to H x W
 * (both align_corners = False), > 0 -- one pass, nothing in between is stored. */
int csm_sam_postprocess(const float *logits, int n, int L, int S, int nh, int nw, int H, int W, uint8_t *masks, void *stream);
/* boxes: DEVICE float [n, 4] xyxy, multiplied by (sx, sy) into the model's S x S input frame -> tokens: DEVICE float NCHW
 * [n, C, n_static + 2, 1]: the n_static constant output tokens, then the two corner embeddings sin | cos(2 pi (2 (p + 0.5) / S - 1) . gauss)
 * + point embedding.  consts: DEVICE float [n_static][C] tokens, [2][C] point embeddings 2 and 3, [2][C / 2] the Gaussian matrix. */
int csm_sam_box_tokens(const float *boxes, int n, double sx, double sy, int S, const float *consts, int C, int n_static, float *tokens,
                       void *stream);

/* ------------------------------------------------------------------------------------
 * Glue around the Inpaint / Refine nets, the depth-adjustment resize branch and AnimeInstances.resize (rounds 1-2 used torch ops here)
 * ---------------------------------------------------------------------------------- */

/* out2 = {x.mean(), x.std(unbiased=False)} over all n elements (pointcloud_inpainting.py:116-119, disparity_refinement.py:97-98);
 * double accumulation, two passes; scratch: csm_mean_std_scratch_bytes() bytes. */
size_t csm_mean_std_scratch_bytes(void);
int csm_mean_std(const float *x, int64_t n, float *out2, void *scratch, void *stream);
/* out = (x - mean) / (std + 1e-7) with {mean, std} read from device memory (:121-131 / :100-107) */
int csm_normalise_mean_std(const float *x, int64_t n, const float *mean_std_dev, float *out, void *stream);
/* out = x * (std + 1e-7) + mean, then mode 0: nothing, 1: clip(0, 1) (tenImage), 2: threshold(0.0, 0.0) (tenDisparity) */
int csm_denormalise_mean_std(const float *x, int64_t n, const float *mean_std_dev, int mode, float *out, void *stream);
/* torch.nn.functional.interpolate(mode='bilinear', align_corners=...) of `planes` [H,W] planes (NCHW with N*C = planes) to [h,w]:
 * depth_adjustment_animesseg's resize round trip (kenburns_effect.py:49-52, :89-90), disparity_estimation's input resize */
int csm_resize_bilinear_planes(const float *in, int planes, int H, int W, int h, int w, int align_corners, float *out, void *stream);
/* AnimeInstances.resize (animeinsseg/anime_instances.py:268-280): interpolate(masks.float(), (h, w), mode='area') > thr on boolean
 * masks [n,H,W] (1 B per pixel) -> [n,h,w] */
int csm_mask_area_resize_threshold(const uint8_t *masks, int n, int H, int W, int h, int w, float thr, uint8_t *out, void *stream);

/* ------------------------------------------------------------------------------------
 * ZoeDepth plumbing around the metric-bins head (CSM_OP_ATTRACTOR / CSM_OP_LOGBINOM) and the pluggable MiDaS core
 * replaces DepthModel.infer / _infer_with_pad_aug / infer_with_flip_aug (depth_modules/zoedepth/models/depth_model.py:57-129),
 * PrepForMidas + Resize (models/base_models/midas.py:49-187) and the tail of _depth_est_zoe (kenburns_effect.py:812-818)
 * ---------------------------------------------------------------------------------- */

/* img [B,3,H,W] (0..1) -> out [B,3,nh,nw] = Normalize(0.5, 0.5)(bilinear_align_corners(reflect_pad(flip ? hflip(img) : img, pad_w,
 * pad_h) -> (nh, nw))) in ONE pass (the padded image never exists); pad < size. */
int csm_zoe_pad_prep(const float *img, int B, int H, int W, int pad_h, int pad_w, int flip, int nh, int nw, float *out, void *stream);
/* d [B,1,h,w] (prediction at the core's resolution for the padded input) -> out [B,1,H,W]: bicubic (aten, A = -0.75,
 * align_corners = false) to the padded size (H + 2 pad_h, W + 2 pad_w), cropped to the original view, mirrored back when unflip;
 * mode 0: out = v; mode 1: out = (out + v) / 2 (second pass of infer_with_flip_aug). */
int csm_zoe_resize_crop(const float *d, int B, int h, int w, int pad_h, int pad_w, int H, int W, int unflip, int mode, float *out,
                        void *stream);
/* disparity = reciprocal(depth + 1e-5) * (focal * baseline); nan / +-inf -> 0   (kenburns_effect.py:816-817) */
int csm_zoe_depth_to_disparity(const float *depth, int64_t n, float focal_times_baseline, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Instance-segmentation post-processing
 * ---------------------------------------------------------------------------------- */

/* np.packbits(mask != 0, bitorder='little'): boolean instance masks (1 B per pixel, as AnimeInstances holds them) -> 1 bit per pixel,
 * the wire format of the per-rank output gather.  out: ceil(n / 8) bytes. */
int csm_pack_mask_bits(const uint8_t *mask, int64_t n, uint8_t *out, void *stream);

/* RTMDet-Ins box decode between the head's raw maps and NMS -- mmdet RTMDetInsHead.predict_by_feat / _predict_by_feat_single /
 * _bbox_mask_post_process + filter_scores_and_topk [EXT mmdet 3.3.0; call site animeinsseg/__init__.py:450 model.test_step], with
 * FIXED shapes and no host sync: per level the `nms_pre` highest scores above score_thr (stable descending order), distance2bbox
 * against the resized-image bounds, rescale to the original image, min_bbox_size filter, then all levels merged in score order.
 * Slots without a valid candidate carry score -1 and sort last (they can never suppress a valid box in the greedy NMS).
 *   cls / reg: HOST arrays of n_levels DEVICE pointers to NHWC maps [nb, h_l, w_l, *] (cls: num_classes sigmoid scores per prior,
 *   reg: 4 relu'd distances in stride units); level_hw {h0, w0, h1, w1, ...}; strides; lds3 {cls, reg, kernel channel pitch} per level.
 *   outputs per image, in NMS order: scores [nb,K], boxes [nb,K,4] xyxy, src [nb,K] (global prior index, level-major), labels [nb,K],
 *   class_offsets [nb,K] = label * (max box coordinate + 1) (written when num_classes > 1; may be NULL otherwise).
 *   K <= csm_det_decode_slots(...) = sum_l min(nms_pre, h_l w_l num_classes) (<= 4096; nms_pre <= 1024; -1 = unsupported).
 *   scratch: csm_det_decode_scratch_bytes(nb, slots). */
int csm_det_decode_slots(const int *level_hw, int n_levels, int num_classes, int nms_pre);
size_t csm_det_decode_scratch_bytes(int nb, int slots);
int csm_det_decode(const float *const *cls, const float *const *reg, const int *level_hw, const int *strides, const int *lds3,
                   int n_levels, int nb, int num_classes, float score_thr, int nms_pre, float clamp_w, float clamp_h,
                   float scale_x, float scale_y, float min_bbox_size, int K, float *scores, float *boxes, int *src, int *labels,
                   float *class_offsets, void *scratch, void *stream);
/* After NMS: for the max_keep slots of keep [nb, max_keep] (indices into the K candidates; slots past the kept count are ignored by
 * the caller) gather scores, boxes, labels, the priors (x, y, stride, stride: MlvlPointGenerator offset 0) and the num_gen_params
 * dynamic-conv parameters from the per-level kernel maps. */
int csm_det_gather(const float *const *kern, const int *level_hw, const int *strides, const int *lds3, int n_levels, int nb, int K,
                   int max_keep, int num_gen_params, const int *keep, const float *scores, const float *boxes, const int *src,
                   const int *labels, float *kept_scores, float *kept_boxes, int *kept_labels, float *kept_priors,
                   float *kept_kernels, void *stream);

/* Greedy NMS, replaces mmcv.ops.batched_nms -> nms (C++/CUDA ext; call site: mmdet head, imported at
 * animeinsseg/models/rtmdet_inshead_custom.py:10).  boxes [n,4] xyxy sorted by descending score;
 * class_offsets [n] (label * (max_coord+1)) or NULL for class-agnostic / single class;
 * suppress iff inter > iou_thr * (Sa + Sb - inter).  keep[<=max_keep] = indices in score order.  n <= 4096. */
size_t csm_nms_scratch_bytes(int n);
int csm_nms(const float *boxes, const float *class_offsets, int n, float iou_thr, int max_keep, int *keep,
            int *n_keep, void *scratch, void *stream);
/* csm_nms for the nb images of a detector run in ONE call (two launches, whatever nb): boxes [nb][n][4], class_offsets [nb][n] or
 * NULL, keep [nb][max_keep], n_keep [nb].  The image is a grid dimension of the same kernels; image b works in its own slice of
 * scratch (csm_nms_batch_scratch_bytes(nb, n) bytes, 8-byte aligned) and gets exactly what csm_nms gives for it. */
size_t csm_nms_batch_scratch_bytes(int nb, int n);
int csm_nms_batch(const float *boxes, const float *class_offsets, int nb, int n, float iou_thr, int max_keep, int *keep,
                  int *n_keep, void *scratch, void *stream);

/* RTMDetInsSepBNHeadCustom._mask_predict_by_feat_single   animeinsseg/models/rtmdet_inshead_custom.py:253-303
 * mask_feat NHWC [h,w,num_prototypes] with channel pitch ld; kernels [n,169]; priors [n,4] = (x,y,stride,stride);
 * logits [n,h,w]. */
int csm_maskhead_logits(const float *mask_feat, int ld, int h, int w, int num_prototypes, int dyconv_channels,
                        const float *kernels, const float *priors, int n, int feat_stride, float *logits,
                        void *stream);

/* mmdet _bbox_mask_post_process tail (mirrored at animeinsseg/__init__.py:361-370), fused:
 * interpolate(scale_factor=up) -> interpolate(size=(rh,rw)) -> [..., :oh, :ow] -> sigmoid() > thr.
 * masks: uint8 [n,oh,ow] (0/1).  The slice cannot enlarge: the caller passes oh = min(rh, ori_h), ow = min(rw, ori_w)
 * (mmdet's ceil(S / scale) lands 1-2 px under the original size for ~20 % of image shapes). */
int csm_mask_resize_threshold(const float *logits, int n, int h, int w, int up, int rh, int rw, int oh, int ow,
                              float thr, uint8_t *masks, void *stream);
/* csm_maskhead_logits + csm_mask_resize_threshold for all nb frames of a detector run in ONE call (one mask-head launch per 16
 * frames and one tail launch), plus the box conversion of AnimeInsSeg._instances_from.  Frame k contributes its first n_k[k]
 * detections (n_k: HOST array of nb entries, read before the call returns, each 0 <= n_k[k] <= max_keep); the instances of all
 * frames form one flat frame-major list of sum(n_k) entries.  mask_feat: frame 0's NHWC prototype map, frame k's starts
 * sample_stride floats further on per frame (the detector workspace's sample stride); kernels [nb][max_keep][169], priors and boxes
 * [nb][max_keep][4] as csm_det_gather wrote them (boxes xyxy float).  Outputs: logits [sum n_k][h][w] (scratch), masks uint8
 * [sum n_k][oh][ow] (0/1) and boxes_xywh int32 [sum n_k][4] = (int)x1, (int)y1, (int)x2 - (int)x1, (int)y2 - (int)y1.  Entry by
 * entry the bits of the per-frame pair of calls; nothing is written past sum(n_k) entries; sum(n_k) == 0 launches nothing. */
int csm_det_masks_batch(const float *mask_feat, int64_t sample_stride, int ld, int h, int w, int num_prototypes,
                        int dyconv_channels, const float *kernels, const float *priors, const float *boxes, int nb, int max_keep,
                        const int *n_k, int feat_stride, int up, int rh, int rw, int oh, int ow, float thr, float *logits,
                        uint8_t *masks, int *boxes_xywh, void *stream);

/* prepare_refine_batch   animeinsseg/__init__.py:37-55 (+ utils/io_utils.py:254-292 resize_pad):
 * img u8 HWC [H,W,3], masks u8 [n,Hm,Wm] -> batch fp32 NCHW [n,4,T,T]; (rh,rw) = keep-ratio size of the image inside T x T,
 * (rhm,rwm) = the same rule applied to the mask's own shape (the reference resize_pad()s every seg by its own size; detector
 * masks can be 1-2 px smaller than the image, see csm_mask_resize_threshold). */
int csm_refine_prepare_batch(const uint8_t *img_hwc, const uint8_t *masks, int n, int H, int W, int rh, int rw, int Hm, int Wm,
                             int rhm, int rwm, int T, float *batch, void *stream);
/* csm_refine_prepare_batch for n items that each name their OWN image (imgs_hwc[i]: u8 HWC [H,W,3]) and their own single mask plane
 * (masks[i]: u8 [Hm,Wm]) -> batch [n,4,T,T], one launch per 16 items.  imgs_hwc and masks are HOST arrays of n device pointers, read
 * before the call returns and passed on by value in kernel arguments (no pointer table in device memory).  Item i gets exactly
 * what csm_refine_prepare_batch(imgs_hwc[i], masks[i], 1, ...) writes. */
int csm_refine_prepare_many(const uint8_t *const *imgs_hwc, const uint8_t *const *masks, int n, int H, int W, int rh, int rw,
                            int Hm, int Wm, int rhm, int rwm, int T, float *batch, void *stream);

/* _postprocess_refine tail   animeinsseg/__init__.py:653-662:
 * sigmoid -> crop [:crop_h,:crop_w] -> bilinear(align_corners=True) to (oh,ow) -> > thr ; masks u8 [n,oh,ow]. */
int csm_refine_threshold(const float *logits, int n, int S_h, int S_w, int crop_h, int crop_w, int oh, int ow, float thr,
                         uint8_t *masks, void *stream);

/* refine_method='animeseg' (animeinsseg/__init__.py:78-115, :623-630) around ISNetDIS(in_ch=3) (anime-seg ISNet-IS).
 * get_mask input   animeinsseg/models/animeseg_refine/__init__.py:169-178: img u8 HWC [H,W,3] -> cv2 INTER_LINEAR u8 to (h,w)
 * -> /255 into the zero s x s canvas at (ph/2, pw/2), ph = s-h, pw = s-w -> out fp32 NCHW [3,s,s] (one slot of a batch).  (h,w)
 * is the host's letterbox rule (long side s, short side int(s * short / long)).  bgr_to_rgb = 1 swaps channels 0 and 2 (the
 * cvtColor of animeseg_refine, :87-88); get_mask's own input is already RGB (0). */
int csm_animeseg_prepare(const uint8_t *img_hwc, int H, int W, int h, int w, int s, int bgr_to_rgb, float *out_nchw, void *stream);

/* get_mask tail   :180-188 (+ the threshold of animeseg_refine, :89-91): logits = d1 [s,s] of the net; sigmoid -> crop
 * [ph/2:ph/2+h, pw/2:pw/2+w] -> cv2 float INTER_LINEAR to (H0,W0) -> prob_out fp32 [H0,W0], fg_out u8 [H0,W0] = prob > thr.
 * Either output may be NULL. */
int csm_animeseg_mask(const float *logits, int s, int h, int w, int H0, int W0, float thr, float *prob_out, uint8_t *fg_out,
                      void *stream);

/* animeseg_refine select   :96-105, in place: masks u8 [k,Hm,Wm] (0/1), fg u8 [>=Hm, W0] (row pitch W0, Wm <= W0).  Instance i
 * becomes mask & fg[:Hm,:Wm] iff sum(mask & fg) / sum(mask) > 0.3 (float64 in the reference; decided exactly in integers), else
 * stays.  counts_scratch: 2k uint32 of device memory.  Two launches, no host sync. */
int csm_animeseg_select(uint8_t *masks_u8, int k, int Hm, int Wm, const uint8_t *fg, int W0, unsigned *counts_scratch,
                        void *stream);

/* COCO compressed RLE of n masks (maskrle.hip): the 'counts' string of utils/io_utils.py:327-333 mask2rle, i.e.
 * pycocotools.mask.encode(np.asfortranarray(m[..., None] > 0).astype(np.uint8))[0]['counts'] (maskApi.c rleEncode + rleToString:
 * column-major runs starting with the value 0, stored as differences to the count two before from the fourth count on).
 * masks u8 [n,H,W] row-major, contiguous; any non-zero byte is set.  H*W <= 2^31-1, n <= 65535.
 * scratch: csm_mask_rle_scratch_bytes(n, H, W) device bytes, O(n*W) (at most n*W*224), shared by the two calls.
 * csm_mask_rle_measure: info device int64 [n][4] = {num_counts, string_bytes, area (pixels set), byte_offset}, byte_offset the
 *   exclusive prefix of string_bytes (total bytes = info[n-1][3] + info[n-1][1]); leaves per-column carries in scratch.
 * csm_mask_rle_write: instance i's string (no terminator) at out + info[i][3], for the same masks and scratch as the measure call
 *   (a unit never writes outside its measured bytes).
 * Five launches + one, async on the stream, no allocation, no sync, no atomics: the output is deterministic. */
size_t csm_mask_rle_scratch_bytes(int n, int H, int W);
int csm_mask_rle_measure(const uint8_t *masks, int n, int H, int W, int64_t *info, void *scratch, void *stream);
int csm_mask_rle_write(const uint8_t *masks, int n, int H, int W, const int64_t *info, char *out, void *scratch, void *stream);

/* PatchMatch inpainting (patchmatch.hip; contract DESIGN.md §4.5, restated in tests/patchmatch_restatement.py, byte-identical):
 * the patch_match.inpaint(img, mask, patch_size) of kenburns_effect.py:497-503, repaint_person.py:122, run_style.py:182.
 * img u8 [H,W,3], mask u8 [H,W] (non-zero = hole), global_mask u8 [H,W] or NULL (non-zero = never inside a source patch);
 * p odd in [3, 15], H, W >= p, H*W <= 2^28.
 * csm_patchmatch_levels: the pyramid levels prepare builds (0 for an invalid shape).
 * csm_patchmatch_scratch_bytes: device scratch shared by the two calls (about 30 B per pixel of the pyramid).
 * csm_patchmatch_prepare: pyramid, roles and ordered lists; info device int32 [levels][4] = {valid sources, targets, hole pixels,
 *   known pixels} per level.  The caller reads info once and schedules the run: the levels used are level 0 and the following
 *   levels while each still has a valid source; with no valid source (or no target) at level 0 the result is the input.
 * csm_patchmatch_run: the EM completion over `levels` levels with info_host = that host copy of info; writes out u8 [H,W,3]
 *   (known pixels unchanged).  The random draws are a counter hash of (seed, level, iteration, pass, pixel, sample).
 * Async on the stream, no allocation, no sync; a few hundred launches at 1024^2. */
int csm_patchmatch_levels(int H, int W, int p);
size_t csm_patchmatch_scratch_bytes(int H, int W, int p);
int csm_patchmatch_prepare(const uint8_t *img, const uint8_t *mask, const uint8_t *global_mask, int H, int W, int p, int *info,
                           void *scratch, void *stream);
int csm_patchmatch_run(int H, int W, int p, int levels, const int *info_host, unsigned seed, uint8_t *out, void *scratch,
                       void *stream);

/* Baseline JPEG of n equally sized frames (mjpeg.hip; contract DESIGN.md §4.6, restated in tests/mjpeg_restatement.py,
 * byte-identical): the frames of a Motion-JPEG AVI.  frames u8 [n,H,W,3] (B, G, R), contiguous; 1 <= H, W <= 65535;
 * quality 1..100 (IJG scaling of the Annex K tables); subsampling 420 (16x16 MCU) or 444 (8x8 MCU).  Every frame is a complete
 * JFIF file: SOI, APP0, two DQT, SOF0, four DHT (Annex K), DRI (= MCUs per row), SOS, one segment per MCU row with RSTm between
 * them, EOI.
 * scratch: csm_jpeg_scratch_bytes(n, H, W, subsampling) device bytes, shared by the two calls: int16 coefficients (3 B per padded
 *   pixel at 4:2:0, 6 B at 4:4:4), 12 B per MCU row, and at most 32 MiB (or one row's worst case) for rows too wide for LDS
 *   (more than 739 blocks: wider than 1968 pixels).  0 for an invalid shape.
 * csm_jpeg_header_bytes: bytes of a frame before its entropy data (the same for every frame).
 * csm_jpeg_measure: transform + bytes of every MCU row; info device int64 [n][2] = {offset, bytes} of each frame in the blob
 *   (offset the exclusive prefix of bytes; total = info[n-1][0] + info[n-1][1]).
 * csm_jpeg_write: frame f at out + info[f][0], for the same arguments and scratch as the measure call (a row never writes
 *   outside its measured bytes).
 * Four launches + one (more for the wide rows), async on the stream, no allocation, no sync; the only atomics are integer ORs of
 * disjoint bits, so the output is deterministic. */
size_t csm_jpeg_scratch_bytes(int n, int H, int W, int subsampling);
int csm_jpeg_header_bytes(void);
int csm_jpeg_measure(const uint8_t *frames, int n, int H, int W, int quality, int subsampling, int64_t *info, void *scratch,
                     void *stream);
int csm_jpeg_write(int n, int H, int W, int quality, int subsampling, const int64_t *info, uint8_t *out, void *scratch,
                   void *stream);

/* The zlib stream of a PNG's IDAT chunk for n equally sized 8-bit images (png.hip; contract DESIGN.md §4.7, restated in
 * tests/png_restatement.py, byte-identical).  images u8 [n,H,W,channels], contiguous; channels 1 (grey) or 3; 1 <= H, W <= 65535,
 * H * (W * channels + 1) < 2^31 and n * H < 2^24.  flags: bit 0 = the three channels are B, G, R in memory (written R, G, B), bit 1 =
 * grey bytes are a mask (any non-zero byte is written as 255).  Per scanline the best of the five PNG filters; per image ONE
 * deflate block of literals and distance-1 matches, whose Huffman code the HOST builds between the two calls.
 * scratch: csm_png_scratch_bytes(n, H, W, channels) device bytes, shared by the two calls: the filtered scanlines
 *   (W * channels + 1 bytes each) and 20 B per scanline.  0 for an invalid shape.  No scanline is staged in LDS, so there is no
 *   width bound and no second path.
 * csm_png_measure: table device uint32 [n][288] = the counts of the 286 literal / length symbols (the end-of-block symbol counted
 *   once), the Adler-32 of the filtered bytes, one spare word.
 * csm_png_write: host_table device uint32 [n][csm_png_table_words() = 384], filled by the host from the measured table:
 *   [0..285] bit-reversed code | code length << 16 of every symbol, [286] bits of the header (the two zlib bytes + the block
 *   header), [287] the Adler-32, [288..289] byte offset of the stream in out (low, high word; a multiple of 4), [290] bits of a
 *   match's all-zero distance code (1 under the dynamic code, 5 under the fixed one), [291] bytes of the stream, [292..383] the
 *   header bits, LSB-first.  out: out_bytes device bytes (a multiple of 4, 4-aligned), zeroed by the call; image f's stream at its
 *   offset: header, every scanline's symbols at its bit offset, the end-of-block symbol, zero bits to the next byte, the Adler-32
 *   big-endian.  Nothing is written at or past the stream's bytes rounded up to 4.  Same n, H, W, channels and scratch as the
 *   measure call.
 * Three launches and a memset per call, async on the stream, no allocation, no sync; the only atomics are integer adds (counts)
 * and integer ORs of disjoint bits, so the output is deterministic. */
size_t csm_png_scratch_bytes(int n, int H, int W, int channels);
int csm_png_table_words(void);
int csm_png_measure(const uint8_t *images, int n, int H, int W, int channels, int flags, uint32_t *table, void *scratch,
                    void *stream);
int csm_png_write(int n, int H, int W, int channels, const uint32_t *host_table, uint8_t *out, int64_t out_bytes, void *scratch,
                  void *stream);

/* Baseline JPEG files to uint8 B, G, R pixels (jpegdec.hip; contract DESIGN.md §4.8, restated in tests/jpegdec_restatement.py,
 * byte-identical).  The host parses the markers (cartoonsegmentation_amd/jpegcode.py) and hands over one blob of device bytes and
 * one descriptor per file; files of different sizes and modes share a call.
 * desc_host: host int32 [n][csm_jpeg_decode_desc_words() = 20]: [0] H, [1] W, [2] components (1 grey, 3 Y Cb Cr), [3] [4] the
 *   luminance sampling factors (1x1, 2x1 or 2x2; chroma is 1x1), [5] restart interval in MCUs (0 = none), [6] [7] offset and length of
 *   the entropy-coded bytes in the blob, [8] offset (a multiple of 4) of the file's table region in the blob, [9..11] / [12..14] the
 *   slot (0..5) of each component's DC / AC Huffman table, [15] [16] the byte offset of the file's pixels in out (low 31 bits,
 *   the bits above; a multiple of 4), the rest 0.
 * table region (5856 bytes): six Huffman tables of 912 bytes (uint16 lut[256]: length << 8 | symbol of the codes of up to 8 bits
 *   by the next 8 bits, else 0; int32 maxcode[18] by length, -1 = none; int32 valoff[18]: symbol index = valoff[length] + code;
 *   uint8 vals[256]), then uint16 [3][64] quantisation tables per component in natural order.
 * out: u8, file i at its offset as [H][W][3].  blob, out and scratch are 16-byte aligned.
 * scratch: csm_jpeg_decode_scratch_bytes(desc_host, n) device bytes (0 for invalid descriptors): 28 B per subsequence, int16
 *   coefficients and uint8 sample planes of the padded components.
 * csm_jpeg_decode_subseq_bytes: bytes of entropy data one lane owns (a compile-time constant).
 * csm_jpeg_decode: info_host (may be NULL) receives [0] the number of synchronisation passes between workgroups.  The call
 *   SYNCHRONISES the stream: once per pass (it reads a 4-byte flag) and once at the end (one error word per file).  Returns
 *   CSM_ERR_DATA for corrupt entropy data; whatever the data, no read leaves a file's entropy bytes and no store its blocks.
 *   No kernel waits on another workgroup; the output is deterministic. */
size_t csm_jpeg_decode_scratch_bytes(const int32_t *desc_host, int n);
int csm_jpeg_decode_subseq_bytes(void);
int csm_jpeg_decode_desc_words(void);
int csm_jpeg_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                    void *scratch, int *info_host, void *stream);

/* Progressive JPEG files (SOF2, Huffman) to uint8 B, G, R pixels (jpegprog.hip; contract DESIGN.md §4.11, the coefficient decode
 * restated in tests/jpegprog_restatement.py, byte-identical; the pixels are csm_jpeg_decode's).  The host parses the markers and
 * checks the scan script (jpegcode.probe(data, progressive=True)); files of different sizes, modes and scripts share a call.
 * desc_host: one csm_jpeg_decode row per file, validated as there; [5] .. [7] (restart interval, entropy range: 0, 0, 0 will do)
 *   and [9] .. [14] (table slots) are not used; [8] is the file's table region, of which only the quantisation tables are read.
 * scan_desc_host: host int32 [n_scans][csm_jpeg_decode_scan_desc_words() = 16], any order: [0] file (index into desc_host),
 *   [1] components of the scan (1, or all of the file's for a DC scan), [2] the first component's index, [3] [4] Ss Se, [5] [6] Ah Al
 *   (Ah = 0 or Al + 1, Al <= 13), [7] [8] offset and length of the scan's entropy-coded bytes in the blob, [9] the restart interval
 *   in force (MCUs in a scan of all components, else blocks), [10] offset (a multiple of 4) of the scan's decode tables in the blob
 *   (912 bytes each as in csm_jpeg_decode: one DC table per component of a DC first scan, one AC table for an AC scan, none for a
 *   DC refinement), [11] dependency level (0..63; the scans of one level must write disjoint coefficients, and a scan's level is
 *   above that of every earlier scan of the file whose coefficients it meets: jpegcode.scan_levels), [12] refinement scans with more than
 *   one restart interval: offset (a multiple of 4) in the blob of int32 [intervals], the byte of the scan's entropy data at which each
 *   interval begins ([0] = 0); the rest 0.  1 <= n_scans <= 64 n.
 * scratch: csm_jpeg_decode_progressive_scratch_bytes(...) device bytes (0 for invalid descriptors): csm_jpeg_decode's, 28 B per
 *   subsequence of every first scan, 8 B per block of every AC refinement scan.
 * csm_jpeg_decode_progressive: info_host (may be NULL) receives [0] the synchronisation passes between workgroups, [1] the levels
 *   launched, [2] [3] 0.  The call SYNCHRONISES the stream: once per pass and once at the end.  Returns CSM_ERR_DATA for corrupt
 *   entropy data (an invalid code, a refinement symbol of size above 1, a coefficient placed past its band, a scan whose data do not
 *   hold its blocks exactly); whatever the data and whatever [12] points at, no read leaves a scan's entropy bytes and no store the
 *   file's blocks.  No kernel waits on another workgroup; the output is deterministic. */
size_t csm_jpeg_decode_progressive_scratch_bytes(const int32_t *desc_host, int n, const int32_t *scan_desc_host, int n_scans);
int csm_jpeg_decode_scan_desc_words(void);
int csm_jpeg_decode_progressive(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, const int32_t *scan_desc_host,
                                int n_scans, uint8_t *out, int64_t out_bytes, void *scratch, int *info_host, void *stream);

/* PNG files to uint8 B, G, R pixels (pngdec.hip; contract DESIGN.md §4.9, restated in tests/pngdec_restatement.py: the result
 * equals utils.io_utils.imread on every byte).  The host parses the chunks (cartoonsegmentation_amd/pngread.py) and hands over one
 * blob of device bytes and one descriptor per file; files of different sizes and colour types share a call.  8 bits per sample,
 * colour types 0, 2, 3, 4, 6, not interlaced; alpha is dropped, a palette is looked up.
 * desc_host: host int32 [n][csm_png_decode_desc_words() = 12]: [0] H, [1] W, [2] colour type, [3] [4] offset (a multiple of 16) and
 *   length of the file's zlib stream (the concatenated IDAT payloads, header and Adler-32 trailer included) in the blob, whose bytes
 *   reach to the stream's end rounded up to 16, [5] offset (a multiple of 16) of 768 palette bytes R, G, B in the blob (read for
 *   colour type 3 only; any valid offset otherwise), [6] 0, [7] [8] the byte offset of the file's pixels in out
 *   (low 31 bits, the bits above; a multiple of 4), the rest 0.  H * (1 + W * bytes per pixel) < 2^31.
 * out: u8, file i at its offset as [H][W][3].  blob, out and scratch are 16-byte aligned.
 * scratch: csm_png_decode_scratch_bytes(desc_host, n) device bytes (0 for invalid descriptors): per raw byte (scanlines with their
 *   filter bytes) 1 B of literals, 4 B of source positions and 8/3 B of match records, plus 8 B per 4096 raw bytes and 200 B per file.
 * csm_png_decode: info_host (may be NULL) receives [0] the pointer-doubling rounds launched, [1] the rounds that did work.  The call
 *   SYNCHRONISES the stream once, at the end (one error word per file, bits as in csrc/csm_inflate.h).  Returns CSM_ERR_DATA for a
 *   corrupt stream (invalid codes, distances or sizes, an Adler-32 that is not the one in the four bytes behind the deflate data, a filter type above 4; bytes behind that
 *   trailer are ignored, as zlib ignores them); whatever the data, no read or
 *   store leaves the file's own ranges.  No kernel waits on another workgroup; the output is deterministic. */
size_t csm_png_decode_scratch_bytes(const int32_t *desc_host, int n);
int csm_png_decode_desc_words(void);
int csm_png_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                   void *scratch, int *info_host, void *stream);

/* GIF files (GIF87a / GIF89a, animated or not) to uint8 B, G, R or B, G, R, A frames (gifdec.hip; contract DESIGN.md §4.17, restated
 * in tests/gifdec_restatement.py: frame i equals what Pillow shows after seek(i) on every byte).  The host parses the container
 * (cartoonsegmentation_amd/gifread.py) and hands over one blob of device bytes (every image's joined LZW sub-blocks and the colour
 * tables), one descriptor per image and one per file; files of different sizes and frame counts share a call.  A call does two
 * things, either of which may be empty: it decodes the LZW data of the images [first, first + count) into idx (1 byte per pixel,
 * stream order), and, when out is not NULL, composes every frame of every file from idx.  So a clip whose images do not fit the
 * scratch one wants to spend is decoded by several calls over groups of images, the last of which (or one more with count = 0)
 * passes out; idx is what stays between them.
 * desc_host: host int32 [n][csm_gif_decode_desc_words() = 16], the images of file 0, then of file 1, ...: [0] [1] height and width of
 *   the image's rectangle, [2] [3] its top and left on the logical screen, [4] [5] offset (a multiple of 16) and length of its LZW
 *   bytes in the blob, whose bytes reach to the stream's end rounded up to 16, [6] minimum code size (2 .. 8), [7] bit 0: interlaced,
 *   [8] transparent index or -1, [9] disposal (0 keep, 2 to background, 3 to previous), [10] offset (a multiple of 16) of the frame's
 *   colour table in the blob, 768 bytes R, G, B, zero-padded, [11] its entries (1 .. 256), [12] [13] the byte offset of the image's
 *   indices in idx (low 31 bits, the bits above; a multiple of 16; an image takes its pixels rounded up to 16), [14] its file, [15] 0.
 * file_desc_host: host int32 [n_files][16]: [0] [1] height and width of the logical screen, [2] [3] first image and image count,
 *   [4] [5] the byte offset of the file's frames in out (low 31 bits, the bits above; a multiple of 4), [6] background index,
 *   [7] bit 0: frame 0 declares a transparent index (the canvas carries alpha), the rest 0.
 * out: u8, file j at its offset as [frames][H][W][channels], channels 3 (B, G, R) or 4 (B, G, R, A).  blob, idx, out and scratch are
 *   16-byte aligned.
 * scratch: csm_gif_decode_scratch_bytes(...) device bytes (0 for invalid descriptors): per pixel of the group's images 4 B of source
 *   positions and 1 B of literals, plus 132 B per image of the group, 88 B per image and 32 B per file of the call.
 * csm_gif_decode: info_host (may be NULL) receives [0] the pointer-doubling rounds launched, [1] the rounds that did work.  With
 *   count > 0 the call SYNCHRONISES the stream once, at the end (one error word per image, bits as in csrc/csm_lzw.h), and returns
 *   CSM_ERR_DATA for corrupt LZW data (a code above the next free entry, a first code that is no literal, data or the end code
 *   before the rectangle is full; data behind a full rectangle are ignored); whatever the data, no read or store leaves the image's
 *   own ranges.  No kernel waits on another workgroup; the output is deterministic. */
size_t csm_gif_decode_scratch_bytes(const int32_t *desc_host, int n, const int32_t *file_desc_host, int n_files, int first, int count);
int csm_gif_decode_desc_words(void);
int csm_gif_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, const int32_t *file_desc_host, int n_files,
                   int first, int count, uint8_t *idx, int64_t idx_bytes, uint8_t *out, int64_t out_bytes, int channels,
                   void *scratch, int *info_host, void *stream);

/* Lossless WebP files (VP8L) to uint8 B, G, R or B, G, R, A pixels (webpdec.hip; contract DESIGN.md §4.15, restated in
 * tests/webpdec_restatement.py: the result equals what libwebp decodes on every byte).  The host parses the RIFF container
 * (cartoonsegmentation_amd/webpread.py) and hands over one blob of device bytes and one descriptor per file; files of different
 * sizes and features share a call.  Everything the format allows inside a stream is taken (the four transforms in any order, every
 * sub-image, a colour cache of 1 .. 11 bits, meta prefix codes, simple and normal codes, every backward reference), with one limit:
 * at most min(2600, ceil(W / 4) * ceil(H / 4)) prefix-code groups per file.
 * desc_host: host int32 [n][csm_webp_decode_desc_words() = 12]: [0] H, [1] W (each 1 .. 16384, as the five bytes of the VP8L header
 *   say), [2] the header's alpha flag (0 / 1), [3] the output channels (3: B, G, R; 4: B, G, R, A), [4] [5] offset (a multiple of
 *   16) and length of the VP8L chunk's payload in the blob, [6] 0, [7] [8] the byte offset of the file's pixels in out (low 31 bits,
 *   the bits above; a multiple of 4), the rest 0.
 * out: u8, file i at its offset as [H][W][channels]; A is 255 where the stream's own header says the file has no alpha.  blob, out
 *   and scratch are 16-byte aligned.
 * scratch: csm_webp_decode_scratch_bytes(desc_host, n) device bytes (0 for invalid descriptors), a function of the descriptors
 *   alone: per file 8 B per pixel (two ARGB buffers), 12 B per 4 x 4 block (the three sub-images), 1 KiB of palette, 8992 B per
 *   group up to the cap (count and direct tables of the five codes, their symbols in canonical order), and 200 B.
 * csm_webp_decode: info_host (may be NULL) receives n words, the error word of every file (bits as in csrc/csm_vp8l.h).  The call
 *   SYNCHRONISES the stream once, at the end.  Returns CSM_ERR_DATA for a corrupt stream (an invalid or over-subscribed code, a
 *   reference before the first or past the last pixel, a second transform of one type, cache bits outside 1 .. 11, a stream that
 *   ends early, a header that contradicts the descriptor).  A file with more groups than the cap is not corrupt: the call
 *   returns CSM_OK (unless another file is corrupt), bit 32 of that file's word is set and its pixels are not written.  Whatever the
 *   data, no read or store leaves the file's own ranges.  No kernel waits on another workgroup; the output is deterministic. */
size_t csm_webp_decode_scratch_bytes(const int32_t *desc_host, int n);
int csm_webp_decode_desc_words(void);
int csm_webp_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                    void *scratch, int *info_host, void *stream);

/* Lossy WebP files (a VP8 key frame, with or without an ALPH chunk) to uint8 B, G, R or B, G, R, A pixels (webplossy.hip; contract
 * DESIGN.md §4.16, restated in tests/webplossy_restatement.py: the result equals what libwebp decodes on every byte).  The host
 * parses the RIFF container (cartoonsegmentation_amd/webpread.py) and hands over one blob of device bytes and one descriptor per
 * file; files of different sizes and features share a call.  Everything a key frame can hold is taken: segmentation with map and
 * absolute or delta values, both loop filters with sharpness and filter deltas, 1 .. 8 token partitions, all six quantiser indices,
 * coefficient-probability updates, skipping on or off, the four whole-block and the ten sub-block modes.  An ALPH chunk may be raw
 * or a VP8L stream (then the lossless decoder's limit of prefix-code groups applies to it), with filter 0 .. 3.
 * desc_host: host int32 [n][csm_webp_lossy_decode_desc_words() = 12]: [0] H, [1] W (each 1 .. 16383, as the frame header says),
 *   [2] 1 if the file has an ALPH chunk, [3] the output channels (3: B, G, R; 4: B, G, R, A), [4] [5] offset (a multiple of 16) and
 *   length of the VP8 chunk's payload in the blob, [6] the first byte of the ALPH chunk (compression, filter, pre-processing),
 *   [7] [8] the byte offset of the file's pixels in out (low 31 bits, the bits above; a multiple of 4), [9] [10] offset (a multiple
 *   of 16) and length of the ALPH chunk's bytes behind its first, [11] 0.
 * out: u8, file i at its offset as [H][W][channels]; A is 255 where the file has no ALPH chunk.  With 3 channels the ALPH chunk is
 *   not looked at.  blob, out and scratch are 16-byte aligned.
 * scratch: csm_webp_lossy_decode_scratch_bytes(desc_host, n) device bytes (0 for invalid descriptors), a function of the
 *   descriptors alone: per macroblock 824 B (a 24-byte record, 25 x 16 int16 coefficients) and 384 B of planes, per macroblock
 *   column 13 B of contexts, with 4 channels and an ALPH chunk 1 B per pixel, and for ALPH chunks of compression 1 what
 *   csm_webp_decode takes for a file of that size.
 * csm_webp_lossy_decode: info_host (may be NULL) receives n words, the error word of every file (bits as in csrc/csm_vp8dec.h; from
 *   bit 8 up the error word of the alpha plane's VP8L stream, csrc/csm_vp8l.h).  The call SYNCHRONISES the stream once, at the end.
 *   Returns CSM_ERR_DATA for a corrupt file (a frame tag, start code or size that contradicts the descriptor, partition sizes that
 *   run past the chunk, a partition that ends early, a bad ALPH chunk).  An alpha stream with more groups than the cap is not
 *   corrupt: the call returns CSM_OK (unless another file is corrupt), bit 32 << 8 of that file's word is set and its alpha is not
 *   written.  Whatever the data, no read or store leaves the file's own ranges.  No kernel waits on another workgroup; the output
 *   is deterministic. */
size_t csm_webp_lossy_decode_scratch_bytes(const int32_t *desc_host, int n);
int csm_webp_lossy_decode_desc_words(void);
int csm_webp_lossy_decode(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes,
                          void *scratch, int *info_host, void *stream);

/* The device half of a GIF file (gif.hip; contract DESIGN.md §4.10, restated in tests/gif_restatement.py, byte-identical): one
 * 256-colour palette per clip and the LZW stream (minimum code size 8) of every frame.  1 <= H, W <= 65535.
 * csm_gif_histogram: frames u8 [pixels][3], contiguous; flags bit 0 = the channels are B, G, R in memory.  table device uint32
 *   [32768][4], zeroed by the call: per cell (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) the pixel count and the sums of r & 7,
 *   g & 7, b & 7.  pixels < 2^29, so no sum wraps.  The host cuts the palette from it (gifcode.build_palette).
 * csm_gif_map: frames u8 [n,H,W,3]; flags bit 0 as above, bit 1 = ordered dither (an 8x8 Bayer offset in [-4, 3] by (y & 7, x & 7),
 *   clamped); palette device u8 [256][3] R, G, B; indices u8 [n,H,W] = the entry nearest in squared distance over all 256 (the
 *   lowest index on ties); a pixel that equals an entry takes it whatever the dither.
 * csm_gif_measure: indices u8 [n,H,W], contiguous, n * ceil(H * W / 3839) < 2^24.  Every segment of 3839 pixels is coded by greedy
 *   LZW from a Clear code; bytes device int64 [n] receives the bytes of each frame's stream (at most
 *   (12 * (H * W + segments + 1) + 7) / 8).  scratch: csm_gif_scratch_bytes(n, H, W) device bytes (0 for an invalid shape), shared
 *   with the write call: 2 B per pixel for the codes and 12 B per segment, 16 B per frame.
 * csm_gif_write: out: out_bytes device bytes (a multiple of 4, 4-aligned), zeroed by the call; frame f's stream starts at the sum of
 *   the streams before it, each rounded up to 4 bytes: Clear, codes, ..., EOI, LSB-first, zero bits to the next byte.  Nothing is
 *   written at or past a stream's bytes rounded up to 4, nor past out_bytes.  Same n, H, W and scratch as the measure call.
 * Async on the stream, no allocation, no sync; the only atomics are integer adds (the table) and integer ORs of disjoint bits, so
 * the output is deterministic. */
size_t csm_gif_scratch_bytes(int n, int H, int W);
int csm_gif_histogram(const uint8_t *frames, int64_t pixels, int flags, uint32_t *table, void *stream);
int csm_gif_map(const uint8_t *frames, int n, int H, int W, int flags, const uint8_t *palette, uint8_t *indices, void *stream);
int csm_gif_measure(const uint8_t *indices, int n, int H, int W, int64_t *bytes, void *scratch, void *stream);
int csm_gif_write(int n, int H, int W, uint8_t *out, int64_t out_bytes, void *scratch, void *stream);

/* The device half of a WebP file (webp.hip; contract DESIGN.md §4.12, restated in tests/webp_restatement.py, byte-identical):
 * every frame as one VP8 key frame.  frames u8 [n,H,W,3] in B, G, R order, contiguous; 1 <= H, W <= 16383; quality 1..100;
 * n * (partitions + 1) < 2^20, partitions = min(8, the largest power of two not above the macroblock rows).
 * csm_webp_measure: colour conversion, the macroblock pass (one workgroup per frame) and the boolean coder (one lane per
 *   partition) into scratch.  info device int64 [n * (partitions + 1) + 1][2]: per frame the (offset in the blob, bytes) of its
 *   first partition and then of each token partition, in order; the last row is (status, total bytes), status != 0 if a partition
 *   met the end of its scratch segment (the segments are sized so that it cannot).  scratch: csm_webp_scratch_bytes(n, H, W)
 *   device bytes (0 for an invalid shape), shared with the write call: per macroblock 768 B of planes, 805 B of levels, modes and
 *   flags, and 6 672 B of token segment (7 bits for each of the 25 * 305 pairs a macroblock can code), plus the first partitions.
 * csm_webp_stage: one stage of csm_webp_measure alone, for timing (tools/time_webp.py): 1 colour, 2 macroblocks, 3 coder,
 *   4 sizes; csm_webp_measure is the four in order.
 * csm_webp_write: out: out_bytes device bytes; every partition's bytes at its offset, back to back.  Nothing is written past
 *   out_bytes.  Same n, H, W and scratch as the measure call.
 * The host adds the 10-byte frame header, the partition sizes and the RIFF chunks (webpcode.py).  Async on the stream, no
 * allocation, no sync, integer arithmetic only: the output is deterministic. */
size_t csm_webp_scratch_bytes(int n, int H, int W);
int csm_webp_stage(int stage, const uint8_t *frames, int n, int H, int W, int quality, int64_t *info, void *scratch, void *stream);
int csm_webp_measure(const uint8_t *frames, int n, int H, int W, int quality, int64_t *info, void *scratch, void *stream);
int csm_webp_write(int n, int H, int W, uint8_t *out, int64_t out_bytes, void *scratch, void *stream);
/* The same four calls with the coding method (contract DESIGN.md §4.12b, restated in tests/webp_m1_restatement.py, byte-identical).
 * method 0 is the calls above, the same kernels and the same bytes.  method 1 adds B_PRED macroblocks (ten 4x4 predictors by SSE,
 * 16x16 against B_PRED by an integer rate-distortion rule) and per-frame coefficient-probability updates: the macroblock pass walks
 * diagonals of slope two, stage 3 counts the frame's branch decisions (k_webp_stats), derives its probabilities (k_webp_probs) and
 * codes with them.  Any other method is CSM_ERR_ARG (scratch bytes 0).  The scratch of method 1 is larger: per macroblock 17 B of
 * sub-block modes and carried Y2 contexts, per frame 10.6 KB of counters and tables, and a first partition sized for 1056 updates
 * of 9 pairs and 117 pairs per macroblock; size it with csm_webp_scratch_bytes_m and pass the same method to every call of a chunk.
 * info, the status word and the guarded stores are those of method 0; still one host read of info per chunk. */
size_t csm_webp_scratch_bytes_m(int n, int H, int W, int method);
int csm_webp_stage_m(int stage, const uint8_t *frames, int n, int H, int W, int quality, int method, int64_t *info, void *scratch,
                     void *stream);
int csm_webp_measure_m(const uint8_t *frames, int n, int H, int W, int quality, int method, int64_t *info, void *scratch, void *stream);
int csm_webp_write_m(int n, int H, int W, int method, uint8_t *out, int64_t out_bytes, void *scratch, void *stream);

/* The VP8L payload of a lossless WebP file for n images of any sizes (webpll.hip; contract DESIGN.md §4.13, restated in
 * tests/webpll_restatement.py, byte-identical).  One descriptor per image, int64 [n][csm_webpll_desc_words() = 8]: [0] the device
 * address of its contiguous u8 pixels [H][W][channels], [1] H, [2] W (1..16384), [3] channels | flags << 8: 1 (grey), 3 (B, G, R) or
 * 4 (B, G, R, A; the header's alpha bit is set exactly then), flag bit 0 = grey bytes are a mask (any non-zero byte is written as
 * 255), [4..6] filled by csm_webpll_plan: the image's first residual pixel, first 16 x 16 block and first row unit in scratch
 * (a row unit is a row of the mode image or of the residual image), [7] 0.  The blocks and the row units of a call each stay
 * below 2^31 - 1.
 * csm_webpll_plan: checks desc_host, fills its words [4..7] and returns the device bytes of scratch the two calls share (0 for
 *   invalid descriptors or n < 1): 4 B per pixel, 4 B per block, 12 B per row unit.
 * csm_webpll_measure: desc_host and desc_dev (a device copy) as planned.  Subtract-green, the predictor mode of every block (the
 *   mode 0..12 with the smallest sum of min(r, 256 - r), ties to the lowest), the residuals, and table device uint32
 *   [2n][csm_webpll_measure_words() = 1088]: for the mode image (row 2i) and the residual image (row 2i + 1) of image i the counts
 *   of green and the 24 length prefixes [0..279], red [280..535], blue [536..791], alpha [792..1047], the 40 distance prefixes
 *   [1048..1087] of the row-wise run parse (four literals, then distance-1 references of up to 4096 pixels).
 * csm_webpll_write: host_table device uint32 [2n][csm_webpll_table_words() = 1352], filled by the host from the measured table:
 *   [0..1087] bit-reversed code | code length << 16 of every symbol (length 0: the one symbol of a simple code, no bits),
 *   [1088..1089] byte offset of the image's payload in out (low, high word; a multiple of 4), [1090] bytes of the payload,
 *   [1091..1092] the bit of the payload at which the plane's pixels begin, [1093] [1094] first 32-bit word and number of words of
 *   the header bits in front of them, [1095..1350] those words, shifted onto the payload's words.  out: out_bytes device bytes (a
 *   multiple of 4, 4-aligned), zeroed by the call.  Nothing is written at or past a payload's bytes rounded up to 4, nor past
 *   out_bytes.  Same descriptors and scratch as the measure call.
 * Async on the stream, no allocation, no sync; the only atomics are integer adds (counts) and integer ORs of disjoint bits, so
 * the output is deterministic. */
int csm_webpll_desc_words(void);
int csm_webpll_measure_words(void);
int csm_webpll_table_words(void);
size_t csm_webpll_plan(int64_t *desc_host, int n);
int csm_webpll_measure(const int64_t *desc_host, const int64_t *desc_dev, int n, uint32_t *table, void *scratch, void *stream);
int csm_webpll_write(const int64_t *desc_host, const int64_t *desc_dev, int n, const uint32_t *host_table, uint8_t *out,
                     int64_t out_bytes, void *scratch, void *stream);

/* Instance cut-outs with transparency (cutout.hip).
 * csm_mask_bbox: masks u8 / bool [n][H][W] (non-zero = set), H * W < 2^31 -> boxes int32 [n][4] = the tight x0, y0, x1, y1,
 *   end-exclusive; 0, 0, 0, 0 for an empty mask.  One workgroup per mask and band of 32 rows, integer min / max atomics.
 * csm_cutout_bgra: img u8 [H][W][3] (B, G, R); masks u8 / bool [n_masks][Hm][Wm] with Hm <= H <= Hm + 2 and Wm <= W <= Wm + 2 (the
 *   overlap is used: a pixel outside the mask is not set); alpha NULL or fp32 [H][W].  jobs: int64 [k][csm_cutout_job_words() = 8],
 *   on the host (checked) and a device copy (read by the kernel): [0] mask index, [1..4] the box x0, y0, x1, y1 inside the frame,
 *   not empty, [5] byte offset of the instance's [y1 - y0][x1 - x0][4] pixels B, G, R, A in out (a multiple of 4), [6] the pixels
 *   of the jobs before it, [7] 0.  A = 255 where the mask is set, or (uint8)(min(max(alpha, 0), 1) * 255.0f) (truncated) there
 *   with an alpha plane, 0 elsewhere; B = G = R = 0 wherever A = 0.  One launch over the pixels of all jobs. */
int csm_mask_bbox(const uint8_t *masks, int n, int H, int W, int32_t *boxes, void *stream);
int csm_cutout_job_words(void);
int csm_cutout_bgra(const uint8_t *img, int H, int W, const uint8_t *masks, int n_masks, int Hm, int Wm, const float *alpha,
                    const int64_t *jobs_host, const int64_t *jobs_dev, int k, uint8_t *out, int64_t out_bytes, void *stream);

/* Instance overlays: box outlines, alpha-blended masks and contours drawn over B, G, R frames (overlay.hip; DESIGN.md §4.14;
 * restated in tests/overlay_restatement.py, byte-identical).  One call draws a chunk of frames of any sizes.
 * jobs: int64 [n_jobs][csm_overlay_job_words() = 16], on the host (checked) and a device copy (read by the kernels): [0] [1] the
 *   device addresses of the frame u8 [H][W][3] and of the picture (same shape, another buffer), [2] of its masks u8 / bool
 *   [n_masks][H][W] (non-zero = set), [3] of its boxes int32 [n_masks][4] = x, y, w, h (device data, any values), [4] H, [5] W
 *   (H * W < 2^31 - 1), [6] n_masks, [7] k, the entries of its draw list, [8] its first entry in `entries`, [9] the line width
 *   t >= 1, [10..12] filled by csm_overlay_plan (its first 128 x 8 tile, tiles per row, tiles), [13..15] 0.  [2] and [3] may be 0 when k = 0.
 * entries: int32 [n_entries], host (checked: 0 <= entry < the job's n_masks) and device copy, the draw lists of all jobs; colors:
 *   device u8 [n_entries][3], the B, G, R of every entry.
 * flags: 1 boxes, 2 masks, 4 contours.  In list order: (1) for every entry the pixels inside
 *   [x - a, x + w + a] x [y - a, y + h + a] and not inside [x + b, x + w - b] x [y + b, y + h - b] (a = t / 2, b = t - a, bounds
 *   inclusive) take its colour; (2) in fp32, for every entry whose mask is set at the pixel, d = fl(fl(d * one_minus_alpha) +
 *   fl(alpha * c)), no fused multiply-add, then d is truncated to u8; (3) every mask pixel with a 4-neighbour outside the mask or
 *   the frame takes the entry's colour.  A frame with k = 0 is copied.
 * csm_overlay_plan: checks jobs_host, fills its words [10..15] and returns the tiles of the call (0 for an invalid table).
 * csm_draw_instances: one launch, a workgroup per tile, every tile walks its frame's whole draw list, so n and the overlap depth
 *   are unbounded and every mask byte is read once.  Mask rows are read as aligned 4-byte words that hold at least one byte of
 *   the row.  Async on the stream, no allocation, no scratch, no sync, no readback, no atomics: the output is deterministic. */
int csm_overlay_job_words(void);
int csm_overlay_plan(int64_t *jobs_host, int n_jobs, int n_entries);
int csm_draw_instances(const int64_t *jobs_host, const int64_t *jobs_dev, int n_jobs, const int32_t *entries_host,
                       const int32_t *entries_dev, const uint8_t *colors_dev, int n_entries, int flags, float alpha,
                       float one_minus_alpha, void *stream);

/* Detector input: mmdet test pipeline Resize(keep_ratio) + Pad(pad_value) + DetDataPreprocessor normalise
 * (call sites animeinsseg/__init__.py:63-76, :212-215, :395-399).  img u8 HWC [H,W,3] (BGR) -> fp32 NCHW
 * [1,3,S_h,S_w]; (rh,rw) resized extent (host computes mmcv rescale_size); mean3/std3 are HOST pointers. */
int csm_det_preprocess(const uint8_t *img_hwc, int H, int W, int rh, int rw, int S_h, int S_w, const float *mean3,
                       const float *std3, float pad_value, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * uint8 image plumbing around the depth net and the frame loop (OpenCV semantics restated, [EXT])
 * ---------------------------------------------------------------------------------- */

/* utils/io_utils.py:254-274 scaledown_maxsize (the frame itself: kenburns_effect.py:917): cv2.resize(INTER_LINEAR) of a uint8
 * HWC image [H,W,C] (C <= 4) to [h,w,C]; the host applies the size rule. */
int csm_resize_u8_linear(const uint8_t *src_hwc, int H, int W, int C, int h, int w, uint8_t *dst_hwc, void *stream);
/* the same for float32 images / masks (resize_pad(seg, ...) of prepare_refine_batch, animeinsseg/__init__.py:47): cv2's float
 * INTER_LINEAR -- horizontal then vertical linear pass in fp32 */
int csm_resize_f32_linear(const float *src_hwc, int H, int W, int C, int h, int w, float *dst_hwc, void *stream);
/* kenburns_effect.py:563-571 + depth_modules/leres/leres/depthmap.py:16-38: BGR u8 HWC [H,W,3] -> cv2 INTER_LINEAR to
 * (h,w) -> /255 -> RGB -> (x-mean)/std (ImageNet) -> fp32 NCHW [1,3,h,w] */
int csm_leres_input(const uint8_t *img_hwc, int H, int W, int h, int w, float *out, void *stream);
/* depth_modules/leres/__init__.py:121-145: min-max -> uint16 -> convertScaleAbs(255/65535) -> bitwise_not.
 * min_max_dev: DEVICE pointer to {min, max} of depth. */
int csm_leres_quantize(const float *depth, int64_t n, const float *min_max_dev, uint8_t *out, void *stream);
/* Small device-side reductions of the per-frame depth glue (no host sync; min / max are order-free, so results equal torch's).
 * csm_minmax: out2 = {min, max} of x[0..n) (x 16-byte aligned); scratch512 = 512 device floats (block partials).
 * csm_fill_zero_min_positive: leres/__init__.py:143-145 `depth[depth == 0] = depth[depth > 0].min()` in place (unchanged when
 *   there is no zero or no positive value); scratch2 = 2 uint32.
 * csm_normalise_disparity: out = (x / minmax[1]) * scale   (kenburns_effect.py:928: disparity / disparity.max() * baseline);
 *   norm_max_out (1 device float, may be NULL) receives max(out).
 * csm_depth_range_stats: out6 (float64, device) = {min, max of the NORMALISED disparity (from the raw {min,max} and scale),
 *   cv2.minMaxLoc(depth[y0:y0+crop_h, x0:x0+crop_w]) = min, max, first row-major argmin, argmax}; scratch2 = 2 uint64. */
int csm_minmax(const float *x, int64_t n, float *out2, float *scratch512, void *stream);
int csm_fill_zero_min_positive(float *x, int64_t n, unsigned *scratch2, void *stream);
int csm_normalise_disparity(const float *x, int64_t n, const float *minmax_dev, float scale, float *out, float *norm_max_out,
                            void *stream);
int csm_depth_range_stats(const float *minmax_raw_dev, float scale, const float *depth, int H, int W, int y0, int x0, int crop_h,
                          int crop_w, unsigned long long *scratch2, double *out6, void *stream);

/* depth_adjustment_animesseg for ONE instance, in place (kenburns_effect.py:68-78, the non-median branch): pixels of `mask`
 * (bool/uint8 [H,W]) take the maximum of disp*mask over the rows from round(top + 0.97 (bottom - top)) down; untouched when the
 * instance plane is empty.  scratch: 2*H + 2 floats (device).  No host sync. */
int csm_depth_adjust_instance(float *disp, const uint8_t *mask, int H, int W, float *scratch, void *stream);
/* The per-frame depth glue of B equally sized frames in ONE asynchronous call (no allocation, no synchronisation, no pointer
 * table in device memory: frames_hwc / coarse / masks / n_inst are HOST arrays of B entries, read before the call returns and
 * passed on by value in kernel arguments, 16 frames per launch).  Frame k gets exactly what the single-frame entry points give,
 * bit for bit (both compile the expressions of csrc/csm_glue.h):
 *   img_out       [B][stride3]  csm_u8_hwc_to_f32_chw of frames_hwc[k] (uint8 [H,W,3])
 *   (scratch)                   a private copy of coarse[k] (float [H,W]) after csm_depth_adjust_instance for the n_inst[k] masks of
 *                               masks[k] (uint8 / bool [n,H,W]) in instance order; n_inst[k] == 0: coarse[k] itself, masks[k] unused
 *   disp_out      [B][stride1]  csm_normalise_disparity(raw, csm_minmax(raw), baseline); nmax_out [B] its norm_max_out
 *   depth_out, valid_out [B][stride1], pts_out, unaltered_out [B][stride3]   csm_disparity_to_points(disp, nmax, focal, baseline, eps)
 *   stats_out     [B][6] float64  csm_depth_range_stats of the crop depth[128:H-128, 128:W-128] (so H, W > 256)
 * stride1 >= H*W and stride3 >= 3*H*W are the frame strides of the outputs in floats (a multiple of 4 keeps every frame 16-byte
 * aligned).  scratch: csm_frame_glue_scratch_bytes(B, H, W) bytes, 16-byte aligned, not shared by calls that may run concurrently. */
size_t csm_frame_glue_scratch_bytes(int B, int H, int W);
int csm_frame_glue_batch(int B, int H, int W, const uint8_t *const *frames_hwc, const float *const *coarse,
                         const uint8_t *const *masks, const int *n_inst, double focal, double baseline, float eps, float *img_out,
                         float *disp_out, float *depth_out, float *valid_out, float *pts_out, float *unaltered_out, int64_t stride1,
                         int64_t stride3, float *nmax_out, double *stats_out, void *scratch, void *stream);
/* The LeReS post-processing of B equally sized net outputs y [B,h,w] in ONE asynchronous call: per sample csm_minmax ->
 * csm_leres_quantize -> csm_resize_u8_to_f32 (h <= H; needs w <= W too) or csm_resize_u8_lanczos4_to_f32 (h > H) ->
 * csm_fill_zero_min_positive, bit for bit.  depth_out [B][out_stride] floats, out_stride >= H*W.
 * scratch: csm_leres_post_scratch_bytes(B, h, w) bytes, 8-byte aligned. */
size_t csm_leres_post_scratch_bytes(int B, int h, int w);
int csm_leres_post_batch(const float *y, int B, int h, int w, int H, int W, float *depth_out, int64_t out_stride, void *scratch,
                         void *stream);
/* kenburns_effect.py:572-575: cv2.resize(u8 depth, (W,H), INTER_AREA) (enlarging) -> float32 */
int csm_resize_u8_to_f32(const uint8_t *src, int h, int w, int H, int W, float *out, void *stream);
/* uint8 [H,W,3] -> float32 [3,H,W] * (1/255): the image tensor of kenburns_effect.py:878-880 (`permute(2,0,1)[None].float() * (1.0 / 255.0)`) */
int csm_u8_hwc_to_f32_chw(const uint8_t *src_hwc, int H, int W, float *out_chw, void *stream);
/* the same line when the 32-aligned LeReS map is larger than the frame (k > 1): cv2.resize(..., INTER_LANCZOS4) -> float32 */
int csm_resize_u8_lanczos4_to_f32(const uint8_t *src, int h, int w, int H, int W, float *out, void *stream);
/* kenburns_effect.py:1069-1070: cv2.getRectSubPix(frame,(patch_w,patch_h),center) + cv2.resize(INTER_LINEAR) to (W,H) */
int csm_crop_resize_u8(const uint8_t *frame_hwc, int H, int W, int patch_h, int patch_w, float center_x, float center_y,
                       uint8_t *out_hwc, void *stream);

/* ------------------------------------------------------------------------------------
 * Bokeh depth-of-field (utils/effects.py:12-181; kenburns_effect.py:1042-1067)
 * ---------------------------------------------------------------------------------- */
/* kernel_bokeh   utils/effects.py:16-74 : one depth-weighted `nsamples`-tap line blur along (dx,dy); img/out fp32 HWC
 * [H,W,3] (the reference kernel indexes raw HWC memory), depth fp32 [H,W] (already x 0.0005). */
int csm_bokeh_pass(const float *img_hwc, const float *depth, float *out_hwc, int H, int W, int nsamples, float dx, float dy,
                   void *stream);
/* (img/255)^lightness  utils/effects.py:155-156 ; n = H*W*3 */
int csm_bokeh_highlight(const uint8_t *img_hwc, float *out_hwc, int64_t n, float lightness, void *stream);
/* the third pass of bokeh_blur fused with its finish: out = uint8(((diag + pass(diag)) / 2)^(1/lightness) * 255), the same
 * operations in the same order as csm_bokeh_pass followed by csm_bokeh_finish (no float plane is written) */
int csm_bokeh_pass_finish(const float *diag_hwc, const float *depth, uint8_t *out_hwc_u8, int H, int W, int nsamples, float dx, float dy,
                          float lightness, void *stream);
/* ((diag+rhom)/2)^(1/lightness)*255 -> uint8  utils/effects.py:172,179-180 */
int csm_bokeh_finish(const float *diag_hwc, const float *rhom_hwc, uint8_t *out_hwc, int64_t n, float lightness, void *stream);
/* depth map of bokeh_blur  utils/effects.py:146-153,162-163: out = (1 - ((dmax - |d - focal|) - mn) / mx2) * 0.0005 ;
 * dmax = max(d), mn = min(dmax - |d-focal|), mx2 = max(that - mn) are scalar reductions supplied by the caller. */
int csm_bokeh_depth(const uint8_t *depth_u8, float *out, int64_t n, float dmax, float focal_plane, float mn, float mx2, void *stream);
/* The same map for the reference's own call forms (utils/effects.py:143-153 defaults: float depth, depth_factor = 2, focal_plane =
 * None): depth is float32 (is_u8 = 0, 16-B aligned) or uint8 (is_u8 = 1); has_focal selects `max(d) - |d - focal_plane|`;
 * depth_factor != 1 applies np.power (2 -> square, else powf).  tmp [n] floats, mm4 [4] floats and scratch512 [512] floats are
 * device scratch; all reductions stay on the device (no host sync). */
int csm_bokeh_depth_general(const void *depth, int is_u8, int64_t n, int has_focal, float focal_plane, float depth_factor,
                            float *tmp, float *mm4, float *scratch512, float *out, void *stream);
/* Focal plane of the depth of field (kenburns_effect.py:1045-1056): out[k] = np.median(values[masks[k] != 0]) for each of the n_inst
 * boolean masks [n_inst, n] (nan when the mask is empty), out[n_inst] = the largest of them, -1 if every mask is empty.  values
 * uint8 [n]; hist: n_inst * 256 uint32 of device scratch (zeroed by the call). */
int csm_masked_u8_median_max(const uint8_t *values, const uint8_t *masks, int n_inst, int64_t n, unsigned *hist, float *out, void *stream);
/* colorize(value, cmap='gray_r')[...,0]  depth_modules/zoedepth/utils/misc.py:97-135 (vmin/vmax = 2nd/85th percentile) */
int csm_colorize_gray_r(const float *value, uint8_t *out, int64_t n, float vmin, float vmax, void *stream);

/* The same three steps without host round trips (frametail.hip) -- the per-frame tail of kenburns_effect.py:1042-1067:
 * csm_percentile_pair: out2 (DEVICE) = {np.percentile(value, q_lo), np.percentile(value, q_hi)} (method 'linear'), exact, by a
 *   3-pass (16 + 8 + 8 bit) radix select instead of a sort, three launches; scratch = csm_percentile_scratch_bytes() device bytes, ZEROED
 *   ONCE by the caller (every call leaves the counting tables it needs next time cleared) and used by one stream at a time.  If a call
 *   finds the tables NOT in that state (e.g. after an aborted launch) its counts do not add up to n: out2 becomes NaN, for that call and
 *   every later one, until the caller zeroes the scratch again -- never a plausible wrong percentile.  NaN inputs are OUTSIDE the
 *   contract (the select orders the bit patterns, numpy propagates NaN); +-inf, +-0 and denormals are inside it.
 * csm_colorize_gray_r_dev: csm_colorize_gray_r with vmin / vmax read from device memory and the matplotlib byte LUT (256 HOST
 *   bytes, index -> grey level) applied in the kernel.
 * csm_bokeh_depth_auto: csm_bokeh_depth with dmax / mn / mx2 derived on the device from the histogram of depth_u8; scratch =
 *   csm_bokeh_depth_scratch_bytes() device bytes.
 * csm_colorize_stats: the frame loop's fused form of csm_colorize_gray_r_dev + the three scalars of csm_bokeh_depth_auto (one launch,
 *   the one csm_kenburns_frame makes): out_u8 as csm_colorize_gray_r_dev; scratch = csm_bokeh_depth_scratch_bytes() device bytes,
 *   ZEROED ONCE by the caller and used by one stream at a time: {dmax, mn, mx2} of out_u8 for focal_plane land in its first three
 *   floats, its ticket (+48) and per-XCD histograms (+64) are left zero by every call.
 * csm_bokeh_prep: the frame loop's fused form of csm_bokeh_depth + csm_bokeh_highlight (one launch): dm [n] from depth_u8 [n] and
 *   stats3_dev = {dmax, mn, mx2} in DEVICE memory, hi [3n] = (img_u8 [3n] / 255)^lightness. */
size_t csm_percentile_scratch_bytes(void);
int csm_percentile_pair(const float *value, int64_t n, double q_lo, double q_hi, float *out2, void *scratch, void *stream);
int csm_colorize_gray_r_dev(const float *value, uint8_t *out, int64_t n, const float *vmin_vmax_dev, const uint8_t *lut256_host,
                            void *stream);
size_t csm_bokeh_depth_scratch_bytes(void);
int csm_bokeh_depth_auto(const uint8_t *depth_u8, float *out, int64_t n, float focal_plane, void *scratch, void *stream);
int csm_colorize_stats(const float *value, uint8_t *out_u8, int64_t n, const float *vmin_vmax_dev, const uint8_t *lut256_host,
                       float focal_plane, void *scratch, void *stream);
int csm_bokeh_prep(const uint8_t *depth_u8, const uint8_t *img_u8, float *dm, float *hi, int64_t n, float focal_plane,
                   const float *stats3_dev, float lightness, void *stream);

/* One output frame of KenBurnsPipeline.process_kenburns (kenburns_effect.py:1027-1072) in ONE call: csm_warp_frame_tiled
 * [-> csm_percentile_pair(2, 85) -> csm_colorize_gray_r_dev -> csm_bokeh_depth_auto -> csm_bokeh_highlight -> 2 x csm_bokeh_pass ->
 * csm_bokeh_pass_finish, when dof != 0 (depth_field, depth_factor 1)] -> csm_crop_resize_u8 into out_hwc.  Same kernels, order and
 * arguments as the separate calls (bit-identical frames); it exists because the host side of a dozen calls per frame was the limit
 * of the frame loop.  warp_scratch as for csm_warp_frame_tiled; render [4,H,W] is required when dof; frame_u8 [H,W,3] receives the
 * un-cropped warp; tail_scratch: csm_kenburns_frame_scratch_bytes(H, W) bytes, zeroed ONCE by the caller (tickets and counting tables: every call leaves them cleared). */
size_t csm_kenburns_frame_scratch_bytes(int H, int W);
int csm_kenburns_frame(const float *pts, const float *rgb, const float *depth, int64_t N, int H, int W, double focal, double baseline,
                       float sx, float sy, float sz, void *warp_scratch, float *render, uint8_t *frame_u8, int dof, float focal_plane,
                       int num_samples, float lightness, const uint8_t *gray_r_lut256_host, void *tail_scratch, int patch_h, int patch_w,
                       float center_x, float center_y, uint8_t *out_hwc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CSM355_H */
