// csm_convcfg.h -- what the convolution kernel files (conv_mfma.hip, conv_dma.hip, conv_patch.hip, netops.hip) share with each other and
// with the executor / tuner in nets.hip: the tile-configuration ids and table rows, the eligibility predicates, a few constants.
#pragma once
#include "csm_conv.h"
#include <span>
#include <utility>

#ifndef CSM_ILV
#define CSM_ILV 1        // persistent conv kernels: DMA pieces interleaved with the MFMA groups (0 = burst behind the barrier; A/B builds)
#endif

#ifdef CSM_CONV_ABLATE
#define CSM_DBG(a) ((a).dbg)          // tuning build only (make ABLATE=1): phases can be switched off at run time
#else
#define CSM_DBG(a) 0
#endif

namespace csmconv {

constexpr int kLdsLd = 36;  // floats per LDS row: 32 + 4 pad (conflict-free b128 reads, see MI355X LDS notes)

typedef float f32x4v __attribute__((ext_vector_type(4)));

// ---- tile configurations ----------------------------------------------------------------------------------
// An id is persisted (tile-cache files, csm_op.tile = id + 1 in its low 6 bits): ids are never renumbered.  Everything else about a
// configuration -- name, kernel family, output-channel width, launcher -- is its ConvCfg row, defined in the family's file next to the
// instantiation it launches; nets.hip indexes the rows by id and decides by FAMILY, never by the order of the ids.
enum { CFG_128x128_4w = 0, CFG_128x64 = 1, CFG_64x64 = 2, CFG_128x128_8w = 3, CFG_128x32 = 4, CFG_64x16 = 5,
       // LDS-DMA kernel (k_conv_dma)
       CFG_D64x64 = 6, CFG_D128x64 = 7, CFG_D128x128 = 8, CFG_D128x128_8w = 9, CFG_D256x128_8w = 10, CFG_D64x128 = 11, CFG_D128x32 = 12,
       CFG_NARROW = 13,   // k_conv_narrow (cout <= 4)
       // odd tile heights (1x4 waves, wave tile 32*TM x 32): more block counts for the tuner to dodge grid quantisation with
       CFG_D96x128 = 14, CFG_D160x128 = 15, CFG_D224x128 = 16, CFG_D192x128 = 17,
       // 3x3 patch re-use kernel (k_conv_patch); _w8 = 8-pixel-wide output tiles for small maps
       CFG_P64x64 = 18, CFG_P128x64 = 19, CFG_P64x128 = 20, CFG_P128x128 = 21, CFG_P256x128 = 22, CFG_P128x32 = 23,
       CFG_P64x64_w8 = 24, CFG_P128x128_w8 = 25, CFG_P128x32_w8 = 26, CFG_P128x128_8w = 27,
       // three LDS stages (loads two chunks ahead) and 256 x 64 tiles (N = 64 layers: the B tile is shared by four 64 x 64 wave tiles)
       CFG_D64x64_s3 = 28, CFG_D128x64_s3 = 29, CFG_D64x128_s3 = 30, CFG_D128x128_s3 = 31, CFG_D128x128_8w_s3 = 32,
       CFG_D256x128_8w_s3 = 33, CFG_D256x64 = 34, CFG_D256x64_s3 = 35, CFG_P256x64 = 36, CFG_D64x64_s4 = 37,
       // persistent blocks, loader one chunk ahead across tile boundaries (k_conv_dma_p); ksplit == 1 layers
       CFG_Q64x64 = 38, CFG_Q128x64 = 39, CFG_Q64x128 = 40, CFG_Q128x128_8w = 41, CFG_Q128x32 = 42,
       // persistent patch kernel (k_conv_patch_p): the next tile's patch is fetched during the current tile's taps
       CFG_R128x32 = 43, CFG_R64x64 = 44, CFG_R128x64 = 45, CFG_R128x32_w8 = 46, CFG_R128x128_8w = 47, CFG_R64x128 = 48, CFG_R64x64_w8 = 49,
       // the 8-wave persistent patch tile capped at 128 VGPRs: two blocks per CU
       CFG_R128x128_8w_o4 = 50,
       // weights-stationary 3x3 (k_conv_ws): 16 x 16 pixel tiles x 32 / 64 output channels, the column tile's whole weight panel in LDS
       CFG_W256x32 = 51, CFG_W256x64 = 52,
       CFG_COUNT = 53 };

enum ConvFamily {
    FAM_MFMA,       // k_conv_mfma: register-staged, any channel count
    FAM_DMA,        // k_conv_dma: LDS-DMA, one tile per block
    FAM_PATCH,      // k_conv_patch: 3x3 stride 1 with the input patch kept in LDS
    FAM_DMA_P,      // k_conv_dma_p: persistent k_conv_dma
    FAM_PATCH_P,    // k_conv_patch_p: persistent k_conv_patch
    FAM_WS,         // k_conv_ws: weights-stationary 3x3
    FAM_NARROW,     // k_conv_narrow: cout <= 4 on the vector pipe
    FAM_COUNT
};
constexpr bool fam_uses_dma(int f) { return f != FAM_MFMA && f != FAM_NARROW; }                  // operands reach LDS by buffer_load ... lds
constexpr bool fam_needs_patch(int f) { return f == FAM_PATCH || f == FAM_PATCH_P || f == FAM_WS; }   // 3x3, stride 1, dilation 1 only
constexpr bool fam_persistent(int f) { return f == FAM_DMA_P || f == FAM_PATCH_P || f == FAM_WS; }    // a block walks several tiles; split K serially only

struct ConvCfg {
    int id;
    const char *name;      // the enum spelling without CFG_
    int family;
    int bn;                // output channels per tile
    int (*launch)(const ConvArgs &, hipStream_t);
};
// the rows each family file defines (every id 0 .. CFG_COUNT - 1 in exactly one of them: checked at first use in nets.hip)
std::span<const ConvCfg> conv_cfgs_mfma();      // conv_mfma.hip
std::span<const ConvCfg> conv_cfgs_dma();       // conv_dma.hip: FAM_DMA, FAM_DMA_P
std::span<const ConvCfg> conv_cfgs_patch();     // conv_patch.hip: FAM_PATCH, FAM_PATCH_P, FAM_WS
std::span<const ConvCfg> conv_cfgs_narrow();    // netops.hip

// ---- eligibility (host): which layers a family can run ---------------------------------------------------------
bool dma_eligible(const ConvArgs &a);           // conv_dma.hip
bool patch_eligible(const ConvArgs &a);         // conv_patch.hip
bool narrow_eligible(const ConvArgs &a);        // netops.hip
constexpr int kWsPatchBytes = 2 * (((16 + 2) * (16 + 2) + 7) / 8 + 1) * 1024;      // two patch stages of k_conv_ws
bool ws_fits(const ConvArgs &a, int BN);        // conv_patch.hip

// ---- pieces of a launch that more than one family uses ------------------------------------------------------------
extern int g_ngroup_enable;                     // nets.hip; csm_debug_conv_tuner_options bit 1 clears it (A/B measurements)
int choose_ngroup(const ConvArgs &a, int BN);   // conv_dma.hip
int launch_reduce(const ConvArgs &a, hipStream_t st);   // netops.hip: k_splitk_reduce behind a parallel split-K launch

// ---- the layer kernels that are not implicit GEMMs (netops.hip) ---------------------------------------------------
int launch_conv_stem(const ConvArgs &a, hipStream_t st);
// dwconv, maxpool, bilinear, nearest, eltwise, attractor, logbinom, gavgpool and the layout transposes; any other kind is an error
int launch_netop(const csm_op &op, int i, const View &in, const View &in1, const View &out, const float *weights, hipStream_t st);

}  // namespace csmconv
