// csm_tokens.h -- launchers of tokens.hip (transformer ops of the layer-program executor), called from run_ops in nets.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace csm {
int launch_layernorm(const float *in, int in_ld, float *out, int out_ld, int64_t rows, int c, const float *gamma, const float *beta,
                     const float *eps /* device pointer */, hipStream_t st);
int launch_attention(const float *qkv, int ld, float *out, int out_ld, int n, int N, int heads, int d, const float *table, int gh, int gw,
                     hipStream_t st);
int launch_tokens(int mode, const float *in, int in_ld, float *out, int out_ld, int n, int np, int c, const float *cls, hipStream_t st);
int launch_depth_to_space(const float *in, int in_ld, float *out, int out_ld, int n, int h, int w, int k, int c, hipStream_t st);
// sam.hip
int launch_attention_relpos(const float *qkv, int ld, float *out, int out_ld, int n, int N, int heads, int d, const float *table, int gh, int gw,
                            hipStream_t st);
int launch_window(int unpart, const float *in, int in_ld, const float *res, int res_ld, float *out, int out_ld, int n, int gh, int gw, int ws, int c,
                  hipStream_t st);
int launch_bcast_add(const float *a, int a_ld, int n0, const float *b, int b_ld, int n1, float *out, int out_ld, int n, int64_t np, int c, const float *aux,
                     int aux_map, hipStream_t st);
int launch_channel_dot(const float *in, int in_ld, const float *h, int h_ld, float *out, int out_ld, int n, int64_t np, int c, hipStream_t st);
int launch_cross_attention(const float *q, int q_ld, const float *kv, int kv_ld, float *out, int out_ld, int n, int Nq, int Nk, int heads, int d,
                           hipStream_t st);
}  // namespace csm
