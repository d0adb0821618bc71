// Functions one translation unit of liblgm_hip.so defines and another calls (C++ linkage, not part of the C-ABI), each
// declared ONCE, default arguments included: lgm_common.h includes this file, so the defining file sees the declaration too
// and a changed signature is a compile error instead of a call that links and misbehaves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lgm_hip.h"

// ---- conv3x3.hip: specialised 3x3 / stride 1 / pad 1 kernels, the fixed-order split-K reducer ----
bool lgm_conv3x3_supported(const LgmConvGeom* g, int gather_channels, int out_channels);
int lgm_conv3x3_splits(const LgmConvGeom* g, int gather_channels, int out_channels);
int lgm_conv3x3_launch(int mode, const LgmConvGeom* g, const float* a, long a_pitch, const float* w, const float* bias,
                       const float* res, long res_pitch, float* out, long out_pitch, void* workspace, long workspace_bytes,
                       hipStream_t s);
int lgm_splitk_reduce_launch(const float* ws, long ws_stride, int splits, const float* bias, const float* res,
                             long res_pitch, float* out, long out_pitch, long M, int N, hipStream_t s);
bool lgm_wgrad3x3_supported(const LgmConvGeom* g);
void lgm_wgrad3x3_plan(const LgmConvGeom* g, int* splits, int* tps, int* total_ts);
int lgm_wgrad3x3_launch(const LgmConvGeom* g, const float* y, long y_pitch, const float* x, long x_pitch, float* out,
                        float* bias_out, float beta, long slab, int splits, int tps, int total_ts, hipStream_t s);

// ---- conv_igemm.hip: the single-layer weight-gradient slab reducer ----
int lgm_wgrad_reduce_launch(const float* ws, long slab, float* gw, long n_w, float* gb, long n_b, int splits, float beta,
                            hipStream_t s);

// ---- wgrad1x1.hip ----
bool lgm_wgrad1x1_supported(const LgmConvGeom* g, long y_pitch, long x_pitch);
void lgm_wgrad1x1_plan(const LgmConvGeom* g, int* splits, int* chunks_per_split);
int lgm_wgrad1x1_launch(const LgmConvGeom* g, const float* y, long y_pitch, const float* x, long x_pitch, float* out,
                        float* bias_out, float beta, long slab, int splits, int chunks_per_split, hipStream_t s);

// ---- gemm_stream.hip: 1x1 convolutions with a resident weight slice, X streamed ----
bool lgm_gemm_stream_supported(long M, int N, int K, long x_pitch, long out_pitch, long res_pitch);
int lgm_gemm_stream_launch(const float* x, long x_pitch, const float* w, const float* bias, const float* res,
                           long res_pitch, float* out, long out_pitch, long M, int N, int K, hipStream_t s);
// ---- gemm_rows.hip: short-reduction 1x1 convolutions with a resident activation tile ----
bool lgm_gemm_rows_supported(long M, int N, int K);
int lgm_gemm_rows_launch(const float* x, long x_pitch, const float* w, const float* bias, const float* res,
                         long res_pitch, float* out, long out_pitch, long M, int N, int K, hipStream_t s);

// ---- winograd.hip: F(2x2,3x3) convolution, weight gradient (always through slabs + the fixed-order reducer) and the
// backward pair (input gradient + weight gradient in ONE launch) ----
bool lgm_wino_supported(const LgmConvGeom* g, int gather_channels, int out_channels);
int lgm_wino_splits(const LgmConvGeom* g, int gather_channels, int out_channels, bool fused = false);
// partial (optional, int64 x 2): the caller's consumer sums the split-K planes itself; receives (splits, plane stride)
int lgm_wino_launch(const LgmConvGeom* g, int yx, const float* a, long a_pitch, const float* u, const float* bias,
                    const float* res, long res_pitch, float* out, long out_pitch, void* workspace, long workspace_bytes,
                    hipStream_t s, int64_t* partial = nullptr);
bool lgm_wino_wgrad_supported(const LgmConvGeom* g);
void lgm_wino_wgrad_plan(const LgmConvGeom* g, int* splits, int* cps, int* total_chunks);
int lgm_wino_wgrad_launch(const LgmConvGeom* g, const float* y, long y_pitch, const float* x, long x_pitch, float* out,
                          int bias, long slab, int splits, int cps, int total_chunks, hipStream_t s);
struct WinoPairPlan {
  int csplits, wsplits, cps, total_chunks;
};
WinoPairPlan lgm_wino_pair_plan(const LgmConvGeom* g, bool fused);
int lgm_wino_pair_launch(const LgmConvGeom* g, const float* gy, long gy_pitch, const float* x, long x_pitch,
                         const float* u_b, const float* res, long res_pitch, float* gx, long gx_pitch, void* dws,
                         long dws_bytes, int64_t* partial, float* slabs, int bias, long slab, hipStream_t s);

// ---- winograd4.hip: F(4x4,3x3) convolution; picks the workgroup form (32-tile here, light in winograd4l.hip) per launch ----
bool lgm_wino4_supported(const LgmConvGeom* g, int gather_channels, int out_channels);
int lgm_wino4_pick_splits(long base, long slots, int phases, int smax, int min_pps);
int lgm_wino4_splits(const LgmConvGeom* g, int gather_channels, int out_channels);
// partial: as lgm_wino_launch; stats: the GroupNorm statistics rows of lgm_conv3x3_wino4_stats
int lgm_wino4_launch(const LgmConvGeom* g, int yx, const float* a, long a_pitch, const float* u, const float* bias,
                     const float* res, long res_pitch, float* out, long out_pitch, void* workspace, long workspace_bytes,
                     hipStream_t s, int64_t* partial = nullptr, float* stats = nullptr);
// ---- winograd4l.hip: the light workgroups (same operands, 16-tile units, 256 threads) ----
bool lgm_wino4l_supported(const LgmConvGeom* g, int gather_channels, int out_channels);
long lgm_wino4l_units(const LgmConvGeom* g, int out_channels);
int lgm_wino4l_stats_parts(const LgmConvGeom* g);
int lgm_wino4l_class(const LgmConvGeom* g);
int lgm_wino4l_splits(const LgmConvGeom* g, int gather_channels, int out_channels);
int lgm_wino4l_launch(const LgmConvGeom* g, int yx, const float* a, long a_pitch, const float* u, const float* bias,
                      const float* res, long res_pitch, float* out, long out_pitch, void* workspace, long workspace_bytes,
                      hipStream_t s, int64_t* partial, float* stats);

// ---- winograd4_wgrad.hip: F(4x4,3x3) weight gradient of the large-map layers, alone or several layers to a launch ----
bool lgm_wino4_wgrad_supported(const LgmConvGeom* g);
bool lgm_wino4_wgrad_use(const LgmConvGeom* g);
void lgm_wino4_wgrad_plan(const LgmConvGeom* g, long budget, int* splits, int* gps, int* total_groups);
int lgm_wino4_wgrad_launch(const LgmConvGeom* g, const float* y, long y_pitch, const float* x, long x_pitch, float* out,
                           int bias, long slab, int splits, int gps, int total, hipStream_t s);
int lgm_wino4_wgradn_launch(int n, const LgmConvGeom* const* gs, const float* const* ys, const long* yps,
                            const float* const* xs, const long* xps, float* const* outs, const int* biases,
                            const long* slabs, const int* splits, const int* gpss, const int* totals, hipStream_t s);

// ---- linattn_mfma.hip, linattn_fused.hip, attention_tiled.hip: the launchers behind attention.hip's entry points ----
int lgm_linattn_ctx_launch(int mode, const float* qkv, long pitch, const float* mem_kv, const float* gout,
                           long gout_pitch, const float* ctx_in, int B, int n, int heads, int M, float scale,
                           float* ctx_out, float* kmax, float* ksum, float* r_out, hipStream_t s,
                           const float* kmax_in = nullptr, const float* ksum_in = nullptr, float* gmem_partial = nullptr);
int lgm_linattn_bwd_launch(const float* qkv, long pitch, const float* mem_kv, const float* gout, long gout_pitch,
                           const float* ctx, const float* gctx, const float* kmax, const float* ksum, const float* rvec,
                           int B, int n, int heads, int M, float scale, float* gqkv, long gq_pitch, float* gmem_partial,
                           hipStream_t s);
int lgm_linattn_bwd_fused_launch(const float* qkv, long pitch, const float* gout, long gout_pitch, const float* ctx,
                                 const float* gctx, const float* kmax, const float* ksum, const float* rvec,
                                 const float* xn, long xn_pitch, const float* wt, int B, int n, float scale, float* gxn,
                                 long gxn_pitch, float* slabs, int* blocks_out, hipStream_t s);
int lgm_linattn_out_fused_launch(const float* qkv, long pitch, const float* ctx, const float* wout, const float* bout,
                                 const float* g, const float* x, long x_pitch, float* ao, long ao_pitch, float* o2,
                                 long o2_pitch, float* y, long y_pitch, int B, int n, int Cout, float scale, hipStream_t s);
int lgm_attn_tiled_fwd_launch(const float* qkv, long pitch, const float* mem_kv, int B, int n, int heads, int M,
                              float scale, float* out, long out_pitch, float* lse, hipStream_t s);
int lgm_attn_tiled_bwd_launch(const float* qkv, long pitch, const float* mem_kv, const float* out, long out_pitch,
                              const float* gout, long gout_pitch, const float* lse, int B, int n, int heads, int M,
                              float scale, float* gqkv, long gq_pitch, float* gmem_partial, hipStream_t s);
