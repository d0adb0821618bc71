/* liblgm_hip.so — C-ABI of the MI355X (gfx950) hot path for lightning-generative-models.
 *
 * The reference (pure Python, /root/reference) has no FFI: every entry point below replaces
 * a group of ATen calls that the reference's nn.Modules issue on the hot path.  Each entry
 * cites the reference lines whose arithmetic it implements.  SURVEY.md §8(b) defines the
 * conventions:
 *   - plain pointers + sizes, no torch types; all device pointers are caller-owned;
 *   - the library never allocates, frees, retains or synchronises; all work is enqueued on
 *     the `stream` argument (a hipStream_t passed as void*);
 *   - return 0 = OK, <0 = invalid argument / unsupported shape, >0 = hipError_t;
 *     lgm_last_error() returns a thread-local description;
 *   - re-entrant per THREAD (safe from the autograd thread next to the main thread): an entry point keeps no state
 *     between calls.  What the library does hold, exactly:
 *       . thread-local: the last error string, the last kernel name (lgm_last_error / lgm_last_kernel) and the
 *         weight-gradient queue a caller switches on itself (lgm_wgrad_queue_enable, below).  What ONE call asks of its
 *         launch sites - a post-op, the record in which lgm_conv_bwd_pair[_post]'s own input-gradient and weight-gradient
 *         dispatchers record instead of launching - lives on that call's stack and travels as an argument;
 *       . process-wide, written once: hipFuncSetAttribute one-shot flags per kernel (idempotent: a race sets the same
 *         attribute twice) and `static const` switches read from the environment on first use;
 *       . process-wide, diagnostics only: the cycle-stamp buffers of lgm_wino_set_debug_buffer /
 *         lgm_wino4_set_debug_buffer (NULL on the product path; a tool sets and clears them around its own launches,
 *         single-threaded).
 *     Callers that launch from several threads at once need no lock.
 *
 * Activation layout: NHWC fp32, addressed as (pointer, pitch) where pitch is the distance
 * in floats between consecutive pixels (>= channels; lets a tensor be a channel-slice of a
 * wider concat buffer).  Pointers and pitches of tensors read through the implicit-GEMM
 * convolutions must be 16-byte aligned / multiples of 4 floats.
 *
 * Convolution weights: physical layout [Nw][KH*KW][Cw] (= torch channels_last memory format
 * of the logical OIHW Conv2d weight; for ConvTranspose2d Nw = in_channels, Cw = out_channels).
 */
#ifndef LGM_HIP_H
#define LGM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_ABI_VERSION 8   /* 2: lgm_posemb takes a frequency table, BatchNorm entry points, *_planes / *_partial;
                             * 3: lgm_conv3x3_wino4*, lgm_gn_fwd_stats, lgm_conv3x3_wino_wgradn* + LgmWgradItem, a negative
                             *    dst offset in lgm_wino_weights table rows means "skip that copy", lgm_kernel_name*;
                             * 4: LgmPostOp carries the BatchNorm-backward sums (bn_*), lgm_bn_reduce3_coef_tiles;
                             * 5: lgm_set_cu_margin / lgm_cu_margin;
                             * 6: lgm_extract_axpby, lgm_model_predictions (GaussianDiffusion's per-sample-time algebra), lgm_time_mlp_*, lgm_weng_*;
                             * 7: lgm_gn_bwd_add, lgm_wgrad1x1_group*, lgm_wgrad_queue_*;
                             * 8: lgm_adam_step / lgm_rmsprop_step take their betas / alpha as doubles
                             * (entry points added since without a change to an existing one keep the number, as the
                             *  lgm_*_obj ones did: lgm_selfcond_estimate, lgm_qsample_target_slice, lgm_sample_step_slice,
                             *  lgm_sample_step_table_slice, lgm_label_emb_fwd, lgm_label_emb_wgrad, lgm_cfg_mix, lgm_dpm_step, lgm_dpm_step_table,
                             *  lgm_dyn_thresh, lgm_sample_step_thresh, lgm_dpm_step_thresh, lgm_model_predictions_thresh,
                             *  lgm_sample_step_inpaint, lgm_dpm_step_inpaint, lgm_vlb_term, lgm_vlb_term_table,
                             *  lgm_grad_sqnorm_*, lgm_grad_clip_scale, lgm_adam_step_scaled, lgm_grad_accumulate, lgm_hybrid_loss_fwd,
                             *  lgm_hybrid_loss_bwd, lgm_sample_step_learned, lgm_sample_step_table_learned, lgm_vlb_term_learned, lgm_gn_plan,
                             *  lgm_tsampler_draw, lgm_tsampler_update, lgm_weighted_mse_fwd_iw / _bwd_iw, lgm_hybrid_loss_fwd_iw / _bwd_iw,
                             *  lgm_lowres_cond, lgm_lowres_emb_fwd, lgm_sample_step_extent, lgm_dpm_step_extent,
                             *  lgm_distill_half_step, lgm_distill_target, lgm_slerp, lgm_slerp_span, lgm_slerp_partials,
                             *  lgm_edm_qsample, lgm_edm_qsample_sigma, lgm_edm_pre, lgm_edm_euler, lgm_edm_heun, lgm_fourier_emb_fwd,
                             *  lgm_fourier_emb_bwd, lgm_mconv_xy, lgm_mconv_yx, lgm_mconv_wgrad, lgm_mconv_wgrad_workspace, lgm_mconv_zero_dead, lgm_gated_fwd, lgm_gated_bwd,
                             *  lgm_softmax_xent_fwd, lgm_softmax_xent_bwd, lgm_pixelcnn_step, lgm_pixelcnn_step_workspace,
                             *  lgm_categorical_draw
                             *  - a library that lacks a declared symbol fails to load) */
#define LGM_OK 0
#define LGM_ERR_INVALID (-1)
#define LGM_ERR_UNSUPPORTED (-2)

int lgm_abi_version(void);
const char* lgm_last_error(void);
/* diagnostic: name (as rocprofv3 prints it, without the argument list) of the primary kernel launched by the calling
 * thread's last convolution-family call (lgm_conv_xy / _yx / _wgrad / lgm_conv3x3_wino) or norm call (lgm_gn_* name the
 * statistics / one-pass kernel of their plan, lgm_rmsnorm_* their instantiation) */
const char* lgm_last_kernel(void);
/* diagnostic: every name lgm_last_kernel() can ever return (one entry per site in the library that notes a name, in link
 * order; duplicates possible).  Each is a prefix of the demangled name of a kernel in liblgm_hip.so - checked on the CPU by
 * tests/test_cabi.py, so that bench.py's per-kernel attribution and the rocprofv3 rows under profiles/ cannot drift apart. */
int lgm_kernel_name_count(void);
const char* lgm_kernel_name(int i);

/* ---------------------------------------------------------------------------------------
 * Convolution family (implicit GEMM on v_mfma_f32_32x32x2_f32, exact fp32).
 * Geometry is always that of the equivalent *forward convolution* X -> Y:
 *   X side: [B, H, W, Cw]   Y side: [B, Ho, Wo, Nw]   weight [Nw][KH*KW][Cw]
 *   Y[b,oh,ow,n] = sum_{kh,kw,c} X[b, oh*stride-pad+kh, ow*stride-pad+kw, c] * Wt[n][kh*KW+kw][c]
 * Replaces: nn.Conv2d / nn.ConvTranspose2d forward+backward at
 *   ddpm.py:96,103,160,187,213,215,252,253,304,377,413,422 (UNet),
 *   dcgan.py:79-87,150-158 (DCGAN G/D), vqvae.py:36-51,74-85, residual.py:14-18.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t B, H, W, Cw;    /* X side */
  int32_t Ho, Wo, Nw;     /* Y side */
  int32_t KH, KW, stride, pad;
} LgmConvGeom;

/* X -> Y  (Conv2d.forward; ConvTranspose2d input-gradient).
 * y = conv(x, w) + bias[n] + res   (bias, res optional = NULL; res may alias y). */
int lgm_conv_xy(const LgmConvGeom* g, const float* x, int64_t x_pitch, const float* w,
                const float* bias, const float* res, int64_t res_pitch,
                float* y, int64_t y_pitch, void* workspace, int64_t workspace_bytes, void* stream);

/* Y -> X  (Conv2d input-gradient; ConvTranspose2d.forward).
 * x = conv_transpose(y, w) + bias[c] + res   (bias, res optional; res may alias x). */
int lgm_conv_yx(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* w,
                const float* w_t, const float* bias, const float* res, int64_t res_pitch,
                float* x, int64_t x_pitch, void* workspace, int64_t workspace_bytes, void* stream);
/* w_t (optional): the same weights transposed to [Cw][KH*KW][Nw]; when given, the 3x3 input-gradient
 * kernel reads its weight fragments with the same 16-byte loads as the forward pass.
 * lgm_transpose_weights refreshes such copies for a whole flat parameter buffer in ONE launch:
 * table rows = (offset, Nw, T, Cw, first_block); dst uses the same offsets as src. */
int lgm_transpose_weights(const float* src, float* dst, const int32_t* table, int n_layers,
                          int total_blocks, void* stream);

/* Optional workspace (bytes) for lgm_conv_xy (yx = 0) / lgm_conv_yx (yx = 1): small-image 3x3
 * layers split the reduction over workgroups and combine the partials in a fixed order.
 * Passing NULL / too few bytes is legal (no split, slower on tiny feature maps). */
int64_t lgm_conv_workspace(const LgmConvGeom* g, int yx);

/* Post-op of a convolution's epilogue: out = act(conv + bias + res), then - backward passes - the ReLU / LeakyReLU
 * mask of a SAVED activation m (its forward output): out *= (m > 0 ? 1 : mask_slope).  Replaces the separate
 * activation launches around the reference's Conv2d -> ReLU pairs (vqvae.py:36-51,74-85, residual.py:14-20) and
 * their autograd mirror images.  act: 0 none, 3 ReLU, 4 LeakyReLU(slope); mask NULL: none.  Applied inside the
 * implicit-GEMM kernels' epilogue / split-K reducer; paths without an epilogue hook finish with one elementwise
 * launch - the result is the same on every path. */
typedef struct {
  int32_t act;
  float slope;
  const float* mask;
  int64_t mask_pitch;
  float mask_slope;
  /* ABI 4.  BatchNorm's backward sums from THIS epilogue (reference: autograd's backward of nn.BatchNorm2d behind a
   * convolution's input gradient, dcgan.py:150-161, wgan.py:117-156): when the finished output `out` is the gradient gn
   * that arrives at a train-mode BatchNorm whose input was `bn_a` (same [rows][channels] shape as `out`, statistics
   * bn_mean / bn_rstd), every full row tile also leaves (sum gn, sum gn * xhat, 0) per channel in
   * bn_partial[tile][3][N] - the layout lgm_bn_reduce3's first stage writes - and *bn_tiles receives the number of
   * tiles; lgm_bn_reduce3_coef_tiles finishes from there and the separate read pass over (gn, a) disappears.
   * *bn_tiles == 0: this launch could not (split-K, ragged tiles, a path without the hook): run lgm_bn_reduce3_coef.
   * bn_a NULL: off. */
  const float* bn_a;
  int64_t bn_a_pitch;
  const float* bn_mean;
  const float* bn_rstd;
  float* bn_partial;
  int64_t bn_partial_floats;     /* capacity of bn_partial */
  int32_t* bn_tiles;             /* out (host memory) */
} LgmPostOp;
int lgm_conv_xy_post(const LgmConvGeom* g, const float* x, int64_t x_pitch, const float* w, const float* bias,
                     const float* res, int64_t res_pitch, float* y, int64_t y_pitch, void* workspace,
                     int64_t workspace_bytes, const LgmPostOp* post, void* stream);
int lgm_conv_yx_post(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* w, const float* w_t,
                     const float* bias, const float* res, int64_t res_pitch, float* x, int64_t x_pitch,
                     void* workspace, int64_t workspace_bytes, const LgmPostOp* post, void* stream);
/* lgm_conv_bwd_pair with lgm_conv_yx_post's post-op on the INPUT gradient (the backward mask of an activation that sat in
 * front of this layer's input - VQ-VAE residual.py:14-20, vqvae.py:36-51): gx = post(W^T gy + res).  Keeps masked layers
 * on the one-launch path. */
int lgm_conv_bwd_pair_post(const LgmConvGeom* g, const float* gy, int64_t gy_pitch, const float* x, int64_t x_pitch,
                           const float* w, const float* w_t, const float* res, int64_t res_pitch, float* gx,
                           int64_t gx_pitch, void* dgrad_ws, int64_t dgrad_ws_bytes, float* gw, float* gbias,
                           float beta, void* wgrad_ws, int64_t wgrad_ws_bytes, int64_t* desc, const LgmPostOp* post,
                           void* stream);


/* Weight gradient: gw[n][tap][c] = beta*gw + sum_{b,oh,ow} Y[b,oh,ow,n] * X[b,ih,iw,c].
 * (Conv2d: Y = grad_output, X = input;  ConvTranspose2d: Y = input, X = grad_output.)
 * Deterministic: split-K partials go to `workspace` and are reduced in a fixed order.
 * lgm_conv_wgrad_workspace() returns the bytes needed for the given geometry. */
int64_t lgm_conv_wgrad_workspace(const LgmConvGeom* g);
/* gbias (optional, [Nw]): fused bias gradient gbias[n] = beta*gbias + sum_{b,oh,ow} Y[b,oh,ow,n]
 * (valid for Conv2d / Linear, where Y is the output gradient). */
int lgm_conv_wgrad(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* x,
                   int64_t x_pitch, float* gw, float* gbias, float beta, void* workspace,
                   int64_t workspace_bytes, void* stream);
/* Backward of ANY convolution / linear layer in one call: weight / bias gradient (lgm_conv_wgrad, or its deferred form
 * when desc != NULL) AND input gradient gx = W^T gy (+ res) (lgm_conv_yx).  When the dispatchers pick the two kernels
 * that can share a grid - the 1x1 convolutions and linears of the UNet at small row counts (to_qkv / to_out
 * ddpm.py:214-223, res_conv :184, Downsample :100-104) - both run in ONE launch (gemm_bwd_pair_kernel: same kernel
 * bodies, bit-identical results); otherwise exactly the two separate calls.  dgrad_ws (lgm_conv_workspace(g, 1) bytes)
 * and wgrad_ws (lgm_conv_wgrad_workspace(g) bytes) must not overlap. */
int lgm_conv_bwd_pair(const LgmConvGeom* g, const float* gy, int64_t gy_pitch, const float* x, int64_t x_pitch,
                      const float* w, const float* w_t, const float* res, int64_t res_pitch, float* gx,
                      int64_t gx_pitch, void* dgrad_ws, int64_t dgrad_ws_bytes, float* gw, float* gbias, float beta,
                      void* wgrad_ws, int64_t wgrad_ws_bytes, int64_t* desc, void* stream);
/* Deferred form (same arithmetic): writes only the per-split partial slabs into `workspace` (which must then
 * stay untouched until the reduction) and fills desc[8] = {workspace, slab stride, gw, n_w, gbias, n_b, splits,
 * beta bits}; lgm_wgrad_reduce_batch then performs the fixed-order slab reductions of MANY layers in one
 * launch (table rows = desc + first block, blocks per row = ceil((n_w + n_b) / 256); rows with splits == 1
 * must be left out: their result is already in gw).  Replaces ~75 tiny reduce launches per DDPM step. */
int lgm_conv_wgrad_deferred(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* x,
                            int64_t x_pitch, float* gw, float* gbias, float beta, void* workspace,
                            int64_t workspace_bytes, int64_t* desc, void* stream);
int lgm_wgrad_reduce_batch(const int64_t* table, int n_entries, int64_t total_blocks, void* stream);

/* Column sums of a [rows, cols] matrix with row pitch: out[c] = beta*out[c] + sum_r a[r,c].
 * Used for conv/linear bias gradients.  Deterministic two-stage; workspace >=
 * lgm_colsum_workspace(rows, cols) bytes. */
int64_t lgm_colsum_workspace(int64_t rows, int64_t cols);
int lgm_colsum(const float* a, int64_t pitch, int64_t rows, int64_t cols, float* out, float beta,
               void* workspace, void* stream);
/* Deferred form: the first stage's partial rows stay in `workspace` (must then stay untouched until the reduction) and
 * desc[8] receives their row for lgm_wgrad_reduce_batch - the bias gradients of transposed convolutions join the
 * bucket's one reduction launch.  cols % 4 == 0 and a 16-byte aligned `out` required. */
int lgm_colsum_deferred(const float* a, int64_t pitch, int64_t rows, int64_t cols, float* out, float beta,
                        void* workspace, int64_t* desc, void* stream);

/* ---------------------------------------------------------------------------------------
 * GroupNorm(+FiLM scale/shift)(+SiLU)(+residual)   — Block.forward ddpm.py:164-173
 *   z = GN(x; gamma, beta, G, eps) * (scale + 1) + shift ;  y = act ? silu(z) : z ;  y += res
 * x, y, res: [B, HW, C] NHWC with pitches.  ss (optional): [B, >=2C] rows, scale = ss[b, c],
 * shift = ss[b, C + c] (the chunk(2) of the time-MLP output, ddpm.py:192-194).
 * Outputs saved for backward: mean, rstd [B, G]; coefA, coefB [B, C]  (z = x*coefA + coefB).
 * ------------------------------------------------------------------------------------- */
int lgm_gn_fwd(const float* x, int64_t x_pitch, int B, int HW, int C, int G, float eps,
               const float* gamma, const float* beta, const float* ss, int64_t ss_pitch, int act,
               const float* res, int64_t res_pitch, float* y, int64_t y_pitch, float* mean,
               float* rstd, float* coefA, float* coefB, void* stream);
/* The same, with x still in pieces: the convolution that produces x (Block.proj, ddpm.py:160-171) split its reduction
 * and left `splits` partial planes [B*HW][C] (dense, `plane_stride` floats apart) instead of running its reducer
 * (lgm_conv3x3_wino_partial).  The planes are summed here in the reducer's fixed order (plane 0, 1, ..., then
 * conv_bias), the finished x is WRITTEN to `x` (the backward pass reads it) and normalised in the same pass: one
 * launch and one round trip of x less per convolution.  Only shapes with lgm_gn_planes_supported(...) == 1. */
int64_t lgm_gn_planes_supported(int B, int HW, int C, int G);
/* 1 when lgm_gn_fwd runs its one-pass kernel for this shape (the slices fit a block's registers), 0: two passes over x */
int64_t lgm_gn_fwd_fused_supported(int B, int HW, int C, int G);
/* diagnostic (host only, no launch): the launch plan of lgm_gn_fwd (bwd = 0) / lgm_gn_bwd (bwd = 1) for this shape: cb
 * channels per block, nt threads per block and nv 16-byte values per thread of the one-pass kernel; nv = 0: the two-pass
 * kernels run, at nt threads.  tests/test_hip_norm_ledger.py checks every row's route against it. */
int lgm_gn_plan(int B, int HW, int C, int G, int bwd, int* cb, int* nt, int* nv);
int lgm_gn_fwd_planes(const float* planes, int64_t plane_stride, int splits, const float* conv_bias, float* x,
                      int64_t x_pitch, int B, int HW, int C, int G, float eps, const float* gamma,
                      const float* beta, const float* ss, int64_t ss_pitch, int act, const float* res,
                      int64_t res_pitch, float* y, int64_t y_pitch, float* mean, float* rstd, float* coefA,
                      float* coefB, void* stream);
/* The same, with the STATISTICS already gathered by the convolution that produced x (lgm_conv3x3_wino4_stats; Block.proj
 * -> Block.norm, ddpm.py:157-173, on maps whose (image, channel block) slices do not fit a one-pass GroupNorm block - the
 * 64 x 64 maps of configs/diffusion/ddpm_64.json): `stats` holds, per image, `parts_per_image` rows of (sum, sum of
 * squares) per channel of the convolution's outputs BEFORE its bias (`conv_bias`, may be NULL), layout
 * [b * parts + q][2][C].  A small kernel combines them in float64 in a fixed order into mean / rstd / coefA / coefB, then
 * the apply pass reads x once.  C / G must divide 64. */
int lgm_gn_fwd_stats(const float* stats, int parts_per_image, const float* conv_bias, const float* x, int64_t x_pitch,
                     int B, int HW, int C, int G, float eps, const float* gamma, const float* beta, const float* ss,
                     int64_t ss_pitch, int act, const float* res, int64_t res_pitch, float* y, int64_t y_pitch,
                     float* mean, float* rstd, float* coefA, float* coefB, void* stream);
/* Backward.  gx (optionally accumulated), ggamma/gbeta (= affine_beta*old + new), gss [B, >=2C]
 * (optional; = gss_beta*old + new).  workspace: 5*B*C floats. */
int lgm_gn_bwd(const float* x, int64_t x_pitch, const float* gy, int64_t gy_pitch, int B, int HW,
               int C, int G, const float* gamma, const float* beta, const float* ss,
               int64_t ss_pitch, int act, const float* mean, const float* rstd, const float* coefA,
               const float* coefB, float* gx, int64_t gx_pitch, int accumulate_gx, float* ggamma,
               float* gbeta, float affine_beta, float* gss, int64_t gss_pitch, float gss_beta,
               float* workspace, void* stream);
/* Backward with gy given as the partial planes of the input-gradient convolution that produces it (ResnetBlock:
 * block2.proj's input gradient feeds only block1.norm's backward, ddpm.py:176-200); gy itself is never written.
 * rows / desc: both NULL (gamma / beta gradients complete on return) or the deferred form of lgm_gn_bwd_deferred. */
int lgm_gn_bwd_planes(const float* x, int64_t x_pitch, const float* gy_planes, int64_t plane_stride, int splits, int B,
                      int HW, int C, int G, const float* gamma, const float* beta, const float* ss,
                      int64_t ss_pitch, int act, const float* mean, const float* rstd, const float* coefA,
                      const float* coefB, float* gx, int64_t gx_pitch, int accumulate_gx, float* ggamma,
                      float* gbeta, float affine_beta, float* gss, int64_t gss_pitch, float gss_beta,
                      float* workspace, float* rows, int64_t* desc, void* stream);
/* ABI 7.  lgm_gn_bwd (rows = desc = NULL) / lgm_gn_bwd_deferred (both given) that ALSO adds gy to a second tensor,
 * add_out[b, p, c] += gy[b, p, c] (add_pitch % 4 == 0, >= C; not gx, not gy): the gradient of ResnetBlock's identity
 * residual - reference ddpm.py:187,200, `return h + self.res_conv(x)` with res_conv = nn.Identity - when the block's input
 * gradient is accumulated into a tensor that already holds another branch's gradient (the skip connections of the UNet's
 * down path, ddpm.py:440-447).  Replaces the separate `gx += gy` pass: block2's GroupNorm backward reads gy anyway. */
int lgm_gn_bwd_add(const float* x, int64_t x_pitch, const float* gy, int64_t gy_pitch, int B, int HW,
                   int C, int G, const float* gamma, const float* beta, const float* ss,
                   int64_t ss_pitch, int act, const float* mean, const float* rstd, const float* coefA,
                   const float* coefB, float* gx, int64_t gx_pitch, int accumulate_gx, float* ggamma,
                   float* gbeta, float affine_beta, float* gss, int64_t gss_pitch, float gss_beta,
                   float* workspace, float* rows, int64_t* desc, float* add_out, int64_t add_pitch, void* stream);
/* Deferred form: when the one-pass kernel applies, the per-image rows [sc*S2 | sc*S1] (B x 2C floats) are left in
 * `rows` and `desc` is filled in the format of lgm_conv_wgrad_deferred (images play the role of splits), so that
 * lgm_wgrad_reduce_batch produces ggamma / gbeta of many layers in one launch; otherwise the gradients are
 * complete on return and desc[6] == 0. */
int lgm_gn_bwd_deferred(const float* x, int64_t x_pitch, const float* gy, int64_t gy_pitch, int B, int HW,
                        int C, int G, const float* gamma, const float* beta, const float* ss,
                        int64_t ss_pitch, int act, const float* mean, const float* rstd, const float* coefA,
                        const float* coefB, float* gx, int64_t gx_pitch, int accumulate_gx, float* ggamma,
                        float* gbeta, float affine_beta, float* gss, int64_t gss_pitch, float gss_beta,
                        float* workspace, float* rows, int64_t* desc, void* stream);

/* RMSNorm over channels — ddpm.py:107-113: y = x / max(||x||_2, 1e-12) * g * sqrt(C) (+ res).
 * Backward: gx = [gx +] d/dx (+ res): `res` (or null) is the gradient arriving over the residual branch
 * around the PreNorm'd attention block (ddpm.py:187-193), added in the same pass. */
int lgm_rmsnorm_fwd(const float* x, int64_t x_pitch, const float* g, const float* res,
                    int64_t res_pitch, float* y, int64_t y_pitch, int64_t npix, int C, void* stream);
int64_t lgm_rmsnorm_bwd_workspace(int64_t npix, int C);
int lgm_rmsnorm_bwd(const float* x, int64_t x_pitch, const float* gy, int64_t gy_pitch,
                    const float* g, float* gx, int64_t gx_pitch, int accumulate_gx, const float* res,
                    int64_t res_pitch, float* gg, float gg_beta, int64_t npix, int C, void* workspace, void* stream);
/* Deferred form: leaves the per-block partial rows of the g gradient in `workspace` and fills a descriptor in
 * the format of lgm_conv_wgrad_deferred (rows play the role of splits), so that lgm_wgrad_reduce_batch sums
 * the g gradients of all RMSNorm layers together with the weight-gradient slabs in one launch. */
int lgm_rmsnorm_bwd_deferred(const float* x, int64_t x_pitch, const float* gy, int64_t gy_pitch,
                             const float* g, float* gx, int64_t gx_pitch, int accumulate_gx, const float* res,
                             int64_t res_pitch, float* gg, float gg_beta, int64_t npix, int C, void* workspace,
                             int64_t* desc, void* stream);

/* ---------------------------------------------------------------------------------------
 * Attention cores on qkv [B, n, 3*heads*32] (channel = which*hidden + head*32 + d).
 * LinearAttention ddpm.py:217-239 (mem_kv [2, heads, 32, M]); Attention ddpm.py:255-271 +
 * modules/attend.py:97-126 (mem_kv [2, heads, M, 32]).  out: [B, n, heads*32].
 * ------------------------------------------------------------------------------------- */
int lgm_linattn_fwd(const float* qkv, int64_t qkv_pitch, const float* mem_kv, int B, int n,
                    int heads, int dim_head, int M, float* out, int64_t out_pitch, float* ctx,
                    float* kmax, float* ksum, void* stream);
/* Head of the attention blocks' forward in one launch (ddpm.py:224-225, :262-263): xn = RMSNorm_g(x) (ddpm.py:115-121)
 * and qkv = to_qkv(xn), a bias-free 1x1 convolution with weight w [N][C]; N = 384, C in {64, 128, 256}
 * (lgm_rms_qkv_fused_supported: 0 = not built, 1 = built, 2 = built and faster than the two separate launches).  xn is
 * written for the weight gradient. */
int64_t lgm_rms_qkv_fused_supported(int C, int N);
int lgm_rms_qkv_fused(const float* x, int64_t x_pitch, const float* g, const float* w, int C, int N, int64_t npix,
                      float* xn, int64_t xn_pitch, float* qkv, int64_t qkv_pitch, void* stream);
/* Forward with its tail fused (ddpm.py:229-239 + the residual around the block): after the context launch ONE launch
 * computes out = softmax_d(q) scale ctx, o2 = to_out[0](out) (wout [Cout][heads*32], bout [Cout]) and
 * y = RMSNorm_g(o2) + x.  `out` and `o2` are written for the backward pass.  Cout in {64, 128, 256}
 * (lgm_linattn_fwd_fused_supported: 0 = not built, 1 = built, 2 = built and faster than the separate launches). */
int64_t lgm_linattn_fwd_fused_supported(int heads, int dim_head, int Cout);
int lgm_linattn_fwd_fused(const float* qkv, int64_t qkv_pitch, const float* mem_kv, int B, int n, int heads,
                          int dim_head, int M, const float* wout, const float* bout, const float* g, int Cout,
                          const float* x, int64_t x_pitch, float* out, int64_t out_pitch, float* o2,
                          int64_t o2_pitch, float* y, int64_t y_pitch, float* ctx, float* kmax, float* ksum,
                          void* stream);
int64_t lgm_linattn_bwd_workspace(int B, int heads, int dim_head, int M);
int lgm_linattn_bwd(const float* qkv, int64_t qkv_pitch, const float* mem_kv, const float* gout,
                    int64_t gout_pitch, const float* ctx, const float* kmax, const float* ksum,
                    int B, int n, int heads, int dim_head, int M, float* gqkv, int64_t gqkv_pitch,
                    float* gmem_kv, float gmem_beta, void* workspace, void* stream);
/* The same backward with its tail fused (autograd of ddpm.py:214-239, i.e. LinearAttention.to_qkv's backward folded
 * into the attention core's): gq / gk / gv of a pixel tile stay on the chip; the launch that computes them also produces
 * to_qkv's input gradient gxn[B n, C] = gqkv Wqkv and to_qkv's weight gradient (per-workgroup slabs in `slabs`,
 * lgm_linattn_bwd_fused_slabs bytes, summed by the fixed-order reducer).  Built for C = 64 input channels
 * (lgm_linattn_bwd_fused_supported).  xn = the RMSNorm output to_qkv was applied to, wqkv_t = to_qkv.weight transposed,
 * [C][3*heads*32].  `gw_desc` / `gmem_desc` (8 int64, rows of lgm_wgrad_reduce_batch; [6] = 0: no row): non-null = the
 * reductions are left to the caller's batched reducer and `slabs` / `gmem_part` (B*2*heads*32*M floats) must stay
 * untouched until it has run; null = reduced here. */
int64_t lgm_linattn_bwd_fused_supported(int heads, int dim_head, int C);
int64_t lgm_linattn_bwd_fused_slabs(int B, int n, int C);
int64_t lgm_linattn_bwd_fused_workspace(int B, int heads, int dim_head);
int lgm_linattn_bwd_fused(const float* qkv, int64_t qkv_pitch, const float* mem_kv, const float* gout,
                          int64_t gout_pitch, const float* ctx, const float* kmax, const float* ksum,
                          const float* xn, int64_t xn_pitch, const float* wqkv_t, int C, int B, int n,
                          int heads, int dim_head, int M, float* gxn, int64_t gxn_pitch, float* gwqkv,
                          float gw_beta, void* slabs, int64_t slab_bytes, int64_t* gw_desc, float* gmem_kv,
                          float gmem_beta, void* gmem_part, int64_t* gmem_desc, void* workspace, void* stream);
/* Deferred forms of the two backward entry points: the per-image partial rows of the mem_kv gradient are left in
 * `gmem_part` (B*2*heads*32*M floats; must stay untouched until the caller's lgm_wgrad_reduce_batch has run) and
 * `gmem_desc` (8 int64) receives their reducer row ([6] = 0: no row) - one batched reduction per exchange bucket instead
 * of a column-sum launch pair per attention block.  gmem_kv must be 16-byte aligned. */
int lgm_linattn_bwd_deferred(const float* qkv, int64_t qkv_pitch, const float* mem_kv, const float* gout,
                             int64_t gout_pitch, const float* ctx, const float* kmax, const float* ksum,
                             int B, int n, int heads, int dim_head, int M, float* gqkv, int64_t gqkv_pitch,
                             float* gmem_kv, float gmem_beta, void* gmem_part, int64_t* gmem_desc,
                             void* workspace, void* stream);
int lgm_attn_bwd_deferred(const float* qkv, int64_t qkv_pitch, const float* mem_kv, const float* out,
                          int64_t out_pitch, const float* gout, int64_t gout_pitch, const float* lse, int B,
                          int n, int heads, int dim_head, int M, float* gqkv, int64_t gqkv_pitch,
                          float* gmem_kv, float gmem_beta, void* gmem_part, int64_t* gmem_desc, void* stream);
int lgm_attn_fwd(const float* qkv, int64_t qkv_pitch, const float* mem_kv, int B, int n, int heads,
                 int dim_head, int M, float* out, int64_t out_pitch, float* lse, void* stream);
int64_t lgm_attn_bwd_workspace(int B, int heads, int dim_head, int M);
int lgm_attn_bwd(const float* qkv, int64_t qkv_pitch, const float* mem_kv, const float* out,
                 int64_t out_pitch, const float* gout, int64_t gout_pitch, const float* lse, int B,
                 int n, int heads, int dim_head, int M, float* gqkv, int64_t gqkv_pitch,
                 float* gmem_kv, float gmem_beta, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Elementwise / data-movement kernels.
 * ------------------------------------------------------------------------------------- */
/* SinusoidalPosEmb ddpm.py:125-132: out[b] = cat(sin(t_b f), cos(t_b f)).  freqs[dim/2] (device) is the
 * table f_i = exp(-i ln(theta)/(dim/2-1)) computed by the caller on the host, as the reference does. */
int lgm_posemb(const int64_t* t, int B, int dim, const float* freqs, float* out, int64_t pitch, void* stream);

#define LGM_ACT_NONE 0
#define LGM_ACT_SILU 1  /* nn.SiLU  ddpm.py:162,180 */
#define LGM_ACT_GELU 2  /* nn.GELU (erf) ddpm.py:331 */
#define LGM_ACT_RELU 3  /* residual.py:13-16, vqvae.py:38-42, dcgan.py:90 */
#define LGM_ACT_LRELU 4 /* dcgan.py:161 (slope 0.2) */
#define LGM_ACT_TANH 5  /* dcgan.py:90, vqvae.py:85 */
/* y = act(x + bias) (+ res);  gx (+)= gy * act'(x + bias).  [rows, cols] matrices with pitches. */
int lgm_act_fwd(const float* x, int64_t x_pitch, const float* bias, const float* res,
                int64_t res_pitch, float* y, int64_t y_pitch, int64_t rows, int cols, int act,
                float slope, void* stream);
int lgm_act_bwd(const float* x, int64_t x_pitch, const float* bias, const float* gy,
                int64_t gy_pitch, float* gx, int64_t gx_pitch, int accumulate, int64_t rows,
                int cols, int act, float slope, void* stream);
/* y = alpha*a + beta*b (b optional) */
int lgm_axpby(const float* a, int64_t a_pitch, float alpha, const float* b, int64_t b_pitch,
              float beta, float* y, int64_t y_pitch, int64_t rows, int cols, void* stream);
/* nn.Upsample(scale_factor=2, mode="nearest") ddpm.py:95; x [B,H,W,C] -> y [B,2H,2W,C] */
int lgm_upsample2x_fwd(const float* x, int64_t x_pitch, float* y, int64_t y_pitch, int B, int H,
                       int W, int C, void* stream);
int lgm_upsample2x_bwd(const float* gy, int64_t gy_pitch, float* gx, int64_t gx_pitch, int B, int H,
                       int W, int C, int accumulate, void* stream);
/* Rearrange("b c (h p1) (w p2) -> b (c p1 p2) h w") ddpm.py:102 in NHWC.  Hlo/Wlo: low-res size,
 * C: high-res channels.  inverse=0: src hi-res [B,2H,2W,C] -> dst lo-res [B,H,W,4C];
 * inverse=1: src lo-res -> dst hi-res (the gradient), optionally accumulated. */
int lgm_pixel_unshuffle(const float* src, int64_t src_pitch, float* dst, int64_t dst_pitch, int B,
                        int Hlo, int Wlo, int C, int inverse, int accumulate, void* stream);
int lgm_nchw_to_nhwc(const float* src, float* dst, int64_t dst_pitch, int B, int C, int HW, int Cpad,
                     void* stream);
int lgm_nhwc_to_nchw(const float* src, int64_t src_pitch, float* dst, int B, int C, int HW,
                     void* stream);

/* lgm_qsample_target_slice with one slice (x_off 0, no sc slice, Cpad lanes), pred_v, no offset noise; kept for ABI 7 */
int lgm_qsample_target(const float* img, const float* noise, const int64_t* t, const float* sqrt_ac,
                       const float* sqrt_1mac, int normalize, float* xt, float* target,
                       int64_t pitch, int B, int C, int HW, int Cpad, void* stream);
/* loss = mean_b( w[t_b] * mean_{chw} (out - target)^2 )  ddpm.py:921-925 (loss_weight NULL => 1) */
int lgm_weighted_mse_fwd(const float* out, const float* target, int64_t pitch, const int64_t* t,
                         const float* loss_weight, int B, int C, int HW, int Cpad, float* per_sample,
                         float* loss, void* stream);
int lgm_weighted_mse_bwd(const float* out, const float* target, int64_t pitch, const int64_t* t,
                         const float* loss_weight, const float* gloss, int B, int C, int HW, int Cpad,
                         float* gout, void* stream);

/* The UNet's time embedding in one launch: SinusoidalPosEmb ddpm.py:119-132 -> time_mlp (Linear, GELU, Linear) :328-333 ->
 * the SiLU every ResnetBlock.mlp applies first :181-183.  t [B] int64; freqs [dim/2] as lgm_posemb takes them; w1 [time_dim][dim],
 * w2 [time_dim][time_dim] (torch Linear layout, dense).  Outputs, all dense and all kept for the backward:
 *   pe [B][dim], a1 = pe w1^T + b1, h = gelu(a1), temb = h w2^T + b2, st = silu(temb)   ([B][time_dim] each).
 * A row's results do not depend on the batch it is part of (fixed per-row summation order). */
int64_t lgm_time_mlp_supported(int dim, int time_dim);   /* 1 / 0: query, not a status code */
int lgm_time_mlp_fwd(const int64_t* t, int B, int dim, const float* freqs, const float* w1, const float* b1,
                     const float* w2, const float* b2, int time_dim, float* pe, float* a1, float* h, float* temb,
                     float* st, void* stream);
/* Its backward from gst = d loss / d st (two launches: the row-local chain, then the batch reductions, rows in order):
 *   gtemb = gst silu'(temb), ga1 = (gtemb w2) gelu'(a1)   (scratch outputs [B][time_dim]),
 *   gw2 = beta gw2 + gtemb^T h, gb2 = beta gb2 + colsum(gtemb), gw1 = beta gw1 + ga1^T pe, gb1 = beta gb1 + colsum(ga1). */
int lgm_time_mlp_bwd(const float* gst, const float* pe, const float* a1, const float* h, const float* temb,
                     const float* w2, int B, int dim, int time_dim, float* gtemb, float* ga1, float* gw1, float* gb1,
                     float* gw2, float* gb2, float beta, void* stream);

/* GaussianDiffusion's per-sample-timestep algebra on dense NCHW tensors (`extract(table, t, shape) * ...`):
 *   out[b][i] = clamp?( (ta[t_b] * x[b][i] + sb * tb[t_b] * y[b][i]) / td[t_b] )     i < per_sample
 * ta / tb / td = NULL read as 1; products and the sum are rounded separately (no contraction), like the reference's ATen
 * expression.  One entry point for q_sample ddpm.py:869-876 (sqrt_ac, sqrt_1mac, +1), predict_v :684-688, predict_start_from_v
 * :690-694, predict_start_from_noise :673-677 (sb = -1), predict_noise_from_start :679-682 (ta = sqrt_recip, tb = NULL,
 * sb = -1, td = sqrt_recipm1) and q_posterior's mean :697-700.  clip != 0: clamp to [-1, 1] (maybe_clip :711-713). */
int lgm_extract_axpby(const float* ta, const float* tb, const float* td, const int64_t* t, const float* x,
                      const float* y, float sb, int clip, float* out, int B, int64_t per_sample, int n_table,
                      void* stream);
/* lgm_model_predictions_obj at objective 2 (pred_v); kept for ABI 7 */
int lgm_model_predictions(const float* x, const float* v, const int64_t* t, const float* sqrt_ac,
                          const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1, int clip,
                          float* pred_noise, float* x_start, int B, int64_t per_sample, int n_table, void* stream);

/* lgm_sample_step_slice with one slice of pitch Cpad (x, v, out, x0_out dense NHWC), pred_v, and the optional x0_out (the
 * clipped x0, pad lanes zero); kept for ABI 7 */
int lgm_sample_step(const float* x, const float* v, const float* noise, float* out, float* x0_out,
                    int B, int C, int HW, int Cpad, float A, float Bv, int clip, float R, float Rm1,
                    float C0, float C1, float C2, float C3, void* stream);

/* A HIP-graph-replayed chain (p_sample_loop ddpm.py:759-780, ddim_sample :782-834 without the per-step host round trip
 * :775,829): lgm_sampler_time writes t[b] = ttable[counter[0]] for the UNet forward of the step.
 * lgm_sample_step_table: lgm_sample_step_table_slice with one slice of pitch Cpad, pred_v, optional x0_out; kept for ABI 7 */
int lgm_sampler_time(const int64_t* ttable, const int32_t* counter, int64_t* t, int B, void* stream);
int lgm_sample_step_table(float* x, const float* v, const float* noise, float* x0_out, int B, int C, int HW,
                          int Cpad, const float* table, const int32_t* counter, int clip, int advance,
                          void* stream);

/* lgm_qsample_target_slice with one slice (x_off 0, no sc slice, Cpad lanes; xt and target share `pitch`); kept for ABI 7 */
int lgm_qsample_target_obj(const float* img, const float* noise, const float* offset, float strength,
                           const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int normalize,
                           int objective, float* xt, float* target, int64_t pitch, int B, int C, int HW, int Cpad,
                           void* stream);
/* model_predictions ddpm.py:707-734 in one pass over dense NCHW tensors with a per-sample t; `out` is the raw network
 * output, objective 0 = pred_noise, 1 = pred_x0, 2 = pred_v (ddpm.py:562):
 *   pred_noise: x_start = maybe_clip(sqrt_recip[t] * x - sqrt_recipm1[t] * out); pred_noise = out, or re-derived from the
 *               clipped x_start as below when clip AND rederive are set (:720-721)
 *   pred_x0   : x_start = maybe_clip(out);  pred_noise = (sqrt_recip[t] * x - x_start) / sqrt_recipm1[t]
 *   pred_v    : x_start = maybe_clip(sqrt_ac[t] * x - sqrt_1mac[t] * out);  pred_noise as for pred_x0 (rederive has no
 *               effect)
 * Launches model_predictions_obj_kernel. */
int lgm_model_predictions_obj(const float* x, const float* out, const int64_t* t, const float* sqrt_ac,
                              const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                              int objective, int clip, int rederive, float* pred_noise, float* x_start, int B,
                              int64_t per_sample, int n_table, void* stream);
/* lgm_sample_step_slice with one slice of pitch Cpad and the optional x0_out; kept for ABI 7 */
int lgm_sample_step_obj(const float* x, const float* v, const float* noise, float* out, float* x0_out, int B,
                        int C, int HW, int Cpad, int objective, float A, float Bv, int clip, int rederive,
                        float R, float Rm1, float C0, float C1, float C2, float C3, void* stream);
/* lgm_sample_step_table_slice with one slice of pitch Cpad and the optional x0_out; kept for ABI 7 */
int lgm_sample_step_table_obj(float* x, const float* v, const float* noise, float* x0_out, int B, int C, int HW,
                              int Cpad, const float* table, const int32_t* counter, int objective, int clip,
                              int rederive, int advance, void* stream);

/* The diffusion elementwise ops on the network's input buffer.  A self-conditioned UNet (ddpm.py:428-435, 899-909) reads ONE
 * NHWC input buffer [B, HW, pitch] with pitch = r4(2 C): lanes [sc_off, sc_off + C) = x_self_cond (sc_off = 0), lanes
 * [x_off, x_off + C) = x (x_off = C) - the order of cat((x_self_cond, x), dim=1) - and zeros in the remaining lanes.  These
 * entry points produce the two slices in place of a concat tensor; loads and stores are scalar, so the slices need no float4
 * alignment (C = 3: lanes 0 and 3 of 8).  sc_off < 0 means "no self-conditioning slice": any other network, with
 * pitch = r4(C) and x_off = 0.  `out` / `v` is the raw network output [B, HW, out_pitch]; objective as above.
 *
 * lgm_selfcond_estimate: xin[sc slice] = unclipped x_start of model_predictions (objective's branch) from xin[x slice] and
 *   `out`, per-sample t.  The x slice and the padding are not written.  Launches selfcond_estimate_kernel.
 * lgm_qsample_target_slice (GaussianDiffusion.forward / q_sample / predict_v ddpm.py:945, 869-876, 684-688; img, noise NCHW
 *   dense): x0 = img*2-1 when normalize; n = noise + strength * offset[b*C+c] (offset noise :889-891, offset [B*C] or NULL),
 *   used for x_t AND for the target; x_t = sqrt_ac[t]*x0 + sqrt_1mac[t]*n into the x slice, zeros into the self-conditioning
 *   slice and the padding; the objective's target (:911-917: n, x0, or v = sqrt_ac[t]*n - sqrt_1mac[t]*x0) into target
 *   [B, HW, target_pitch] with Cpad lanes written (may be NULL).  Launches qsample_slice_kernel.
 * lgm_sample_step_slice: one reverse-diffusion update at a shared timestep (p_sample :748-757, ddim_sample loop body
 *   :805-829), with (x0, eps) = model_predictions' branch from (A, -Bv, R, Rm1) = (sqrt_ac, sqrt_1mac, sqrt_recip,
 *   sqrt_recipm1)[t] (p_sample passes clip only, ddim_sample clip and rederive):
 *     out = C0*x0 + C1*x + C2*eps + C3*noise            (noise: NCHW dense or NULL)
 *   x from the x slice of xin, the next x into the x slice of xout (xout may be xin), the x0 the reference hands to the next
 *   step (clipped when clip is set) into xout's self-conditioning slice, zeros into its padding.
 * lgm_sample_step_table_slice: the same IN PLACE with the scalars from row counter[0] of table[n_steps][8] = (A, Bv, R, Rm1,
 *   C0, C1, C2, C3); advance != 0 appends counter[0] += 1 (the last node of a graph-replayed step).
 *   Both launch sample_step_slice_kernel. */
int lgm_selfcond_estimate(float* xin, int64_t pitch, int x_off, int sc_off, const float* out, int64_t out_pitch,
                          const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip,
                          const float* sqrt_recipm1, int objective, int B, int C, int HW, int n_table, void* stream);
int lgm_qsample_target_slice(const float* img, const float* noise, const float* offset, float strength,
                             const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int normalize,
                             int objective, float* xin, int64_t pitch, int x_off, int sc_off, float* target,
                             int64_t target_pitch, int B, int C, int HW, int Cpad, void* stream);
int lgm_sample_step_slice(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                          int64_t v_pitch, const float* noise, int B, int C, int HW, int objective, float A, float Bv,
                          int clip, int rederive, float R, float Rm1, float C0, float C1, float C2, float C3,
                          void* stream);
int lgm_sample_step_table_slice(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                                const float* noise, int B, int C, int HW, const float* table, const int32_t* counter,
                                int objective, int clip, int rederive, int advance, void* stream);

/* Class conditioning and classifier-free guidance (csrc/classcond.hip; an extension of the reference's Unet /
 * GaussianDiffusion, like `objective` and `self_condition`).  emb is the label embedding [num_classes + 1][time_dim], row
 * num_classes = the null label; y holds one int64 label per sample and is clamped to [0, num_classes] on the device (a
 * caller that can see the labels rejects others beforehand).  time_dim % 4 == 0, 16-byte aligned rows.
 *
 * lgm_label_emb_fwd: temb[b] += emb[y[b]], st[b] = SiLU(temb[b]) - behind the time MLP (ddpm.py:430, 181-183), in place.
 * lgm_label_emb_wgrad: gemb[k] = beta * gemb[k] + sum over the samples with y[b] = k of gtemb[b], in ascending b: every row
 *   is written, a class no sample has gets beta * its old value.  No atomics: the same bits on every run.
 * lgm_cfg_mix: out_cond[r][c] = out_null[r][c] + scale * (out_cond[r][c] - out_null[r][c]) for c < C, in place in out_cond
 *   [rows][cond_pitch]; scale == 1 keeps out_cond and scale == 0 takes out_null, bit for bit; lanes >= C keep their value.
 *   scale_dev != NULL: the scale is read from that device float instead (a captured sampling step).  Pitches % 4 == 0. */
int lgm_label_emb_fwd(float* temb, float* st, const float* emb, const int64_t* y, int B, int time_dim, int num_classes,
                      void* stream);
int lgm_label_emb_wgrad(const float* gtemb, const int64_t* y, float* gemb, float beta, int B, int time_dim,
                        int num_classes, void* stream);
int lgm_cfg_mix(float* out_cond, int64_t cond_pitch, const float* out_null, int64_t null_pitch, float scale,
                const float* scale_dev, int64_t rows, int C, void* stream);

/* Low-resolution conditioning of a cascaded super-resolution stage (csrc/lowres.hip; SR3 / Cascaded Diffusion Models / Imagen;
 * an extension of the reference).  A conditioned UNet reads cat((lowres_cond_img, x), dim=1) from ONE input buffer [B, H W,
 * pitch], pitch = r4(2 C): lanes [cond_off, cond_off + C) = the conditioning image (cond_off = 0), lanes [C, 2 C) = x.
 *
 * lgm_lowres_cond: the producer of the conditioning slice, one launch.  Exactly one source is non-NULL: img [B, C, H, W]
 *   (training: the batch q_sample reads) or low [B, C, H / r, W / r] (sampling), both NCHW dense; r in {2, 4, 8} divides H and
 *   W; C <= 64.  Per element, float32 without contraction, in this order:
 *     l   = mean of img over the r x r block (img source; each row of r by the halving tree v[i] += v[i + n/2], n = r, r/2, ..,
 *           the r row sums by the same tree, times 1 / r^2: 2 log2 r roundings)   |   low (low source)
 *     n   = 2 l - 1 when normalize (1 rounding; applied to the low-resolution value: the bilinear weights sum to one exactly)
 *     u   = (n00 wx0 + n01 wx1) wy0 + (n10 wx0 + n11 wx1) wy1, the taps of torch's bilinear align_corners=False rule: source
 *           coordinate (dst + 0.5) / r - 0.5 clamped at 0, the upper tap clamped at the last row / column; the weights are
 *           exact for these r (4 roundings: tap product, row sum, row product, column sum)
 *     out = sqrt_ac[s[b]] u + sqrt_1mac[s[b]] eps[b, c, p]  (2 roundings; s int64 [B], clamped to [0, n_table) on the device;
 *           the s == 0 row is a row like any other)        |   u, bit for bit, when eps == NULL (s and the tables unread)
 *   out goes to lane cond_off + c of pixel p; no other lane of xin is written.  The low-resolution tile of a workgroup and its
 *   one-pixel halo are staged in LDS, so img is read about once (x 1.41 at most) and nothing is averaged twice per output.  No
 *   atomics, no cross-thread sums: the same bits on every run, and from both sources when low holds the averages above.
 *   Launches lowres_cond_kernel<r>.
 * lgm_lowres_emb_fwd: temb[b] += add[b], st[b] = SiLU(temb[b]) (st may be NULL) - the augmentation-level embedding joins the
 *   time embedding behind the time MLP, in place, like lgm_label_emb_fwd.  time_dim % 4 == 0, 16-byte aligned rows.
 * lgm_sample_step_extent / lgm_dpm_step_extent: the reverse updates of lgm_sample_step_thresh / lgm_dpm_step_thresh (both forms
 *   of the row; thresh may be NULL: the static clamp; learned != 0: the row and the v lanes of lgm_sample_step_learned) that
 *   own lanes [lane0, lane0 + lanes) of the pitch only: x in [x_off, x_off + C) inside them, zeros in the rest of them, every
 *   other lane untouched - the conditioning slice is written once per chain and survives it.  No self-conditioning slice;
 *   x0_out (optional) has x0_pitch >= lanes and gets x0 in its lanes [0, C).  x0 is always clipped. */
int lgm_lowres_cond(const float* img, const float* low, const float* eps, const int64_t* s, const float* sqrt_ac,
                    const float* sqrt_1mac, int n_table, int normalize, float* xin, int64_t pitch, int cond_off, int B, int C,
                    int H, int W, int r, void* stream);
int lgm_lowres_emb_fwd(float* temb, float* st, const float* add, int B, int time_dim, void* stream);
int lgm_sample_step_extent(const float* xin, float* xout, int64_t pitch, int lane0, int lanes, int x_off, const float* v,
                           int64_t v_pitch, const float* noise, float* x0_out, int64_t x0_pitch, int B, int C, int HW,
                           int objective, int rederive, float A, float Bv, float R, float Rm1, float C0, float C1, float C2,
                           float C3, const float* table, const int32_t* counter, int advance, const float* thresh,
                           int learned, void* stream);
int lgm_dpm_step_extent(const float* xin, float* xout, int64_t pitch, int lane0, int lanes, int x_off, const float* v,
                        int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective, float A,
                        float Bv, float R, float Rm1, float Kx, float K0, float K1, float Kn, const float* table,
                        const int32_t* counter, int advance, const float* thresh, void* stream);

/* Progressive distillation (csrc/distill.hip; Salimans & Ho 2022, Algorithm 2; an extension of the reference): one DDIM step
 * t -> t'' of the student is trained to land where two DDIM steps t -> t' -> t'' of a frozen teacher land (eta = 0).  Both
 * entry points read table [n_table][16] float32 at row t[b] (int64 [B], clamped to [0, n_table) on the device; 16-byte
 * aligned; lgm_hip.distill.distill_plan, float64 rounded once):
 *     (A_t, S_t, R_t, Rm1_t,  A_m, S_m, R_m, Rm1_m,  A_n, S_n, cX, cZ,  iS_t, t', den, t'')
 *   (A, S, R, Rm1) = (sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1) at t and at t' (m); (A_n, S_n) = (alpha, sigma) at t'', (1, 0)
 *   for t'' = -1; den = A_n - (S_n / S_t) A_t, cX = 1 / den, cZ = -(S_n / S_t) / den ((1, 0) for t'' = -1); iS_t = 1 / S_t; t' as
 *   a float.  Buffers are NHWC with their pitch in floats; the x slices are lanes [off, off + C) of their buffer, r4(C) lanes from
 *   off must lie inside the pitch.  pred(z, o, head) is lgm_model_predictions_obj's branch for the TEACHER's objective with
 *   rederive_pred_noise set: x0 (clamped to [-1, 1] when clip) and the noise derived from it - what ddim_sample forms.
 * lgm_distill_half_step: (x1, e1) = pred(z_t, out, head_t), z_t' = A_m x1 + S_m e1 into lanes [mid_off, mid_off + C) of xmid and
 *   zeros into the r4(C) - C lanes behind them; t_mid[b] = t'.  z_t is read from the x slice of xin; out is the teacher's output at
 *   (z_t, t).  Launches distill_half_step_kernel.
 * lgm_distill_target: (x2, e2) = pred(z_t', out, head_m) with out the teacher's output at (z_t', t'), z_t'' = A_n x2 + S_n e2,
 *   x~ = cX z_t'' + cZ z_t, e~ = (z_t - A_t x~) iS_t; target lanes [0, C) = x~ (student objective 1), e~ (0) or A_t e~ - S_t x~ (2),
 *   lanes [C, r4(C)) = 0.  Launches distill_target_kernel.
 * Every product and sum rounds once (no contraction), in the order written.  16-byte accesses when every base is 16-byte aligned
 * and every pitch and offset a multiple of 4, else one lane per thread: the same bits.  No atomics. */
int lgm_distill_half_step(const float* xin, int64_t in_pitch, int x_off, const float* out, int64_t out_pitch, const int64_t* t,
                          const float* table, int n_table, int teacher_objective, int clip, float* xmid, int64_t mid_pitch,
                          int mid_off, int64_t* t_mid, int B, int C, int HW, void* stream);
int lgm_distill_target(const float* xin, int64_t in_pitch, int x_off, const float* xmid, int64_t mid_pitch, int mid_off,
                       const float* out, int64_t out_pitch, const int64_t* t, const float* table, int n_table,
                       int teacher_objective, int student_objective, int clip, float* target, int64_t target_pitch, int B, int C,
                       int HW, void* stream);

/* Spherical interpolation of two latents (csrc/slerp.hip; the latent interpolation of Song et al. 2021, fig. 6; an extension
 * of the reference).  a, b, out: NHWC [B, HW, pitch] with C live lanes from lane `off` on (off + C <= pitch), so each may be
 * the x slice of a network input buffer; out may be a or b.  lam: float[B] on the device.  Per sample, in double:
 *     c = a.b / sqrt(a.a b.b), clamped to [-1, 1]
 *     (c0, c1) = (1 - lam, lam) when 1 - c^2 < 1e-3 or a norm is 0, else (sin((1 - lam) W), sin(lam W)) / sin W, W = acos c
 *   each rounded once to float32, then out = fmaf(c1, b, c0 * a): three roundings per element on the way from (c0, c1).
 *   Lanes of out outside [off, off + C) are not written.  coef_out (optional): float[B][2] = (c0, c1).
 * Two launches, no atomics: slerp_partial_kernel (grid (spans, B): a workgroup reduces lgm_slerp_span() pixels of one sample
 * to the three doubles a.a, b.b, a.b, products and sums in double in a fixed order) into partials, then slerp_blend_kernel
 * (grid (spans, B): every workgroup sums its sample's partials in index order and blends its span).  partials: the caller's,
 * lgm_slerp_partials(B, HW) = 3 B ceil(HW / span) doubles, 8-byte aligned.  Both queries are host-only and depend on their
 * arguments alone (not on lgm_cu_margin()).  16-byte accesses when every base is 16-byte aligned, every pitch and offset a
 * multiple of 4 and r4(C) lanes from off lie inside the pitch, else one float at a time: the same bits. */
int64_t lgm_slerp_span(void);
int64_t lgm_slerp_partials(int64_t B, int64_t HW);
int lgm_slerp(const float* a, int64_t a_pitch, int a_off, const float* b, int64_t b_pitch, int b_off, const float* lam,
              float* out, int64_t out_pitch, int out_off, double* partials, float* coef_out, int B, int C, int HW,
              void* stream);

/* ---------------------------------------------------------------------------------------
 * DPM-Solver++(2M) sampling (Lu et al. 2022, data prediction; an extension of the reference).  Buffers as for
 * lgm_sample_step_slice; `hist` [B, HW, r4(C)] NHWC is the one piece of solver state, a buffer of its own.
 * lgm_dpm_step: one update at a shared timestep from the row (A, Bv, R, Rm1, Kx, K0, K1, Kn) of lgm_hip.sampler.dpm_coeffs:
 *     x0  = the objective's model_predictions branch from (A, -Bv, R, Rm1), clipped to [-1, 1] when clip is set
 *     out = Kx*x + K0*x0 [+ K1*hist when K1 != 0] [+ Kn*noise when noise != NULL and Kn != 0]    (no contraction, this order)
 *   out into the x slice of xout (xout may be xin), x0 into hist (pad lanes zero) and into xout's self-conditioning slice
 *   (sc_off >= 0), zeros into xout's padding.  hist is not read when K1 == 0 (the first step of a chain), the noise (NCHW
 *   dense) not when Kn == 0.
 * lgm_dpm_step_table: the same IN PLACE with row counter[0] of table[n_steps][8]; advance != 0 appends counter[0] += 1.
 *   Both launch dpm_step_kernel. */
int lgm_dpm_step(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                 const float* noise, float* hist, int B, int C, int HW, int objective, float A, float Bv, int clip,
                 float R, float Rm1, float Kx, float K0, float K1, float Kn, void* stream);
int lgm_dpm_step_table(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                       const float* noise, float* hist, int B, int C, int HW, const float* table,
                       const int32_t* counter, int objective, int clip, int advance, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dynamic thresholding of x0 (Saharia et al. 2022, 2.3; an extension of the reference): per sample
 *     s = max(1, quantile_p(|x0|)) over its C * HW values,   x0 <- clamp(x0, -s, s) / s
 * in place of the static clamp to [-1, 1].  A thresholded step is: network -> [lgm_cfg_mix] -> lgm_dyn_thresh -> one of the
 * *_thresh update entry points, which read thresh[b].
 * lgm_dyn_thresh: thresh[b] = fmaxf(lo + w * (hi - lo), 1) in float32 without contraction, lo / hi the k-th / (k+1)-th
 *   smallest |x0| of sample b (0-based; hi = lo at k = C * HW - 1), (k, w) = lgm_hip.sampler.dyn_rank(C * HW, p):
 *   torch.quantile's "linear" rule.  x0 is the UNCLIPPED model_predictions branch of `objective` from lanes [x_off, x_off + C)
 *   of xin [B, HW, pitch] and lanes [0, C) of v [B, HW, v_pitch] with the head (A, Bv, R, Rm1) - by value, or row counter[0]
 *   of table[n_steps][8] when table != NULL: the bits the update kernel computes.  Other lanes (padding, the self-
 *   conditioning slice) are never read.  Exact (an integer radix select on the bit pattern of |x0|, one workgroup per
 *   sample): the same bits on every run and under graph replay.  Inputs are assumed finite: a NaN sorts above Inf, so
 *   non-finite values reach s only when the rank reaches them, and s is then Inf, or 1 for a NaN.  C * HW < 2^31.
 *   Launches dyn_thresh_kernel.
 * lgm_sample_step_thresh / lgm_dpm_step_thresh: lgm_sample_step_slice / lgm_dpm_step with clip set and the clip replaced by
 *   x0 = fminf(fmaxf(x0, -s), s) / s, s = thresh[b] (one correctly rounded quotient: thresh[b] == 1 gives the static clamp's
 *   bits); the re-derived noise (rederive) comes from that x0.  table != NULL (then counter != NULL and xout == xin): the row
 *   is row counter[0] of the table and the eight scalars are ignored; advance != 0 appends counter[0] += 1.  x0_out
 *   (lgm_sample_step_thresh, optional): [B, HW, pitch], x0 in lanes [0, C) and zeros in the others.  They launch
 *   sample_step_slice_kernel / dpm_step_kernel, as the entry points without thresholds do.
 * lgm_model_predictions_thresh: lgm_model_predictions_obj with clip set and thresh [B] (from lgm_dyn_thresh over the dense
 *   unclipped x_start as a C = 1, HW = per_sample, pitch = 1, objective = pred_x0 problem). */
int lgm_dyn_thresh(const float* xin, int64_t pitch, int x_off, const float* v, int64_t v_pitch, int B, int C, int HW,
                   int objective, float A, float Bv, float R, float Rm1, const float* table, const int32_t* counter,
                   int k, float w, float* thresh, void* stream);
int lgm_sample_step_thresh(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                           int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW, int objective,
                           int rederive, float A, float Bv, float R, float Rm1, float C0, float C1, float C2, float C3,
                           const float* table, const int32_t* counter, int advance, const float* thresh, void* stream);
int lgm_dpm_step_thresh(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                        int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective, float A,
                        float Bv, float R, float Rm1, float Kx, float K0, float K1, float Kn, const float* table,
                        const int32_t* counter, int advance, const float* thresh, void* stream);
int lgm_model_predictions_thresh(const float* x, const float* out, const int64_t* t, const float* sqrt_ac,
                                 const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                                 int objective, int rederive, float* pred_noise, float* x_start, int B,
                                 int64_t per_sample, int n_table, const float* thresh, void* stream);

/* ---------------------------------------------------------------------------------------
 * Inpainting (RePaint, Lugmayr et al. 2022, Algorithm 1; an extension of the reference): a step of lgm_sample_step_thresh /
 * lgm_dpm_step_thresh to level s (thresh may be NULL here: the static clamp; clip is always set), followed in the same
 * kernel, per element, by
 *     known_s = Ma*known + Mn*eps_k                                   the given image at level s
 *     y       = m*known_s + (1 - m)*x_s                               m = 1: keep the known pixel
 *     out     = (Jx, Jn) == (1, 0) ? y : Jx*y + Jn*eps_j              the jump back up to level u
 * every product and sum rounded separately in this order (no contraction): m == 1 gives known_s and m == 0 gives x_s bit
 * for bit.  (Ma, Mn, Jx, Jn) is a row of lgm_hip.sampler's inpainting plan: Ma = sqrt(acp[s]), Mn = sqrt(1 - acp[s]) ((1, 0)
 * on the step that lands on the clean image), Jx = sqrt(acp[u] / acp[s]), Jn = sqrt(1 - acp[u] / acp[s]).
 *   known  [B, HW, r4(C)] NHWC, pad lanes never read;   mask [B, HW] in [0, 1], shared by the channels;
 *   eps_k, eps_j  [B, C, HW] NCHW dense like `noise`; eps_k is read only where Mn != 0, eps_j only where Jn != 0, and either
 *   may be NULL where its weight is passed by value as zero.
 * table != NULL (then counter and itable != NULL and xout == xin): the rows are row counter[0] of table[n_steps][8] and of
 * itable[n_steps][4], the twelve scalars are ignored and both draws must be given; advance != 0 appends counter[0] += 1.
 * The x0 that goes into the self-conditioning slice, into hist and into x0_out is the step's clipped prediction, not blended.
 * known == NULL (then mask, eps_k, eps_j and itable NULL too): the update alone.  A mask without known is an error.
 * They launch sample_step_slice_kernel / dpm_step_kernel, as every other update entry point does. */
int lgm_sample_step_inpaint(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                            int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW, int objective,
                            int rederive, float A, float Bv, float R, float Rm1, float C0, float C1, float C2, float C3,
                            const float* table, const int32_t* counter, int advance, const float* thresh,
                            const float* known, const float* mask, const float* eps_k, const float* eps_j, float Ma,
                            float Mn, float Jx, float Jn, const float* itable, void* stream);
int lgm_dpm_step_inpaint(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                         int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective, float A,
                         float Bv, float R, float Rm1, float Kx, float K0, float K1, float Kn, const float* table,
                         const int32_t* counter, int advance, const float* thresh, const float* known, const float* mask,
                         const float* eps_k, const float* eps_j, float Ma, float Mn, float Jx, float Jn,
                         const float* itable, void* stream);

/* ---------------------------------------------------------------------------------------
 * Variational-bound likelihood in bits per dimension (Ho et al. 2020, eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop; an
 * extension of the reference).  One evaluated timestep is: lgm_qsample_target_slice -> network -> one of the two entry points
 * below, which reduce over a sample's C * HW elements, one workgroup per sample, into out[n_rows][3][B] (float32):
 *     out[r][0][b]  the term of the bound in bits per dimension (below)
 *     out[r][1][b]  mean (x0_pred - x0)^2          out[r][2][b]  mean (eps_pred - noise)^2
 * img [B, C, HW] NCHW dense (x0 = img * 2 - 1 when normalize), noise NCHW dense (the draw q_sample used), x_t in lanes [x_off,
 * x_off + C) of xin [B, HW, pitch], the network output in lanes [0, C) of v [B, HW, v_pitch]; no other lane is read.  (x0_pred,
 * eps_pred) is model_predictions' branch of `objective` from the head (A, S, R, Rm1) = (sqrt_ac, sqrt_1mac, sqrt_recip,
 * sqrt_recipm1)[t], x0_pred clamped to [-1, 1] when clip is set and the noise then re-derived from it.  By kind:
 *   0  KL(q(x_{t-1} | x_t, x0) || p(x_{t-1} | x_t)), t >= 1:  (KC + KW * mean(d^2)) / ln 2, d = P1 * (x0_pred - x0) - the difference of
 *      the two posterior means, which share P2 * x_t; KC = 0.5 (-1 + lv_p - lv_q + exp(lv_q - lv_p)), KW = 0.5 exp(-lv_p)
 *   1  decoder, t = 0:  -mean(log p) / ln 2, log p the discretised Gaussian log-likelihood of x0 on the 8-bit grid under mean
 *      P1 * x0_pred + P2 * x_t and standard deviation 1 / inv_std with the tanh approximation of the normal CDF, probabilities
 *      floored at 1e-12, evaluated in a cancellation-free form (csrc/elementwise.hip vlb_decoder_logp)
 *   2  prior KL(q(x_T | x0) || N(0, I)):  (KC + KW * mean(x0^2)) / ln 2 with KC = 0.5 (-1 - log(1 - acp) + (1 - acp)), KW = 0.5 acp
 *      from the host; reads img only (noise, xin, v may be NULL), out[r][1] and out[r][2] come out 0
 * No contraction; the sums in a fixed order, no atomics: the same bits on every run and under graph replay.
 * lgm_vlb_term: the row by value, output row out_row.  lgm_vlb_term_table: the row is table[stride * counter[0] ...] = (A, S, R,
 *   Rm1, P1, P2, kind, KC, KW, inv_std, ., .) (stride >= 12; lgm_hip.likelihood.vlb_plan), the output row counter[0]; a counter
 *   outside [0, n_rows) writes nothing; advance != 0 appends counter[0] += 1.  Both launch vlb_term_kernel. */
int lgm_vlb_term(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch, int x_off,
                 const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip, float A, float S, float R,
                 float Rm1, float P1, float P2, int kind, float KC, float KW, float inv_std, float* out, int n_rows,
                 int out_row, void* stream);
int lgm_vlb_term_table(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch, int x_off,
                       const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip, const float* table,
                       int stride, const int32_t* counter, float* out, int n_rows, int advance, void* stream);

/* ---------------------------------------------------------------------------------------
 * Learned variance (Nichol & Dhariwal 2021; the reference's Unet(learned_variance=True), which its diffusion never trains):
 * the network output v [B, HW, v_pitch] carries 2 C lanes, [0, C) the objective's prediction and [C, 2 C) the interpolation
 * coefficient.  The model's log-variance of an element is lv = f * log_beta + (1 - f) * log_tilde with f = (v + 1) / 2 (f outside
 * [0, 1] is legal), log_beta = log beta_t and log_tilde = posterior_log_variance_clipped[t], log beta~_1 at t = 0.  One device
 * function (csrc/elementwise.hip learned_term) gives the bound's term of an element in nats and its derivative in lv:
 *   t >= 1  KL = 0.5 (-1 + lv - lv_q + exp(lv_q - lv) + d^2 exp(-lv)), d = P1 (x0_pred - x0), lv_q = log_tilde
 *   t = 0   -log p of lgm_vlb_term's decoder with standard deviation exp(0.5 lv); the derivative in the same cancellation-free
 *           form, 0 where the probability is floored at 1e-12
 * lgm_hybrid_loss_fwd / _bwd (training): L = mean_b(lw[t_b] mse_b) + vb_weight mean_b(vb_b); mse_b = mean over lanes [0, C) of
 *   (out - target)^2 as lgm_weighted_mse_fwd forms it, vb_b = mean(term) / ln 2 at t_b with the model mean P1 x0_pred + P2 x_t
 *   detached and built from the UNCLIPPED x0_pred.  out [B, HW, pitch >= 2 C], target [B, HW, target_pitch >= C], img NCHW dense
 *   (x0 = img * 2 - 1 when normalize), x_t in lanes [x_off, x_off + C) of xin [B, HW, x_pitch]; the four head tables and
 *   loss_weight (NULL => 1) as lgm_model_predictions_obj takes them; tab [n_table][8] = (log beta_t, log_tilde, lv_q, P1, P2, 0,
 *   0, 0) (GaussianDiffusion.learned_table).  fwd: one workgroup per sample, fixed-order sums, no atomics; per [2][B] =
 *   (lw mse_b, vb_b); loss [1] (optional) by a one-workgroup second stage.  bwd: elementwise over the pitch; gout lanes [0, C)
 *   exactly what lgm_weighted_mse_bwd writes, lanes [C, 2 C) = gloss * vb_weight / (B * C * HW * ln 2) * dterm/dlv * 0.5 * (log_beta
 *   - log_tilde), every other lane 0.  They launch hybrid_loss_fwd_kernel (+ hybrid_mean_kernel) / hybrid_loss_bwd_kernel.
 * lgm_sample_step_learned / lgm_sample_step_table_learned (ancestral sampling): lgm_sample_step_slice / _table_slice with clip
 *   set and the row (A, Bv, R, Rm1, P1, P2, log_beta, log_tilde): x_{t-1} = P1 x0 + P2 x_t + exp(0.5 lv) noise, lv per element;
 *   log_tilde = -inf marks the step without noise (t = 0).  x0_out (optional, pitch = `pitch`) as lgm_sample_step_thresh.  The
 *   same launch of sample_step_slice_kernel as every other update.
 * lgm_vlb_term_learned (likelihood): lgm_vlb_term / lgm_vlb_term_table behind one entry point (table != NULL: row counter[0],
 *   else the scalars) for kind 3 (KL) and 4 (decoder) of a learned-variance network; table rows carry log_beta / log_tilde in
 *   slots 10 / 11.  v_pitch >= 2 C.  lgm_vlb_term_table given such a row for an output without the head writes nothing. */
int lgm_hybrid_loss_fwd(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                        int normalize, const float* xin, int64_t x_pitch, int x_off, const int64_t* t,
                        const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                        const float* loss_weight, const float* tab, int n_table, int objective, float vb_weight, int B,
                        int C, int HW, float* per, float* loss, void* stream);
int lgm_hybrid_loss_bwd(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                        int normalize, const float* xin, int64_t x_pitch, int x_off, const int64_t* t,
                        const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                        const float* loss_weight, const float* tab, int n_table, int objective, float vb_weight,
                        const float* gloss, int B, int C, int HW, float* gout, void* stream);
int lgm_sample_step_learned(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                            int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW, int objective,
                            float A, float Bv, float R, float Rm1, float P1, float P2, float log_beta, float log_tilde,
                            void* stream);
int lgm_sample_step_table_learned(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                                  const float* noise, int B, int C, int HW, const float* table, const int32_t* counter,
                                  int objective, int advance, void* stream);
int lgm_vlb_term_learned(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch, int x_off,
                         const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip, float A, float S,
                         float R, float Rm1, float P1, float P2, int kind, float log_beta, float log_tilde,
                         const float* table, int stride, const int32_t* counter, float* out, int n_rows, int out_row,
                         int advance, void* stream);

/* ---------------------------------------------------------------------------------------
 * Timestep samplers of the training step (GaussianDiffusion(t_sampler=...); Nichol & Dhariwal 2021, 3.3 and Kingma et al. 2021,
 * VDM App. I.1).  State of the loss-aware sampler: history [T][H] float32 (per timestep its last H per-sample losses, oldest
 * first), counts [T] int32 (entries held, at most H).  The PLAN the next draw reads: cdf [T], iw [T] float32.
 * lgm_tsampler_draw: t_out [B] int64.  mode 0 (stratified): u [1], u_b = u[0] + (float) b / (float) B (a division, then an add),
 *   minus 1 where that is >= 1, t_b = min(T - 1, floor((float) T u_b)); cdf is not read.  mode 1 (cdf): u [B], t_b = the first index
 *   with cdf[t] > u_b by binary search, T - 1 where there is none.  Launches tsampler_draw_kernel.
 * lgm_tsampler_update: ONE launch of ONE workgroup (tsampler_update_kernel), no atomics.  Phase one: L_b = per[b] (n_terms 1) or
 *   per[b] + vb_weight * per[B + b] (n_terms 2; product and sum rounded separately) is appended to row t_b in batch order; a row
 *   keeps its last H entries, counts[t] = min(H, counts[t] + 1); a non-finite L_b or a t_b outside [0, T) is not recorded.  The
 *   batch is staged in LDS 1024 samples at a time, every thread scans it for the rows it owns (t mod 1024): no two writers per
 *   row.  Phase two, from the updated state: warm = every counts[t] == H; w_t = sqrt(mean_h history[t][h]^2); not warm, or
 *   sum(w) zero or not finite: p_t = 1 / T and iw_t = 1.0f exactly; else p_t = (1 - q) w_t / sum(w) + q / T, iw_t = 1 / (T p_t).
 *   cdf = inclusive prefix sum of p in a fixed two-level sequential order (never decreasing), clamped to 1, cdf[T - 1] = 1.0f.
 *   Every sum is float32 in a fixed association: replays, eager launches and every CU margin give the same bits.  B == 0 (t and
 *   per may be NULL) rebuilds the plan only.  cdf must not alias any other operand.  T <= 2^20.
 * The loss under the plan, mean_b(iw[t_b] L_b): the *_iw forms launch the per-sample kernels of their plain forms unchanged (per
 *   holds the UNWEIGHTED terms), then iw_mean_kernel, which also writes wb [B] = iw[t_b] (t clamped to [0, n_table)) for the
 *   backward; the *_bwd_iw forms are the plain launches with every element of sample b multiplied by wb[b] at the end.  With
 *   iw = 1 the loss and the gradient are the plain forms' bit for bit. */
int lgm_tsampler_draw(const float* u, const float* cdf, int T, int mode, int64_t* t_out, int B, void* stream);
int lgm_tsampler_update(const int64_t* t, const float* per, int n_terms, float vb_weight, float* history, int32_t* counts,
                        int H, float q, int T, int B, float* cdf, float* iw, void* stream);
int lgm_weighted_mse_fwd_iw(const float* out, const float* target, int64_t pitch, const int64_t* t, const float* loss_weight,
                            const float* iw, int n_table, int B, int C, int HW, int Cpad, float* per_sample, float* wb,
                            float* loss, void* stream);
int lgm_weighted_mse_bwd_iw(const float* out, const float* target, int64_t pitch, const int64_t* t, const float* loss_weight,
                            const float* wb, const float* gloss, int B, int C, int HW, int Cpad, float* gout, void* stream);
int lgm_hybrid_loss_fwd_iw(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                           int normalize, const float* xin, int64_t x_pitch, int x_off, const int64_t* t,
                           const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                           const float* loss_weight, const float* tab, int n_table, int objective, float vb_weight,
                           const float* iw, int B, int C, int HW, float* per, float* wb, float* loss, void* stream);
int lgm_hybrid_loss_bwd_iw(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                           int normalize, const float* xin, int64_t x_pitch, int x_off, const int64_t* t,
                           const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                           const float* loss_weight, const float* tab, int n_table, int objective, float vb_weight,
                           const float* wb, const float* gloss, int B, int C, int HW, float* gout, void* stream);

/* ---------------------------------------------------------------------------------------
 * Non-fused Winograd engine (csrc/winograd_eng.hip): input transform launch -> ONE batched weight-stationary fp32 MFMA GEMM
 * -> output transform launch, for the layers the fused Winograd kernels' workgroup shapes cannot fill:
 *   f43      3x3 / stride 1 / pad 1 as F(4x4, 3x3) (Block.proj ddpm.py:160 on the 4 x 4 maps: one tile per image);
 *   f42 xy   4x4 / stride 2 / pad 1 Conv2d forward (Discriminator dcgan.py:150-158) as F(4x4, 2x2) on the four pixel phases of
 *            the input, the phases summed inside the GEMM (k = (2p + q) * C + c): 100 products per 16 outputs instead of 256;
 *   f42 yx   the same layer's input gradient = ConvTranspose2d forward (Generator dcgan.py:79-87): four per-phase problems.
 * Tensors: V[xi][T][K], U[xi][N][K] (prepared by the caller: lgm_hip/weng.py), M[xi][T][N], all dense fp32; T = tiles.
 * ------------------------------------------------------------------------------------- */
/* C[b][m][n] = sum_k A[b][m][k] * Bm[b][n][k], b < batch (strides in floats).  K, lda, ldb, batch strides % 4 == 0. */
int lgm_weng_gemm(const float* A, const float* Bm, float* C, int M, int N, int K, int lda, int ldb, int ldc, int batch,
                  int64_t a_batch, int64_t b_batch, int64_t c_batch, void* stream);
/* The same kernel as ONE un-split GEMM with a bias / residual epilogue: C[m][n] = bias[n] + res[m][ldr ...] + sum_k A[m][k] Bm[n][k]
 * (a 1x1 Conv2d / Linear: ddpm.py:96-103, 187, 213-215, 252-253; weights [N][K] as the library stores them; res may alias C). */
int lgm_weng_gemm_epi(const float* A, const float* Bm, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                      const float* bias, const float* res, int ldr, void* stream);
/* x [B][H][W][C] (pitch) -> V[36][T][C], T = B (H/4) (W/4);  M[36][T][N] -> y [B][H][W][N] (pitch) + bias */
int lgm_weng_f43_in(const float* x, int64_t x_pitch, int B, int H, int W, int C, float* V, void* stream);
int lgm_weng_f43_out(const float* M, int B, int H, int W, int N, const float* bias, float* y, int64_t y_pitch,
                     void* stream);
/* x [B][H][W][C] -> V[25][T][4C], T = B (H/8) (W/8);  M[25][T][N] -> y [B][H/2][W/2][N] + bias */
int lgm_weng_f42_in_xy(const float* x, int64_t x_pitch, int B, int H, int W, int C, float* V, void* stream);
int lgm_weng_f42_out_xy(const float* M, int B, int Ho, int Wo, int N, const float* bias, float* y, int64_t y_pitch,
                        void* stream);
/* dy [B][Ho][Wo][Ny] -> V[4][25][T][Ny], T = B (Ho/4) (Wo/4);  M[4][25][T][C] -> dx [B][2 Ho][2 Wo][C] + bias */
int lgm_weng_f42_in_yx(const float* dy, int64_t pitch, int B, int Ho, int Wo, int Ny, float* V, void* stream);
int lgm_weng_f42_out_yx(const float* M, int B, int Ho, int Wo, int C, const float* bias, float* dx, int64_t pitch,
                        void* stream);
/* The output transforms with LgmPostOp's elementwise part in them: out = act(v + bias) (act 0 / 3 ReLU / 4 LeakyReLU), then
 * * (mask > 0 ? 1 : mask_slope) with mask = a saved activation of the output's shape (NULL: none). */
int lgm_weng_f42_out_xy_post(const float* M, int B, int Ho, int Wo, int N, const float* bias, float* y, int64_t y_pitch,
                             int act, float slope, const float* mask, int64_t mask_pitch, float mask_slope, void* stream);
int lgm_weng_f42_out_yx_post(const float* M, int B, int Ho, int Wo, int C, const float* bias, float* dx, int64_t pitch,
                             int act, float slope, const float* mask, int64_t mask_pitch, float mask_slope, void* stream);
/* U of a 4x4 / stride-2 layer for both directions from its weights w [Nw][16][Cw] (float64 arithmetic, rounded once):
 * Uxy [25][Nw][4 Cw], Uyx [4][25][Cw][Nw]; either may be NULL. */
int lgm_weng_f42_weights(const float* w, int Nw, int Cw, float* Uxy, float* Uyx, void* stream);

/* ---------------------------------------------------------------------------------------
 * Vector quantiser (VQ-VAE) — models/modules/vector_quantizer.py.
 * x: latents as [N = B*H*W, D] rows (NHWC), codebook [K, D].
 * ------------------------------------------------------------------------------------- */
/* _quantize :53-60: indices[n] = argmin_k ( ||x_n||^2 + ||e_k||^2 - (2 x_n).e_k ), int64, lowest
 * index on ties; min_dist optional.  The [N,K] distance matrix is never materialised. */
int lgm_vq_assign(const float* x, int64_t x_pitch, const float* codebook, int N, int K, int D,
                  int64_t* indices, float* min_dist, void* stream);
/* one-hot^T @ x and one-hot.sum(0) (:132-143) without the one-hot: dw [K,D], counts [K];
 * deterministic (rows visited in ascending order). */
int lgm_vq_segment_sum(const float* x, int64_t x_pitch, const int64_t* indices, int N, int K, int D,
                       float* dw, float* counts, void* stream);
/* VectorQuantizerEMA._ema_update :128-147 (in place on the two buffers and the codebook). */
int lgm_vq_ema_update(float* cluster_size, float* ema_embedding, float* codebook,
                      const float* counts, const float* dw, int K, int D, float decay, float eps,
                      void* stream);
/* q[n] = codebook[indices[n]]; out3 = { vq_loss = mse + commitment*mse (:76-78),
 * perplexity (:87-88), mse }.  workspace: lgm_vq_gather_workspace bytes. */
int64_t lgm_vq_gather_workspace(int N, int D);
int lgm_vq_gather_loss(const float* x, int64_t x_pitch, const float* codebook,
                       const int64_t* indices, const float* counts, int N, int K, int D,
                       float commitment, float* q, int64_t q_pitch, float* out3, void* workspace,
                       void* stream);
/* Backward: gx = gq (straight-through :90-93, optional) + g*commitment*2(x-q)/(ND);
 * gcodebook = beta*gcodebook + g*2(counts*e - dw)/(ND);  g = *g_vq_loss (device scalar). */
int lgm_vq_bwd(const float* x, int64_t x_pitch, const float* q, int64_t q_pitch, const float* gq,
               int64_t gq_pitch, const float* codebook, const float* dw, const float* counts,
               const float* g_vq_loss, float commitment, int N, int K, int D, float* gx,
               int64_t gx_pitch, float* gcodebook, float gcb_beta, void* stream);

/* ---------------------------------------------------------------------------------------
 * Train-mode BatchNorm2d primitives over [M = B*H*W, C] NHWC matrices (dcgan.py:86-90,158-161)
 * and the WGAN-GP loss pieces (wgan.py:84-156).  xhat = (a - mean) * rstd per channel.
 * ------------------------------------------------------------------------------------- */
int64_t lgm_bn_workspace(int64_t rows, int C);
/* batch mean / rstd (biased variance, eps), running stats updated with torch semantics */
int lgm_bn_stats(const float* a, int64_t a_pitch, int64_t rows, int C, float eps, float momentum,
                 float* mean, float* rstd, float* running_mean, float* running_var, void* workspace,
                 void* stream);
/* BatchNorm statistics folded into the producing convolution (dcgan.py:86-90,158-161: Conv2d / ConvTranspose2d
 * followed by BatchNorm2d): lgm_conv_xy_stats / lgm_conv_yx_stats are lgm_conv_xy / lgm_conv_yx without bias and
 * residual that also leave, per row tile, (sum, squared deviations from the tile's mean, rows) of every output
 * column in stats[tile][3][C]; *stats_tiles = tiles written, 0 when this geometry cannot (then call lgm_bn_stats).
 * stats holds lgm_conv_stats_floats(g, yx) floats.  lgm_bn_stats_from_tiles finishes mean / rstd / running stats. */
int64_t lgm_conv_stats_floats(const LgmConvGeom* g, int yx);
int lgm_conv_xy_stats(const LgmConvGeom* g, const float* x, int64_t x_pitch, const float* w, float* y,
                      int64_t y_pitch, void* workspace, int64_t workspace_bytes, float* stats,
                      int* stats_tiles, void* stream);
int lgm_conv_yx_stats(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* w,
                      const float* w_t, float* x, int64_t x_pitch, void* workspace, int64_t workspace_bytes,
                      float* stats, int* stats_tiles, void* stream);
int lgm_bn_stats_from_tiles(const float* partial, int ntiles, int C, int64_t rows, float eps, float momentum,
                            float* mean, float* rstd, float* running_mean, float* running_var,
                            void* stream);
/* sums3 = [sum v1, sum v1*xhat, sum v1*v2] per channel ([3][C]); a / v2 optional */
int lgm_bn_reduce3(const float* v1, int64_t v1_pitch, const float* v2, int64_t v2_pitch,
                   const float* a, int64_t a_pitch, const float* mean, const float* rstd,
                   int64_t rows, int C, float* sums3, void* workspace, void* stream);
/* per-channel coefficient vectors coef4 = [A1,A2,A3,A4][C]:
 * mode 0: BN backward operator T(v) = c (v - mean v - xhat mean(v xhat)); optional ggamma/gbeta
 *         (= beta_acc*old + sums) and m_out = [mean v, mean v*xhat];
 * mode 1: adjoint of T's dependence on the batch statistics (gradient-penalty second order). */
int lgm_bn_coef(int mode, const float* sums3, const float* gamma, const float* rstd,
                const float* saved_m, int C, int64_t M, float* coef4, float* ggamma, float* gbeta,
                float beta_acc, float* m_out, void* stream);
/* lgm_bn_reduce3 followed by lgm_bn_coef, the coefficient math run inside the second reduction stage (two
 * launches): modes bit 0 -> mode-0 set into coef8[0..4C) with ggamma0 / gbeta0 / m_out, bit 1 -> mode-1 set into
 * coef8[4C..8C) with ggamma1 (needs saved_m).  sums3 (optional) also receives [S1,S2,S3]. */
int lgm_bn_reduce3_coef(int modes, const float* v1, int64_t v1_pitch, const float* v2, int64_t v2_pitch,
                        const float* a, int64_t a_pitch, const float* mean, const float* rstd,
                        const float* gamma, const float* saved_m, int64_t rows, int C, float* coef8,
                        float* ggamma0, float* gbeta0, float beta_acc0, float* m_out, float* ggamma1,
                        float beta_acc1, float* sums3, void* workspace, void* stream);
/* the same second stage over partial sums a convolution's epilogue left (LgmPostOp.bn_partial, `tiles` row tiles) */
int lgm_bn_reduce3_coef_tiles(int modes, const float* partial, int tiles, const float* gamma, const float* rstd,
                              const float* saved_m, int64_t rows, int C, float* coef8, float* ggamma0, float* gbeta0,
                              float beta_acc0, float* m_out, float* ggamma1, float beta_acc1, float* sums3, void* stream);
/* out_k = A1k*v1 + A2k*v2 + A3k*xhat + A4k for the two coefficient sets of coef8 = [2][4][C] (set 0 without its
 * v2 term), one pass over v1, v2, a */
int lgm_bn_affine3x2(const float* v1, int64_t v1_pitch, const float* v2, int64_t v2_pitch, const float* a,
                     int64_t a_pitch, const float* mean, const float* rstd, const float* coef8, float* out0,
                     int64_t out0_pitch, float* out1, int64_t out1_pitch, int64_t rows, int C, void* stream);
/* out (+)= act( A1*v1 + A2*v2 + A3*xhat + A4 )   (any of the terms optional = NULL) */
int lgm_bn_affine3(const float* v1, int64_t v1_pitch, const float* v2, int64_t v2_pitch,
                   const float* a, int64_t a_pitch, const float* mean, const float* rstd,
                   const float* A1, const float* A2, const float* A3, const float* A4, float* out,
                   int64_t out_pitch, int accumulate, int act, float slope, int64_t rows, int C,
                   void* stream);
/* Input pipeline of the reference DataModule on the device (data/datamodule.py:41-53, data/utils.py:7-35):
 * src u8 [B,H,W,C] (decoded images) -> dst fp32 NCHW [B,C,S,S] = Normalize(ToTensor(.)), centre-cropped to
 * min(H,W), resized to SxS (bilinear, antialias=True), flipped horizontally where flip[b] != 0 (NULL: none). */
int lgm_image_transform(const unsigned char* src, int64_t B, int H, int W, int C, const unsigned char* flip,
                        float* dst, int S, void* stream);
/* interpolated_images = alpha*x + (1-alpha)*x_hat (wgan.py:137), alpha [B] */
int lgm_lerp_rows(const float* x, const float* y, const float* alpha, float* out, int64_t B,
                  int64_t rowlen, void* stream);
/* gradient penalty with the reference's channel-only norm (wgan.py:153-156):
 * loss_out = lambda * mean_p (||g_p||_c - 1)^2 ; gbar = d(gscale*loss)/dg.  g, gbar dense NHWC4. */
int64_t lgm_gp_penalty_workspace(int64_t npix);
int lgm_gp_penalty(const float* g, int64_t npix, int C, float lambda, const float* gscale,
                   float* loss_out, float* gbar, void* workspace, void* stream);
/* R1 regulariser on real data (r1gan.py:74-77): loss_out = 0.5 * mean_b sum_{chw} g^2 (the caller
 * applies hparams.r1_penalty); gbar = d(gscale*loss)/dg = gscale/B * g.  g, gbar dense NHWC4 with a
 * zero padding lane; workspace as lgm_gp_penalty_workspace(npix). */
int lgm_r1_penalty(const float* g, int64_t npix, int64_t B, const float* gscale, float* loss_out,
                   float* gbar, void* workspace, void* stream);
/* out = scale * mean_i v[i*pitch]  (critic score means, wgan.py:85-87) */
int lgm_mean_col(const float* v, int64_t pitch, int64_t n, float scale, float* out, void* stream);
/* out[r][c] = (c == col) ? scale * (vptr ? *vptr : 1) : 0 */
int lgm_fill_col(float* out, int64_t pitch, int64_t n, int ncols, int col, float scale,
                 const float* vptr, void* stream);
/* vals4 = (real, fake, gp, d_loss): d_loss = fake - real + gp (wgan.py:87,98) */
int lgm_wgan_dloss(float* vals4, void* stream);
/* VQVAE._common_step's scalar tail (vqvae.py:184-194) in one launch: vals4 = (recon * w_recon + vq * w_vq, recon, vq,
 * perplexity) with out3 = (vq_loss, perplexity, .) as lgm_vq_gather_loss leaves it; and its mirror image for the
 * backward pass: out2 = (g * w0, g * w1). */
int lgm_vqvae_loss(const float* recon, const float* out3, float w_recon, float w_vq, float* vals4, void* stream);
/* The same from the per-sample reconstruction terms lgm_weighted_mse_fwd leaves (its `loss` may be NULL: no mean launch):
 * their mean is taken here, in mean_kernel's order. */
int lgm_vqvae_loss_samples(const float* per_sample, int n, const float* out3, float w_recon, float w_vq, float* vals4,
                           void* stream);
/* VQ-VAE decoder end (vqvae.py:85-88, :130): x_hat = tanh(pre) and the per-sample reconstruction terms in one pass; and
 * its backward with the loss weights folded in - gpre = d loss / d pre for loss = w_recon mse + ..., g2 = (gloss w_recon,
 * gloss w_vq) left for the quantiser's backward (lgm_vq_bwd's g_vq_loss = g2 + 1). */
int lgm_tanh_mse_fwd(const float* pre, const float* target, int64_t pitch, int B, int C, int HW, int Cpad, float* xh,
                     float* per_sample, void* stream);
int lgm_tanh_mse_bwd(const float* xh, const float* target, int64_t pitch, const float* gloss, float w_recon, float w_vq,
                     int B, int C, int HW, int Cpad, float* gpre, float* g2, void* stream);

/* The VQ-VAE's ResidualStack forward in ONE launch (models/modules/residual.py:5-43; vqvae.py:45-47, :71-73): per layer
 * y = relu(conv3x3(cur)), cur' = relu(conv1x1(y) + cur).  x [B,H,W,Cin] arrives with the first in-place ReLU applied;
 * w3[l] [Rh][9][Cin], w1[l] [hidden][1][Rh] (the flat parameter layouts, no bias); y[l] [B,H,W,Rh] and z[l]
 * [B,H,W,hidden] (contiguous) receive every layer's two activations (the backward pass reads them).  Built for 4 x 4
 * maps, Cin = hidden = 128, Rh = 32, <= 4 layers (lgm_resstack_fwd_supported). */
int64_t lgm_resstack_fwd_supported(int H, int W, int Cin, int hidden, int Rh, int layers);
int lgm_resstack_fwd(const float* x, int64_t x_pitch, int B, int H, int W, int Cin, int hidden, int Rh, int layers,
                     const float* const* w3, const float* const* w1, float* const* y, float* const* z, void* stream);
int lgm_scale_pair(const float* g, float w0, float w1, float* out2, void* stream);

/* ---------------------------------------------------------------------------------------
 * OPT-IN split-precision 3x3 convolution (SURVEY.md "bf16x3 ... behind a flag, only if it holds 1e-4";
 * never used unless the caller asks for it): each fp32 operand is split exactly into three bf16 pieces
 * and the product evaluated with six bf16 MFMAs and fp32 accumulation (fp32-level error, measured in
 * tests/test_hip_bf16x3.py).  Same contract as lgm_conv_xy / lgm_conv_yx for 3x3 / stride 1 / pad 1
 * (Block.proj ddpm.py:160-171 and its input gradient), except that the weights are passed as the three
 * planes produced by lgm_split_bf16x3 from the fp32 weights [Nw][9][Cw] (mode 0, forward) or from their
 * transposed copy [Cw][9][Nw] (mode 1, input gradient); plane p starts at w_planes + p*plane_elems.
 * ------------------------------------------------------------------------------------- */
int64_t lgm_conv3x3_bf16x3_supported(const LgmConvGeom* g, int mode, int64_t a_pitch);   /* 1 / 0 */
/* table rows (int32 x 5): element offset of the slot (same in src and in every dst plane), rows, taps, K,
 * first chunk; rows %% 32 == 0, K %% 16 == 0; total_chunks = sum rows*taps*K/8.  The planes are written in the
 * MFMA fragment order the kernel reads (one contiguous 1 KB read per wave and fragment). */
int lgm_split_bf16x3(const float* src, uint16_t* dst, const int32_t* table, int n_slots, int64_t total_chunks,
                     int64_t plane_elems, void* stream);
int lgm_conv3x3_bf16x3(int mode, const LgmConvGeom* g, const float* a, int64_t a_pitch,
                       const uint16_t* w_planes, int64_t plane_elems, const float* bias, const float* res,
                       int64_t res_pitch, float* out, int64_t out_pitch, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Winograd F(2x2, 3x3) convolution in exact fp32 arithmetic (csrc/winograd.hip): the 3x3 / stride 1 / pad 1
 * layers (Block.proj ddpm.py:160-171, Upsample's conv :93-97, the last stages' 3x3 convs :377,413) and their
 * input gradients with 2.25x fewer MFMA FLOPs than the direct form.  Same contract as lgm_conv_xy (yx = 0) /
 * lgm_conv_yx (yx = 1) except that the weights are passed TRANSFORMED: U = G g G^T in MFMA fragment order, as
 * lgm_wino_weights writes them.
 *   lgm_wino_weights: table rows (int64 x 6) = source offset (floats) of a slot w[Np][9][Cp] inside `src`,
 *   Np, Cp (both multiples of 32), destination offset of the forward operand inside dst_f (Np*Cp*16 floats,
 *   layout [Np/32][Cp/8][16][2][32][4]), destination offset of the input-gradient operand inside dst_b
 *   (mirrored taps, roles of Np / Cp swapped), first block; one block per 32 x 32 (n, c) tile, total_blocks =
 *   sum Np/32 * Cp/32.  Either destination may be NULL.
 * ------------------------------------------------------------------------------------- */
int64_t lgm_conv3x3_wino_supported(const LgmConvGeom* g, int yx);   /* 1 / 0 (dense operands fit 32-bit offsets) */
/* 1 when the caller's pitched operands also fit the kernel's 32-bit byte offsets (res_pitch 0: no residual) */
int64_t lgm_conv3x3_wino_fits(const LgmConvGeom* g, int64_t a_pitch, int64_t out_pitch, int64_t res_pitch);
/* Partial form: the split-K planes stay in `workspace` for a consumer that sums them itself (lgm_gn_fwd_planes /
 * lgm_gn_bwd_planes) - no reducer launch, and the split count is planned without its cost.  partial[0] = planes
 * left (1: none, `out` is complete incl. bias), partial[1] = plane stride in floats.  With planes, `out` is not
 * written and `bias` not applied (the consumer adds it). */
int64_t lgm_conv3x3_wino_workspace_partial(const LgmConvGeom* g, int yx);
/* Backward PAIR of a 3x3 layer (autograd's conv backward, Block.proj ddpm.py:160-171): the input gradient
 * gx = W^T * gy (+ res) and the weight / bias gradient gw = beta*gw + gy (x) x in ONE launch - at the per-GPU batches
 * of a strong-scaled run each of them fills a fraction of the chip and is latency-bound, side by side they take
 * the time of one.  Same kernels' code and arithmetic as lgm_conv3x3_wino(yx = 1) + lgm_conv_wgrad: bit-identical.
 * u_b = the input-gradient operand lgm_wino_weights writes; dgrad_ws / partial as lgm_conv3x3_wino[_partial]
 * (partial NULL: finished gx); workspace sizes from lgm_conv3x3_wino_bwd_workspaces; desc NULL: gw complete on return, else
 * the deferred form of lgm_conv_wgrad_deferred. */
int64_t lgm_conv3x3_wino_bwd_supported(const LgmConvGeom* g, int64_t gy_pitch, int64_t x_pitch, int64_t gx_pitch,
                                       int64_t res_pitch);
/* out[0] / out[1] = bytes of dgrad_ws / wgrad_ws the pair needs (its two split counts are planned jointly, so they
 * differ from the stand-alone kernels'); partial != 0: for the partial-planes form */
int lgm_conv3x3_wino_bwd_workspaces(const LgmConvGeom* g, int partial, int64_t* out);
int lgm_conv3x3_wino_bwd(const LgmConvGeom* g, const float* gy, int64_t gy_pitch, const float* x, int64_t x_pitch,
                         const float* u_b, const float* res, int64_t res_pitch, float* gx, int64_t gx_pitch,
                         void* dgrad_ws, int64_t dgrad_ws_bytes, int64_t* partial, float* gw, float* gbias, float beta,
                         void* wgrad_ws, int64_t wgrad_ws_bytes, int64_t* desc, void* stream);
/* Weight gradients of TWO 3x3 layers in one launch (deferred slab reduction: both descriptors as lgm_conv_wgrad_deferred
 * fills them): the chip's workgroups are shared in proportion to the layers' work, each workgroup takes twice the pixels
 * with one prologue and one slab - for the large-map layers whose weights are small and whose input gradient runs apart
 * (lgm_conv3x3_wino4).  Workspace sizes: lgm_conv3x3_wino_wgrad2_workspaces. */
int64_t lgm_conv3x3_wino_wgrad2_supported(const LgmConvGeom* ga, const LgmConvGeom* gb);
/* The same for 2 ... 4 layers (up to 8 when every layer takes the F(4x4) weight-gradient kernel).  LgmWgradItem = one
 * layer's arguments of lgm_conv_wgrad_deferred. */
typedef struct {
  const LgmConvGeom* g;
  const float* y;
  int64_t y_pitch;
  const float* x;
  int64_t x_pitch;
  float* gw;
  float* gbias;
  float beta;
  void* ws;
  int64_t ws_bytes;
  int64_t* desc;
} LgmWgradItem;
/* ABI 7.  The same for the weight / bias gradients of 2 ... 4 1x1 convolutions (reference: autograd's backward of res_conv
 * ddpm.py:187, to_out :215,253, to_qkv :213,252): ONE launch of the streaming 1x1 weight-gradient kernel, every layer on its
 * share of the chip.  All layers must take that kernel on their own (channel counts in whole 64-blocks, whole 64-pixel
 * chunks) and use the same block tile (Nw % 128 and Cw % 128 agree).  Descriptors as lgm_conv_wgrad_deferred (desc[6] = 1:
 * that layer's gradient is complete on return). */
int64_t lgm_wgrad1x1_group_supported(int n, const LgmConvGeom* const* geoms);
/* ABI 7.  Stand-alone launches of the generic weight-gradient kernel may wait for each other (per calling thread): while
 * the queue is ON, lgm_conv_wgrad_deferred / lgm_conv_bwd_pair[_post] with a descriptor do not launch that kernel but queue
 * it; four queued layers - or lgm_wgrad_queue_flush - issue ONE launch with the layers' grids one after the other (each
 * layer's own plan: results are bit-identical to separate launches).  The caller keeps the operands (y, x, workspaces)
 * alive until the flush and flushes before lgm_wgrad_reduce_batch / any reader of the gradients.  lgm_wgrad_queue_enable
 * returns the previous state (on < 0: switch off AND discard what is queued - the start of a pass, in case an earlier one
 * was abandoned half-way); the queue is OFF by default.  (Reference: autograd's weight gradients of the 1x1 / 7x7 /
 * 2x2 convolutions and linears, ddpm.py:103,180,304,330-332,422 - none is read before the optimizer step.) */
int lgm_wgrad_queue_enable(int on);
int lgm_wgrad_queue_flush(void);
int lgm_wgrad1x1_group_workspaces(int n, const LgmConvGeom* const* geoms, int64_t* out);     /* bytes per layer */
int lgm_wgrad1x1_group(int n, const LgmWgradItem* items, void* stream);
int64_t lgm_conv3x3_wino_wgradn_supported(int n, const LgmConvGeom* const* geoms);
int lgm_conv3x3_wino_wgradn_workspaces(int n, const LgmConvGeom* const* geoms, int64_t* out);
int lgm_conv3x3_wino_wgradn(int n, const LgmWgradItem* items, void* stream);
int lgm_conv3x3_wino_wgrad2_workspaces(const LgmConvGeom* ga, const LgmConvGeom* gb, int64_t* out);   /* bytes, a / b */
int lgm_conv3x3_wino_wgrad2(const LgmConvGeom* ga, const float* ya, int64_t ya_pitch, const float* xa, int64_t xa_pitch,
                            float* gwa, float* gba, float beta_a, void* wsa, int64_t wsa_bytes, int64_t* desca,
                            const LgmConvGeom* gb, const float* yb, int64_t yb_pitch, const float* xb, int64_t xb_pitch,
                            float* gwb, float* gbb, float beta_b, void* wsb, int64_t wsb_bytes, int64_t* descb,
                            void* stream);
int lgm_conv3x3_wino_partial(int yx, const LgmConvGeom* g, const float* a, int64_t a_pitch, const float* u,
                             const float* bias, float* out, int64_t out_pitch, void* workspace,
                             int64_t workspace_bytes, int64_t* partial, void* stream);
int64_t lgm_conv3x3_wino_workspace(const LgmConvGeom* g, int yx);   /* split-K partial outputs (bytes) */
int lgm_wino_weights(const float* src, float* dst_f, float* dst_b, const int64_t* table, int n_slots,
                     int64_t total_blocks, void* stream);
/* diagnostic only: buf != NULL makes lgm_conv3x3_wino run its cycle-stamped build (64 int64 per workgroup) */
int lgm_wino_set_debug_buffer(void* buf, int mode);
int lgm_conv3x3_wino(int yx, const LgmConvGeom* g, const float* a, int64_t a_pitch, const float* u,
                     const float* bias, const float* res, int64_t res_pitch, float* out, int64_t out_pitch,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Winograd F(4x4, 3x3) convolution in fp32 (csrc/winograd4.hip): the same layers and the same contract as
 * lgm_conv3x3_wino on the LARGE maps (16 x 16, or H % 16 == 0 and W % 32 == 0; reduction channels % 32, produced
 * channels % 64): 2.25 multiplies per output instead of 4, 1.78x fewer MFMA FLOPs than F(2x2, 3x3) (reference ops:
 * Block.proj ddpm.py:157-173 and its input gradient).  fp32 throughout; error against float64 a few 1e-6 of the output
 * scale (interpolation points 0, +-1, +-2, inf).  Weights are passed TRANSFORMED by lgm_wino4_weights:
 *   table rows as lgm_wino_weights; forward operand Np*Cp*36 floats, layout [Np/64][Cp/8][36][2][2][32][4]; input-gradient
 *   operand with mirrored taps and the roles of Np / Cp swapped; one block per 32 x 32 (n, c) tile.
 * ------------------------------------------------------------------------------------- */
int64_t lgm_conv3x3_wino4_supported(const LgmConvGeom* g, int yx);
int64_t lgm_conv3x3_wino4_workspace(const LgmConvGeom* g, int yx);   /* split-K partial outputs (bytes) */
/* 1 when this layer is expected to run faster here than through lgm_conv3x3_wino (measured table: enough units to fill
 * the chip without deep split-K); callers take F(4x4) only then */
int64_t lgm_conv3x3_wino4_preferred(const LgmConvGeom* g, int yx);
/* partial form, as lgm_conv3x3_wino_partial (same workspace size as lgm_conv3x3_wino4_workspace) */
int lgm_conv3x3_wino4_partial(int yx, const LgmConvGeom* g, const float* a, int64_t a_pitch, const float* u,
                              const float* bias, float* out, int64_t out_pitch, void* workspace,
                              int64_t workspace_bytes, int64_t* partial, void* stream);
/* Forward with the consumer GroupNorm's raw statistics from the epilogue: floats the `stats` buffer needs (0: this
 * geometry does not take it - maps that are multiples of 16 x 32, an unsplit reduction) and the rows per image;
 * lgm_gn_fwd_stats consumes them.  No residual operand. */
int64_t lgm_conv3x3_wino4_stats_floats(const LgmConvGeom* g, int* parts_per_image);
int lgm_conv3x3_wino4_stats(const LgmConvGeom* g, const float* x, int64_t x_pitch, const float* u, const float* bias,
                            float* y, int64_t y_pitch, float* stats, int64_t stats_floats, void* stream);
int lgm_wino4_weights(const float* src, float* dst_f, float* dst_b, const int64_t* table, int n_slots,
                      int64_t total_blocks, void* stream);
/* diagnostic only: buf != NULL makes lgm_conv3x3_wino4 run its cycle-stamped build (32 int64 per workgroup) */
int lgm_wino4_set_debug_buffer(void* buf, int exp);   /* exp: attribution build (drops parts of the phase: wrong results) */
int lgm_conv3x3_wino4(int yx, const LgmConvGeom* g, const float* a, int64_t a_pitch, const float* u,
                      const float* bias, const float* res, int64_t res_pitch, float* out, int64_t out_pitch,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* The same convolution (same operands, same U from lgm_wino4_weights, same contract) from LIGHT workgroups
 * (csrc/winograd4l.hip; reference ops as above, ddpm.py:157-173): 16-tile units, 256 threads, one wave per SIMD, 74 KB of LDS,
 * so that two fit a CU and one fits beside a foreign resident workgroup (a collective's kernel).  Maps 8 x 8 (B % 4 == 0),
 * 16 x 16, or H % 8 == 0 and W % 32 == 0.  Direct entry points for tests and tools; lgm_conv3x3_wino4* choose between the
 * two workgroup sizes themselves (LGM_WINO4_LIGHT). */
/* diagnostic / tests: 1 = light workgroups wherever they take the geometry, 0 = 32-tile workgroups only, -1 = what the
 * environment says (LGM_WINO4_LIGHT; default: light when WORLD_SIZE > 1).  Process-wide; callers that cache plans (split counts, workspace sizes)
 * must not flip it between a size query and the launch it sizes. */
int lgm_wino4_set_light(int mode);

/* Workgroup slots the launch planners leave to a collective resident beside the step (one process per GPU, RCCL's kernel
 * holds a CU per channel): split-K / slab / persistent-range plans are sized for 256 - margin CUs.  Default: LGM_CU_MARGIN,
 * else 16 when WORLD_SIZE > 1, else 0; margin < 0 returns to that default; margin <= 128.  Plans made before the call keep
 * their grids (captured graphs included).  lgm_cu_margin() reads the value in force. */
int lgm_set_cu_margin(int margin);
int lgm_cu_margin(void);
int64_t lgm_conv3x3_wino4l_supported(const LgmConvGeom* g, int yx);
int64_t lgm_conv3x3_wino4l_workspace(const LgmConvGeom* g, int yx);   /* split-K partial outputs (bytes) */
int lgm_conv3x3_wino4l(int yx, const LgmConvGeom* g, const float* a, int64_t a_pitch, const float* u,
                       const float* bias, const float* res, int64_t res_pitch, float* out, int64_t out_pitch,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Weight gradient of those layers in F(4x4,3x3) form (csrc/winograd4_wgrad.hip; maps with W % 16 == 0, H % 4 == 0,
 * Nw % 64 == 0, Cw % 32 == 0): dU = sum over tiles of (A dY A^T) (.) (B^T x B), dw = G^T dU G, fused bias sums.  Slabs only:
 * `workspace` receives desc[6] slabs for the batched fixed-order reducer; desc as lgm_conv_wgrad_deferred fills it. */
int64_t lgm_conv3x3_wino4_wgrad_supported(const LgmConvGeom* g);
int64_t lgm_conv3x3_wino4_wgrad_workspace(const LgmConvGeom* g);
int lgm_conv3x3_wino4_wgrad(const LgmConvGeom* g, const float* y, int64_t y_pitch, const float* x, int64_t x_pitch,
                            float* gw, float* gbias, float beta, void* workspace, int64_t workspace_bytes,
                            int64_t* desc, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser kernels on flat storage.
 * torch.optim.Adam (coupled L2; decoupled=1 gives AdamW) — ddpm.py:1053-1059, vqvae.py:207-214,
 * wgan.py:183-195.  step: 1-based count (host value, or read from step_dev when non-NULL).
 * b1, b2 are the caller's doubles: torch forms 1 - beta and 1 - beta^step in doubles, and so do these (a float32 0.999
 * puts 1 - b2 off by 1.3e-5).  Host step and step_dev give the same bits.
 * ------------------------------------------------------------------------------------- */
int lgm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1,
                  double b2, float eps, float weight_decay, float step, const float* step_dev,
                  float grad_scale, int decoupled, void* stream);
/* torch.optim.RMSprop with its defaults (momentum 0, not centred) - the critic / generator optimiser
 * of the weight-clipping WGAN (wgan.py:171-181): sq = alpha*sq + (1-alpha)*g^2; p -= lr*g/(sqrt(sq)+eps) */
int lgm_rmsprop_step(float* p, const float* g, float* sq, int64_t n, float lr, double alpha, float eps,
                     float weight_decay, float grad_scale, void* stream);
/* WGAN weight clipping, param.data.clamp_(-c, c) over the critic's flat parameter buffer (wgan.py:158-168) */
int lgm_clamp(float* x, int64_t n, float lo, float hi, void* stream);
/* ema_pytorch.EMA.update (ddpm.py:1047-1048): shadow += (online - shadow) * w; w = 1 copies online bit for bit, w = 0
 * leaves the shadow's bits */
int lgm_ema_lerp(float* shadow, const float* online, int64_t n, float w, void* stream);
int lgm_add_scalar(float* x, float a, void* stream);
int lgm_fill(float* x, int64_t n, float val, void* stream);

/* ---------------------------------------------------------------------------------------
 * The gradient tail: global-norm clipping (torch.nn.utils.clip_grad_norm_, norm type 2, error_if_nonfinite=False) and
 * gradient accumulation, between "the flat gradient is final" and the Adam launch.  No host read anywhere.
 *
 * lgm_grad_sqnorm_partial: sum of g^2 as per-workgroup partial sums in double (products and sums formed in double from the
 * first add: at most n * 2^-53 relative).  Workgroup b covers the contiguous span [b * span, (b + 1) * span) and writes ONE
 * double to partials[b]; lgm_grad_sqnorm_span(n) and lgm_grad_sqnorm_partials(n) = ceil(n / span) are host-only queries that
 * depend on n alone (not on lgm_cu_margin()).  No atomics: two runs give equal bits.  g 16-byte aligned.
 * lgm_grad_clip_scale: ONE workgroup sums `count` partials (those of several flat buffers laid end to end) in a fixed tree
 * and forms, in double, norm = |grad_scale| sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)) (NaN propagates, an infinite
 * norm gives 0), out2[0] = (float)(grad_scale * coef), out2[1] = (float)norm.
 * lgm_adam_step_scaled: lgm_adam_step with the gradient scale read from scale_dev[0] (= out2) in place of grad_scale; the
 * same kernel, the same bits for the same scale.  Weight decay is applied after the scale.
 * lgm_grad_accumulate: dst = overwrite ? src : dst + src over a flat 16-byte aligned slice (one float add per element).
 * ------------------------------------------------------------------------------------- */
int64_t lgm_grad_sqnorm_span(int64_t n);
int64_t lgm_grad_sqnorm_partials(int64_t n);
int lgm_grad_sqnorm_partial(const float* g, int64_t n, double* partials, void* stream);
int lgm_grad_clip_scale(const double* partials, int64_t count, float grad_scale, float max_norm,
                        float* out2, void* stream);
int lgm_adam_step_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1,
                         double b2, float eps, float weight_decay, float step, const float* step_dev,
                         const float* scale_dev, int decoupled, void* stream);
int lgm_grad_accumulate(float* dst, const float* src, int64_t n, int overwrite, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dropout without a mask tensor (additions under ABI 8; csrc/lgm_philox.h).
 * For an activation [B, HW, C] (C % 4 == 0) the mask is a pure function of (key, layer, pass, element):
 *   n = (b HW + pix) C + c (the logical index, pitches play no part), q = n >> 2 as a 64-bit number,
 *   Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) of
 *   counter (q & 0xffffffff, q >> 32, layer, pass) under key (key[0], key[1]) gives four words = channels c .. c + 3,
 *   an element is kept iff its word >= thr, thr = min(2^32 - 1, floor(p 2^32)); kept -> fl32(v * scale), dropped -> +0,
 *   scale = float32(1 / (1 - p)).  `key`: DEVICE pointer to two uint32 (8-byte aligned), read by the kernels, so that a graph
 *   replay sees the key its own draw wrote.  `thr` crosses as int64 (0 ... 2^32 - 1).
 * lgm_dropout_fwd / lgm_dropout_bwd: in place on a pitched tensor (the activation / the gradient arriving for it).
 * lgm_gn_fwd_drop: lgm_gn_fwd (planes == NULL) or lgm_gn_fwd_planes whose stored y goes through the mask, in the same launch on
 *   the one-pass plans (lgm_gn_plan nv > 0); on the two-pass plans lgm_dropout_fwd's kernel follows on y.
 * lgm_gn_bwd_drop: lgm_gn_bwd / lgm_gn_bwd_deferred (gy given, gy_planes NULL) or lgm_gn_bwd_planes (gy NULL) whose gy goes
 *   through the mask as it is loaded (planes: after they are summed).  On the two-pass plans lgm_dropout_bwd's kernel masks
 *   gy IN PLACE first: gy must be the caller's to overwrite.  rows / desc: both NULL or both given.
 * ------------------------------------------------------------------------------------- */
int lgm_dropout_fwd(float* x, int64_t pitch, int B, int HW, int C, const void* key, int layer, int pass, int64_t thr,
                    float scale, void* stream);
int lgm_dropout_bwd(float* g, int64_t pitch, int B, int HW, int C, const void* key, int layer, int pass, int64_t thr,
                    float scale, void* stream);
int lgm_gn_fwd_drop(const float* planes, int64_t plane_stride, int splits, const float* conv_bias, float* x,
                    int64_t x_pitch, int B, int HW, int C, int G, float eps, const float* gamma, const float* beta,
                    const float* ss, int64_t ss_pitch, int act, const float* res, int64_t res_pitch, float* y,
                    int64_t y_pitch, float* mean, float* rstd, float* coefA, float* coefB, const void* key, int layer,
                    int pass, int64_t thr, float scale, void* stream);
int lgm_gn_bwd_drop(const float* x, int64_t x_pitch, float* gy, int64_t gy_pitch, const float* gy_planes,
                    int64_t plane_stride, int splits, int B, int HW, int C, int G, const float* gamma, const float* beta,
                    const float* ss, int64_t ss_pitch, int act, const float* mean, const float* rstd, const float* coefA,
                    const float* coefB, float* gx, int64_t gx_pitch, int accumulate_gx, float* ggamma, float* gbeta,
                    float affine_beta, float* gss, int64_t gss_pitch, float gss_beta, float* workspace, float* rows,
                    int64_t* desc, const void* key, int layer, int pass, int64_t thr, float scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * Elucidated diffusion (csrc/edm.hip; Karras et al. 2022, Table 1 "Ours" and Algorithm 2; an extension of the reference) and
 * the reference's random / learned Fourier embedding of a real-valued time (ddpm.py:135-151) its network reads.  With
 * s_d = sigma_data: c_in = 1 / sqrt(s^2 + s_d^2), c_skip = s_d^2 / (s^2 + s_d^2), c_out = s s_d / sqrt(s^2 + s_d^2), c_noise = ln(s) / 4,
 * D(x, s) = c_skip x + c_out F(c_in x, c_noise).  Buffers are NHWC with their pitch in floats; the network's input buffer holds
 * c_in x in lanes [x_off, x_off + C) (r4(C) lanes from x_off must lie inside the pitch, the padding behind the C lanes is zeroed);
 * the target, the sample state x, x^ and d are buffers of their own with r4(C) written lanes a pixel (padding zero); img and
 * noise are dense NCHW.  Every product, quotient and sum rounds once (no contraction), in the order written.  16-byte accesses
 * when every base is 16-byte aligned and every pitch and offset a multiple of 4, else one lane per thread: the same bits.
 * No atomics.  B <= 65535.
 * lgm_edm_qsample: s_b = exp(P_mean + P_std n_b), c_noise_b = (P_mean + P_std n_b) / 4 from the normal draw n [B]; y = img
 *   (2 img - 1 when normalize), x = y + s eps; c_in x into the input buffer, F* = (y - c_skip x) / c_out into the target, s and
 *   c_noise into sigma_out / cnoise_out [B].  lgm_edm_qsample_sigma: the same with s [B] given, c_noise = log(s) / 4.  Both launch
 *   edm_qsample_kernel.
 * A sampling step's row is 16 floats (lgm_hip.edm.edm_plan, float64 rounded once):
 *     (s_i, s^, coef = sqrt(s^^2 - s_i^2) S_noise, s',  c_in, c_noise, c_skip, c_out at s^,  the same four at s' (zeros when s' = 0),
 *      dt = s' - s^, gamma, 0, 0)
 *   by value (`row`, 16 host floats) or row counter[0] of the 16-byte aligned device `table`; exactly one of the two is given.
 * lgm_edm_pre: x^ = x + coef eps where noise is given and coef != 0, else x^ = x; c_in(s^) x^ into the input buffer, cnoise[b] =
 *   c_noise(s^).  xhat is a buffer of its own (not x).  Launches edm_pre_kernel.
 * lgm_edm_euler: D = c_skip(s^) x^ + c_out(s^) F (clamped to [-1, 1] when clip), d = (x^ - D) / s^, x' = x^ + dt d into the state x.
 *   second: also d, c_in(s') x' into the input buffer and cnoise[b] = c_noise(s') (d, xin, cnoise may be NULL otherwise).  advance
 *   (table form, not with second): counter[0] += 1 behind the launch.  Launches edm_euler_kernel.
 * lgm_edm_heun: D' = c_skip(s') x' + c_out(s') F' with x' read from the state (clamped when clip), d' = (x' - D') / s',
 *   x_next = x^ + dt ((d + d') / 2) into the state.  advance as above.  Launches edm_heun_kernel.
 * lgm_fourier_emb_fwd: out[b] = (x_b, sin(f_b0) .. sin(f_b,half-1), cos(f_b0) .. cos(f_b,half-1)), f_bd = ((x_b w_d) 2) pi in
 *   float32, lanes [2 half + 1, pitch) zero; x [B] float32.  Launches fourier_emb_fwd_kernel.
 * lgm_fourier_emb_bwd: gweights[d] = beta gweights[d] + 2 pi sum_b x_b (cos_bd g_sin_bd - sin_bd g_cos_bd) from the forward's own
 *   rows `emb` and the gradient rows `gemb`, summed over b in ascending order by one workgroup: the same bits on every run.
 *   Launches fourier_emb_bwd_kernel.
 * ------------------------------------------------------------------------------------- */
int lgm_edm_qsample(const float* img, const float* noise, const float* n, float P_mean, float P_std, float sigma_data,
                    int normalize, float* xin, int64_t pitch, int x_off, float* target, int64_t target_pitch, float* sigma_out,
                    float* cnoise_out, int B, int C, int HW, void* stream);
int lgm_edm_qsample_sigma(const float* img, const float* noise, const float* sigma, float sigma_data, int normalize, float* xin,
                          int64_t pitch, int x_off, float* target, int64_t target_pitch, float* sigma_out, float* cnoise_out,
                          int B, int C, int HW, void* stream);
int lgm_edm_pre(const float* x, int64_t state_pitch, const float* noise, const float* row, const float* table,
                const int32_t* counter, float* xhat, float* xin, int64_t pitch, int x_off, float* cnoise, int B, int C, int HW,
                void* stream);
int lgm_edm_euler(const float* F, int64_t f_pitch, const float* xhat, int64_t state_pitch, const float* row, const float* table,
                  int32_t* counter, int clip, int second, float* x, float* d, float* xin, int64_t pitch, int x_off, float* cnoise,
                  int advance, int B, int C, int HW, void* stream);
int lgm_edm_heun(const float* F, int64_t f_pitch, const float* xhat, const float* d, int64_t state_pitch, const float* row,
                 const float* table, int32_t* counter, int clip, float* x, int advance, int B, int C, int HW, void* stream);
int lgm_fourier_emb_fwd(const float* x, const float* weights, int B, int half, float* out, int64_t pitch, void* stream);
int lgm_fourier_emb_bwd(const float* emb, int64_t pitch, const float* gemb, int64_t gpitch, int B, int half, float* gweights,
                        float beta, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gated PixelCNN prior over the VQ-VAE's codes (csrc/pixelcnn.hip; reference models/generative/autoregressive/pixelcnn.py:
 * MaskedConv2d :8-23, GatedBlock :26-45, PixelCNN :48-106).
 * Masked convolutions: geometry as the convolution family's with stride 1, odd KH = KW and pad = KH / 2; NHWC fp32 operands
 * with pitches (16-byte aligned, pitch % 4 == 0), weight [Nw][KH*KW][Cw].  A type-A / type-B mask keeps the taps whose
 * row-major index kh KW + kw is below taps_live = (KH / 2) KW + KW / 2 + [type B] (24 / 25 of 49 for 7 x 7): the kernels stop
 * at tap taps_live - 1 and NEVER read a weight at a tap index >= taps_live.  Exact fp32 on v_mfma_f32_32x32x2_f32; a wave
 * owns its output tile's whole reduction in a fixed order; only the weight gradient splits its reduction, into runs of
 * positions whose count follows from the geometry alone (2048 positions a run, at most 16), their slabs added in ascending
 * order by a second launch.  No atomics: the same bits on every run and under every lgm_set_cu_margin.
 * lgm_mconv_xy: y = conv_live(x, w) + bias (bias optional).  Launches mconv_xy_kernel.
 * lgm_mconv_yx: gx = conv_live^T(gy, w) + res (res optional, may alias gx).  Launches mconv_yx_kernel.
 * lgm_mconv_wgrad: gw[n][t][c] = beta gw + sum_m gy[m, n] x[m + d(t), c] for t < taps_live, positions in ascending order;
 *   the dead taps receive exact zeros when beta == 0 and are left alone otherwise; gbias (optional) = beta gbias + sum_m gy.
 *   Launches mconv_wgrad_kernel (+ mconv_wgrad_reduce_kernel, mconv_dead_zero_kernel, mconv_bias_grad_kernel).
 * lgm_mconv_zero_dead: exact zeros into the taps >= taps_live of a weight gradient [Nw][KH*KW][Cw] that lgm_conv_wgrad wrote on
 *   zero-masked weights (the route of a shape on which the generic kernel is the faster one).  Launches mconv_dead_zero_kernel.
 * lgm_gated_fwd: y[m, h] = x[m, h] + tanh(a) sigmoid(b), (a, b) = pre[m, h], pre[m, H + h]; H % 4 == 0, 16-byte accesses.
 * lgm_gated_bwd: (ga, gb) = (gy s (1 - t^2), gy t s (1 - s)) into lanes [0, H), [H, 2H) of gpre (which may be pre itself);
 *   gx (optional) += gy.
 * lgm_softmax_xent_fwd: per row m of logits [M, K]: lse[m] = log sum_k exp(l_k), loss_rows[m] = lse[m] - l[target[m]] (NaN for
 *   a target outside [0, K)); mean (optional) = sum_m loss_rows[m] / M by ONE workgroup in a fixed order.  One wave per row.
 * lgm_softmax_xent_bwd: glogits[m, k] = (exp(l_k - lse[m]) - [k == target[m]]) gloss[0] / M for k < K, 0 for K <= k < lanes.
 * lgm_pixelcnn_step: one layer at the ONE position p = counter[0] (read on the device; outside [0, H W): nothing is written):
 *   o[b, n] = bias[n] + sum_{t < taps_live} sum_c w[n][t][c] cache_in[b, p + d(t), c], zeros outside the map, one workgroup
 *   row per tap into `workspace` (lgm_pixelcnn_step_workspace bytes), the taps' planes added in ascending order.  gate: the
 *   result is cache_in[b, p, h] + tanh(o[b, h]) sigmoid(o[b, Nw / 2 + h]) (Nw / 2 lanes), else o (Nw lanes); out_at_p: `out` is a
 *   [B, H, W, .] map written at p, else a [B, .] matrix.  taps_live = 1 on a 1 x 1 geometry is a plain 1 x 1 layer.
 *   Launches pixelcnn_step_partial_kernel + pixelcnn_step_finish_kernel.
 * lgm_categorical_draw: one wave per sample: e_k = exp(logits[b, k] / temperature - max); the class drawn is the first with
 *   e_k > 0 whose cumulative sum (ascending classes, fixed order) exceeds u[b] sum_k e_k, else the last class with e_k > 0.  codes[b, p] =
 *   the class (int64, codes [B, HW]); lanes [0, C) of xin[b, p] = codebook[class] (or float(class) when codebook is NULL);
 *   advance: counter[0] += 1 behind the launch.  Launches categorical_draw_kernel.
 * ------------------------------------------------------------------------------------- */
int lgm_mconv_xy(const LgmConvGeom* g, int taps_live, const float* x, int64_t x_pitch, const float* w, const float* bias,
                 float* y, int64_t y_pitch, void* stream);
int lgm_mconv_yx(const LgmConvGeom* g, int taps_live, const float* gy, int64_t gy_pitch, const float* w, const float* res,
                 int64_t res_pitch, float* gx, int64_t gx_pitch, void* stream);
int64_t lgm_mconv_wgrad_workspace(const LgmConvGeom* g, int taps_live);   /* bytes of the slabs (0: one run) */
int lgm_mconv_wgrad(const LgmConvGeom* g, int taps_live, const float* gy, int64_t gy_pitch, const float* x, int64_t x_pitch,
                    float* gw, float* gbias, float beta, void* workspace, int64_t workspace_bytes, void* stream);
int lgm_mconv_zero_dead(const LgmConvGeom* g, int taps_live, float* gw, void* stream);
int lgm_gated_fwd(const float* x, int64_t x_pitch, const float* pre, int64_t pre_pitch, int64_t M, int H, float* y,
                  int64_t y_pitch, void* stream);
int lgm_gated_bwd(const float* gy, int64_t gy_pitch, const float* pre, int64_t pre_pitch, int64_t M, int H, float* gx,
                  int64_t gx_pitch, float* gpre, int64_t gpre_pitch, void* stream);
int lgm_softmax_xent_fwd(const float* logits, int64_t pitch, const int64_t* target, int64_t M, int K, float* loss_rows,
                         float* lse, float* mean, void* stream);
int lgm_softmax_xent_bwd(const float* logits, int64_t pitch, const int64_t* target, const float* lse, const float* gloss,
                         int64_t M, int K, int lanes, float* glogits, int64_t g_pitch, void* stream);
int64_t lgm_pixelcnn_step_workspace(const LgmConvGeom* g, int taps_live);
int lgm_pixelcnn_step(const LgmConvGeom* g, int taps_live, int gate, const float* cache_in, int64_t in_pitch, const float* w,
                      const float* bias, const int32_t* counter, float* out, int64_t out_pitch, int out_at_p, void* workspace,
                      int64_t workspace_bytes, void* stream);
int lgm_categorical_draw(const float* logits, int64_t pitch, int B, int K, float temperature, const float* u,
                         const float* codebook, int64_t cb_pitch, int C, int HW, int32_t* counter, int64_t* codes, float* xin,
                         int64_t xin_pitch, int advance, void* stream);

/* ---- Fully connected layers with few rows, and the MLP VAE's heads and loss (csrc/dense.hip; reference vae.py:15-215) -----
 * Activations are row-major [B, pitch] float32; an OUTPUT has pitch >= round_up(C, 4) and its pad lanes [C, round_up(C, 4))
 * are written 0; an INPUT needs pitch >= C only and may start at any 4-byte address (x.view(B, C S S) of an NCHW batch).
 * Weights [N, K] in FlatParams' layout [Np][Kp] (16-byte aligned; padding rows are never read), vectors padded to 4.
 * act: LGM_ACT_NONE, LGM_ACT_RELU, LGM_ACT_LRELU (slope) or LGM_ACT_TANH.  All sums have a fixed order that depends on the shape alone
 * (not on lgm_cu_margin()); no atomics, no workgroup waits for another.  rc < 0 before any launch on a null pointer,
 * B < 1, a pitch below the channel count, an unknown act or a workspace that is too small.
 * lgm_dense_fwd   y = act(x W^T + bias) (bias may be NULL).  Launches dense_gemm_kernel (+ dense_reduce_kernel when the
 *   reduction is split: lgm_dense_fwd_workspace(B, K, N) > 0 bytes of partial planes).
 * lgm_dense_bwd   g = gy * act'(y) with act' read from the saved output y (LeakyReLU: y > 0 ? 1 : slope; tanh: 1 - y^2; y may
 *   be NULL for LGM_ACT_NONE);  gb = beta gb + colsum(g) (gb may be NULL);  gx = g W (gx may be NULL: first layer) from wt, the
 *   transposed copy [Kp][Np] of the weights;  gw = beta gw + g^T x.  Launches dense_g_kernel, dense_gemm_kernel
 *   (+ dense_reduce_kernel), dense_gw_kernel.  16-byte aligned workspace of lgm_dense_bwd_workspace bytes.
 * lgm_vae_head_fwd   mu = h Wmu^T + bmu, log_var = h Wlv^T + blv, z = mu + eps exp(log_var / 2) ([B][round_up(L, 4)] each,
 *   eps [B][L]), kld_part[b] = sum_j 1 + log_var - mu^2 - exp(log_var) (j ascending).  One launch: vae_head_fwd_kernel.
 * lgm_vae_head_bwd   with c = kld_weight gloss[0] / (B L): gmu = gz + c mu, glv = gz eps 0.5 exp(log_var / 2) +
 *   c 0.5 (exp(log_var) - 1); gh = gmu Wmu + glv Wlv; the two heads' gw / gb = beta . + (as lgm_dense_bwd).  Launches
 *   vae_head_g_kernel, vae_head_gh_kernel, 2 x dense_g_kernel, 2 x dense_gw_kernel.
 * lgm_tanh_l1_fwd   xh = tanh(pre), row_part[b] = sum_d |xh - x|.   lgm_tanh_l1_bwd   gpre = sign(xh - x) (gloss[0] / (B D))
 *   (1 - xh^2), sign(0) = 0.   lgm_vae_loss   vals3 = (recon + kld_weight kld, recon = sum(row_part) / (B D),
 *   kld = -0.5 sum(kld_part) / (B L)), one wave, fixed order.
 * ------------------------------------------------------------------------------------- */
int64_t lgm_dense_fwd_workspace(int B, int K, int N);
int lgm_dense_fwd(const float* x, int64_t x_pitch, const float* w, const float* bias, int B, int K, int N, int act,
                  float slope, float* y, int64_t y_pitch, void* workspace, int64_t workspace_bytes, void* stream);
int64_t lgm_dense_bwd_workspace(int B, int K, int N, int need_gx);
int lgm_dense_bwd(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* x, int64_t x_pitch,
                  const float* wt, int B, int K, int N, int act, float slope, float* gx, int64_t gx_pitch, float* gw,
                  float* gb, float beta, void* workspace, int64_t workspace_bytes, void* stream);
int lgm_vae_head_fwd(const float* h, int64_t h_pitch, const float* w_mu, const float* b_mu, const float* w_lv,
                     const float* b_lv, const float* eps, int B, int K, int L, float* mu, float* log_var, float* z,
                     float* kld_part, void* stream);
int64_t lgm_vae_head_bwd_workspace(int B, int L);
int lgm_vae_head_bwd(const float* gz, const float* mu, const float* log_var, const float* eps, const float* gloss,
                     float kld_weight, const float* h, int64_t h_pitch, const float* w_mu, const float* w_lv, int B, int K,
                     int L, float* gh, int64_t gh_pitch, float* gw_mu, float* gb_mu, float* gw_lv, float* gb_lv, float beta,
                     void* workspace, int64_t workspace_bytes, void* stream);
int lgm_tanh_l1_fwd(const float* pre, int64_t pre_pitch, const float* x, int64_t x_pitch, int B, int D, float* xh,
                    int64_t xh_pitch, float* row_part, void* stream);
int lgm_tanh_l1_bwd(const float* xh, int64_t xh_pitch, const float* x, int64_t x_pitch, const float* gloss, int B, int D,
                    float* gpre, int64_t gpre_pitch, void* stream);
int lgm_vae_loss(const float* row_part, const float* kld_part, int B, int D, int L, float kld_weight, float* vals3,
                 void* stream);
/* lgm_dense_dgrad   the input gradient of lgm_dense_bwd alone (gx = (gy * act'(y)) W from wt; no gw, no gb): the sweep
 *   through a network whose parameters are not being updated.  Same launches, same bits in gx; a workspace of
 *   lgm_dense_bwd_workspace(B, K, N, 1) bytes. */
int lgm_dense_dgrad(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* wt, int B, int K, int N,
                    int act, float slope, float* gx, int64_t gx_pitch, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ---- BatchNorm1d over few rows and the MLP GAN's loss head (csrc/bn1d.hip; reference gan/gan.py:15-89, :258-308) ----------
 * Activations as in the dense section: row-major [B, pitch] float32, an OUTPUT has pitch >= round_up(F, 4) and its pad lanes
 * are written 0, an INPUT needs pitch >= F only and its pad lanes are never read.  gamma, beta, running_*, mean, rstd: [F].
 * One launch each; one workgroup owns 32 columns and all B rows (lgm_bn1d_supported: 1 <= B <= 512).  Every sum has a fixed
 * order that depends on (B, F) alone (not on lgm_cu_margin()); no atomics, no workgroup waits for another.
 * act: LGM_ACT_NONE or LGM_ACT_LRELU (slope).  rc < 0 before any launch on a null pointer, an unsupported B, a pitch below
 * the feature count, an unknown act, or training with B = 1.
 * lgm_bn1d_fwd   training: mean = sum_b a / B, var = sum_b (a - mean)^2 / B (centred, from the rows held on chip),
 *   rstd = 1 / sqrt(var + eps), running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with
 *   var B / (B - 1);  eval (training = 0): mean = running_mean, rstd = 1 / sqrt(running_var + eps), nothing else is written
 *   to the running statistics.  y = act(gamma ((a - mean) rstd) + beta); mean and rstd are outputs (the backward reads them).
 * lgm_bn1d_bwd   g = gy * act'(y) (act' from the saved output y; y may be NULL for LGM_ACT_NONE), xhat = (a - mean) rstd,
 *   s1 = sum_b g, s2 = sum_b g xhat;  gbeta = beta_acc gbeta + s1, ggamma = beta_acc ggamma + s2;
 *   ga = (gamma rstd) ((g - s1 / B) - xhat (s2 / B)) - the backward of the training-mode forward.
 * lgm_gan_bce_d   bce(s, t) = max(s, 0) - s t + log1p(exp(-|s|)).  vals5 = (mean_b bce(real, 1), mean_b bce(fake, 0), their
 *   mean, mean real, mean fake); score vectors are column 0 of a [B, pitch] matrix.  One wave, fixed order.
 * lgm_gan_bce_g   vals2 = (g_loss, mean s): loss_type 0 (non-saturating) mean bce(s, 1), 1 (min-max) -mean bce(s, 0).
 * lgm_gan_bce_bwd  g_k[b][0] = (gloss[0] factor_k / B) (sigmoid(s_k[b]) - t_k), t_k in {0, 1}, lanes 1 .. 3 of the row 0;
 *   k = 0 and, when s1 / g1 are given, k = 1 in the same launch (the discriminator loss: factors 0.5, targets 1 and 0).
 * ------------------------------------------------------------------------------------- */
int64_t lgm_bn1d_supported(int B, int F);
int lgm_bn1d_fwd(const float* a, int64_t a_pitch, int B, int F, const float* gamma, const float* beta, float eps,
                 float momentum, int training, int act, float slope, float* running_mean, float* running_var, float* y,
                 int64_t y_pitch, float* mean, float* rstd, void* stream);
int lgm_bn1d_bwd(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* a, int64_t a_pitch,
                 const float* mean, const float* rstd, const float* gamma, int B, int F, int act, float slope, float* ga,
                 int64_t ga_pitch, float* ggamma, float* gbeta, float beta_acc, void* stream);
int lgm_gan_bce_d(const float* real, int64_t real_pitch, const float* fake, int64_t fake_pitch, int B, float* vals5,
                  void* stream);
int lgm_gan_bce_g(const float* s, int64_t pitch, int B, int loss_type, float* vals2, void* stream);
int lgm_gan_bce_bwd(const float* s0, int64_t s0_pitch, float t0, float factor0, float* g0, int64_t g0_pitch, const float* s1,
                    int64_t s1_pitch, float t1, float factor1, float* g1, int64_t g1_pitch, int B, const float* gloss,
                    void* stream);

/* ---- The denoising autoencoder: corruption, tanh + squared error, loss (csrc/dae.hip; reference autoencoder/dae.py) -------
 * Its Linear layers are lgm_dense_fwd / _bwd with LGM_ACT_RELU (the dense section accepts it: y = v > 0 ? v : +0, the
 * derivative from the saved output y > 0 ? 1 : 0).  Activations as in the dense section: row-major [B, pitch] float32, an
 * OUTPUT has pitch >= round_up(D, 4) and its pad lanes are written +0, an INPUT needs pitch >= D only, may start at any
 * 4-byte address and its pad lanes are never read (16-byte accesses where every operand's base and pitch allow them, guarded
 * scalar ones otherwise: the same bits).  No atomics, no workgroup waits for another, every sum in a fixed order that depends
 * on (B, D) alone; no product is contracted into a sum.  B, D <= 2^20 and B round_up(D, 4) <= 2^31.  rc < 0 before any
 * launch on a null pointer, B or D out of that range, a pitch below D, an output whose span of B rows shares a byte with an
 * input's span, an unknown mode or a negative level.
 * lgm_dae_corrupt        out = fl(x + fl(noise * level)): two roundings (torch's x + randn_like(x) * level).
 * lgm_dae_corrupt_mask   the corruption is drawn in registers by Philox4x32-10 (csrc/lgm_philox.h) under the 64-bit key that
 *   `key` (device, int64 [1]) holds when the kernel runs.  Element n = b D + d (the logical index), q = n >> 2:
 *   w_s = philox(counter = (q lo, q hi, 0, 0))[n & 3], w_p = philox(counter = (q lo, q hi, 1, 0))[n & 3].
 *   mode 0 (salt_and_pepper): out = w_p < thr ? 0 : (w_s < thr ? 1 : x), thr = lgm_dae_mask_threshold(0, level)
 *     = min(2^32 - 1, floor(level / 2 * 2^32));  mode 1 (masking): out = w_s < thr ? 0 : x, thr = min(2^32 - 1,
 *     floor(level * 2^32)).  Untouched elements keep x's bits.  lgm_dae_mask_threshold is host-only (-1: bad mode or level).
 * lgm_dae_tanh_mse_fwd   xh = tanhf(pre), row_part[b] = sum_d (x - xh)^2.  (lgm_tanh_mse_fwd is the VQ-VAE's NHWC kernel.)
 * lgm_dae_tanh_mse_bwd   gpre = ((2 gloss[0] / (B D)) (xh - x)) (1 - xh^2), gloss on the device; 0 where xh == x.
 * lgm_dae_loss           vals[0] = sum_b row_part[b] / (B D): one wave, lane l adds rows l, l + 64, .., then a fixed tree.
 * ------------------------------------------------------------------------------------- */
int lgm_dae_corrupt(const float* x, int64_t x_pitch, const float* noise, int64_t noise_pitch, float level, int B, int D,
                    float* out, int64_t out_pitch, void* stream);
int64_t lgm_dae_mask_threshold(int mode, double level);
int lgm_dae_corrupt_mask(const float* x, int64_t x_pitch, const int64_t* key, int mode, double level, int B, int D,
                         float* out, int64_t out_pitch, void* stream);
int lgm_dae_tanh_mse_fwd(const float* pre, int64_t pre_pitch, const float* x, int64_t x_pitch, int B, int D, float* xh,
                         int64_t xh_pitch, float* row_part, void* stream);
int lgm_dae_tanh_mse_bwd(const float* xh, int64_t xh_pitch, const float* x, int64_t x_pitch, const float* gloss, int B, int D,
                         float* gpre, int64_t gpre_pitch, void* stream);
int lgm_dae_loss(const float* row_part, int B, int D, float* vals, void* stream);

/* ---- The NICE flow: additive coupling, scaling layer, log-likelihood (csrc/nice.hip; reference flow/nice.py) ---------------
 * The coupling nets' Linear layers are lgm_dense_fwd / _bwd with LGM_ACT_LRELU; their conditioning half and the gradient
 * of the shifted half are pitched views of the state buffers.  Activations as in the dense section: row-major [B, pitch]
 * float32; an output has pitch >= round_up(D, 4) and its pad lanes are written +0; an input needs pitch >= D, may start at
 * any 4-byte address, and its pad lanes are never read.  16-byte accesses where every operand's base, pitch and lane offset
 * allow them, guarded scalar ones otherwise: the same bits.  No atomics; every sum runs in a fixed order that depends on
 * (B, D) alone; no product is contracted into a sum.  1 <= B, D <= 2^20 with B round_up(D, 4) <= 2^31.  rc < 0 before any
 * launch on a null pointer, B or D out of that range, a slice outside [0, D), a pitch below its lane count, or an output
 * whose span of B rows shares a byte with an input's span (lgm_nice_couple alone accepts out == x with equal pitches).
 * lgm_nice_couple     out[b][d] = fl(x[b][d] + sign t[b][d - off]) for d in [off, off + n), x[b][d]'s bits elsewhere;
 *   sign is +1 or -1; one rounding.  The forward, the inverse (sign = -1) and the backward (g[:, cond] += gx, in place).
 * lgm_nice_scale_fwd  z = fl(h expf(reverse ? -log_scale[d] : log_scale[d])), row_part[b] = sum_d z^2: a thread adds the
 *   elements of quads t, t + 256, .. in ascending d, then a fixed tree over the workgroup.  row_part may be NULL (the inverse).
 * lgm_nice_loss       one wave.  vals3 = (loss, mean_ll, sum_d log_scale[d]), mean_ll = (-0.5 sum_b row_part[b]) / B -
 *   fl(0.5 D log 2 pi); loss = -(mean_ll + sum) with exact, -(mean_ll - sum) (the reference's sign) without.
 * lgm_nice_scale_bwd  c = gloss[0] / B (gloss on the device): gh = (c z) expf(log_scale[d]);
 *   gls[d] = beta gls[d] + (sum_b (c z[b][d]) z[b][d] + (exact ? -gloss[0] : gloss[0])), b ascending from 0, any B; beta = 0
 *   overwrites.  gls holds D floats; nothing is written beyond them.
 * ------------------------------------------------------------------------------------- */
int lgm_nice_couple(const float* x, int64_t x_pitch, const float* t, int64_t t_pitch, int B, int D, int off, int n, int sign,
                    float* out, int64_t out_pitch, void* stream);
int lgm_nice_scale_fwd(const float* h, int64_t h_pitch, const float* log_scale, int B, int D, int reverse, float* z,
                       int64_t z_pitch, float* row_part, void* stream);
int lgm_nice_loss(const float* row_part, const float* log_scale, int B, int D, int exact, float* vals3, void* stream);
int lgm_nice_scale_bwd(const float* z, int64_t z_pitch, const float* log_scale, const float* gloss, int B, int D, int exact,
                       float* gh, int64_t gh_pitch, float* gls, float beta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGM_HIP_H */
