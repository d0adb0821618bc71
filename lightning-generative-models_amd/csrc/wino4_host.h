// Host half of the F(4x4, 3x3) convolution, written once for its two workgroup forms: the 32-tile workgroups of
// winograd4.hip and the light (16-tile) ones of winograd4l.hip.  A form F describes itself:
//
//   F::Args                       the kernel's argument struct (lgmwino4dev::ConvArgs + its own members)
//   F::THREADS, F::MBUF           workgroup size; floats of dynamic LDS (the epilogue exchange sets it)
//   F::UH, F::UW                  output rows / columns of a class-0 unit (one image, maps of whole units)
//   F::NCLS, F::NI[cls]           map classes 0 (H % UH == 0, W % UW == 0), 1 (16 x 16), 2 (8 x 8), 3 (4 x 4, if NCLS == 4) and the
//                                 images a unit of each class takes - also what the batch must be a multiple of
//   F::LAUNCHER                   the name a failed launch is reported under
//   F::splits(g, gc, oc)          its split-K rule (front: split_front below)
//   F::launch(p, cls, res, partial, stats, smem, s)   picks and launches its kernel (launch_kernel below); 0 or an error code
//
// A GroupNorm-statistics launch (class 0) leaves four rows per unit in either form.
#pragma once
#include "wino4_device.h"

namespace lgmwino4host {
namespace {      // internal linkage: each form's translation unit gets its own instances, the library exports none
using lgmwino4dev::KC;

template <class F>
int unit_class(int H, int W) {
  if (F::NCLS > 3 && H == 4 && W == 4) return 3;
  if (H == 8 && W == 8) return 2;
  if (H == 16 && W == 16) return 1;
  if (H >= F::UH && W >= F::UW && H % F::UH == 0 && W % F::UW == 0) return 0;
  return -1;
}

template <class F>
long unit_count(int cls, int B, int H, int W) {     // units per 64 produced channels, before split-K
  return cls == 0 ? (long)B * (H / F::UH) * (W / F::UW) : B / F::NI[cls];
}

template <class F>
bool supported(const LgmConvGeom* g, int gather_channels, int out_channels) {
  if (!(g->KH == 3 && g->KW == 3 && g->stride == 1 && g->pad == 1)) return false;
  if (gather_channels % 32 != 0 || out_channels % 64 != 0) return false;
  const int cls = unit_class<F>(g->H, g->W);
  if (cls < 0) return false;
  const long pix = (long)g->B * g->H * g->W + g->W + 1;
  if (pix * gather_channels >= (1L << 29) || pix * out_channels >= (1L << 29)) return false;
  if ((long)gather_channels * out_channels * 36 >= (1L << 29)) return false;
  return g->B % F::NI[cls] == 0;
}

// rows of GroupNorm statistics one image contributes per channel (STATS build, class-0 maps); 0: not taken
template <class F>
int stats_parts(const LgmConvGeom* g) {
  return unit_class<F>(g->H, g->W) == 0 ? (g->H / F::UH) * (g->W / F::UW) * 4 : 0;
}

// The front of both split-K rules: > 0 = the answer (`forced` by the form's environment knob, or 1 because the launch
// already covers 3/4 of the workgroup slots), 0 = the form's own rule decides among 1 ... *smax.
int split_front(long base, long slots, int phases, int forced, int* smax) {
  *smax = phases / 2 < 16 ? phases / 2 : 16;
  if (*smax < 1) *smax = 1;
  if (forced > 0) return forced < *smax ? forced : *smax;
  return base >= slots * 3 / 4 ? 1 : 0;
}

// How the kernel walks its units (lgmwino4dev::conv_unit): xcd_ranges and tn_slowest of a launch over M pixels
void unit_order(lgmwino4dev::ConvArgs& p, long M) {
  static const bool no_ranges = lgm_env_set("LGM_WINO4_NO_XCD_RANGES");
  p.xcd_ranges = no_ranges ? 0 : 1;
  // bytes the chip's eight L2s fetch under either order: patches once (x 1.2 halo) and all of U per XCD, or patches once per
  // channel block and U once
  static const int forced = lgm_env_int("LGM_WINO4_TN_SLOWEST", -1);
  const double in_b = 1.2 * (double)M * p.C * 4.0, u_b = 36.0 * p.C * p.N * 4.0;
  p.tn_slowest = forced >= 0 ? forced : ((in_b + 8.0 * u_b > in_b * p.tiles_n + u_b) ? 1 : 0);
}

// Opt-in to more than 64 KB of dynamic LDS, once per kernel and process; then the launch
template <auto KERN, int THREADS, class A>
void launch_kernel(const A& p, size_t smem, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    attr = true;
  }
  hipLaunchKernelGGL(KERN, dim3((unsigned)p.units), dim3(THREADS), smem, s, p);
}

// partial (optional, int64 x 2): as lgm_wino_launch - the caller's consumer sums the split-K planes itself
template <class F>
int conv_launch(const LgmConvGeom* g, int yx, const float* a, long a_pitch, const float* u, const float* bias,
                const float* res, long res_pitch, float* out, long out_pitch, void* workspace, long workspace_bytes,
                hipStream_t s, int64_t* partial, float* stats) {
  typename F::Args p{};
  p.stats = stats;
  p.a = a; p.u = u; p.bias = bias; p.res = res; p.out = out;
  p.a_pitch = a_pitch; p.res_pitch = res_pitch; p.out_pitch = out_pitch;
  p.B = g->B; p.H = g->H; p.W = g->W;
  p.C = yx ? g->Nw : g->Cw;
  p.N = yx ? g->Cw : g->Nw;
  const int cls = unit_class<F>(g->H, g->W);
  p.tb_h = cls == 0 ? g->H / F::UH : 1;
  p.tb_w = cls == 0 ? g->W / F::UW : 1;
  p.nbg = g->B / F::NI[cls];
  p.tiles_n = p.N / 64;
  const long M = (long)g->B * g->H * g->W;
  p.splits = F::splits(g, p.C, p.N);
  if (p.splits > 1) {
    const long need = (long)p.splits * M * p.N * (long)sizeof(float);
    if (!workspace || workspace_bytes < need || !lgm_aligned16(workspace)) p.splits = 1;
  }
  p.ws = (float*)workspace;
  p.ws_stride = M * p.N;
  p.pps = lgm_cdiv(p.C / KC, p.splits);
  p.splits = lgm_cdiv(p.C / KC, p.pps);
  p.units = (int)((long)p.nbg * p.tb_h * p.tb_w * p.tiles_n * p.splits);
  unit_order(p, M);
  if (const int rc = F::launch(p, cls, res != nullptr, partial != nullptr, stats != nullptr, (size_t)F::MBUF * sizeof(float), s))
    return rc;
  if (partial) {
    partial[0] = p.splits;
    partial[1] = p.ws_stride;
    LGM_LAUNCH_CHECK_AS(F::LAUNCHER);
    return LGM_OK;
  }
  if (p.splits > 1)
    return lgm_splitk_reduce_launch(p.ws, p.ws_stride, p.splits, bias, res, res_pitch, out, out_pitch, M, p.N, s);
  LGM_LAUNCH_CHECK_AS(F::LAUNCHER);
  return LGM_OK;
}

}  // namespace
}  // namespace lgmwino4host
