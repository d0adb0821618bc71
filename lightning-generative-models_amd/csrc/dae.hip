// The denoising autoencoder's own kernels (reference models/generative/autoencoder/dae.py): the corruption of the input
// batch, the tanh + squared-error head of its decoder and the loss.  Its four Linear layers run on csrc/dense.hip.  DESIGN
// section 6 has the definitions and the rounding counts.
//
// dae_corrupt_kernel<VEC>        out = fl(x + fl(noise * level)): two roundings, torch's order.
// dae_corrupt_mask_kernel<VEC>   salt-and-pepper or masking noise from Philox4x32-10 words drawn in registers (lgm_philox.h):
//   element n = b D + d (the LOGICAL index: pitches play no part) takes word n & 3 of the call with counter
//   (q lo, q hi, pass, 0), q = n >> 2; pass 0 is the salt (or masking) draw, pass 1 the pepper draw.  A thread owns four
//   consecutive d of one row; with D % 4 != 0 they straddle two counters and the thread evaluates both.
// dae_tanh_mse_fwd_kernel<VEC>   one workgroup per row: xh = tanhf(pre), row_part[b] = sum_d (x - xh)^2.  Thread t adds
//   the elements of quads t, t + 256, .. in ascending order, then lgm_block_sum: the order depends on D alone and is the
//   same in both load forms.
// dae_tanh_mse_bwd_kernel<VEC>   gpre = ((2 gloss / (B D)) (xh - x)) (1 - xh^2).
// dae_loss_kernel                one wave: lane l adds rows l, l + 64, .. in order, then the fixed shuffle tree; / (B D).
// VEC: every operand starts at a 16-byte boundary with a pitch that is a multiple of 4 - whole quads inside [0, D) move as
// one 16-byte access; the quad that holds the row's end, and every quad of the other form, moves lane by lane under a
// guard.  Pad lanes of an input are never read; pad lanes [D, round_up(D, 4)) of an output are written +0, nothing beyond.
// No atomics, no workgroup waits for another, every grid is a function of (B, D) alone.
#include "lgm_common.h"
#include "lgm_philox.h"

namespace {

constexpr int DAE_MAX_DIM = 1 << 20;
constexpr int DAE_EW_THREADS = 64;            // elementwise: one quad per thread; B = 32, D = 784 spreads over 98 workgroups

inline int r4(int n) { return (n + 3) / 4 * 4; }

template <bool VEC>
__device__ __forceinline__ f32x4 dae_load4(const float* row, int d, int D) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC && d + 3 < D) return *reinterpret_cast<const f32x4*>(row + d);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) v[e] = row[d + e];
  return v;
}

// lanes [d, d + 4) lie below Dp = round_up(D, 4): the whole quad is the output's
template <bool VEC>
__device__ __forceinline__ void dae_store4(float* row, int d, f32x4 v) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(row + d) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) row[d + e] = v[e];
  }
}

template <bool VEC>
__global__ __launch_bounds__(DAE_EW_THREADS) void dae_corrupt_kernel(const float* __restrict__ x, long x_pitch,
                                                                    const float* __restrict__ noise, long n_pitch, float level,
                                                                    int B, int D, int Q, float* __restrict__ out,
                                                                    long out_pitch) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * DAE_EW_THREADS + threadIdx.x;
  if (i >= (long)B * Q) return;
  const int b = (int)(i / Q), d = 4 * (int)(i - (long)b * Q);
  const f32x4 xv = dae_load4<VEC>(x + (long)b * x_pitch, d, D);
  const f32x4 nv = dae_load4<VEC>(noise + (long)b * n_pitch, d, D);
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) {
      const float t = nv[e] * level;
      o[e] = xv[e] + t;
    }
  dae_store4<VEC>(out + (long)b * out_pitch, d, o);
}

constexpr int DAE_MODE_SP = 0, DAE_MODE_MASK = 1;

template <bool VEC>
__global__ __launch_bounds__(DAE_EW_THREADS) void dae_corrupt_mask_kernel(const float* __restrict__ x, long x_pitch,
                                                                         const unsigned* __restrict__ key, int mode,
                                                                         unsigned thr, int B, int D, int Q,
                                                                         float* __restrict__ out, long out_pitch) {
  const long i = (long)blockIdx.x * DAE_EW_THREADS + threadIdx.x;
  if (i >= (long)B * Q) return;
  const int b = (int)(i / Q), d = 4 * (int)(i - (long)b * Q);
  const f32x4 xv = dae_load4<VEC>(x + (long)b * x_pitch, d, D);
  const unsigned k0 = key[0], k1 = key[1];
  const unsigned long n0 = (unsigned long)b * (unsigned long)D + (unsigned long)d;
  const unsigned long q0 = n0 >> 2;
  const int off = (int)(n0 & 3);               // != 0 only with D % 4 != 0: the quad straddles counters q0 and q0 + 1
  unsigned ws[8], wp[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) ws[e] = wp[e] = 0xffffffffu;
  lgm_philox4x32_10((unsigned)(q0 & 0xffffffffu), (unsigned)(q0 >> 32), 0u, 0u, k0, k1, ws);
  if (mode == DAE_MODE_SP) lgm_philox4x32_10((unsigned)(q0 & 0xffffffffu), (unsigned)(q0 >> 32), 1u, 0u, k0, k1, wp);
  if (off != 0) {
    const unsigned long q1 = q0 + 1;
    lgm_philox4x32_10((unsigned)(q1 & 0xffffffffu), (unsigned)(q1 >> 32), 0u, 0u, k0, k1, ws + 4);
    if (mode == DAE_MODE_SP) lgm_philox4x32_10((unsigned)(q1 & 0xffffffffu), (unsigned)(q1 >> 32), 1u, 0u, k0, k1, wp + 4);
  }
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (d + e >= D) continue;
    // word off + e of the eight, picked without a dynamic register index
    unsigned s = 0u, p = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j == off + e) {
        s = ws[j];
        p = wp[j];
      }
    float v = xv[e];
    if (mode == DAE_MODE_SP) v = p < thr ? 0.f : (s < thr ? 1.f : v);   // pepper wins where both hit
    else v = s < thr ? 0.f : v;
    o[e] = v;
  }
  dae_store4<VEC>(out + (long)b * out_pitch, d, o);
}

template <bool VEC>
__global__ __launch_bounds__(256) void dae_tanh_mse_fwd_kernel(const float* __restrict__ pre, long pre_pitch,
                                                               const float* __restrict__ x, long x_pitch, int D, int Dp,
                                                               float* __restrict__ xh, long xh_pitch,
                                                               float* __restrict__ row_part) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int d = 4 * threadIdx.x; d < Dp; d += 4 * 256) {
    const f32x4 pv = dae_load4<VEC>(pre + (long)b * pre_pitch, d, D);
    const f32x4 xv = dae_load4<VEC>(x + (long)b * x_pitch, d, D);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (d + e < D) {
        o[e] = tanhf(pv[e]);
        const float df = xv[e] - o[e];
        s = s + df * df;
      }
    dae_store4<VEC>(xh + (long)b * xh_pitch, d, o);
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) row_part[b] = s;
}

template <bool VEC>
__global__ __launch_bounds__(DAE_EW_THREADS) void dae_tanh_mse_bwd_kernel(const float* __restrict__ xh, long xh_pitch,
                                                                         const float* __restrict__ x, long x_pitch,
                                                                         const float* __restrict__ gloss, int B, int D, int Q,
                                                                         float* __restrict__ gpre, long gpre_pitch) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * DAE_EW_THREADS + threadIdx.x;
  if (i >= (long)B * Q) return;
  const int b = (int)(i / Q), d = 4 * (int)(i - (long)b * Q);
  const f32x4 hv = dae_load4<VEC>(xh + (long)b * xh_pitch, d, D);
  const f32x4 xv = dae_load4<VEC>(x + (long)b * x_pitch, d, D);
  const float c = (2.f * gloss[0]) / (float)((long)B * D);
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) {
      const float v = hv[e];
      const float df = v - xv[e];
      o[e] = (c * df) * (1.f - v * v);
    }
  dae_store4<VEC>(gpre + (long)b * gpre_pitch, d, o);
}

__global__ __launch_bounds__(64) void dae_loss_kernel(const float* __restrict__ row_part, int B, int D,
                                                      float* __restrict__ vals) {
#pragma clang fp contract(off)
  float r = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) r = r + row_part[b];
  r = lgm_wave_sum(r);
  if (threadIdx.x == 0) vals[0] = r / (float)((long)B * D);
}

inline bool vec_ok(const void* p, long pitch) { return lgm_aligned16(p) && pitch % 4 == 0; }
// B D <= 2^31 elements: the one-wave elementwise grids then hold at most 2^23 workgroups
constexpr long DAE_MAX_ELEMS = 1L << 31;
inline bool dims_ok(int B, int D) {
  return B >= 1 && B <= DAE_MAX_DIM && D >= 1 && D <= DAE_MAX_DIM && (long)B * r4(D) <= DAE_MAX_ELEMS;
}
// do the B rows of `w` floats at a (pitch ap) and at b (pitch bp) share a byte?  Whole spans are compared: rows that
// interleave without touching are refused too
inline bool overlaps(const float* a, long ap, const float* b, long bp, int B, int wa, int wb) {
  const float* ae = a + (long)(B - 1) * ap + wa;
  const float* be = b + (long)(B - 1) * bp + wb;
  return a < be && b < ae;
}

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), like csrc/dense.hip's and for the same reason:
// tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it; tests/test_hip_dae.py runs these.

extern "C" int lgm_dae_corrupt(const float* x, int64_t x_pitch, const float* noise, int64_t noise_pitch, float level, int B,
                               int D, float* out, int64_t out_pitch, void* stream) {
  LGM_REQUIRE(x && noise && out, "dae_corrupt: null argument");
  LGM_REQUIRE(dims_ok(B, D), "dae_corrupt: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(x_pitch >= D && noise_pitch >= D && out_pitch >= r4(D), "dae_corrupt: pitches below the channel count %d", D);
  LGM_REQUIRE(!overlaps(out, (long)out_pitch, x, (long)x_pitch, B, r4(D), D) &&
                  !overlaps(out, (long)out_pitch, noise, (long)noise_pitch, B, r4(D), D),
              "dae_corrupt: out must not overlap an input");
  const int Q = r4(D) / 4;
  const dim3 grid(lgm_cdiv((long)B * Q, DAE_EW_THREADS)), block(DAE_EW_THREADS);
  const bool vec = vec_ok(x, (long)x_pitch) && vec_ok(noise, (long)noise_pitch) && vec_ok(out, (long)out_pitch);
  lgm_note_kernel(vec ? "dae_corrupt_kernel<true>" : "dae_corrupt_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(dae_corrupt_kernel<true>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch, noise, (long)noise_pitch,
                       level, B, D, Q, out, (long)out_pitch);
  else
    hipLaunchKernelGGL(dae_corrupt_kernel<false>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch, noise, (long)noise_pitch,
                       level, B, D, Q, out, (long)out_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

// the threshold of a corruption probability p: min(2^32 - 1, floor(p 2^32)), in double; host-only
extern "C" int64_t lgm_dae_mask_threshold(int mode, double level) {
  if ((mode != DAE_MODE_SP && mode != DAE_MODE_MASK) || !(level >= 0.0)) return -1;
  const double p = mode == DAE_MODE_SP ? level / 2.0 : level;
  const double t = floor(p * 4294967296.0);
  return t >= 4294967295.0 ? (int64_t)4294967295LL : (int64_t)t;
}

extern "C" int lgm_dae_corrupt_mask(const float* x, int64_t x_pitch, const int64_t* key, int mode, double level, int B, int D,
                                    float* out, int64_t out_pitch, void* stream) {
  LGM_REQUIRE(x && key && out, "dae_corrupt_mask: null argument");
  LGM_REQUIRE(dims_ok(B, D), "dae_corrupt_mask: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(x_pitch >= D && out_pitch >= r4(D), "dae_corrupt_mask: pitches below the channel count %d", D);
  LGM_REQUIRE(!overlaps(out, (long)out_pitch, x, (long)x_pitch, B, r4(D), D), "dae_corrupt_mask: out must not overlap x");
  const int64_t thr = lgm_dae_mask_threshold(mode, level);
  LGM_REQUIRE(thr >= 0, "dae_corrupt_mask: mode 0 (salt_and_pepper) or 1 (masking) and level >= 0 required, got %d %g", mode, level);
  const int Q = r4(D) / 4;
  const dim3 grid(lgm_cdiv((long)B * Q, DAE_EW_THREADS)), block(DAE_EW_THREADS);
  const bool vec = vec_ok(x, (long)x_pitch) && vec_ok(out, (long)out_pitch);
  lgm_note_kernel(vec ? "dae_corrupt_mask_kernel<true>" : "dae_corrupt_mask_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(dae_corrupt_mask_kernel<true>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch,
                       (const unsigned*)key, mode, (unsigned)thr, B, D, Q, out, (long)out_pitch);
  else
    hipLaunchKernelGGL(dae_corrupt_mask_kernel<false>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch,
                       (const unsigned*)key, mode, (unsigned)thr, B, D, Q, out, (long)out_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_dae_tanh_mse_fwd(const float* pre, int64_t pre_pitch, const float* x, int64_t x_pitch, int B, int D,
                                    float* xh, int64_t xh_pitch, float* row_part, void* stream) {
  LGM_REQUIRE(pre && x && xh && row_part, "dae_tanh_mse_fwd: null argument");
  LGM_REQUIRE(dims_ok(B, D), "dae_tanh_mse_fwd: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(pre_pitch >= D && x_pitch >= D && xh_pitch >= r4(D), "dae_tanh_mse_fwd: pitches below the channel count %d", D);
  LGM_REQUIRE(!overlaps(xh, (long)xh_pitch, x, (long)x_pitch, B, r4(D), D) &&
                  !overlaps(xh, (long)xh_pitch, pre, (long)pre_pitch, B, r4(D), D),
              "dae_tanh_mse_fwd: xh must not overlap an input");
  const bool vec = vec_ok(pre, (long)pre_pitch) && vec_ok(x, (long)x_pitch) && vec_ok(xh, (long)xh_pitch);
  lgm_note_kernel(vec ? "dae_tanh_mse_fwd_kernel<true>" : "dae_tanh_mse_fwd_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(dae_tanh_mse_fwd_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, pre, (long)pre_pitch, x,
                       (long)x_pitch, D, r4(D), xh, (long)xh_pitch, row_part);
  else
    hipLaunchKernelGGL(dae_tanh_mse_fwd_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, pre, (long)pre_pitch, x,
                       (long)x_pitch, D, r4(D), xh, (long)xh_pitch, row_part);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_dae_tanh_mse_bwd(const float* xh, int64_t xh_pitch, const float* x, int64_t x_pitch, const float* gloss,
                                    int B, int D, float* gpre, int64_t gpre_pitch, void* stream) {
  LGM_REQUIRE(xh && x && gloss && gpre, "dae_tanh_mse_bwd: null argument");
  LGM_REQUIRE(dims_ok(B, D), "dae_tanh_mse_bwd: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(xh_pitch >= D && x_pitch >= D && gpre_pitch >= r4(D), "dae_tanh_mse_bwd: pitches below the channel count %d", D);
  LGM_REQUIRE(!overlaps(gpre, (long)gpre_pitch, x, (long)x_pitch, B, r4(D), D) &&
                  !overlaps(gpre, (long)gpre_pitch, xh, (long)xh_pitch, B, r4(D), D),
              "dae_tanh_mse_bwd: gpre must not overlap an input");
  const int Q = r4(D) / 4;
  const dim3 grid(lgm_cdiv((long)B * Q, DAE_EW_THREADS)), block(DAE_EW_THREADS);
  const bool vec = vec_ok(xh, (long)xh_pitch) && vec_ok(x, (long)x_pitch) && vec_ok(gpre, (long)gpre_pitch);
  lgm_note_kernel(vec ? "dae_tanh_mse_bwd_kernel<true>" : "dae_tanh_mse_bwd_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(dae_tanh_mse_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, xh, (long)xh_pitch, x, (long)x_pitch,
                       gloss, B, D, Q, gpre, (long)gpre_pitch);
  else
    hipLaunchKernelGGL(dae_tanh_mse_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, xh, (long)xh_pitch, x, (long)x_pitch,
                       gloss, B, D, Q, gpre, (long)gpre_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_dae_loss(const float* row_part, int B, int D, float* vals, void* stream) {
  LGM_REQUIRE(row_part && vals, "dae_loss: null argument");
  LGM_REQUIRE(dims_ok(B, D), "dae_loss: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  lgm_note_kernel("dae_loss_kernel");
  hipLaunchKernelGGL(dae_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_part, B, D, vals);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
