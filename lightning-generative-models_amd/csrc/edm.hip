// Elucidated diffusion (Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative Models"): the
// elementwise launches around the network's forwards, and the random / learned Fourier embedding of a real-valued time
// (reference ddpm.py:135-151) that lets the network read a continuous noise level.
//
// With s_d = sigma_data (Table 1, "Ours"):
//     c_in = 1 / sqrt(s^2 + s_d^2)   c_skip = s_d^2 / (s^2 + s_d^2)   c_out = s s_d / sqrt(s^2 + s_d^2)   c_noise = ln(s) / 4
//     D(x, s) = c_skip x + c_out F(c_in x, c_noise)
//
// edm_qsample_kernel   training: y = img (normalised when asked), x = y + s eps; c_in x into the x slice of the network's input
//                      buffer, F* = (y - c_skip x) / c_out into the target, s[B] and c_noise[B].  s = exp(P_mean + P_std n) and
//                      c_noise = (P_mean + P_std n) / 4 from the per-sample normal n (no log of an exp), or s given and
//                      c_noise = log(s) / 4.  lambda(s) c_out^2 = 1, so the loss is the plain MSE between F and F*.
// edm_pre_kernel       sampling: x^ = x + coef eps (noise given) or x^ = x, c_in(s^) x^ into the input buffer, c_noise(s^)[B].
// edm_euler_kernel     D = c_skip(s^) x^ + c_out(s^) F (clamped to [-1, 1] when clip), d = (x^ - D) / s^, x' = x^ + (s' - s^) d
//                      into the state; `second`: also d and c_in(s') x' / c_noise(s') for the second evaluation.
// edm_heun_kernel      D' = c_skip(s') x' + c_out(s') F', d' = (x' - D') / s', x_next = x^ + (s' - s^) ((d + d') / 2) into the state.
//
// A sampling step's row is EDM_K = 16 floats, planned on the host in float64 and rounded once (lgm_hip/edm.py):
//     0..3    s_i   s^   coef = sqrt(s^^2 - s_i^2) S_noise   s'
//     4..7    c_in  c_noise  c_skip  c_out      at s^
//     8..11   the same at s'  (zeros when s' = 0: the last step has no second evaluation)
//     12      dt = s' - s^
//     13..15  gamma, 0, 0                       not read here
// by value, or row counter[0] of a device table; edm_advance_kernel is the step's last node then.
//
// The state, x^, d and the target are NHWC buffers of their own with r4(C) lanes a pixel; the network's input buffer holds
// c_in x alone.  All kernels are streaming: one thread per (pixel, four lanes) with 16-byte loads and stores where every base
// is 16-byte aligned and every pitch and offset a multiple of four floats, else one thread per (pixel, lane): the same bits.
// blockIdx.y is the sample, so the coefficients are wave-uniform.  No atomics, no cross-thread value.  Contraction is off:
// every product, quotient and sum rounds once, in the order written.
#include "lgm_common.h"

namespace {

constexpr int EDM_K = 16;
constexpr float EDM_TWO_PI_HALF = 3.14159265358979323846f;      // float32(pi): the reference multiplies by 2, then by pi

struct EdmRow { float v[EDM_K]; };

struct EdmCoef { float c_in, c_noise, c_skip, c_out, sigma; };

// the four coefficients from a float32 sigma: s2 = s s + sd sd (3 roundings), r = sqrt(s2), c_in = 1 / r (5 in all),
// c_skip = (sd sd) / s2 (5), c_out = (s sd) / r (6)
__device__ __forceinline__ EdmCoef edm_coef(float sigma, float sd) {
#pragma clang fp contract(off)
  EdmCoef k;
  const float sd2 = sd * sd;
  const float s2 = sigma * sigma + sd2;
  const float r = sqrtf(s2);
  k.sigma = sigma;
  k.c_in = 1.f / r;
  k.c_skip = sd2 / s2;
  k.c_out = (sigma * sd) / r;
  k.c_noise = 0.f;
  return k;
}

__device__ __forceinline__ void edm_qsample_one(const EdmCoef& k, int normalize, float y, float eps, float& xin, float& tgt) {
#pragma clang fp contract(off)
  if (normalize) y = y * 2.f - 1.f;
  const float x = y + k.sigma * eps;
  xin = k.c_in * x;
  tgt = (y - k.c_skip * x) / k.c_out;
}

// per = HW * (VEC ? Cpad / 4 : Cpad) work items of one sample; img / noise are NCHW, everything written is NHWC
template <bool VEC>
__global__ __launch_bounds__(256) void edm_qsample_kernel(const float* __restrict__ img, const float* __restrict__ noise,
                                                          const float* __restrict__ n, const float* __restrict__ sigma_in,
                                                          float P_mean, float P_std, float sd, int normalize,
                                                          float* __restrict__ xin, long pitch, int x_off,
                                                          float* __restrict__ target, long tpitch, float* __restrict__ sigma_out,
                                                          float* __restrict__ cnoise_out, int C, int Cpad, int HW, long per) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  float sigma, cn;
  if (n) {
    const float ls = P_mean + P_std * n[b];
    sigma = expf(ls);
    cn = 0.25f * ls;
  } else {
    sigma = sigma_in[b];
    cn = 0.25f * logf(sigma);
  }
  const EdmCoef k = edm_coef(sigma, sd);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) sigma_out[b] = sigma, cnoise_out[b] = cn;
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long p = i / Q, pix = (long)b * HW + p;
    f32x4 xv, tv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xv[j] = 0.f, tv[j] = 0.f;
      if (c0 + j < C) {
        const long s = ((long)b * C + c0 + j) * HW + p;
        float a, t;
        edm_qsample_one(k, normalize, img[s], noise[s], a, t);
        xv[j] = a, tv[j] = t;
      }
    }
    *reinterpret_cast<f32x4*>(xin + pix * pitch + x_off + c0) = xv;
    *reinterpret_cast<f32x4*>(target + pix * tpitch + c0) = tv;
  } else {
    const int c = (int)(i % Cpad);
    const long p = i / Cpad, pix = (long)b * HW + p;
    float a = 0.f, t = 0.f;
    if (c < C) {
      const long s = ((long)b * C + c) * HW + p;
      edm_qsample_one(k, normalize, img[s], noise[s], a, t);
    }
    xin[pix * pitch + x_off + c] = a;
    target[pix * tpitch + c] = t;
  }
}

__device__ __forceinline__ const float* edm_row(const EdmRow& byval, const float* __restrict__ table,
                                                const int* __restrict__ counter) {
  return table ? table + (long)EDM_K * counter[0] : byval.v;
}

__device__ __forceinline__ float edm_hat_one(float x, float coef, float eps, bool noisy) {
#pragma clang fp contract(off)
  return noisy ? x + coef * eps : x;
}

template <bool VEC>
__global__ __launch_bounds__(256) void edm_pre_kernel(const float* __restrict__ x, long spitch, const float* __restrict__ noise,
                                                      EdmRow byval, const float* __restrict__ table,
                                                      const int* __restrict__ counter, float* __restrict__ xhat,
                                                      float* __restrict__ xin, long pitch, int x_off,
                                                      float* __restrict__ cnoise, int C, int Cpad, int HW, long per) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const float* row = edm_row(byval, table, counter);
  const float coef = row[2], c_in = row[4];
  const bool noisy = noise != nullptr && coef != 0.f;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) cnoise[b] = row[5];
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long p = i / Q, pix = (long)b * HW + p;
    const f32x4 xs = *reinterpret_cast<const f32x4*>(x + pix * spitch + c0);
    f32x4 h, a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = 0.f, a[j] = 0.f;
      if (c0 + j < C) {
        h[j] = edm_hat_one(xs[j], coef, noisy ? noise[((long)b * C + c0 + j) * HW + p] : 0.f, noisy);
        a[j] = c_in * h[j];
      }
    }
    *reinterpret_cast<f32x4*>(xhat + pix * spitch + c0) = h;
    *reinterpret_cast<f32x4*>(xin + pix * pitch + x_off + c0) = a;
  } else {
    const int c = (int)(i % Cpad);
    const long p = i / Cpad, pix = (long)b * HW + p;
    float h = 0.f, a = 0.f;
    if (c < C) {
      h = edm_hat_one(x[pix * spitch + c], coef, noisy ? noise[((long)b * C + c) * HW + p] : 0.f, noisy);
      a = c_in * h;
    }
    xhat[pix * spitch + c] = h;
    xin[pix * pitch + x_off + c] = a;
  }
}

// D, d and the Euler point from one element: c = (c_skip, c_out), s the level the slope is taken at
__device__ __forceinline__ void edm_slope_one(float c_skip, float c_out, float s, int clip, float xv, float F, float& d) {
#pragma clang fp contract(off)
  float D = c_skip * xv + c_out * F;
  if (clip) D = fminf(fmaxf(D, -1.f), 1.f);
  d = (xv - D) / s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void edm_euler_kernel(const float* __restrict__ F, long fpitch, const float* __restrict__ xhat,
                                                        long spitch, EdmRow byval, const float* __restrict__ table,
                                                        const int* __restrict__ counter, int clip, int second,
                                                        float* __restrict__ x, float* __restrict__ dout,
                                                        float* __restrict__ xin, long pitch, int x_off,
                                                        float* __restrict__ cnoise, int C, int Cpad, int HW, long per) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const float* row = edm_row(byval, table, counter);
  const float s_hat = row[1], c_skip = row[6], c_out = row[7], c_in_n = row[8], dt = row[12];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (second && i == 0) cnoise[b] = row[9];
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long pix = (long)b * HW + i / Q;
    const f32x4 h = *reinterpret_cast<const f32x4*>(xhat + pix * spitch + c0);
    const f32x4 f = *reinterpret_cast<const f32x4*>(F + pix * fpitch + c0);
    f32x4 xp, dv, a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xp[j] = 0.f, dv[j] = 0.f, a[j] = 0.f;
      if (c0 + j < C) {
        float d;
        edm_slope_one(c_skip, c_out, s_hat, clip, h[j], f[j], d);
        dv[j] = d;
        xp[j] = h[j] + dt * d;
        a[j] = c_in_n * xp[j];
      }
    }
    *reinterpret_cast<f32x4*>(x + pix * spitch + c0) = xp;
    if (second) {
      *reinterpret_cast<f32x4*>(dout + pix * spitch + c0) = dv;
      *reinterpret_cast<f32x4*>(xin + pix * pitch + x_off + c0) = a;
    }
  } else {
    const int c = (int)(i % Cpad);
    const long pix = (long)b * HW + i / Cpad;
    float xp = 0.f, d = 0.f;
    if (c < C) {
      const float h = xhat[pix * spitch + c];
      edm_slope_one(c_skip, c_out, s_hat, clip, h, F[pix * fpitch + c], d);
      xp = h + dt * d;
    }
    x[pix * spitch + c] = xp;
    if (second) {
      dout[pix * spitch + c] = d;
      xin[pix * pitch + x_off + c] = c_in_n * xp;
    }
  }
}

__device__ __forceinline__ float edm_heun_one(const float* row, int clip, float h, float xp, float d, float F) {
#pragma clang fp contract(off)
  float d2;
  edm_slope_one(row[10], row[11], row[3], clip, xp, F, d2);
  const float m = (d + d2) * 0.5f;
  return h + row[12] * m;
}

template <bool VEC>
__global__ __launch_bounds__(256) void edm_heun_kernel(const float* __restrict__ F, long fpitch, const float* __restrict__ xhat,
                                                       const float* __restrict__ d, long spitch, EdmRow byval,
                                                       const float* __restrict__ table, const int* __restrict__ counter,
                                                       int clip, float* __restrict__ x, int C, int Cpad, int HW, long per) {
  const int b = blockIdx.y;
  const float* row = edm_row(byval, table, counter);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long pix = (long)b * HW + i / Q;
    const f32x4 h = *reinterpret_cast<const f32x4*>(xhat + pix * spitch + c0);
    const f32x4 dv = *reinterpret_cast<const f32x4*>(d + pix * spitch + c0);
    const f32x4 xp = *reinterpret_cast<const f32x4*>(x + pix * spitch + c0);
    const f32x4 f = *reinterpret_cast<const f32x4*>(F + pix * fpitch + c0);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = c0 + j < C ? edm_heun_one(row, clip, h[j], xp[j], dv[j], f[j]) : 0.f;
    *reinterpret_cast<f32x4*>(x + pix * spitch + c0) = r;
  } else {
    const int c = (int)(i % Cpad);
    const long o = ((long)b * HW + i / Cpad) * spitch + c;
    x[o] = c < C ? edm_heun_one(row, clip, xhat[o], x[o], d[o], F[((long)b * HW + i / Cpad) * fpitch + c]) : 0.f;
  }
}

__global__ void edm_advance_kernel(int* counter) { counter[0] += 1; }

// RandomOrLearnedSinusoidalPosEmb (reference ddpm.py:146-151): row b = (x_b, sin(f_b0..), cos(f_b0..)) with
// f_bd = ((x_b w_d) 2) pi in float32 as the reference forms it; lanes [2 half + 1, pitch) zero.  One thread per (row, lane).
__global__ __launch_bounds__(256) void fourier_emb_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int B,
                                                              int half, float* __restrict__ out, long pitch) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * pitch) return;
  const int b = (int)(i / pitch), c = (int)(i % pitch);
  const float xb = x[b];
  float r = 0.f;
  if (c == 0) {
    r = xb;
  } else if (c <= 2 * half) {
    const int dd = c <= half ? c - 1 : c - 1 - half;
    const float f = ((xb * w[dd]) * 2.f) * EDM_TWO_PI_HALF;
    r = c <= half ? sinf(f) : cosf(f);
  }
  out[(long)b * pitch + c] = r;
}

// g_w[d] = beta g_w[d] + 2 pi sum_b x_b (cos_bd g_sin_bd - sin_bd g_cos_bd): d f / d w = 2 pi x.  One workgroup; thread d walks
// the rows in ascending order, so the sum has one order whatever runs beside it.  emb is the forward's own row (x, sin, cos).
__global__ __launch_bounds__(256) void fourier_emb_bwd_kernel(const float* __restrict__ emb, long pitch,
                                                              const float* __restrict__ gemb, long gpitch, int B, int half,
                                                              float* __restrict__ gw, float beta) {
#pragma clang fp contract(off)
  for (int dd = threadIdx.x; dd < half; dd += 256) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float* e = emb + (long)b * pitch;
      const float* g = gemb + (long)b * gpitch;
      const float term = e[1 + half + dd] * g[1 + dd] - e[1 + dd] * g[1 + half + dd];
      acc = acc + e[0] * term;
    }
    const float r = (acc * 2.f) * EDM_TWO_PI_HALF;
    gw[dd] = beta != 0.f ? beta * gw[dd] + r : r;
  }
}

inline bool edm_vec_ok(const void* p, int64_t pitch, int off) { return lgm_aligned16(p) && pitch % 4 == 0 && off % 4 == 0; }

inline int edm_row_args_ok(const float* table, const int32_t* counter, int advance) {
  return (table == nullptr) == (counter == nullptr) && (table || !advance) && (!table || lgm_aligned16(table));
}

inline EdmRow edm_row_of(const float* row) {
  EdmRow r{};
  if (row)
    for (int k = 0; k < EDM_K; ++k) r.v[k] = row[k];
  return r;
}

int edm_advance(int advance, int32_t* counter, void* stream) {
  if (advance) {
    hipLaunchKernelGGL(edm_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)counter);
    LGM_LAUNCH_CHECK_AS("edm_advance");
  }
  return LGM_OK;
}

int edm_qsample_launch(const float* img, const float* noise, const float* n, const float* sigma_in, float P_mean, float P_std,
                       float sigma_data, int normalize, float* xin, int64_t pitch, int x_off, float* target,
                       int64_t target_pitch, float* sigma_out, float* cnoise_out, int B, int C, int HW, void* stream) {
  LGM_REQUIRE(img && noise && (n || sigma_in) && xin && target && sigma_out && cnoise_out && B > 0 && B <= 65535 && C > 0 &&
                  HW > 0 && sigma_data > 0.f,
              "edm_qsample: operands, positive sizes (B <= 65535) and sigma_data > 0 required");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(x_off >= 0 && x_off + Cpad <= pitch && target_pitch >= Cpad,
              "edm_qsample: the x slice, the target and their padding (r4(C) = %d lanes) must lie inside the pitches", Cpad);
  LGM_REQUIRE((const void*)xin != (const void*)img && (const void*)xin != (const void*)noise && target != xin &&
                  (const void*)target != (const void*)img && (const void*)target != (const void*)noise,
              "edm_qsample: the outputs must not alias a source or each other");
  const bool vec = edm_vec_ok(xin, pitch, x_off) && edm_vec_ok(target, target_pitch, 0);
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("edm_qsample_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  if (vec)
    hipLaunchKernelGGL(edm_qsample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, img, noise, n, sigma_in, P_mean, P_std,
                       sigma_data, normalize, xin, (long)pitch, x_off, target, (long)target_pitch, sigma_out, cnoise_out, C, Cpad,
                       HW, per);
  else
    hipLaunchKernelGGL(edm_qsample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, img, noise, n, sigma_in, P_mean, P_std,
                       sigma_data, normalize, xin, (long)pitch, x_off, target, (long)target_pitch, sigma_out, cnoise_out, C, Cpad,
                       HW, per);
  LGM_LAUNCH_CHECK_AS("edm_qsample");
  return LGM_OK;
}

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), like distill.hip's and lowres.hip's and for the same
// reason: tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it, and tests/test_hip_edm.py,
// which runs these kernels, is not on that list.
extern "C" int lgm_edm_qsample(const float* img, const float* noise, const float* n, float P_mean, float P_std, float sigma_data,
                               int normalize, float* xin, int64_t pitch, int x_off, float* target, int64_t target_pitch,
                               float* sigma_out, float* cnoise_out, int B, int C, int HW, void* stream) {
  LGM_REQUIRE(n, "edm_qsample: the per-sample normal draw is required");
  return edm_qsample_launch(img, noise, n, nullptr, P_mean, P_std, sigma_data, normalize, xin, pitch, x_off, target,
                            target_pitch, sigma_out, cnoise_out, B, C, HW, stream);
}

extern "C" int lgm_edm_qsample_sigma(const float* img, const float* noise, const float* sigma, float sigma_data, int normalize,
                                     float* xin, int64_t pitch, int x_off, float* target, int64_t target_pitch, float* sigma_out,
                                     float* cnoise_out, int B, int C, int HW, void* stream) {
  LGM_REQUIRE(sigma && sigma != sigma_out, "edm_qsample_sigma: sigma is required and is not written in place");
  return edm_qsample_launch(img, noise, nullptr, sigma, 0.f, 0.f, sigma_data, normalize, xin, pitch, x_off, target, target_pitch,
                            sigma_out, cnoise_out, B, C, HW, stream);
}

extern "C" int lgm_edm_pre(const float* x, int64_t state_pitch, const float* noise, const float* row, const float* table,
                           const int32_t* counter, float* xhat, float* xin, int64_t pitch, int x_off, float* cnoise, int B, int C,
                           int HW, void* stream) {
  LGM_REQUIRE(x && xhat && xin && cnoise && B > 0 && B <= 65535 && C > 0 && HW > 0 && (row != nullptr) != (table != nullptr) &&
                  edm_row_args_ok(table, counter, 0),
              "edm_pre: operands, positive sizes (B <= 65535) and either a row or a 16-byte aligned table with its counter");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(x_off >= 0 && x_off + Cpad <= pitch && state_pitch >= Cpad,
              "edm_pre: the x slice and the state's r4(C) = %d lanes must lie inside the pitches", Cpad);
  LGM_REQUIRE(xhat != x && xin != x && xin != xhat && (const void*)xin != (const void*)noise &&
                  (const void*)xhat != (const void*)noise,
              "edm_pre: x^ and the input buffer must not alias the state or each other and nothing may alias the noise");
  const bool vec = edm_vec_ok(x, state_pitch, 0) && edm_vec_ok(xhat, state_pitch, 0) && edm_vec_ok(xin, pitch, x_off);
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("edm_pre_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  const EdmRow r = edm_row_of(row);
  if (vec)
    hipLaunchKernelGGL(edm_pre_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (long)state_pitch, noise, r, table,
                       (const int*)counter, xhat, xin, (long)pitch, x_off, cnoise, C, Cpad, HW, per);
  else
    hipLaunchKernelGGL(edm_pre_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (long)state_pitch, noise, r, table,
                       (const int*)counter, xhat, xin, (long)pitch, x_off, cnoise, C, Cpad, HW, per);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_edm_euler(const float* F, int64_t f_pitch, const float* xhat, int64_t state_pitch, const float* row,
                             const float* table, int32_t* counter, int clip, int second, float* x, float* d, float* xin,
                             int64_t pitch, int x_off, float* cnoise, int advance, int B, int C, int HW, void* stream) {
  LGM_REQUIRE(F && xhat && x && B > 0 && B <= 65535 && C > 0 && HW > 0 && (row != nullptr) != (table != nullptr) &&
                  edm_row_args_ok(table, counter, advance) && (!second || (d && xin && cnoise)) && !(second && advance),
              "edm_euler: operands, positive sizes (B <= 65535), a row or a table with its counter; a step with a second "
              "evaluation needs d, the input buffer and c_noise and advances behind lgm_edm_heun");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(state_pitch >= Cpad && f_pitch >= Cpad && (!second || (x_off >= 0 && x_off + Cpad <= pitch)),
              "edm_euler: r4(C) = %d lanes must lie inside the pitches", Cpad);
  LGM_REQUIRE(x != F && x != xhat &&
                  (!second || (d != x && d != xhat && d != F && xin != x && xin != xhat && xin != F && xin != d)),
              "edm_euler: the outputs must not alias each other or a source");
  const bool vec = edm_vec_ok(F, f_pitch, 0) && edm_vec_ok(xhat, state_pitch, 0) && edm_vec_ok(x, state_pitch, 0) &&
                   (!second || (edm_vec_ok(d, state_pitch, 0) && edm_vec_ok(xin, pitch, x_off)));
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("edm_euler_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  const EdmRow r = edm_row_of(row);
  if (vec)
    hipLaunchKernelGGL(edm_euler_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, F, (long)f_pitch, xhat, (long)state_pitch,
                       r, table, (const int*)counter, clip, second, x, d, xin, (long)pitch, x_off, cnoise, C, Cpad, HW, per);
  else
    hipLaunchKernelGGL(edm_euler_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, F, (long)f_pitch, xhat, (long)state_pitch,
                       r, table, (const int*)counter, clip, second, x, d, xin, (long)pitch, x_off, cnoise, C, Cpad, HW, per);
  LGM_LAUNCH_CHECK();
  return edm_advance(advance, counter, stream);
}

extern "C" int lgm_edm_heun(const float* F, int64_t f_pitch, const float* xhat, const float* d, int64_t state_pitch,
                            const float* row, const float* table, int32_t* counter, int clip, float* x, int advance, int B, int C,
                            int HW, void* stream) {
  LGM_REQUIRE(F && xhat && d && x && B > 0 && B <= 65535 && C > 0 && HW > 0 && (row != nullptr) != (table != nullptr) &&
                  edm_row_args_ok(table, counter, advance),
              "edm_heun: operands, positive sizes (B <= 65535) and either a row or a 16-byte aligned table with its counter");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(state_pitch >= Cpad && f_pitch >= Cpad, "edm_heun: r4(C) = %d lanes must lie inside the pitches", Cpad);
  LGM_REQUIRE(x != F && x != xhat && x != d, "edm_heun: the state (x' in, x_next out) must not alias another operand");
  const bool vec = edm_vec_ok(F, f_pitch, 0) && edm_vec_ok(xhat, state_pitch, 0) && edm_vec_ok(d, state_pitch, 0) &&
                   edm_vec_ok(x, state_pitch, 0);
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("edm_heun_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  const EdmRow r = edm_row_of(row);
  if (vec)
    hipLaunchKernelGGL(edm_heun_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, F, (long)f_pitch, xhat, d,
                       (long)state_pitch, r, table, (const int*)counter, clip, x, C, Cpad, HW, per);
  else
    hipLaunchKernelGGL(edm_heun_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, F, (long)f_pitch, xhat, d,
                       (long)state_pitch, r, table, (const int*)counter, clip, x, C, Cpad, HW, per);
  LGM_LAUNCH_CHECK();
  return edm_advance(advance, counter, stream);
}

extern "C" int lgm_fourier_emb_fwd(const float* x, const float* weights, int B, int half, float* out, int64_t pitch,
                                   void* stream) {
  LGM_REQUIRE(x && weights && out && B > 0 && half > 0 && pitch >= 2 * half + 1 && out != x && out != weights,
              "fourier_emb_fwd: operands, positive sizes and a pitch of at least 2 half + 1 lanes required");
  lgm_note_kernel("fourier_emb_fwd_kernel");
  hipLaunchKernelGGL(fourier_emb_fwd_kernel, dim3(lgm_cdiv((long)B * pitch, 256)), dim3(256), 0, (hipStream_t)stream, x, weights,
                     B, half, out, (long)pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_fourier_emb_bwd(const float* emb, int64_t pitch, const float* gemb, int64_t gpitch, int B, int half,
                                   float* gweights, float beta, void* stream) {
  LGM_REQUIRE(emb && gemb && gweights && B > 0 && half > 0 && pitch >= 2 * half + 1 && gpitch >= 2 * half + 1 &&
                  gweights != emb && gweights != gemb,
              "fourier_emb_bwd: operands, positive sizes and pitches of at least 2 half + 1 lanes required");
  lgm_note_kernel("fourier_emb_bwd_kernel");
  hipLaunchKernelGGL(fourier_emb_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, emb, (long)pitch, gemb, (long)gpitch, B,
                     half, gweights, beta);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
