// Fused optimiser kernels over FLAT parameter storage (one launch per optimiser step).
//   lgm_adam_step : torch.optim.Adam semantics (coupled L2 weight decay, no amsgrad), replaces the
//                   per-tensor foreach kernels of ddpm.py:1053-1059, vqvae.py:207-214, wgan.py:183-195.
//   lgm_ema_lerp  : ema_pytorch-style shadow update  shadow += (online - shadow) * w  (ddpm.py:1047-1048); w = 1 copies.
// Pure HBM streaming: 16 B/lane accesses, 28 B/param (Adam) and 12 B/param (EMA).
#include "lgm_common.h"

namespace {

// Hyperparameters arrive as torch has them.  The complements 1 - beta are formed in doubles on the host and rounded once
// (1.f - 0.999f is 1.3e-5 off 1e-3); the bias corrections 1 - beta^step = -expm1(step * log(beta)) are formed in doubles HERE,
// because step may live on the device (step_dev, graph replay).  One thread per workgroup does the double-precision work and
// hands step_size and 1/sqrt(bc2) over through LDS, so the streaming path carries none of it.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                   float b2, float omb1, float omb2, double log_b1, double log_b2,
                                                   float eps, float wd, float step_host,
                                                   const float* __restrict__ step_dev, float grad_scale,
                                                   int decoupled) {
  __shared__ float sc[2];
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const bool whole = i + 3 < n;
  f32x4 pv, gv, mv, vv;
  if (whole) {                                // in flight while thread 0 forms the bias corrections
    pv = *reinterpret_cast<const f32x4*>(p + i);
    gv = *reinterpret_cast<const f32x4*>(g + i);
    mv = *reinterpret_cast<const f32x4*>(m + i);
    vv = *reinterpret_cast<const f32x4*>(v + i);
  }
  if (threadIdx.x == 0) {
    const double step = step_dev ? (double)step_dev[0] : (double)step_host;
    const double bc1 = -expm1(step * log_b1);
    const double bc2 = -expm1(step * log_b2);
    sc[0] = (float)((double)lr / bc1);
    sc[1] = (float)(1.0 / sqrt(bc2));
  }
  __syncthreads();
  const float step_size = sc[0];
  const float inv_sqrt_bc2 = sc[1];
  if (i >= n) return;
  if (whole) {
    gv *= grad_scale;
    if (decoupled)
      pv *= (1.f - lr * wd);
    else if (wd != 0.f)
      gv += pv * wd;
    mv += (gv - mv) * omb1;
    vv = vv * b2 + gv * gv * omb2;
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[k] -= step_size * (mv[k] / (sqrtf(vv[k]) * inv_sqrt_bc2 + eps));
    *reinterpret_cast<f32x4*>(p + i) = pv;
    *reinterpret_cast<f32x4*>(m + i) = mv;
    *reinterpret_cast<f32x4*>(v + i) = vv;
  } else {
    for (long j = i; j < n; ++j) {
      float pv = p[j], gv = g[j] * grad_scale, mv = m[j], vv = v[j];
      if (decoupled)
        pv *= (1.f - lr * wd);
      else if (wd != 0.f)
        gv += pv * wd;
      mv += (gv - mv) * omb1;
      vv = vv * b2 + gv * gv * omb2;
      pv -= step_size * (mv / (sqrtf(vv) * inv_sqrt_bc2 + eps));
      p[j] = pv;
      m[j] = mv;
      v[j] = vv;
    }
  }
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ shadow, const float* __restrict__ online, long n,
                                                  float w) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 3 < n) {
    f32x4 s = *reinterpret_cast<const f32x4*>(shadow + i);
    const f32x4 o = *reinterpret_cast<const f32x4*>(online + i);
    s = w == 1.f ? o : s + (o - s) * w;      // w = 1 is the reference's COPY: s + (o - s) is not o in float32
    *reinterpret_cast<f32x4*>(shadow + i) = s;
  } else {
    for (long j = i; j < n; ++j) shadow[j] = w == 1.f ? online[j] : shadow[j] + (online[j] - shadow[j]) * w;
  }
}

__global__ void add_scalar_kernel(float* x, float a) { x[0] += a; }

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ x, long n, float val) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 3 < n)
    *reinterpret_cast<f32x4*>(x + i) = f32x4{val, val, val, val};
  else
    for (long j = i; j < n; ++j) x[j] = val;
}

}  // namespace

extern "C" int lgm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1, double b2,
                             float eps, float weight_decay, float step, const float* step_dev, float grad_scale,
                             int decoupled, void* stream) {
  LGM_REQUIRE(p && g && m && v && n > 0, "adam_step: bad arguments");
  LGM_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "adam_step: betas must lie in [0, 1)");
  LGM_REQUIRE(lgm_aligned16(p) && lgm_aligned16(g) && lgm_aligned16(m) && lgm_aligned16(v),
              "adam_step: buffers must be 16B aligned");
  LGM_REQUIRE(step_dev || step >= 1.f, "adam_step: step must be >= 1");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n,
                     lr, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), log(b1), log(b2), eps, weight_decay, step, step_dev,
                     grad_scale, decoupled);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

namespace {
// torch.optim.RMSprop defaults (momentum = 0, centered = False): sq = alpha*sq + (1-alpha)*g^2;
// p -= lr * g / (sqrt(sq) + eps).  Coupled weight decay like torch (g += wd * p).
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ sq, long n, float lr, float alpha,
                                                      float oma, float eps, float wd, float grad_scale) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const int cnt = (i + 3 < n) ? 4 : (int)(n - i);
  for (int k = 0; k < cnt; ++k) {
    float pv = p[i + k], gv = g[i + k] * grad_scale, sv = sq[i + k];
    if (wd != 0.f) gv += pv * wd;
    sv = sv * alpha + gv * gv * oma;
    pv -= lr * (gv / (sqrtf(sv) + eps));
    p[i + k] = pv;
    sq[i + k] = sv;
  }
}

__global__ __launch_bounds__(256) void clamp_kernel(float* __restrict__ x, long n, float lo, float hi) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const int cnt = (i + 3 < n) ? 4 : (int)(n - i);
  for (int k = 0; k < cnt; ++k) x[i + k] = fminf(fmaxf(x[i + k], lo), hi);
}
}  // namespace

extern "C" int lgm_rmsprop_step(float* p, const float* g, float* sq, int64_t n, float lr, double alpha, float eps,
                                float weight_decay, float grad_scale, void* stream) {
  LGM_REQUIRE(p && g && sq && n > 0, "rmsprop_step: bad arguments");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(rmsprop_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, p, g, sq, (long)n,
                     lr, (float)alpha, (float)(1.0 - alpha), eps, weight_decay, grad_scale);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_clamp(float* x, int64_t n, float lo, float hi, void* stream) {
  LGM_REQUIRE(x && n > 0 && lo <= hi, "clamp: bad arguments");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(clamp_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)n, lo, hi);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_ema_lerp(float* shadow, const float* online, int64_t n, float w, void* stream) {
  LGM_REQUIRE(shadow && online && n > 0 && lgm_aligned16(shadow) && lgm_aligned16(online), "ema_lerp: bad arguments");
  if (w == 0.f) return LGM_OK;               // the shadow keeps its bits (s + (o - s) * 0 turns -0.0 into 0.0)
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(ema_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, shadow, online,
                     (long)n, w);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_add_scalar(float* x, float a, void* stream) {
  LGM_REQUIRE(x, "add_scalar: null pointer");
  hipLaunchKernelGGL(add_scalar_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, x, a);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_fill(float* x, int64_t n, float val, void* stream) {
  LGM_REQUIRE(x && n > 0 && lgm_aligned16(x), "fill: bad arguments");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(fill_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)n, val);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
