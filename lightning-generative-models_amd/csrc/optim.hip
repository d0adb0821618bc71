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
                                                   int decoupled, const float* __restrict__ scale_dev) {
  // scale_dev (lgm_adam_step_scaled): the clipped gradient scale grad_clip_scale_kernel left on the device takes
  // grad_scale's place; thread 0 reads it beside the bias corrections, the streaming path carries nothing new.
  __shared__ float sc[3];
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
    if (scale_dev) sc[2] = scale_dev[0];
  }
  __syncthreads();
  const float step_size = sc[0];
  const float inv_sqrt_bc2 = sc[1];
  if (scale_dev) grad_scale = sc[2];
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

static int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1, double b2, float eps,
                       float weight_decay, float step, const float* step_dev, float grad_scale, int decoupled,
                       const float* scale_dev, void* stream) {
  LGM_REQUIRE(p && g && m && v && n > 0, "adam_step: bad arguments");
  LGM_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "adam_step: betas must lie in [0, 1)");
  LGM_REQUIRE(lgm_aligned16(p) && lgm_aligned16(g) && lgm_aligned16(m) && lgm_aligned16(v),
              "adam_step: buffers must be 16B aligned");
  LGM_REQUIRE(step_dev || step >= 1.f, "adam_step: step must be >= 1");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n,
                     lr, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), log(b1), log(b2), eps, weight_decay, step, step_dev,
                     grad_scale, decoupled, scale_dev);
  LGM_LAUNCH_CHECK_AS("lgm_adam_step");
  return LGM_OK;
}

extern "C" int lgm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1, double b2,
                             float eps, float weight_decay, float step, const float* step_dev, float grad_scale,
                             int decoupled, void* stream) {
  return adam_launch(p, g, m, v, n, lr, b1, b2, eps, weight_decay, step, step_dev, grad_scale, decoupled, nullptr, stream);
}

// The same kernel with the gradient scale read from the device (scale_dev[0], written by lgm_grad_clip_scale): the clipped
// step needs no host read.  Weight decay is applied after the scale, as torch clips before the optimizer adds wd * p.
extern "C" int lgm_adam_step_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1, double b2,
                                    float eps, float weight_decay, float step, const float* step_dev,
                                    const float* scale_dev, int decoupled, void* stream) {
  LGM_REQUIRE(scale_dev, "adam_step_scaled: scale_dev is null");
  return adam_launch(p, g, m, v, n, lr, b1, b2, eps, weight_decay, step, step_dev, 1.f, decoupled, scale_dev, stream);
}

// ---- gradient tail: global-norm clipping and accumulation ---------------------------------------------------------------------
// Sum g^2 over a flat buffer as per-workgroup partial sums in double: workgroup b covers the fixed span
// [b * SQNORM_SPAN, (b + 1) * SQNORM_SPAN) and writes ONE double.  The span is a constant, so the partial count depends on n
// alone (not on lgm_cu_budget(): a rank with a CU margin and a single GPU give equal bits).  A float x float product is exact in
// double and every add is a double add from the first one, so the only error is the summation's: at most n * 2^-53 relative on a
// sum of non-negative terms, in whatever order.  The order is fixed all the same (lane-sequential, shuffle tree, the four waves
// in order; no atomics), so two runs give equal bits.  One 4 B/element read; four double FMAs per 16-B load.
constexpr long SQNORM_SPAN = 8192;              // floats per workgroup: 8 loads of 16 B per lane
constexpr int SQNORM_ITERS = SQNORM_SPAN / (256 * 4);

namespace {
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// block-wide double sum of 256 threads in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ double sq4(double acc, const f32x4 g) {
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = fma((double)g[k], (double)g[k], acc);
  return acc;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
  __shared__ double sh[4];
  const long base = (long)blockIdx.x * SQNORM_SPAN + (long)threadIdx.x * 4;
  double acc = 0.0;
  if ((long)(blockIdx.x + 1) * SQNORM_SPAN <= n) {          // a whole span: every load in flight before the first add
    f32x4 gv[SQNORM_ITERS];
#pragma unroll
    for (int j = 0; j < SQNORM_ITERS; ++j) gv[j] = *reinterpret_cast<const f32x4*>(g + base + (long)j * 1024);
#pragma unroll
    for (int j = 0; j < SQNORM_ITERS; ++j) acc = sq4(acc, gv[j]);
  } else {
    for (int j = 0; j < SQNORM_ITERS; ++j) {
      const long i = base + (long)j * 1024;
      if (i + 3 < n)
        acc = sq4(acc, *reinterpret_cast<const f32x4*>(g + i));
      else
        for (long k = i; k < n; ++k) acc = fma((double)g[k], (double)g[k], acc);
    }
  }
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// ONE workgroup: the partials (of several flat buffers laid end to end) in a fixed tree, then torch's clip_grad_norm_
// (norm type 2, error_if_nonfinite=False) on the gradient the optimizer would see, grad_scale * g, in double:
//   norm = |grad_scale| sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)), out2 = (grad_scale * coef, norm).
// The min propagates NaN as torch's clamp does (fminf(1, NaN) is 1); an infinite norm gives coefficient 0.
__global__ __launch_bounds__(256) void grad_clip_scale_kernel(const double* __restrict__ partials, long count, float grad_scale,
                                                              float max_norm, float* __restrict__ out2) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (long i = threadIdx.x; i < count; i += 256) acc += partials[i];
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) {
    const double norm = fabs((double)grad_scale) * sqrt(acc);
    const double r = (double)max_norm / (norm + 1e-6);
    const double coef = r > 1.0 ? 1.0 : r;                  // NaN > 1 is false: NaN stays
    out2[0] = (float)((double)grad_scale * coef);
    out2[1] = (float)norm;
  }
}

// dst = overwrite ? src : dst + src: one float add per element (nothing to contract), the bits of torch's dst + src
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long n,
                                                              int overwrite) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 3 < n) {
    f32x4 s = *reinterpret_cast<const f32x4*>(src + i);
    if (!overwrite) s += *reinterpret_cast<const f32x4*>(dst + i);
    *reinterpret_cast<f32x4*>(dst + i) = s;
  } else {
    for (long j = i; j < n; ++j) dst[j] = overwrite ? src[j] : dst[j] + src[j];
  }
}
}  // namespace

extern "C" int64_t lgm_grad_sqnorm_span(int64_t n) { return n > 0 ? SQNORM_SPAN : -1; }

extern "C" int64_t lgm_grad_sqnorm_partials(int64_t n) { return n > 0 ? (n + SQNORM_SPAN - 1) / SQNORM_SPAN : -1; }

extern "C" int lgm_grad_sqnorm_partial(const float* g, int64_t n, double* partials, void* stream) {
  LGM_REQUIRE(g && partials && n > 0 && lgm_aligned16(g) && (((uintptr_t)partials) & 7u) == 0,
              "grad_sqnorm_partial: bad arguments");
  LGM_REQUIRE(lgm_grad_sqnorm_partials(n) <= 0x7fffffffL, "grad_sqnorm_partial: buffer too large");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)lgm_grad_sqnorm_partials(n)), dim3(256), 0, (hipStream_t)stream, g,
                     (long)n, partials);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_grad_clip_scale(const double* partials, int64_t count, float grad_scale, float max_norm, float* out2,
                                   void* stream) {
  LGM_REQUIRE(partials && out2 && count > 0 && (((uintptr_t)partials) & 7u) == 0, "grad_clip_scale: bad arguments");
  LGM_REQUIRE(max_norm >= 0.f, "grad_clip_scale: max_norm must not be negative");
  hipLaunchKernelGGL(grad_clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)count, grad_scale,
                     max_norm, out2);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_grad_accumulate(float* dst, const float* src, int64_t n, int overwrite, void* stream) {
  LGM_REQUIRE(dst && src && n > 0 && lgm_aligned16(dst) && lgm_aligned16(src), "grad_accumulate: bad arguments");
  const long nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3(lgm_cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, dst, src,
                     (long)n, overwrite);
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
