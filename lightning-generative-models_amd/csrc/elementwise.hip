// Small HBM-bound kernels: column sums, time embedding, activations, resampling copies,
// NCHW<->NHWC conversion, diffusion q_sample / v-target / weighted-MSE loss.
#include <atomic>
#include <stdarg.h>

#include "lgm_common.h"

// ---------------------------------------------------------------------------------------
// error string + ABI version
// ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void lgm_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* lgm_last_error(void) { return g_err; }
static thread_local const char* g_kernel = "";
void lgm_note_kernel(const char* name) { g_kernel = name; }
extern "C" const char* lgm_last_kernel(void) { return g_kernel; }
// the name registry: one pointer per LGM_KNAME site of the whole library (section bounds from the linker)
extern "C" const char* const __start_lgm_knames[];
extern "C" const char* const __stop_lgm_knames[];
// CU margin: lgm_set_cu_margin(margin) (-1: back to the default), else LGM_CU_MARGIN, else 0.  The library no longer derives
// it from WORLD_SIZE (round 6): lgm_hip.lightning.FlatGradSync sets 16 for a rank whose exchange overlaps its backward pass
// on RCCL - the one case in which a collective's workgroups hold CUs beside the launches.  Measured with 16
// foreign 256-thread workgroups resident (tools/cu_hog_step.py, light F(4x4) workgroups, ms per step, margin 0 / 16 / 32):
// B = 64: 8.15 / 7.48 / 7.49 (alone 6.75 / 6.86 / 6.92); B = 16: 4.90 / 4.70 / 4.69 (alone 4.48 / 4.49 / 4.50).
static std::atomic<int> lgm_cu_margin_override{-1};
extern "C" int lgm_cu_margin(void) { return 256 - lgm_cu_budget(); }
extern "C" int lgm_set_cu_margin(int margin) {
  LGM_REQUIRE(margin <= 128, "lgm_set_cu_margin: margin %d leaves less than half of the chip", margin);
  lgm_cu_margin_override.store(margin, std::memory_order_relaxed);
  return LGM_OK;
}
int lgm_cu_budget() {
  static const int env_margin = getenv("LGM_CU_MARGIN") ? atoi(getenv("LGM_CU_MARGIN")) : 0;
  const int ov = lgm_cu_margin_override.load(std::memory_order_relaxed);
  int m = ov >= 0 ? ov : env_margin;
  if (m < 0) m = 0;
  if (m > 128) m = 128;
  return 256 - m;
}

extern "C" int lgm_kernel_name_count(void) { return (int)(__stop_lgm_knames - __start_lgm_knames); }
extern "C" const char* lgm_kernel_name(int i) {
  return (i >= 0 && i < lgm_kernel_name_count()) ? __start_lgm_knames[i] : nullptr;
}
extern "C" int lgm_abi_version(void) { return LGM_ABI_VERSION; }

namespace {

// ---------------------------------------------------------------------------------------
// colsum: out[c] = beta*out[c] + sum_r a[r, c]
// ---------------------------------------------------------------------------------------
// rows per stage-1 block: at least 64, and at most 128 splits overall
static inline long cs_rows(long rows) {
  long r = (rows + 127) / 128;
  if (r < 64) r = 64;
  return (r + 3) / 4 * 4;
}

// block = CL columns x (256 / CL) row lanes, CL = the power of two >= min(cols, 64) (a 4-column matrix - the bias
// gradient of an image-end layer - used 4 of 64 column lanes and ran 512 dependent loads per thread: 63 us for
// 4 MB); sums rows [r0, r1) of `a` (fixed order => deterministic)
__global__ __launch_bounds__(256) void colsum_stage(const float* __restrict__ a, long pitch, long rows, long cols,
                                                    long rows_per_block, float* __restrict__ out, long out_pitch,
                                                    float beta, int lg_cl) {
  __shared__ float sh[256];
  const int CL = 1 << lg_cl, RL = 256 >> lg_cl;
  const int cl = threadIdx.x & (CL - 1), rl = threadIdx.x >> lg_cl;
  const long c = (long)blockIdx.x * CL + cl;
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  float s0 = 0.f, s1 = 0.f;
  if (c < cols) {
    long r = r0 + rl;
    for (; r + RL < r1; r += 2 * RL) {   // two independent chains keep more loads in flight
      s0 += a[r * pitch + c];
      s1 += a[(r + RL) * pitch + c];
    }
    if (r < r1) s0 += a[r * pitch + c];
  }
  sh[threadIdx.x] = s0 + s1;
  __syncthreads();
  if (rl == 0 && c < cols) {
    float v = 0.f;
    for (int k = 0; k < RL; ++k) v += sh[(k << lg_cl) + cl];
    float* o = out + (long)blockIdx.y * out_pitch + c;
    if (beta != 0.f) v += beta * o[0];
    o[0] = v;
  }
}

// second stage of a split colsum: out[c] = beta*out[c] + sum_k planes[k][c], in the ORDER of the batched reducer that sums the
// same planes for lgm_colsum_deferred (wgrad_reduce_batch_kernel: four lanes, plane k on lane k % 4 in chain (k % 16) / 4,
// chains and lanes joined pairwise) - the direct and the deferred form give the same bits
__global__ __launch_bounds__(256) void colsum_planes_kernel(const float* __restrict__ planes, long cols, int splits,
                                                            float* __restrict__ out, float beta) {
  __shared__ float sh[4][64];
  const int col = threadIdx.x & 63, lane = threadIdx.x >> 6;
  const long c = (long)blockIdx.x * 64 + col;
  float s = 0.f;
  if (c < cols) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    for (int k = lane; k < splits; k += 16) {
      t0 += planes[(long)k * cols + c];
      if (k + 4 < splits) t1 += planes[(long)(k + 4) * cols + c];
      if (k + 8 < splits) t2 += planes[(long)(k + 8) * cols + c];
      if (k + 12 < splits) t3 += planes[(long)(k + 12) * cols + c];
    }
    s = (t0 + t1) + (t2 + t3);
  }
  sh[lane][col] = s;
  __syncthreads();
  if (lane == 0 && c < cols) {
    float t = (sh[0][col] + sh[1][col]) + (sh[2][col] + sh[3][col]);
    if (beta != 0.f) t += out[c] * beta;
    out[c] = t;
  }
}

}  // namespace

extern "C" int64_t lgm_colsum_workspace(int64_t rows, int64_t cols) {
  return (int64_t)lgm_cdiv(rows, cs_rows(rows)) * cols * (int64_t)sizeof(float) + 16;
}

extern "C" int lgm_colsum(const float* a, int64_t pitch, int64_t rows, int64_t cols, float* out, float beta,
                          void* workspace, void* stream) {
  LGM_REQUIRE(a && out && workspace && rows > 0 && cols > 0, "colsum: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long rpb = cs_rows(rows);
  const int ns = lgm_cdiv(rows, rpb);
  int lg = 2;                                    // column lanes: 4 ... 64
  while (lg < 6 && (1L << lg) < cols) ++lg;
  const int cl = 1 << lg;
  if (ns == 1) {
    hipLaunchKernelGGL(colsum_stage, dim3(lgm_cdiv(cols, cl), 1), dim3(256), 0, s, a, (long)pitch, (long)rows,
                       (long)cols, rpb, out, 0L, beta, lg);
  } else {
    hipLaunchKernelGGL(colsum_stage, dim3(lgm_cdiv(cols, cl), ns), dim3(256), 0, s, a, (long)pitch, (long)rows,
                       (long)cols, rpb, (float*)workspace, (long)cols, 0.f, lg);
    hipLaunchKernelGGL(colsum_planes_kernel, dim3(lgm_cdiv(cols, 64)), dim3(256), 0, s, (const float*)workspace, (long)cols, ns,
                       out, beta);
  }
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_colsum_deferred(const float* a, int64_t pitch, int64_t rows, int64_t cols, float* out, float beta,
                                   void* workspace, int64_t* desc, void* stream) {
  LGM_REQUIRE(a && out && workspace && desc && rows > 0 && cols > 0, "colsum_deferred: bad arguments");
  LGM_REQUIRE(cols % 4 == 0 && lgm_aligned16(out) && lgm_aligned16(workspace),
              "colsum_deferred: cols %% 4 == 0 and 16-byte aligned out / workspace required");
  const long rpb = cs_rows(rows);
  const int ns = lgm_cdiv(rows, rpb);
  int lg = 2;
  while (lg < 6 && (1L << lg) < cols) ++lg;
  hipLaunchKernelGGL(colsum_stage, dim3(lgm_cdiv(cols, 1 << lg), ns), dim3(256), 0, (hipStream_t)stream, a, (long)pitch,
                     (long)rows, (long)cols, rpb, (float*)workspace, (long)cols, 0.f, lg);
  LGM_LAUNCH_CHECK();
  union { float f; int64_t i; } bb;
  bb.i = 0; bb.f = beta;
  desc[0] = (int64_t)(uintptr_t)workspace; desc[1] = cols; desc[2] = (int64_t)(uintptr_t)out; desc[3] = cols;
  desc[4] = 0; desc[5] = 0; desc[6] = ns; desc[7] = bb.i;
  return LGM_OK;
}

// ---------------------------------------------------------------------------------------
// Sinusoidal position embedding  (ddpm.py:125-132): emb[b] = cat(sin(t*f), cos(t*f)).  The frequency
// table f[i] = exp(i * -(ln(theta)/(half-1))) is computed by the CALLER on the host exactly as the
// reference computes it (torch.exp on the CPU): a device expf differs by an ulp, which times t = 999 is
// 1e-4 in the argument.
// ---------------------------------------------------------------------------------------
namespace {
__global__ void posemb_kernel(const int64_t* __restrict__ t, int B, int dim, const float* __restrict__ freqs,
                              float* __restrict__ out, long pitch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (i >= B * half) return;
  const int b = i / half, j = i % half;
  const float arg = (float)t[b] * freqs[j];
  out[(long)b * pitch + j] = sinf(arg);
  out[(long)b * pitch + half + j] = cosf(arg);
}

enum { ACT_SILU = 1, ACT_GELU = 2, ACT_RELU = 3, ACT_LRELU = 4, ACT_TANH = 5 };

__device__ __forceinline__ float act_fwd(float x, int act, float slope) {
  switch (act) {
    case ACT_SILU: return x / (1.f + expf(-x));
    case ACT_GELU: return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f));
    case ACT_RELU: return x > 0.f ? x : 0.f;
    case ACT_LRELU: return x > 0.f ? x : x * slope;
    case ACT_TANH: return tanhf(x);
  }
  return x;
}
// derivative w.r.t. the pre-activation x
__device__ __forceinline__ float act_bwd(float x, int act, float slope) {
  switch (act) {
    case ACT_SILU: {
      const float s = 1.f / (1.f + expf(-x));
      return s * (1.f + x * (1.f - s));
    }
    case ACT_GELU: {
      const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
      return cdf + x * pdf;
    }
    case ACT_RELU: return x > 0.f ? 1.f : 0.f;
    case ACT_LRELU: return x > 0.f ? 1.f : slope;
    case ACT_TANH: {
      const float t = tanhf(x);
      return 1.f - t * t;
    }
  }
  return 1.f;
}

// y[r, c] = act(x[r, c] + bias[c]) (+ res[r,c])   rows x cols with pitches; cols % 4 == 0
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ x, long x_pitch,
                                                      const float* __restrict__ bias, const float* __restrict__ res,
                                                      long res_pitch, float* __restrict__ y, long y_pitch, long rows,
                                                      int cols, int act, float slope) {
  const int c4n = cols / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * c4n) return;
  const long r = i / c4n;
  const int c = (int)(i % c4n) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(x + r * x_pitch + c);
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = act_fwd(v[k], act, slope);
  if (res) v += *reinterpret_cast<const f32x4*>(res + r * res_pitch + c);
  *reinterpret_cast<f32x4*>(y + r * y_pitch + c) = v;
}

// gx = gy * act'(x + bias)  (optionally accumulated)
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ x, long x_pitch,
                                                      const float* __restrict__ bias, const float* __restrict__ gy,
                                                      long gy_pitch, float* __restrict__ gx, long gx_pitch,
                                                      int accumulate, long rows, int cols, int act, float slope) {
  const int c4n = cols / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * c4n) return;
  const long r = i / c4n;
  const int c = (int)(i % c4n) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(x + r * x_pitch + c);
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + c);
  f32x4 g = *reinterpret_cast<const f32x4*>(gy + r * gy_pitch + c);
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] *= act_bwd(v[k], act, slope);
  float* o = gx + r * gx_pitch + c;
  if (accumulate) g += *reinterpret_cast<const f32x4*>(o);
  *reinterpret_cast<f32x4*>(o) = g;
}

// y = alpha*a + beta*b  on strided [rows, cols] matrices (b optional)
__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ a, long a_pitch, float alpha,
                                                    const float* __restrict__ b, long b_pitch, float beta,
                                                    float* __restrict__ y, long y_pitch, long rows, int cols) {
  const int c4n = cols / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * c4n) return;
  const long r = i / c4n;
  const int c = (int)(i % c4n) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(a + r * a_pitch + c) * alpha;
  if (b) v += *reinterpret_cast<const f32x4*>(b + r * b_pitch + c) * beta;
  *reinterpret_cast<f32x4*>(y + r * y_pitch + c) = v;
}

// nearest-neighbour x2 upsample, NHWC: y[b, 2h+i, 2w+j, :] = x[b, h, w, :]
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const float* __restrict__ x, long x_pitch,
                                                             float* __restrict__ y, long y_pitch, int B, int H, int W,
                                                             int C) {
  const int c4n = C / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * 2 * H * 2 * W * c4n;
  if (i >= total) return;
  const int c = (int)(i % c4n) * 4;
  long pix = i / c4n;
  const int ow = (int)(pix % (2 * W));
  pix /= 2 * W;
  const int oh = (int)(pix % (2 * H));
  const int b = (int)(pix / (2 * H));
  const long src = ((long)(b * H + (oh >> 1)) * W + (ow >> 1)) * x_pitch + c;
  const long dst = ((long)(b * 2 * H + oh) * 2 * W + ow) * y_pitch + c;
  *reinterpret_cast<f32x4*>(y + dst) = *reinterpret_cast<const f32x4*>(x + src);
}
// gx[b,h,w,:] = sum of the 4 gy children (fixed order)
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const float* __restrict__ gy, long gy_pitch,
                                                             float* __restrict__ gx, long gx_pitch, int B, int H, int W,
                                                             int C, int accumulate) {
  const int c4n = C / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * H * W * c4n;
  if (i >= total) return;
  const int c = (int)(i % c4n) * 4;
  long pix = i / c4n;
  const int w = (int)(pix % W);
  pix /= W;
  const int h = (int)(pix % H);
  const int b = (int)(pix / H);
  const long base = ((long)(b * 2 * H + 2 * h) * 2 * W + 2 * w) * gy_pitch + c;
  const long rowp = (long)2 * W * gy_pitch;
  f32x4 s = (*reinterpret_cast<const f32x4*>(gy + base) + *reinterpret_cast<const f32x4*>(gy + base + gy_pitch)) +
            (*reinterpret_cast<const f32x4*>(gy + base + rowp) +
             *reinterpret_cast<const f32x4*>(gy + base + rowp + gy_pitch));
  float* o = gx + ((long)(b * H + h) * W + w) * gx_pitch + c;
  if (accumulate) s += *reinterpret_cast<const f32x4*>(o);
  *reinterpret_cast<f32x4*>(o) = s;
}

// pixel-unshuffle "b c (h p1) (w p2) -> b (c p1 p2) h w" (ddpm.py:102) in NHWC:
// y[b, h, w, c*4 + p1*2 + p2] = x[b, 2h+p1, 2w+p2, c].  dir = 0 forward, 1 = inverse (gradient).
__global__ __launch_bounds__(256) void unshuffle_kernel(const float* __restrict__ src, long src_pitch,
                                                        float* __restrict__ dst, long dst_pitch, int B, int H, int W,
                                                        int C, int dir, int accumulate) {
  // H, W are the LOW-resolution sizes; C the high-resolution channel count.
  // one thread per (low-res pixel, channel c): moves the 4 (p1,p2) values -> float4 on the 4C side.
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * H * W * C;
  if (i >= total) return;
  const int c = (int)(i % C);
  long pix = i / C;
  const int w = (int)(pix % W);
  pix /= W;
  const int h = (int)(pix % H);
  const int b = (int)(pix / H);
  const long hi00 = ((long)(b * 2 * H + 2 * h) * 2 * W + 2 * w);
  const long lo = ((long)(b * H + h) * W + w);
  if (dir == 0) {
    f32x4 v;
    v[0] = src[(hi00)*src_pitch + c];
    v[1] = src[(hi00 + 1) * src_pitch + c];
    v[2] = src[(hi00 + 2 * W) * src_pitch + c];
    v[3] = src[(hi00 + 2 * W + 1) * src_pitch + c];
    *reinterpret_cast<f32x4*>(dst + lo * dst_pitch + c * 4) = v;
  } else {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + lo * src_pitch + c * 4);
    float* d = dst;
    if (accumulate) {
      d[(hi00)*dst_pitch + c] += v[0];
      d[(hi00 + 1) * dst_pitch + c] += v[1];
      d[(hi00 + 2 * W) * dst_pitch + c] += v[2];
      d[(hi00 + 2 * W + 1) * dst_pitch + c] += v[3];
    } else {
      d[(hi00)*dst_pitch + c] = v[0];
      d[(hi00 + 1) * dst_pitch + c] = v[1];
      d[(hi00 + 2 * W) * dst_pitch + c] = v[2];
      d[(hi00 + 2 * W + 1) * dst_pitch + c] = v[3];
    }
  }
}

// NCHW [B,C,H,W] dense  <->  NHWC with pitch (pad channels written as zero on the way in)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           long dst_pitch, int B, int C, int HW, int Cpad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * HW * Cpad;
  if (i >= total) return;
  const int c = (int)(i % Cpad);
  const long pix = i / Cpad;
  const int b = (int)(pix / HW);
  const int p = (int)(pix % HW);
  dst[pix * dst_pitch + c] = c < C ? src[((long)b * C + c) * HW + p] : 0.f;
}
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ src, long src_pitch,
                                                           float* __restrict__ dst, int B, int C, int HW) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * C * HW;
  if (i >= total) return;
  const int p = (int)(i % HW);
  const long bc = i / HW;
  const int c = (int)(bc % C);
  const int b = (int)(bc / C);
  dst[i] = src[((long)b * HW + p) * src_pitch + c];
}

// ---------------------------------------------------------------------------------------
// Diffusion training loss (ddpm.py:921-925, 945); q_sample and the objective's target are further down
// ---------------------------------------------------------------------------------------
// per-sample weighted MSE (ddpm.py:921-925): loss = mean_b( w[t_b] * mean_{chw} (out-target)^2 )
// stage 1: one block per sample -> per-sample value; stage 2: one block -> scalar.  Also emits
// gout = gscale * 2 * w[t_b] * (out - target) / (C*HW*B) when gout != null (gscale read from device).
__global__ __launch_bounds__(256) void mse_sample_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                         long pitch, const int64_t* __restrict__ t,
                                                         const float* __restrict__ lw, int C, int HW, int Cpad,
                                                         float* __restrict__ per_sample) {
  __shared__ float sh[16];
  const int b = blockIdx.x;
  const long n = (long)HW * Cpad;
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = (int)(i % Cpad);
    const long pix = (long)b * HW + i / Cpad;
    if (c < C) {
      const float d = out[pix * pitch + c] - target[pix * pitch + c];
      s += d * d;
    }
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) per_sample[b] = s / ((float)C * (float)HW) * (lw ? lw[t[b]] : 1.f);
}
// the same with one 16-byte load per pixel and operand (Cpad == 4: the three image channels + one lane of padding): the scalar
// form above spends 12.8 us per launch at every batch on sixteen dependent rounds of 64-bit divisions and 4-byte loads
__global__ __launch_bounds__(256) void mse_sample4_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                          long pitch, const int64_t* __restrict__ t,
                                                          const float* __restrict__ lw, int C, int HW,
                                                          float* __restrict__ per_sample) {
  __shared__ float sh[16];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int p0 = 0; p0 < HW; p0 += 1024) {                 // four pixels per thread and round: eight loads in flight
    f32x4 o[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int px = p0 + threadIdx.x + 256 * u;
      const long off = ((long)b * HW + (px < HW ? px : HW - 1)) * pitch;
      o[u] = *reinterpret_cast<const f32x4*>(out + off);
      g[u] = *reinterpret_cast<const f32x4*>(target + off);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool live = p0 + threadIdx.x + 256 * u < HW;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float d = o[u][c] - g[u][c];
        s += (live && c < C) ? d * d : 0.f;
      }
    }
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) per_sample[b] = s / ((float)C * (float)HW) * (lw ? lw[t[b]] : 1.f);
}
__global__ void mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = s / (float)n;
}
__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                      long pitch, const int64_t* __restrict__ t,
                                                      const float* __restrict__ lw, const float* __restrict__ gloss,
                                                      int B, int C, int HW, int Cpad, float* __restrict__ gout,
                                                      const float* __restrict__ wb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * HW * Cpad;
  if (i >= total) return;
  const int c = (int)(i % Cpad);
  const long pix = i / Cpad;
  const int b = (int)(pix / HW);
  float g = 0.f;
  if (c < C) {
    const float w = lw ? lw[t[b]] : 1.f;
    const float scale = gloss[0] * 2.f * w / ((float)C * (float)HW * (float)B);
    g = scale * (out[pix * pitch + c] - target[pix * pitch + c]);
    if (wb) g = g * wb[b];               // lgm_weighted_mse_bwd_iw: the sample's importance weight, one more rounding
  }
  gout[pix * pitch + c] = g;
}
// mean_kernel (n_terms 1) and hybrid_mean_kernel (n_terms 2) under a timestep sampler's plan: every per-sample term times
// iw[t_b], the same strided partial sums and block sums - with iw = 1 the plain kernels' bits.  wb[b] = iw[t_b] for the backward.
__global__ void iw_mean_kernel(const float* __restrict__ per, int n_terms, float vb_weight, const long* __restrict__ t,
                               const float* __restrict__ iw, int T, int B, float* __restrict__ wb, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  float s = 0.f, sv = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    long ti = t[i];
    ti = ti < 0 ? 0 : (ti >= T ? T - 1 : ti);
    const float w = iw[ti];
    wb[i] = w;
    s += w * per[i];
    if (n_terms == 2) sv += w * per[B + i];
  }
  s = lgm_block_sum(s, sh);
  if (n_terms == 2) {
    sv = lgm_block_sum(sv, sh);
    if (threadIdx.x == 0) loss[0] = s / (float)B + vb_weight * (sv / (float)B);
  } else if (threadIdx.x == 0) {
    loss[0] = s / (float)B;
  }
}

// GaussianDiffusion's `extract(table, t, shape) * tensor` algebra with a PER-SAMPLE timestep (ddpm.py:673-705, 869-876) on
// dense NCHW tensors: one thread per element, the three table values of the sample are wave-uniform loads.  Contraction is
// off: the reference rounds both products and the sum separately.  A timestep outside the table is clamped to it (the
// reference's gather raises; a device kernel must not fault).
__device__ __forceinline__ float extract_axpby_one(float a, float bb, float d, float xv, float yv, int clip) {
#pragma clang fp contract(off)
  float o = a * xv + bb * yv;
  if (d != 1.f) o = o / d;
  if (clip) o = fminf(fmaxf(o, -1.f), 1.f);
  return o;
}
__global__ __launch_bounds__(256) void extract_axpby_kernel(const float* __restrict__ ta, const float* __restrict__ tb,
                                                            const float* __restrict__ td, const long* __restrict__ t,
                                                            const float* __restrict__ x, const float* __restrict__ y,
                                                            float sb, int clip, float* __restrict__ out, long per,
                                                            int n_table) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  long ti = t[b];
  ti = ti < 0 ? 0 : (ti >= n_table ? n_table - 1 : ti);
  const float a = ta ? ta[ti] : 1.f, bb = sb * (tb ? tb[ti] : 1.f), d = td ? td[ti] : 1.f;
  const long base = (long)b * per;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x)
    out[base + i] = extract_axpby_one(a, bb, d, x[base + i], y ? y[base + i] : 0.f, clip);
}
// Graph-replayed sampling (lgm_hip/sampler.py): the per-step scalars come from a device table indexed by a
// device-side step counter, so ONE captured graph serves every step of a chain.
//   sampler_time_kernel      : t[b] = ttable[counter]                         (before the UNet forward)
//   sample_step_slice_kernel : row `counter` of table[n][8] = (A, Bv, R, Rm1, C0, C1, C2, C3), in place
//   sampler_advance_kernel   : counter += 1                                   (last node of the graph)
__global__ void sampler_time_kernel(const long* __restrict__ ttable, const int* __restrict__ counter,
                                    long* __restrict__ t, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) t[i] = ttable[counter[0]];
}
__global__ void sampler_advance_kernel(int* counter) { counter[0] += 1; }

// ---------------------------------------------------------------------------------------
// Diffusion elementwise (ddpm.py:869-876, 684-688, 707-757, 805-829) for every objective GaussianDiffusion accepts
// (ddpm.py:562): objective 0 = pred_noise (the network predicts eps), 1 = pred_x0 (it predicts the image), 2 = pred_v.
//   q_sample + target : x0 = img*2-1 (auto_normalize) ; x_t = sa[t]*x0 + sb[t]*noise ; v = sa[t]*noise - sb[t]*x0
//   reverse update    : (x0, eps) = model_predictions(x, network output) ; out = C0*x0 + C1*x + C2*eps + C3*noise
// img / noise NCHW dense [B,C,HW]; the network's buffers NHWC with a pitch, pad lanes written as zero.
// ---------------------------------------------------------------------------------------
// offset noise (ddpm.py:889-891, `noise += strength * offset[b, c]`): product and sum rounded separately, like the two
// ATen operations of the reference
__device__ __forceinline__ float offset_noise_one(float n, float strength, float off) {
#pragma clang fp contract(off)
  const float d = strength * off;
  return n + d;
}
// x_t as the reference's q_sample rounds it (two products, one sum) and v with one fused multiply-add, spelled out so that
// the bits do not depend on what the optimiser does here
__device__ __forceinline__ void qsample_one(float a, float bb, float x0, float n, float& xt, float& v) {
#pragma clang fp contract(off)
  xt = a * x0 + bb * n;
  v = fmaf(a, n, -(bb * x0));
}
// model_predictions ddpm.py:707-734, all three branches, from the network output `out` and the head (A, S, R, Rm1) =
// (sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1)[t].  pred_noise keeps the RAW network output unless clip and rederive are
// both set (:720-721).  Contraction off: the reference rounds every product and sum separately.  Written with selects on
// the (wave-uniform) objective, not branches: one straight-line body for the three objectives.
// dyn (uniform: the launch has a threshold buffer): the clip is dynamic thresholding (Saharia et al. 2022, 2.3) with the
// sample's s >= 1 from dyn_thresh_kernel, x0 = clamp(x0, -s, s) / s - one correctly rounded IEEE quotient (the build has no
// fast-math flag: the same reliance as (R * xv - x0) / Rm1 below), so s == 1 gives the static clamp's bits.
__device__ __forceinline__ void predictions_one(int objective, float xv, float ov, float A, float S, float R, float Rm1,
                                                int clip, int rederive, float& pn, float& x0, bool dyn = false,
                                                float s = 1.f) {
#pragma clang fp contract(off)
  const float p = objective == 0 ? R : A, q = objective == 0 ? Rm1 : S;
  const float lin = p * xv - q * ov;                 // predict_start_from_noise :673-677 / predict_start_from_v :690-694
  x0 = objective == 1 ? ov : lin;
  if (clip) {
    if (dyn) x0 = fminf(fmaxf(x0, -s), s) / s;
    else x0 = fminf(fmaxf(x0, -1.f), 1.f);
  }
  const float derived = (R * xv - x0) / Rm1;         // predict_noise_from_start :679-682
  pn = (objective == 0 && !(clip && rederive)) ? ov : derived;
}
__global__ __launch_bounds__(256) void model_predictions_obj_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                                    const long* __restrict__ t, const float* __restrict__ sa,
                                                                    const float* __restrict__ s1, const float* __restrict__ r,
                                                                    const float* __restrict__ rm1, int objective, int clip,
                                                                    int rederive, float* __restrict__ pn,
                                                                    float* __restrict__ xs, long per, int n_table,
                                                                    const float* __restrict__ thresh) {
  const int b = blockIdx.y;
  long ti = t[b];
  ti = ti < 0 ? 0 : (ti >= n_table ? n_table - 1 : ti);
  const float A = sa[ti], S = s1[ti], R = r[ti], Rm1 = rm1[ti];
  const bool dyn = thresh != nullptr;
  const float s = dyn ? thresh[b] : 1.f;
  const long base = (long)b * per;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x) {
    float e, x0;
    predictions_one(objective, x[base + i], out[base + i], A, S, R, Rm1, clip, rederive, e, x0, dyn, s);
    xs[base + i] = x0;
    pn[base + i] = e;
  }
}

// one reverse-diffusion update of one element: head (A, Bv, R, Rm1) of the coefficient row with Bv = -sqrt_1mac[t]; pred_v
// reads all four, pred_noise reads (R, Rm1), pred_x0 reads them for eps only
__device__ __forceinline__ void sample_update_obj(int objective, float xv, float ov, float nz, float A, float Bv, int clip,
                                                  int rederive, float R, float Rm1, float C0, float C1, float C2,
                                                  float C3, float& o, float& x0, bool dyn = false, float s = 1.f) {
#pragma clang fp contract(off)
  float eps;
  predictions_one(objective, xv, ov, A, -Bv, R, Rm1, clip, rederive, eps, x0, dyn, s);
  o = C0 * x0 + C1 * xv + C2 * eps;
  if (C3 != 0.f) o += C3 * nz;
}
// ---------------------------------------------------------------------------------------
// Self-conditioning (ddpm.py:428-435, 899-909): the UNet reads ONE NHWC input buffer [B, HW, pitch] whose lanes
// [sc_off, sc_off + C) hold x_self_cond and [x_off, x_off + C) hold x (cat((x_self_cond, x), dim=1): sc_off = 0, x_off = C,
// pitch = r4(2 C)); every other lane is padding and stays zero.  The kernels below are the producers of those two slices.
// With C = 3 the slices start at lanes 0 and 3 of a pitch of 8: scalar loads and stores only, nothing assumes float4
// alignment.  One thread per (pixel, lane); the lanes c < C do the arithmetic of channel c and write BOTH slices, the others
// write the zeros of the padding they sit on (or nothing).  sc_off < 0: no self-conditioning slice (a network without
// self-conditioning: pitch = r4(C), x_off = 0).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool slice_pad_lane(int lane, int x_off, int sc_off, int C) {
  return !(lane >= x_off && lane < x_off + C) && !(sc_off >= 0 && lane >= sc_off && lane < sc_off + C);
}
// x_start estimate of the first pass (:901-903, model_predictions with clip_x_start=False): reads x_t from the x slice and the
// network output, writes the self-conditioning slice; the x slice and the padding are not touched
__global__ __launch_bounds__(256) void selfcond_estimate_kernel(float* __restrict__ xin, long pitch, int x_off, int sc_off,
                                                                const float* __restrict__ out, long out_pitch,
                                                                const long* __restrict__ t, const float* __restrict__ sa,
                                                                const float* __restrict__ s1, const float* __restrict__ r,
                                                                const float* __restrict__ rm1, int objective, int B, int C,
                                                                int HW, int n_table) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * HW * C) return;
  const int c = (int)(i % C);
  const long pix = i / C;
  long ti = t[pix / HW];
  ti = ti < 0 ? 0 : (ti >= n_table ? n_table - 1 : ti);
  float e, x0;
  predictions_one(objective, xin[pix * pitch + x_off + c], out[pix * out_pitch + c], sa[ti], s1[ti], r[ti], rm1[ti], 0, 0, e,
                  x0);
  xin[pix * pitch + sc_off + c] = x0;
}
// q_sample with the target of the objective (ddpm.py:911-917) and the optional offset noise, which goes into x_t AND into
// the target as in the reference (it is added before q_sample).  x_t into the x slice, zeros into the self-conditioning
// slice and the padding: `lanes` lanes of the pitch are written; the target buffer has pitch tpitch, tCpad lanes written
__global__ __launch_bounds__(256) void qsample_slice_kernel(const float* __restrict__ img, const float* __restrict__ noise,
                                                            const float* __restrict__ offset, float strength,
                                                            const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                            const float* __restrict__ sb, int normalize, int objective,
                                                            float* __restrict__ xin, long pitch, int lanes, int x_off,
                                                            int sc_off, float* __restrict__ target, long tpitch, int tCpad,
                                                            int B, int C, int HW) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * HW * lanes) return;
  const int c = (int)(i % lanes);
  const long pix = i / lanes;
  if (c < C) {
    const int b = (int)(pix / HW);
    const int p = (int)(pix % HW);
    const long s = ((long)b * C + c) * HW + p;
    float x0 = img[s];
    if (normalize) x0 = x0 * 2.f - 1.f;
    float n = noise[s];
    if (offset) n = offset_noise_one(n, strength, offset[(long)b * C + c]);
    const float a = sa[t[b]], bb = sb[t[b]];
    float xv, v;
    qsample_one(a, bb, x0, n, xv, v);
    xin[pix * pitch + x_off + c] = xv;
    if (sc_off >= 0) xin[pix * pitch + sc_off + c] = 0.f;
    if (target) target[pix * tpitch + c] = objective == 0 ? n : (objective == 1 ? x0 : v);
  } else if (target && c < tCpad) {
    target[pix * tpitch + c] = 0.f;
  }
  if (slice_pad_lane(c, x_off, sc_off, C)) xin[pix * pitch + c] = 0.f;
}
// The reverse update for a whole batch at a shared timestep: x from the x slice of `xin`, the next x into the x slice of
// `xout` (xout == xin: in place - a thread reads and writes its own lanes only), x0 as the reference hands it on (clipped
// where it clips) into the self-conditioning slice of `xout` and, when x0_out is given, into lanes [0, C) of that buffer
// (its other lanes zero); zeros into xout's padding.  table == null: the scalars by value in `byval`.  thresh != null ([B],
// from dyn_thresh_kernel): the clip is dynamic thresholding with s = thresh[b]; null: the static clamp, the launch there was.
struct SampleRow { float v[8]; };
__device__ __forceinline__ float learned_logvar(float v, float log_beta, float log_tilde);
// x_{t-1} = mean + exp(0.5 lv) noise of the learned-variance ancestral step, product and sum rounded separately
__device__ __forceinline__ float learned_step_noise(float mean, float nz, float vv, float log_beta, float log_tilde) {
#pragma clang fp contract(off)
  return mean + expf(0.5f * learned_logvar(vv, log_beta, log_tilde)) * nz;
}
// Inpainting (RePaint, Lugmayr et al. 2022, Algorithm 1; lgm_hip/sampler.py inpaint_walk): the operands of the tail both
// update kernels run after their own body when `known` is non-null.  known NHWC [B, HW, r4(C)] (pad lanes never read), mask
// [B, HW] (1 = keep the known pixel, shared by the channels), eps_k / eps_j NCHW dense like the step's noise; the row (M_a,
// M_n, J_x, J_n) by value in `row`, or row counter[0] of table[n][4] (the counter the 8-wide table is read with).
struct InpaintOps {
  const float* known;
  const float* mask;
  const float* eps_k;
  const float* eps_j;
  const float* table;
  float row[4];
};
// known_s = the given image at the level the step lands on, blended with the step's x_s where the mask says so, then the jump
// back up (one affine Gaussian step however many levels) unless the row says (1, 0).  Contraction off, this order: m == 1
// gives known_s and m == 0 gives x_s, bit for bit.
__device__ __forceinline__ float inpaint_tail_one(float xs, float kv, float m, float ek, float ej, float Ma, float Mn,
                                                  float Jx, float Jn) {
#pragma clang fp contract(off)
  const float known_s = Ma * kv + Mn * ek;
  const float y = m * known_s + (1.f - m) * xs;
  return (Jx == 1.f && Jn == 0.f) ? y : Jx * y + Jn * ej;
}
// the tail for element (pix, c) of sample b: loads what its row weighs with something other than zero
__device__ __forceinline__ float inpaint_tail(const InpaintOps& ip, const int* __restrict__ counter, float xs, long pix, int c,
                                              int C, int HW) {
  const long r = ip.table ? 4L * counter[0] : 0;
  const float Ma = ip.table ? ip.table[r + 0] : ip.row[0], Mn = ip.table ? ip.table[r + 1] : ip.row[1];
  const float Jx = ip.table ? ip.table[r + 2] : ip.row[2], Jn = ip.table ? ip.table[r + 3] : ip.row[3];
  const long b = pix / HW, p = pix % HW;
  const long dense = (b * C + c) * HW + p;
  const float ek = Mn != 0.f ? ip.eps_k[dense] : 0.f;
  const float ej = Jn != 0.f ? ip.eps_j[dense] : 0.f;
  return inpaint_tail_one(xs, ip.known[pix * ((C + 3) & ~3) + c], ip.mask[pix], ek, ej, Ma, Mn, Jx, Jn);
}
__global__ __launch_bounds__(256) void sample_step_slice_kernel(const float* xin, float* xout, long pitch, int lanes, int x_off,
                                                                int sc_off, const float* __restrict__ v, long v_pitch,
                                                                const float* __restrict__ noise, int B, int C, int HW,
                                                                SampleRow byval, const float* __restrict__ table,
                                                                const int* __restrict__ counter, int objective, int clip,
                                                                int rederive, float* __restrict__ x0_out, long x0_pitch,
                                                                const float* __restrict__ thresh, InpaintOps ip,
                                                                int learned) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * HW * lanes) return;
  const float* row = table ? table + 8 * counter[0] : byval.v;
  const float A = row[0], Bv = row[1], R = row[2], Rm1 = row[3], C0 = row[4], C1 = row[5];
  // learned (uniform; ancestral step of a learned-variance network): slots 6 / 7 are (log beta_t, log beta~_t), the noise is
  // weighed per element with exp(0.5 lv), lv from lanes [C, 2 C) of v; log beta~_t = -inf marks the step without noise (t = 0)
  const float LB = row[6], LT = row[7];
  const float C2 = learned ? 0.f : row[6], C3 = learned ? (LT == -INFINITY ? 0.f : 1.f) : row[7];
  const int c = (int)(i % lanes);
  const long pix = i / lanes;
  float x0 = 0.f;
  if (c < C) {
    float nz = 0.f;
    if (noise && C3 != 0.f) {
      const int b = (int)(pix / HW), p = (int)(pix % HW);
      nz = noise[((long)b * C + c) * HW + p];
    }
    float o;
    const bool dyn = thresh != nullptr;
    const float s = dyn ? thresh[pix / HW] : 1.f;
    sample_update_obj(objective, xin[pix * pitch + x_off + c], v[pix * v_pitch + c], nz, A, Bv, clip, rederive, R, Rm1, C0,
                      C1, C2, noise && !learned ? C3 : 0.f, o, x0, dyn, s);
    if (learned && noise && C3 != 0.f) o = learned_step_noise(o, nz, v[pix * v_pitch + C + c], LB, LT);
    if (ip.known) o = inpaint_tail(ip, counter, o, pix, c, C, HW);
    xout[pix * pitch + x_off + c] = o;
    if (sc_off >= 0) xout[pix * pitch + sc_off + c] = x0;
  }
  if (x0_out) x0_out[pix * x0_pitch + c] = x0;
  if (slice_pad_lane(c, x_off, sc_off, C)) xout[pix * pitch + c] = 0.f;
}
// DPM-Solver++ (Lu et al. 2022, data prediction; lgm_hip/sampler.py dpm_plan) for one element, from the row (A, Bv, R, Rm1,
// K_x, K_0, K_1, K_n):  x0 = clipped model_predictions branch,  o = K_x x + K_0 x0 [+ K_1 hist] [+ K_n noise].  Contraction
// off and the sum in exactly this order: seven roundings on the longest path (p x, q v, their difference; K_0 x0, the first
// sum; with K_1 hist and K_n noise one sum each - the products K_x x, K_1 hist, K_n noise round beside that path).
__device__ __forceinline__ void dpm_update_one(int objective, float xv, float ov, float hv, float nz, float A, float Bv,
                                               float R, float Rm1, int clip, float Kx, float K0, float K1, float Kn, float& o,
                                               float& x0, bool dyn = false, float s = 1.f) {
#pragma clang fp contract(off)
  float eps;
  predictions_one(objective, xv, ov, A, -Bv, R, Rm1, clip, 0, eps, x0, dyn, s);
  o = Kx * xv + K0 * x0;
  if (K1 != 0.f) o += K1 * hv;
  if (Kn != 0.f) o += Kn * nz;
}
// One DPM-Solver++ step for a whole batch at a shared timestep, laid out like sample_step_slice_kernel: x from the x slice of
// `xin`, the next x into the x slice of `xout` (xout == xin: in place), the clipped x0 into `hist` (NHWC, pitch r4(C) <=
// pitch, pad lanes zero: the x0_prev of the next step) and into xout's self-conditioning slice, zeros into xout's padding.
// hist is read only where K_1 != 0 and the noise only where K_n != 0: the first step of a chain runs on a history buffer
// nobody has written.  One (pixel, lane) per trip of a grid-stride loop, scalar loads and stores only.  thresh as in
// sample_step_slice_kernel: the history and the self-conditioning slice then hold the thresholded x0.
__global__ __launch_bounds__(256) void dpm_step_kernel(const float* xin, float* xout, long pitch, int lanes, int x_off,
                                                       int sc_off, const float* __restrict__ v, long v_pitch,
                                                       const float* __restrict__ noise, float* hist, int B, int C, int HW,
                                                       SampleRow byval, const float* __restrict__ table,
                                                       const int* __restrict__ counter, int objective, int clip,
                                                       const float* __restrict__ thresh, InpaintOps ip) {
  const float* row = table ? table + 8 * counter[0] : byval.v;
  const float A = row[0], Bv = row[1], R = row[2], Rm1 = row[3], Kx = row[4], K0 = row[5], K1 = row[6];
  const float Kn = noise ? row[7] : 0.f;
  const bool dyn = thresh != nullptr;
  const int hp = (C + 3) & ~3;
  const long total = (long)B * HW * lanes;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % lanes);
    const long pix = i / lanes;
    if (c < C) {
      float nz = 0.f, hv = 0.f;
      if (Kn != 0.f) {
        const int b = (int)(pix / HW), p = (int)(pix % HW);
        nz = noise[((long)b * C + c) * HW + p];
      }
      if (K1 != 0.f) hv = hist[pix * hp + c];
      float o, x0;
      const float s = dyn ? thresh[pix / HW] : 1.f;
      dpm_update_one(objective, xin[pix * pitch + x_off + c], v[pix * v_pitch + c], hv, nz, A, Bv, R, Rm1, clip, Kx, K0, K1,
                     Kn, o, x0, dyn, s);
      if (ip.known) o = inpaint_tail(ip, counter, o, pix, c, C, HW);
      xout[pix * pitch + x_off + c] = o;
      if (sc_off >= 0) xout[pix * pitch + sc_off + c] = x0;
      hist[pix * hp + c] = x0;
    } else if (c < hp) {
      hist[pix * hp + c] = 0.f;
    }
    if (slice_pad_lane(c, x_off, sc_off, C)) xout[pix * pitch + c] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// Dynamic thresholding (Saharia et al. 2022, 2.3): s[b] = max(1, quantile_p(|x0[b]|)) over the C * HW values of a sample, the
// quantile by torch.quantile's "linear" rule: q = lo + w (hi - lo) with lo, hi the k-th and (k+1)-th smallest |x0| (0-based;
// (k, w) = lgm_hip.sampler.dyn_rank(n, p) from the host), evaluated in float32 without contraction.
// One workgroup per sample; x0 is recomputed per pass from the x slice and the network output with predictions_one(clip = 0)
// - the bits the update kernel will see - and never stored: three reads of a sample that sits in L2 beside a UNet forward.
// The selection is exact: a radix select on the bit pattern of |x0| (sign bit cleared, a non-negative float orders like its
// uint32 bits) in three passes of 11 + 10 + 10 bits.  A pass counts the digit of every element whose higher bits equal the
// prefix found so far into an LDS histogram of integers, scans the bins and narrows the prefix to the bin that holds rank k;
// after the third the prefix IS the key of lo.  hi is lo again when the last bin holds more elements than the rank left in it
// needs, else the smallest key above lo: the next non-empty bin of the last histogram or, above that bucket, a running
// minimum the last pass keeps.  Integer counts and minima: the result does not depend on the order in which lanes arrive,
// so graph replay equals eager launches bit for bit.  Counting reduces in the wave first: the lanes that share the first
// lane's digit add their number once (a batch of near-equal magnitudes is one LDS atomic per wave, not 64 on one address).
// NaN / Inf: inputs are assumed finite.  A NaN's key lies above Inf's, so non-finite values sort to the top and reach s only
// when the rank does; an infinite s makes NaN of the Inf elements in the update (Inf / Inf), a NaN q gives s = 1.
// ---------------------------------------------------------------------------------------
constexpr int DT_THREADS = 1024;
constexpr int DT_BINS = 2048;
__device__ __forceinline__ void dyn_count(unsigned* hist, unsigned digit) {
  const unsigned lead = __builtin_amdgcn_readfirstlane(digit);
  const unsigned long long same = __ballot(digit == lead);          // of the lanes that are here
  if (digit == lead) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&hist[lead], (unsigned)__popcll(same));
  } else {
    atomicAdd(&hist[digit], 1u);
  }
}
__device__ __forceinline__ float dyn_interp(float lo, float hi, float w) {
#pragma clang fp contract(off)
  const float d = hi - lo;
  const float q = lo + w * d;
  return fmaxf(q, 1.f);
}
__global__ __launch_bounds__(DT_THREADS) void dyn_thresh_kernel(const float* __restrict__ xin, long pitch, int x_off,
                                                                const float* __restrict__ v, long v_pitch, int C, int HW,
                                                                SampleRow byval, const float* __restrict__ table,
                                                                const int* __restrict__ counter, int objective, unsigned k,
                                                                float w, float* __restrict__ thresh) {
  __shared__ unsigned hist[DT_BINS];
  __shared__ unsigned wsum[DT_THREADS / 64];
  __shared__ unsigned sel[4];            // the bin of rank k, the rank left inside it, its count; the smallest key above lo
  const float* row = table ? table + 8 * counter[0] : byval.v;
  const float A = row[0], Bv = row[1], R = row[2], Rm1 = row[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long base = (long)blockIdx.x * HW;
  unsigned prefix = 0, krem = k, above = 0xffffffffu, bin = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = 20 - 10 * pass;                     // digits: bits 30..20, 19..10, 9..0
    const int nb = pass == 0 ? 2048 : 1024;
    const int hs = pass == 0 ? 31 : shift + 10;           // key >> hs: the bits above this pass's digit (pass 0: none)
    for (int i = tid; i < DT_BINS; i += DT_THREADS) hist[i] = 0;
    if (tid == 0) sel[3] = 0xffffffffu;
    __syncthreads();
    for (int p = tid; p < HW; p += DT_THREADS) {
      const float* xp = xin + (base + p) * pitch + x_off;
      const float* vp = v + (base + p) * v_pitch;
      for (int c = 0; c < C; ++c) {
        float e, x0;
        predictions_one(objective, xp[c], vp[c], A, -Bv, R, Rm1, 0, 0, e, x0);
        const unsigned key = __float_as_uint(x0) & 0x7fffffffu;
        const unsigned up = key >> hs;
        if (up == prefix) dyn_count(hist, (key >> shift) & (unsigned)(nb - 1));
        else if (pass == 2 && up > prefix) above = key < above ? key : above;
      }
    }
    __syncthreads();
    // exclusive scan of the bins, nb / 1024 consecutive bins per thread: the one thread whose bins hold rank krem publishes
    const int per = nb / DT_THREADS;
    unsigned loc = 0;
    for (int j = 0; j < per; ++j) loc += hist[tid * per + j];
    unsigned inc = loc;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned ex = inc - loc;
    for (int j = 0; j < wave; ++j) ex += wsum[j];
    if (krem >= ex && krem < ex + loc) {
      unsigned cum = ex;
      int bsel = tid * per;
      for (int j = 0; j < per; ++j) {
        const unsigned cnt = hist[tid * per + j];
        if (krem < cum + cnt) { bsel = tid * per + j; break; }
        cum += cnt;
      }
      sel[0] = (unsigned)bsel; sel[1] = krem - cum; sel[2] = hist[bsel];
    }
    __syncthreads();
    bin = sel[0];
    krem = sel[1];
    prefix = (prefix << (pass == 0 ? 11 : 10)) | bin;
  }
  // prefix = the key of lo.  The smallest key above it: the next non-empty bin of the last histogram, else `above`
  unsigned cand = above;
  if ((unsigned)tid > bin && hist[tid] != 0) {
    const unsigned kk = (prefix & ~1023u) | (unsigned)tid;
    cand = kk < cand ? kk : cand;
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned o = __shfl_xor(cand, d, 64);
    cand = o < cand ? o : cand;
  }
  if (lane == 0 && cand != 0xffffffffu) atomicMin(&sel[3], cand);
  __syncthreads();
  if (tid == 0) {
    unsigned hik = krem + 1 < sel[2] ? prefix : sel[3];
    if (hik == 0xffffffffu) hik = prefix;                 // k = n - 1: nothing above lo
    thresh[blockIdx.x] = dyn_interp(__uint_as_float(prefix), __uint_as_float(hik), w);
  }
}

// ---------------------------------------------------------------------------------------
// Variational-bound terms in bits per dimension (Ho et al. 2020, eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop; an extension
// of the reference; lgm_hip/likelihood.py vlb_plan): per sample b and evaluated timestep (row r)
//     out[r][0][b]  the term of the bound   out[r][1][b] = mean (x0_pred - x0)^2   out[r][2][b] = mean (eps_pred - noise)^2
// from the image x0 (NCHW, normalised here when `normalize`), the noise q_sample drew (NCHW), x_t in the x slice of the network's
// input buffer and the network output, with (x0_pred, eps_pred) = predictions_one(rederive = 1).  The row of VLB_ROW floats
//     (A, S, R, Rm1, P1, P2, kind, KC, KW, inv_std, ., .)        P1, P2 = posterior_mean_coef1/2[t]
//   kind 0, KL (t >= 1):  (KC + KW mean(d^2)) / ln 2,  d = P1 (x0_pred - x0).  Both posterior means share P2 x_t, so the
//           difference of the means IS P1 (x0_pred - x0); at large t, P1 is 1e-2 ... 1e-4 and two O(1) means formed in float32
//           and subtracted would keep three to four digits less.
//   kind 1, decoder (t = 0):  -mean(log p) / ln 2,  log p = vlb_decoder_logp below.
//   kind 3 / 4, KL / decoder of a learned-variance network: mean(learned_term) / ln 2 with the element's own log-variance from
//           lanes [C, 2 C) of the network output and slots 10 / 11 = (log beta_t, log beta~_t); these kinds read 12 slots.
//   kind 2, prior:  (KC + KW mean(x0^2)) / ln 2 with the host's KC = 0.5 (-1 - log(1 - acp) + (1 - acp)), KW = 0.5 acp: the
//           sum in KC cancels to ~acp^2 / 2 and is formed in float64 on the host.  Reads img only; [1] and [2] come out 0.
// One workgroup per sample; a lane owns pixels and loops over the channels (the NCHW reads coalesce over pixels); three sums
// through lgm_block_sum in its fixed order - no atomics, no second stage: eager launches and graph replays give the same
// bits.  kind is launch-uniform.  A row index outside [0, n_rows) writes nothing.
// ---------------------------------------------------------------------------------------
constexpr int VLB_ROW = 12;
constexpr int VLB_THREADS = 256;
struct VlbRow { float v[VLB_ROW]; };
__device__ __forceinline__ float vlb_softplus(float x) { return x > 0.f ? x + log1pf(expf(-x)) : log1pf(expf(x)); }
// log(1 - exp(-y)) for y > 0 without cancellation at either end
__device__ __forceinline__ float vlb_log1mexp(float y) { return y > 0.69314718f ? log1pf(-expf(-y)) : logf(-expm1f(-y)); }
// Discretised Gaussian log-likelihood (Nichol & Dhariwal 2021, discretized_gaussian_log_likelihood) of x on the 8-bit grid
// of [-1, 1] under N(mean, 1 / inv_std^2) with the tanh approximation of the normal CDF, Phi(z) = (1 + tanh(k (z + 0.044715
// z^3))) / 2 = sigmoid(2 u(z)), k = sqrt(2 / pi): log Phi(z+) for x < -0.999, log(1 - Phi(z-)) for x > 0.999, else log(Phi(z+) -
// Phi(z-)), z+- = inv_std (x - mean +- 1/255), every probability floored at 1e-12.  1 - tanh(u) has no float32 bits left from
// |z| ~ 4.6 while the floor only takes over at |z| ~ 6.1, so the same function is evaluated without cancellation: with a =
// 2 u(z+), b = 2 u(z-), h = (a - b) / 2 > 0 and m = (a + b) / 2
//     sigmoid(a) - sigmoid(b) = sinh(h) / (cosh(m) + cosh(h)),   log sigmoid(a) = -softplus(-a),   log(1 - sigmoid(b)) = -softplus(b)
// h and m come from the polynomial identities in (z_c, delta) = (inv_std (x - mean), inv_std / 255), not from a difference of
// two values of u, and the logarithm of the quotient is taken with max(|m|, h) factored out, so no exponential overflows.
__device__ __forceinline__ float vlb_decoder_logp(float x, float mean, float inv_std) {
#pragma clang fp contract(off)
  const float K = 0.7978845608f, C3 = 0.044715f, FLOOR = -27.6310211f;     // sqrt(2 / pi); log 1e-12
  const float zc = inv_std * (x - mean), dl = inv_std * (1.f / 255.f);
  float lp;
  if (x < -0.999f || x > 0.999f) {
    const float z = x < 0.f ? zc + dl : zc - dl;
    const float a = 2.f * (K * (z + C3 * (z * z * z)));
    lp = -vlb_softplus(x < 0.f ? -a : a);
  } else {
    const float h = K * (2.f * dl + C3 * (6.f * (zc * zc) * dl + 2.f * (dl * dl * dl)));
    const float m = fabsf(K * (2.f * zc + C3 * (2.f * (zc * zc * zc) + 6.f * zc * (dl * dl))));
    // log sinh h = h + log(1 - e^{-2h}) - ln 2;  log(cosh m + cosh h) = M + log(1 + rest) - ln 2,  M = max(m, h)
    const float rest = h >= m ? expf(m - h) + expf(-m - h) + expf(-2.f * h) : expf(h - m) + expf(-h - m) + expf(-2.f * m);
    lp = (h >= m ? 0.f : h - m) + vlb_log1mexp(2.f * h) - log1pf(rest);
  }
  return fmaxf(lp, FLOOR);
}
// ---------------------------------------------------------------------------------------
// Learned variance (Nichol & Dhariwal 2021, 3.1): the network's lanes [C, 2 C) hold v, and the model's log-variance of an
// element is lv = f log beta_t + (1 - f) log beta~_t with f = (v + 1) / 2 (f outside [0, 1] is legal; log beta~_1 at t = 0,
// lgm_hip/likelihood.py's convention).  learned_logvar is that interpolation, learned_term the bound's term of ONE element in
// nats with the model mean P1 x0_pred + P2 x_t and, when dlv is given, its derivative with respect to lv - the one function
// behind the training loss (hybrid_loss_*_kernel) and the likelihood (vlb_term_kernel, kinds 3 and 4).
//   KL (t >= 1):  0.5 (-1 + lv - lv_q + exp(lv_q - lv) + d^2 exp(-lv)),  d = P1 (x0_pred - x0)
//                 d/dlv = 0.5 (1 - exp(lv_q - lv) - d^2 exp(-lv))
//   decoder (t = 0):  -vlb_decoder_logp(x0, mean, s),  s = exp(-0.5 lv).  z+-, and with them a, h, m of vlb_decoder_logp, are
//                 proportional to s up to the cubic term, so s d/ds of them is the same polynomial with the cubic term tripled
//                 (az, hs, ms below) and d(-log p)/dlv = 0.5 s dlog p/ds.  In the same cancellation-free form:
//                 end bins     s dlog p/ds = sigmoid(-a) az  (x < -0.999),  -sigmoid(a) az  (x > 0.999)
//                 interior     dlog p/dh = coth h - sinh h / (cosh m + cosh h) = (cosh h cosh m + 1) / (sinh h (cosh m + cosh h)),
//                              dlog p/d|m| = -sinh |m| / (cosh m + cosh h), both with e^{max(|m|, h)} factored out
//                 A floored probability has gradient 0, as clamp(min = 1e-12) gives.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float learned_logvar(float v, float log_beta, float log_tilde) {
#pragma clang fp contract(off)
  const float f = 0.5f * (v + 1.f);
  return f * log_beta + (1.f - f) * log_tilde;
}
__device__ __forceinline__ float learned_term(bool decoder, float x0, float x0p, float xv, float P1, float P2, float lv,
                                              float lv_q, float* dlv) {
#pragma clang fp contract(off)
  if (!decoder) {
    const float d = P1 * (x0p - x0);
    const float r = expf(lv_q - lv), q = (d * d) * expf(-lv);
    if (dlv) *dlv = 0.5f * ((1.f - r) - q);
    return 0.5f * (((-1.f + (lv - lv_q)) + r) + q);
  }
  const float K = 0.7978845608f, C3 = 0.044715f, FLOOR = -27.6310211f;
  const float inv_std = expf(-0.5f * lv);
  const float mean = P1 * x0p + P2 * xv;
  const float lp = vlb_decoder_logp(x0, mean, inv_std);
  if (dlv) {
    const float zc = inv_std * (x0 - mean), dl = inv_std * (1.f / 255.f);
    float g;                                   // s dlog p / ds
    if (x0 < -0.999f || x0 > 0.999f) {
      const float z = x0 < 0.f ? zc + dl : zc - dl;
      const float a = 2.f * (K * (z + C3 * (z * z * z)));
      const float az = 2.f * (K * (z + 3.f * C3 * (z * z * z)));
      g = x0 < 0.f ? az / (1.f + expf(a)) : -(az / (1.f + expf(-a)));
    } else {
      const float h = K * (2.f * dl + C3 * (6.f * (zc * zc) * dl + 2.f * (dl * dl * dl)));
      const float m = fabsf(K * (2.f * zc + C3 * (2.f * (zc * zc * zc) + 6.f * zc * (dl * dl))));
      const float hs = K * (2.f * dl + 3.f * C3 * (6.f * (zc * zc) * dl + 2.f * (dl * dl * dl)));
      const float ms = fabsf(K * (2.f * zc + 3.f * C3 * (2.f * (zc * zc * zc) + 6.f * zc * (dl * dl))));
      const float E = expf(-2.f * h), F = expf(-2.f * m);
      const float omE = -expm1f(-2.f * h), omF = -expm1f(-2.f * m);
      float num, den, sm;
      if (m >= h) {
        const float e = expf(h - m);
        den = (1.f + F) + e * (1.f + E);
        num = (1.f + E) * (1.f + F) + 4.f * expf(-h - m);
        sm = omF;
      } else {
        const float e = expf(m - h);
        den = e * (1.f + F) + (1.f + E);
        num = e * ((1.f + E) * (1.f + F)) + 4.f * E;
        sm = e * omF;
      }
      g = (num / (omE * den)) * hs - (sm / den) * ms;
    }
    *dlv = lp > FLOOR ? 0.5f * g : 0.f;
  }
  return -lp;
}
// ---------------------------------------------------------------------------------------
// Hybrid loss of a learned-variance network (Nichol & Dhariwal 2021, eq. 16; lgm_hybrid_loss_fwd / _bwd):
//     L = mean_b(lw[t_b] mse_b) + vb_weight mean_b(vb_b)
// mse_b over lanes [0, C) as mse_sample_kernel forms it, vb_b the bound's term at t_b in bits per dimension (learned_term; the
// mean is detached and built from the UNCLIPPED x0 prediction).  tab [T][8] = (log beta_t, log beta~_t, lv_q, P1, P2, 0, 0, 0).
// Forward: one workgroup per sample, two sums through lgm_block_sum in its fixed order, per[b] = lw mse_b, per[B + b] = vb_b;
// a one-workgroup second stage writes the scalar.  Backward: elementwise over the output's pitch; lanes [0, C) as
// mse_bwd_kernel writes them, lanes [C, 2 C) the gradient through lv alone, every other lane zero.
// ---------------------------------------------------------------------------------------
struct HybridTables {
  const float* sa;
  const float* s1;
  const float* r;
  const float* rm1;
  const float* lw;
  const float* tab;
  int n_table;
};
__device__ __forceinline__ float hybrid_element(const HybridTables& T, long ti, int objective, float x0, float xv, float ov,
                                                float vv, float* dlv) {
  const float* row = T.tab + 8 * ti;
  float e, x0p;
  predictions_one(objective, xv, ov, T.sa[ti], T.s1[ti], T.r[ti], T.rm1[ti], 0, 0, e, x0p);
  const float lv = learned_logvar(vv, row[0], row[1]);
  return learned_term(ti == 0, x0, x0p, xv, row[3], row[4], lv, row[2], dlv);
}
__global__ __launch_bounds__(256) void hybrid_loss_fwd_kernel(const float* __restrict__ out, long pitch,
                                                              const float* __restrict__ target, long t_pitch,
                                                              const float* __restrict__ img, int normalize,
                                                              const float* __restrict__ xin, long x_pitch, int x_off,
                                                              const long* __restrict__ t, HybridTables T, int objective,
                                                              int C, int HW, float* __restrict__ per, int B) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const int b = blockIdx.x;
  long ti = t[b];
  ti = ti < 0 ? 0 : (ti >= T.n_table ? T.n_table - 1 : ti);
  float s = 0.f, sv = 0.f;
  for (int p = threadIdx.x; p < HW; p += 256) {
    const long pix = (long)b * HW + p;
    for (int c = 0; c < C; ++c) {
      const float ov = out[pix * pitch + c];
      const float d = ov - target[pix * t_pitch + c];
      s += d * d;
      float x0 = img[((long)b * C + c) * HW + p];
      if (normalize) x0 = x0 * 2.f - 1.f;
      sv += hybrid_element(T, ti, objective, x0, xin[pix * x_pitch + x_off + c], ov, out[pix * pitch + C + c], nullptr);
    }
  }
  s = lgm_block_sum(s, sh);
  sv = lgm_block_sum(sv, sh);
  if (threadIdx.x == 0) {
    const float n = (float)C * (float)HW;
    per[b] = s / n * (T.lw ? T.lw[ti] : 1.f);
    per[B + b] = sv / n / 0.69314718f;
  }
}
__global__ void hybrid_mean_kernel(const float* __restrict__ per, int B, float vb_weight, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  float s = 0.f, sv = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    s += per[i];
    sv += per[B + i];
  }
  s = lgm_block_sum(s, sh);
  sv = lgm_block_sum(sv, sh);
  if (threadIdx.x == 0) loss[0] = s / (float)B + vb_weight * (sv / (float)B);
}
__global__ __launch_bounds__(256) void hybrid_loss_bwd_kernel(const float* __restrict__ out, long pitch,
                                                              const float* __restrict__ target, long t_pitch,
                                                              const float* __restrict__ img, int normalize,
                                                              const float* __restrict__ xin, long x_pitch, int x_off,
                                                              const long* __restrict__ t, HybridTables T, int objective,
                                                              const float* __restrict__ gloss, float vb_weight, int B,
                                                              int C, int HW, float* __restrict__ gout,
                                                              const float* __restrict__ wb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * HW * pitch;
  if (i >= total) return;
  const int c = (int)(i % pitch);
  const long pix = i / pitch;
  const int b = (int)(pix / HW);
  float g = 0.f;
  if (c < 2 * C) {
    long ti = t[b];
    ti = ti < 0 ? 0 : (ti >= T.n_table ? T.n_table - 1 : ti);
    if (c < C) {
      const float w = T.lw ? T.lw[ti] : 1.f;
      const float scale = gloss[0] * 2.f * w / ((float)C * (float)HW * (float)B);
      g = scale * (out[pix * pitch + c] - target[pix * t_pitch + c]);
    } else {
#pragma clang fp contract(off)
      const int cc = c - C, p = (int)(pix % HW);
      float x0 = img[((long)b * C + cc) * HW + p];
      if (normalize) x0 = x0 * 2.f - 1.f;
      float dlv;
      hybrid_element(T, ti, objective, x0, xin[pix * x_pitch + x_off + cc], out[pix * pitch + cc], out[pix * pitch + c], &dlv);
      const float* row = T.tab + 8 * ti;
      const float scale = gloss[0] * vb_weight / ((float)B * ((float)C * (float)HW) * 0.69314718f);
      g = scale * dlv * (0.5f * (row[0] - row[1]));
    }
    if (wb) g = g * wb[b];               // lgm_hybrid_loss_bwd_iw: the sample's importance weight, as mse_bwd_kernel applies it
  }
  gout[pix * pitch + c] = g;
}
__global__ __launch_bounds__(VLB_THREADS) void vlb_term_kernel(const float* __restrict__ img, const float* __restrict__ noise,
                                                               int normalize, const float* __restrict__ xin, long pitch,
                                                               int x_off, const float* __restrict__ v, long v_pitch, int B,
                                                               int C, int HW, VlbRow byval, const float* __restrict__ table,
                                                               int stride, const int* __restrict__ counter, int out_row,
                                                               int objective, int clip, float* __restrict__ out, int n_rows,
                                                               int v_lanes) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const int r = table ? counter[0] : out_row;
  if (r < 0 || r >= n_rows) return;
  const float* row = table ? table + (long)stride * r : byval.v;
  const float A = row[0], S = row[1], R = row[2], Rm1 = row[3], P1 = row[4], P2 = row[5];
  const int kind = (int)row[6];
  const float KC = row[7], KW = row[8], inv_std = row[9];
  if (kind < 0 || kind > 4 || (kind >= 3 && v_lanes < 2 * C)) return;     // a learned row on an output without the head
  const bool learned = kind == 3 || kind == 4;          // slots 10 / 11: log beta_t, log beta~_t; lanes [C, 2 C) of v: the head
  const float LB = learned ? row[10] : 0.f, LT = learned ? row[11] : 0.f;
  const int b = blockIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int p = threadIdx.x; p < HW; p += VLB_THREADS) {
    const long pix = (long)b * HW + p;
    for (int c = 0; c < C; ++c) {
      const long dense = ((long)b * C + c) * HW + p;
      float x0 = img[dense];
      if (normalize) x0 = x0 * 2.f - 1.f;
      if (kind == 2) {
        s0 += x0 * x0;
        continue;
      }
      const float xv = xin[pix * pitch + x_off + c];
      float e, x0p;
      predictions_one(objective, xv, v[pix * v_pitch + c], A, S, R, Rm1, clip, 1, e, x0p);
      const float d0 = x0p - x0, de = e - noise[dense];
      s1 += d0 * d0;
      s2 += de * de;
      if (learned) {
        s0 += learned_term(kind == 4, x0, x0p, xv, P1, P2, learned_logvar(v[pix * v_pitch + C + c], LB, LT), LT, nullptr);
      } else if (kind == 0) {
        const float d = P1 * d0;
        s0 += d * d;
      } else {
        s0 += vlb_decoder_logp(x0, P1 * x0p + P2 * xv, inv_std);
      }
    }
  }
  s0 = lgm_block_sum(s0, sh);
  s1 = lgm_block_sum(s1, sh);
  s2 = lgm_block_sum(s2, sh);
  if (threadIdx.x == 0) {
    const float n = (float)C * (float)HW, LN2 = 0.69314718f;
    float* o = out + (long)r * 3 * B + b;
    o[0] = (learned ? s0 / n : kind == 1 ? -(s0 / n) : KC + KW * (s0 / n)) / LN2;
    o[B] = s1 / n;
    o[2 * B] = s2 / n;
  }
}

// ---------------------------------------------------------------------------------------
// The UNet's time embedding in ONE launch (reference ddpm.py:119-132 SinusoidalPosEmb, :328-333 time_mlp = Linear ->
// GELU -> Linear, and the SiLU in front of every ResnetBlock.mlp's Linear :181-183).  It was six launches of 4 - 7 us that
// no batch size shrinks (posemb, GEMM, GELU, split-K GEMM, reducer, SiLU): ~32 us of every training step and of every
// sampling step.  A workgroup owns RB rows of the batch for the whole chain; a row's vectors live in LDS / registers; a
// weight row is read by lpr = min(64, K / 4) lanes together (16 bytes each: one coalesced instruction per row, or per
// 64 / lpr rows) and summed by a fixed xor-butterfly, so a row's result does not depend on the batch it arrives in
// (2 ranks x B/2 rows == 1 rank x B rows bit for bit).
// ---------------------------------------------------------------------------------------
// One linear layer of the chain for the RB rows a workgroup owns: out[r][n] = bias[n] + sum_k xs[r][k] W[n][k], K <= 256.
// lpr = K / 4 lanes share a weight row (16 bytes each; k order per lane k = 4 sub + j, then a fixed xor-butterfly); a wave
// owns the rows n = wave * rpp + grp + u * stride.  EVERY global load of a layer (U weight rows + their bias per lane) is
// issued by tm_fetch() before anything is computed - for both layers at kernel entry - because a load that misses costs
// 1 - 2 us here (every launch starts cold): the first version (one weight row per loop trip, bias read in the epilogue) spent
// 140 us in ~70 dependent round trips, the second (eight rows per trip) 50 us.
constexpr int TM_RB = 4;
constexpr int TM_THREADS = 512;    // 8 waves, two per SIMD: 256 registers per lane for the prefetched weight rows
template <int U>
struct TmRows {
  f32x4 w[U];
  float b[U];
};
typedef unsigned tm_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tm_rsrc(const float* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                           __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
// Raw buffer loads: ONE lane offset per operand (row wave * rpp + grp, column 4 sub) and a compile-time scalar offset per u
// (rows u * stride apart: stride * K = nwaves * 256 floats whatever K is), so the U loads of a wave need no address
// registers (64-bit flat addresses for 32 rows spilled 340 registers); a row >= N is outside the descriptor's range and
// reads as zeros.
template <int U>
__device__ __forceinline__ void tm_fetch(TmRows<U>& R, const float* __restrict__ W, const float* __restrict__ bias, int K,
                                         int N) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NW = TM_THREADS / 64;
  const int lpr = K / 4, rpp = 64 / lpr, sub = lane % lpr, grp = lane / lpr;
  const __amdgpu_buffer_rsrc_t rw = tm_rsrc(W, (unsigned)N * (unsigned)K * 4u);
  const __amdgpu_buffer_rsrc_t rb = tm_rsrc(bias, (unsigned)N * 4u);
  const unsigned vw = ((unsigned)(wave * rpp + grp) * (unsigned)K + 4u * (unsigned)sub) * 4u;
  const unsigned vb = (unsigned)(wave * rpp + grp) * 4u;
  const unsigned sb = (unsigned)(NW * rpp) * 4u;      // bias: rows are stride apart (wave-uniform, runtime)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    R.w[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, vw, (unsigned)u * (NW * 256u * 4u), 0));
    R.b[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, vb, (unsigned)u * sb, 0));
  }
}
template <int U, class Emit>
__device__ __forceinline__ void tm_rows(const TmRows<U>& R, const float* __restrict__ xs, int K, int N, Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int lpr = K / 4, rpp = 64 / lpr, sub = lane % lpr, grp = lane / lpr, stride = nwaves * rpp;
  float xin[TM_RB][4];
#pragma unroll
  for (int r = 0; r < TM_RB; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) xin[r][j] = xs[r * K + 4 * sub + j];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int nb = wave * rpp + u * stride;           // wave-uniform: the butterfly below is never divergent
    if (nb >= N) break;
    float acc[TM_RB];
#pragma unroll
    for (int r = 0; r < TM_RB; ++r) {
      acc[r] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[r] = fmaf(xin[r][j], R.w[u][j], acc[r]);
    }
    for (int off = lpr >> 1; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < TM_RB; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
    if (sub == 0 && nb + grp < N) emit(nb + grp, R.b[u], acc);
  }
}

__global__ __launch_bounds__(TM_THREADS) void time_mlp_fwd_kernel(const long* __restrict__ t, int B, int dim,
                                                                  const float* __restrict__ freqs,
                                                                  const float* __restrict__ W1, const float* __restrict__ b1,
                                                                  const float* __restrict__ W2, const float* __restrict__ b2,
                                                                  int td, float* __restrict__ pe, float* __restrict__ a1,
                                                                  float* __restrict__ h, float* __restrict__ temb,
                                                                  float* __restrict__ st) {
  extern __shared__ float tm_sm[];
  float* spe = tm_sm;                    // [RB][dim]
  float* sh = tm_sm + TM_RB * dim;       // [RB][td]  activations (the next layer's input)
  float* sa = sh + TM_RB * td;           // [RB][td]  pre-activations
  const int r0 = blockIdx.x * TM_RB, half = dim / 2;
  // 8 waves.  Layer 2 (K = td <= 256): at most 32 weight rows per wave (rpp = 1 at td = 256); layer 1: td * dim / 2048 <= 8
  // (host check: time_dim * dim <= 16384).
  TmRows<8> R1;
  TmRows<32> R2;
  tm_fetch(R1, W1, b1, dim, td);
  for (int i = threadIdx.x; i < TM_RB * half; i += blockDim.x) {
    const int r = i / half, j = i % half, b = r0 + r;
    float sv = 0.f, cv = 0.f;
    if (b < B) {                         // posemb_kernel's arithmetic
      const float arg = (float)t[b] * freqs[j];
      sv = sinf(arg), cv = cosf(arg);
      pe[(long)b * dim + j] = sv;
      pe[(long)b * dim + half + j] = cv;
    }
    spe[r * dim + j] = sv;
    spe[r * dim + half + j] = cv;
  }
  tm_fetch(R2, W2, b2, td, td);          // in flight while layer 1 is computed
  __syncthreads();
  // the activations run in their own elementwise passes: inside the unrolled row loop 32 inlined erff / expf bodies cost
  // 310 spilled registers
  tm_rows(R1, spe, dim, td, [&](int n, float bias, const float* acc) {
#pragma unroll
    for (int r = 0; r < TM_RB; ++r) sa[r * td + n] = acc[r] + bias;
  });
  __syncthreads();
  for (int i = threadIdx.x; i < TM_RB * td; i += blockDim.x) {
    const int r = i / td, n = i % td;
    const float a = sa[i], g = act_fwd(a, ACT_GELU, 0.f);
    sh[i] = g;
    if (r0 + r < B) a1[(long)(r0 + r) * td + n] = a, h[(long)(r0 + r) * td + n] = g;
  }
  __syncthreads();
  tm_rows(R2, sh, td, td, [&](int n, float bias, const float* acc) {
#pragma unroll
    for (int r = 0; r < TM_RB; ++r) sa[r * td + n] = acc[r] + bias;
  });
  __syncthreads();
  for (int i = threadIdx.x; i < TM_RB * td; i += blockDim.x) {
    const int r = i / td, n = i % td;
    if (r0 + r < B) {
      const float e = sa[i];
      temb[(long)(r0 + r) * td + n] = e;
      st[(long)(r0 + r) * td + n] = act_fwd(e, ACT_SILU, 0.f);
    }
  }
}

// backward, row-local half: gtemb = gst * silu'(temb); gh = gtemb W2 (thread = (k, quarter of the n range): coalesced weight
// rows, eight of them requested per trip, LDS-broadcast gtemb; the four quarters are added in order); ga1 = gh * gelu'(a1)
__global__ __launch_bounds__(TM_THREADS) void time_mlp_bwd_rows_kernel(const float* __restrict__ gst,
                                                                       const float* __restrict__ a1,
                                                                       const float* __restrict__ temb,
                                                                       const float* __restrict__ W2, int B, int td,
                                                                       float* __restrict__ gtemb, float* __restrict__ ga1) {
  extern __shared__ float tm_sm[];       // [td][RB] (one 16-byte broadcast read per n), then [4][td][RB] partial sums
  float* part = tm_sm + td * TM_RB;
  const int r0 = blockIdx.x * TM_RB;
  for (int i = threadIdx.x; i < TM_RB * td; i += blockDim.x) {
    const int r = i / td, n = i % td, b = r0 + r;
    float g = 0.f;
    if (b < B) {
      g = gst[(long)b * td + n] * act_bwd(temb[(long)b * td + n], ACT_SILU, 0.f);
      gtemb[(long)b * td + n] = g;
    }
    tm_sm[n * TM_RB + r] = g;
  }
  __syncthreads();
  const int kq = blockDim.x / 4;                      // threads along k per quarter (256)
  const int q = threadIdx.x / kq, kt = threadIdx.x % kq;
  const int nq = td / 4;                              // n range of a quarter (td % 16 == 0)
  for (int k = kt; k < td; k += kq) {
    float acc[TM_RB];
#pragma unroll
    for (int r = 0; r < TM_RB; ++r) acc[r] = 0.f;
    for (int n = q * nq; n < (q + 1) * nq; n += 8) {
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = W2[(long)(n + u) * td + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(tm_sm + (n + u) * TM_RB);
#pragma unroll
        for (int r = 0; r < TM_RB; ++r) acc[r] = fmaf(g[r], w[u], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < TM_RB; ++r) part[(q * td + k) * TM_RB + r] = acc[r];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TM_RB * td; i += blockDim.x) {
    const int k = i / TM_RB, r = i % TM_RB;
    if (r0 + r < B) {
      const float gh = ((part[(0 * td + k) * TM_RB + r] + part[(1 * td + k) * TM_RB + r]) + part[(2 * td + k) * TM_RB + r]) +
                       part[(3 * td + k) * TM_RB + r];
      ga1[(long)(r0 + r) * td + k] = gh * act_bwd(a1[(long)(r0 + r) * td + k], ACT_GELU, 0.f);
    }
  }
}

// backward, batch-reducing half: gW[n][k] = beta gW[n][k] + sum_r gy[r][n] x[r][k], gb[n] = beta gb[n] + sum_r gy[r][n], rows in
// order (deterministic).  A workgroup owns TN consecutive n; 32 rows of x and gy at a time are staged in LDS by all threads
// (many loads in flight: the row-by-row version spent its 120 us waiting for one load per trip), thread = (k, n slice).
// blockIdx.y = 0: the second linear (x = h, K = td), 1: the first (x = pe, K = dim).  K <= 256.
__global__ __launch_bounds__(256) void time_mlp_bwd_wgrad_kernel(const float* __restrict__ gtemb, const float* __restrict__ h,
                                                                 const float* __restrict__ ga1, const float* __restrict__ pe,
                                                                 int B, int dim, int td, float* __restrict__ gw2,
                                                                 float* __restrict__ gb2, float* __restrict__ gw1,
                                                                 float* __restrict__ gb1, float beta) {
  constexpr int TN = 16, RC = 32;
  const bool first = blockIdx.y == 1;
  const float* gy = first ? ga1 : gtemb;
  const float* x = first ? pe : h;
  const int K = first ? dim : td;
  float* gw = first ? gw1 : gw2;
  float* gb = first ? gb1 : gb2;
  const int n0 = blockIdx.x * TN;
  __shared__ float sgy[RC][TN];
  __shared__ float sx[RC * 256];
  const int kthreads = K;                            // threads along k (K <= 256, a power of two >= 16)
  const int nsl = 256 / kthreads;                    // n slices
  const int per = TN / nsl;                          // outputs per thread along n
  const int kk = threadIdx.x % kthreads, sl = threadIdx.x / kthreads;
  float acc[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) acc[i] = 0.f;
  float bsum = 0.f;
  for (int rb = 0; rb < B; rb += RC) {
    const int rows = B - rb < RC ? B - rb : RC;
    __syncthreads();
    {   // all of a chunk's loads first, then the LDS writes (a load -> store loop is one round trip per trip)
      float tg[RC * TN / 256], tx[RC];
#pragma unroll
      for (int q = 0; q < RC * TN / 256; ++q) {
        const int i = threadIdx.x + 256 * q, r = i / TN, j = i % TN;
        tg[q] = r < rows ? gy[(long)(rb + r) * td + n0 + j] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < RC; ++q) {
        const int i = threadIdx.x + 256 * q;          // rows are dense: one flat copy of rows * K floats
        tx[q] = i < rows * K ? x[(long)rb * K + i] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < RC * TN / 256; ++q) {
        const int i = threadIdx.x + 256 * q;
        sgy[i / TN][i % TN] = tg[q];
      }
#pragma unroll
      for (int q = 0; q < RC; ++q)
        if (threadIdx.x + 256 * q < RC * K) sx[threadIdx.x + 256 * q] = tx[q];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const float xv = sx[r * K + kk];
#pragma unroll
      for (int i = 0; i < TN; ++i)
        if (i < per) acc[i] = fmaf(sgy[r][sl * per + i], xv, acc[i]);
    }
    if (threadIdx.x < TN)
      for (int r = 0; r < rows; ++r) bsum += sgy[r][threadIdx.x];
  }
#pragma unroll
  for (int i = 0; i < TN; ++i)
    if (i < per) {
      float* d = gw + (long)(n0 + sl * per + i) * K + kk;
      *d = beta != 0.f ? beta * *d + acc[i] : acc[i];
    }
  if (threadIdx.x < TN) {
    float* d = gb + n0 + threadIdx.x;
    *d = beta != 0.f ? beta * *d + bsum : bsum;
  }
}
}  // namespace

extern "C" int lgm_extract_axpby(const float* ta, const float* tb, const float* td, const int64_t* t, const float* x,
                                 const float* y, float sb, int clip, float* out, int B, int64_t per_sample, int n_table,
                                 void* stream) {
  LGM_REQUIRE(t && x && out && B > 0 && B <= 65535 && per_sample > 0 && n_table > 0, "extract_axpby: bad arguments");
  LGM_REQUIRE(y || !tb, "extract_axpby: a second table without a second tensor");
  const int gx = (int)(per_sample < 256L * 4096 ? lgm_cdiv(per_sample, 256) : 4096);
  hipLaunchKernelGGL(extract_axpby_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, ta, tb, td, (const long*)t, x,
                     y, sb, clip, out, (long)per_sample, n_table);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
static bool tm_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static bool tm_dims_ok(int dim, int td) {
  // K / 4 lanes per weight row must be a power of two <= 64, or K a multiple of 256 up to 1024
  auto ok = [](int K) { return K >= 16 && K <= 256 && K % 4 == 0 && tm_pow2(K / 4); };   // K / 4 lanes share a weight row
  return ok(dim) && ok(td) && td % 32 == 0 && dim % 2 == 0 && (long)td * dim <= 16384;
}
extern "C" int64_t lgm_time_mlp_supported(int dim, int time_dim) { return tm_dims_ok(dim, time_dim) ? 1 : 0; }
extern "C" int lgm_time_mlp_fwd(const int64_t* t, int B, int dim, const float* freqs, const float* w1, const float* b1,
                                const float* w2, const float* b2, int time_dim, float* pe, float* a1, float* h,
                                float* temb, float* st, void* stream) {
  LGM_REQUIRE(t && freqs && w1 && b1 && w2 && b2 && pe && a1 && h && temb && st && B > 0, "time_mlp_fwd: bad arguments");
  LGM_REQUIRE(tm_dims_ok(dim, time_dim), "time_mlp_fwd: dim %d / time_dim %d not taken (lgm_time_mlp_supported)", dim, time_dim);
  LGM_REQUIRE(lgm_aligned16(w1) && lgm_aligned16(w2), "time_mlp_fwd: weights must be 16-byte aligned");
  const size_t sm = sizeof(float) * TM_RB * (size_t)(dim + 2 * time_dim);
  hipLaunchKernelGGL(time_mlp_fwd_kernel, dim3(lgm_cdiv(B, TM_RB)), dim3(TM_THREADS), sm, (hipStream_t)stream, (const long*)t, B,
                     dim, freqs, w1, b1, w2, b2, time_dim, pe, a1, h, temb, st);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
extern "C" int lgm_time_mlp_bwd(const float* gst, const float* pe, const float* a1, const float* h, const float* temb,
                                const float* w2, int B, int dim, int time_dim, float* gtemb, float* ga1, float* gw1,
                                float* gb1, float* gw2, float* gb2, float beta, void* stream) {
  LGM_REQUIRE(gst && pe && a1 && h && temb && w2 && gtemb && ga1 && gw1 && gb1 && gw2 && gb2 && B > 0,
              "time_mlp_bwd: bad arguments");
  LGM_REQUIRE(tm_dims_ok(dim, time_dim), "time_mlp_bwd: dim %d / time_dim %d not taken (lgm_time_mlp_supported)", dim, time_dim);
  hipLaunchKernelGGL(time_mlp_bwd_rows_kernel, dim3(lgm_cdiv(B, TM_RB)), dim3(TM_THREADS), sizeof(float) * TM_RB * time_dim * 5,
                     (hipStream_t)stream, gst, a1, temb, w2, B, time_dim, gtemb, ga1);
  hipLaunchKernelGGL(time_mlp_bwd_wgrad_kernel, dim3(time_dim / 16, 2), dim3(256), 0, (hipStream_t)stream, gtemb, h, ga1, pe,
                     B, dim, time_dim, gw2, gb2, gw1, gb1, beta);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
extern "C" int lgm_sampler_time(const int64_t* ttable, const int32_t* counter, int64_t* t, int B, void* stream) {
  LGM_REQUIRE(ttable && counter && t && B > 0, "sampler_time: bad arguments");
  hipLaunchKernelGGL(sampler_time_kernel, dim3(lgm_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long*)ttable, (const int*)counter, (long*)t, B);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_posemb(const int64_t* t, int B, int dim, const float* freqs, float* out, int64_t pitch,
                          void* stream) {
  LGM_REQUIRE(t && out && freqs && B > 0 && dim >= 4 && dim % 2 == 0 && pitch >= dim, "posemb: bad arguments");
  hipLaunchKernelGGL(posemb_kernel, dim3(lgm_cdiv((long)B * dim / 2, 256)), dim3(256), 0, (hipStream_t)stream, t, B,
                     dim, freqs, out, (long)pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

static int check_mat(const void* a, int64_t pitch, int64_t rows, int cols, const char* who) {
  LGM_REQUIRE(a && rows > 0 && cols > 0 && cols % 4 == 0 && pitch % 4 == 0 && pitch >= cols && lgm_aligned16(a),
              "%s: matrix must be non-null, 16B aligned, cols/pitch multiples of 4", who);
  return LGM_OK;
}

extern "C" int lgm_act_fwd(const float* x, int64_t x_pitch, const float* bias, const float* res, int64_t res_pitch,
                           float* y, int64_t y_pitch, int64_t rows, int cols, int act, float slope, void* stream) {
  if (int rc = check_mat(x, x_pitch, rows, cols, "act_fwd(x)")) return rc;
  if (int rc = check_mat(y, y_pitch, rows, cols, "act_fwd(y)")) return rc;
  if (res) if (int rc = check_mat(res, res_pitch, rows, cols, "act_fwd(res)")) return rc;
  hipLaunchKernelGGL(act_fwd_kernel, dim3(lgm_cdiv(rows * (cols / 4), 256)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)x_pitch, bias, res, (long)res_pitch, y, (long)y_pitch, (long)rows, cols, act, slope);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_act_bwd(const float* x, int64_t x_pitch, const float* bias, const float* gy, int64_t gy_pitch,
                           float* gx, int64_t gx_pitch, int accumulate, int64_t rows, int cols, int act, float slope,
                           void* stream) {
  if (int rc = check_mat(x, x_pitch, rows, cols, "act_bwd(x)")) return rc;
  if (int rc = check_mat(gy, gy_pitch, rows, cols, "act_bwd(gy)")) return rc;
  if (int rc = check_mat(gx, gx_pitch, rows, cols, "act_bwd(gx)")) return rc;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(lgm_cdiv(rows * (cols / 4), 256)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)x_pitch, bias, gy, (long)gy_pitch, gx, (long)gx_pitch, accumulate, (long)rows, cols, act, slope);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_axpby(const float* a, int64_t a_pitch, float alpha, const float* b, int64_t b_pitch, float beta,
                         float* y, int64_t y_pitch, int64_t rows, int cols, void* stream) {
  if (int rc = check_mat(a, a_pitch, rows, cols, "axpby(a)")) return rc;
  if (int rc = check_mat(y, y_pitch, rows, cols, "axpby(y)")) return rc;
  if (b) if (int rc = check_mat(b, b_pitch, rows, cols, "axpby(b)")) return rc;
  hipLaunchKernelGGL(axpby_kernel, dim3(lgm_cdiv(rows * (cols / 4), 256)), dim3(256), 0, (hipStream_t)stream, a,
                     (long)a_pitch, alpha, b, (long)b_pitch, beta, y, (long)y_pitch, (long)rows, cols);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_upsample2x_fwd(const float* x, int64_t x_pitch, float* y, int64_t y_pitch, int B, int H, int W,
                                  int C, void* stream) {
  if (int rc = check_mat(x, x_pitch, (long)B * H * W, C, "upsample2x_fwd(x)")) return rc;
  if (int rc = check_mat(y, y_pitch, (long)B * H * W * 4, C, "upsample2x_fwd(y)")) return rc;
  const long total = (long)B * 4 * H * W * (C / 4);
  hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3(lgm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)x_pitch, y, (long)y_pitch, B, H, W, C);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_upsample2x_bwd(const float* gy, int64_t gy_pitch, float* gx, int64_t gx_pitch, int B, int H, int W,
                                  int C, int accumulate, void* stream) {
  if (int rc = check_mat(gx, gx_pitch, (long)B * H * W, C, "upsample2x_bwd(gx)")) return rc;
  if (int rc = check_mat(gy, gy_pitch, (long)B * H * W * 4, C, "upsample2x_bwd(gy)")) return rc;
  const long total = (long)B * H * W * (C / 4);
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(lgm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, gy,
                     (long)gy_pitch, gx, (long)gx_pitch, B, H, W, C, accumulate);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_pixel_unshuffle(const float* src, int64_t src_pitch, float* dst, int64_t dst_pitch, int B,
                                   int Hlo, int Wlo, int C, int inverse, int accumulate, void* stream) {
  LGM_REQUIRE(src && dst && B > 0 && Hlo > 0 && Wlo > 0 && C > 0, "pixel_unshuffle: bad arguments");
  LGM_REQUIRE((inverse ? src_pitch : dst_pitch) % 4 == 0, "pixel_unshuffle: 4C-side pitch %% 4 != 0");
  const long total = (long)B * Hlo * Wlo * C;
  hipLaunchKernelGGL(unshuffle_kernel, dim3(lgm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (long)src_pitch, dst, (long)dst_pitch, B, Hlo, Wlo, C, inverse, accumulate);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_nchw_to_nhwc(const float* src, float* dst, int64_t dst_pitch, int B, int C, int HW, int Cpad,
                                void* stream) {
  LGM_REQUIRE(src && dst && B > 0 && C > 0 && HW > 0 && Cpad >= C && dst_pitch >= Cpad, "nchw_to_nhwc: bad arguments");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(lgm_cdiv((long)B * HW * Cpad, 256)), dim3(256), 0, (hipStream_t)stream,
                     src, dst, (long)dst_pitch, B, C, HW, Cpad);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_nhwc_to_nchw(const float* src, int64_t src_pitch, float* dst, int B, int C, int HW, void* stream) {
  LGM_REQUIRE(src && dst && B > 0 && C > 0 && HW > 0 && src_pitch >= C, "nhwc_to_nchw: bad arguments");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(lgm_cdiv((long)B * C * HW, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (long)src_pitch, dst, B, C, HW);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

namespace {
// x_hat = tanh(pre) and the per-sample reconstruction term mean_{chw} (x_hat - target)^2 in one pass (VQ-VAE decoder end,
// vqvae.py:85-88 + the recon loss :130): one block per sample, like mse_sample_kernel
__global__ __launch_bounds__(256) void tanh_mse_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ target,
                                                           long pitch, int C, int HW, int Cpad, float* __restrict__ xh,
                                                           float* __restrict__ per_sample) {
  __shared__ float sh[16];
  const int b = blockIdx.x;
  const long n = (long)HW * Cpad;
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = (int)(i % Cpad);
    const long pix = (long)b * HW + i / Cpad;
    const float t = tanhf(pre[pix * pitch + c]);
    xh[pix * pitch + c] = t;
    if (c < C) {
      const float d = t - target[pix * pitch + c];
      s += d * d;
    }
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) per_sample[b] = s / ((float)C * (float)HW);
}
// (one 16-byte load / store per pixel when Cpad == 4, as mse_sample4_kernel)
__global__ __launch_bounds__(256) void tanh_mse_fwd4_kernel(const float* __restrict__ pre, const float* __restrict__ target,
                                                            long pitch, int C, int HW, float* __restrict__ xh,
                                                            float* __restrict__ per_sample) {
  __shared__ float sh[16];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int p0 = 0; p0 < HW; p0 += 1024) {
    f32x4 o[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int px = p0 + threadIdx.x + 256 * u;
      const long off = ((long)b * HW + (px < HW ? px : HW - 1)) * pitch;
      o[u] = *reinterpret_cast<const f32x4*>(pre + off);
      g[u] = *reinterpret_cast<const f32x4*>(target + off);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int px = p0 + threadIdx.x + 256 * u;
      if (px < HW) {
        f32x4 tv;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          tv[c] = tanhf(o[u][c]);
          const float d = tv[c] - g[u][c];
          s += c < C ? d * d : 0.f;
        }
        *reinterpret_cast<f32x4*>(xh + ((long)b * HW + px) * pitch) = tv;
      }
    }
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) per_sample[b] = s / ((float)C * (float)HW);
}
// its backward, with the loss weights folded in: gpre = (gloss w_recon) 2 (x_hat - target) / (C HW B) (1 - x_hat^2);
// g2[0] = gloss w_recon, g2[1] = gloss w_vq for the quantiser's backward later in the stream
__global__ __launch_bounds__(256) void tanh_mse_bwd_kernel(const float* __restrict__ xh, const float* __restrict__ target,
                                                           long pitch, const float* __restrict__ gloss, float w_recon,
                                                           float w_vq, int B, int C, int HW, int Cpad,
                                                           float* __restrict__ gpre, float* __restrict__ g2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * HW * Cpad;
  const float gr = gloss[0] * w_recon;
  if (i == 0) {
    g2[0] = gr;
    g2[1] = gloss[0] * w_vq;
  }
  if (i >= total) return;
  const int c = (int)(i % Cpad);
  const long pix = i / Cpad;
  float g = 0.f;
  if (c < C) {
    const float t = xh[pix * pitch + c];
    const float scale = gr * 2.f * 1.f / ((float)C * (float)HW * (float)B);
    g = scale * (t - target[pix * pitch + c]);
    g = g * (1.f - t * t);
  }
  gpre[pix * pitch + c] = g;
}

// ---------------------------------------------------------------------------------------
// Timestep samplers of the diffusion training step (lgm_tsampler_draw / lgm_tsampler_update, include/lgm_hip.h)
// ---------------------------------------------------------------------------------------
// mode 0: stratified from ONE uniform (a division, then an add: numpy float32 restates it bit for bit); mode 1: the first
// index with cdf[t] > u_b.  cdf[T - 1] = 1 > u, so the search ends inside the table for every u < 1; any other u (1, NaN) ends
// at T - 1 as well, because hi never leaves it.
__global__ __launch_bounds__(256) void tsampler_draw_kernel(const float* __restrict__ u, const float* __restrict__ cdf, int T,
                                                            int mode, long* __restrict__ t_out, int B) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long ti;
  if (mode == 0) {
    float ub = u[0] + (float)b / (float)B;
    if (ub >= 1.f) ub = ub - 1.f;
    const float f = floorf((float)T * ub);
    ti = f >= 0.f ? (f < (float)T ? (long)f : (long)T - 1) : 0;      // (a NaN draw: 0)
  } else {
    const float ub = u[b];
    int lo = 0, hi = T - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] > ub) hi = mid;
      else lo = mid + 1;
    }
    ti = lo;
  }
  t_out[b] = ti > (long)T - 1 ? (long)T - 1 : ti;
}

// The loss-second-moment sampler's state update and plan, ONE workgroup.  A thread owns the timesteps t with t mod TS_THREADS ==
// threadIdx.x: it alone writes their history rows, counts, iw and (first pass) cdf entries, so a batch that repeats a timestep
// lands in batch order without atomics.  Row update, c entries held, m new ones: the last H of (row[0..c) ++ new) - shift the
// survivors of the row down by drop = max(0, c + m - H) (ascending, in place), then the k-th new value goes to c - drop + k
// where that is not negative.  The prefix sum is two-level and sequential at both levels: thread j sums segment j of `seg_len`
// entries in order, thread 0 sums the segment totals in order, cdf[i] = offset[segment] + local[i].  Rounding is monotone and
// the next segment's offset is computed exactly as the last entry of this one, so cdf never decreases.
constexpr int TS_THREADS = 1024;
__global__ __launch_bounds__(TS_THREADS) void tsampler_update_kernel(const long* __restrict__ t, const float* __restrict__ per,
                                                                     int n_terms, float vb_weight, float* __restrict__ history,
                                                                     int* __restrict__ counts, int H, float q, int T, int B,
                                                                     float* cdf, float* __restrict__ iw, int seg_len) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) int st_t[TS_THREADS];
  __shared__ float st_l[TS_THREADS];
  __shared__ float seg[TS_THREADS];
  __shared__ float sh[16];
  __shared__ int shi[16];
  const int tid = threadIdx.x;
  // ---- phase one: the batch into the rows ----
  for (int b0 = 0; b0 < B; b0 += TS_THREADS) {
    const int nb = B - b0 < TS_THREADS ? B - b0 : TS_THREADS;
    __syncthreads();                                   // the previous chunk has been read by everyone
    const int nb4 = (nb + 3) & ~3;                     // the scans read four staged timesteps per LDS load: -1 fills the tail
    if (tid < nb) {
      const int b = b0 + tid;
      float L = per[b];
      if (n_terms == 2) L = L + vb_weight * per[B + b];
      const long ti = t[b];
      st_t[tid] = (ti >= 0 && ti < T && isfinite(L)) ? (int)ti : -1;
      st_l[tid] = L;
    } else if (tid < nb4) {
      st_t[tid] = -1;
    }
    __syncthreads();
    for (int row = tid; row < T; row += TS_THREADS) {
      int m = 0;
      for (int i = 0; i < nb4; i += 4) {
        const int4 s4 = *reinterpret_cast<const int4*>(st_t + i);
        m += (s4.x == row ? 1 : 0) + (s4.y == row ? 1 : 0) + (s4.z == row ? 1 : 0) + (s4.w == row ? 1 : 0);
      }
      if (m == 0) continue;
      float* hr = history + (long)row * H;
      int c = counts[row];
      c = c < 0 ? 0 : (c > H ? H : c);
      const int drop = c + m > H ? c + m - H : 0;
      // eight loads, then their eight stores: every load of a round reads an index no earlier round and no store of this
      // round in front of it has written (drop >= 1 here), and the loads of a round are in flight together
      for (int j = 0; j + drop < c; j += 8) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = j + e + drop < c ? hr[j + e + drop] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (j + e + drop < c) hr[j + e] = v[e];
      }
      int k = c - drop;
      for (int i = 0; i < nb4; i += 4) {
        const int4 s4 = *reinterpret_cast<const int4*>(st_t + i);
        const int tt[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (tt[e] != row) continue;
          if (k >= 0) hr[k] = st_l[i + e];
          ++k;
        }
      }
      counts[row] = c + m > H ? H : c + m;
    }
  }
  // ---- phase two: the plan from the updated rows (every thread reads only what it wrote itself) ----
  int cmin = H;
  float wsum = 0.f;
  for (int row = tid; row < T; row += TS_THREADS) {
    const int c = counts[row];
    cmin = c < cmin ? c : cmin;
    const float* hr = history + (long)row * H;
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += hr[h] * hr[h];
    const float w = sqrtf(s / (float)H);
    cdf[row] = w;
    wsum += w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(cmin, off, 64);
    cmin = o < cmin ? o : cmin;
  }
  if ((tid & 63) == 0) shi[tid >> 6] = cmin;
  const float W = lgm_block_sum(wsum, sh);               // (its barriers also publish shi)
  for (int i = 0; i < TS_THREADS / 64; ++i) cmin = shi[i] < cmin ? shi[i] : cmin;
  const bool weighted = cmin >= H && W > 0.f && isfinite(W);
  const float uniform = 1.f / (float)T;
  for (int row = tid; row < T; row += TS_THREADS) {
    float p = uniform, w = 1.f;
    if (weighted) {
      p = (1.f - q) * cdf[row] / W + q / (float)T;
      w = 1.f / ((float)T * p);
    }
    cdf[row] = p;
    iw[row] = w;
  }
  __syncthreads();
  const int nseg = (T + seg_len - 1) / seg_len;          // <= TS_THREADS (the launcher's seg_len)
  if (tid < nseg) {
    const int lo = tid * seg_len, hi = lo + seg_len < T ? lo + seg_len : T;
    float run = 0.f;
    for (int i0 = lo; i0 < hi; i0 += 8) {                // (loads of a round in front of its stores, as above; the sum stays in order)
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = i0 + e < hi ? cdf[i0 + e] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (i0 + e < hi) {
          run += v[e];
          cdf[i0 + e] = run;
        }
      }
    }
    seg[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    float off = 0.f;
    for (int j = 0; j < nseg; ++j) {
      const float total = seg[j];
      seg[j] = off;
      off += total;
    }
  }
  __syncthreads();
  for (int row = tid; row < T; row += TS_THREADS) {
    const float v = seg[row / seg_len] + cdf[row];
    cdf[row] = row == T - 1 ? 1.f : fminf(v, 1.f);
  }
}
}  // namespace

extern "C" int lgm_tanh_mse_fwd(const float* pre, const float* target, int64_t pitch, int B, int C, int HW, int Cpad,
                                float* xh, float* per_sample, void* stream) {
  LGM_REQUIRE(pre && target && xh && per_sample && B > 0, "tanh_mse_fwd: bad arguments");
  if (Cpad == 4 && pitch % 4 == 0 && lgm_aligned16(pre) && lgm_aligned16(target) && lgm_aligned16(xh))
    hipLaunchKernelGGL(tanh_mse_fwd4_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pre, target, (long)pitch, C, HW, xh,
                       per_sample);
  else
    hipLaunchKernelGGL(tanh_mse_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pre, target, (long)pitch, C, HW, Cpad,
                       xh, per_sample);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_tanh_mse_bwd(const float* xh, const float* target, int64_t pitch, const float* gloss, float w_recon,
                                float w_vq, int B, int C, int HW, int Cpad, float* gpre, float* g2, void* stream) {
  LGM_REQUIRE(xh && target && gloss && gpre && g2 && B > 0, "tanh_mse_bwd: bad arguments");
  hipLaunchKernelGGL(tanh_mse_bwd_kernel, dim3(lgm_cdiv((long)B * HW * Cpad, 256)), dim3(256), 0, (hipStream_t)stream, xh,
                     target, (long)pitch, gloss, w_recon, w_vq, B, C, HW, Cpad, gpre, g2);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_weighted_mse_fwd(const float* out, const float* target, int64_t pitch, const int64_t* t,
                                    const float* loss_weight, int B, int C, int HW, int Cpad, float* per_sample,
                                    float* loss, void* stream) {
  LGM_REQUIRE(out && target && per_sample && B > 0 && (!loss_weight || t), "weighted_mse_fwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (Cpad == 4 && pitch % 4 == 0 && lgm_aligned16(out) && lgm_aligned16(target))
    hipLaunchKernelGGL(mse_sample4_kernel, dim3(B), dim3(256), 0, s, out, target, (long)pitch, t, loss_weight, C, HW, per_sample);
  else
    hipLaunchKernelGGL(mse_sample_kernel, dim3(B), dim3(256), 0, s, out, target, (long)pitch, t, loss_weight, C, HW, Cpad,
                       per_sample);
  if (loss) hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, (const float*)per_sample, B, loss);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

// (wb: the per-sample weights a forward under a timestep sampler's plan left, or nullptr; so in hybrid_bwd_launch)
static void mse_bwd_launch(const float* out, const float* target, int64_t pitch, const int64_t* t, const float* loss_weight,
                           const float* wb, const float* gloss, int B, int C, int HW, int Cpad, float* gout, void* stream) {
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(lgm_cdiv((long)B * HW * Cpad, 256)), dim3(256), 0, (hipStream_t)stream, out,
                     target, (long)pitch, t, loss_weight, gloss, B, C, HW, Cpad, gout, wb);
}
extern "C" int lgm_weighted_mse_bwd(const float* out, const float* target, int64_t pitch, const int64_t* t,
                                    const float* loss_weight, const float* gloss, int B, int C, int HW, int Cpad,
                                    float* gout, void* stream) {
  LGM_REQUIRE(out && target && gloss && gout && B > 0 && (!loss_weight || t), "weighted_mse_bwd: bad arguments");
  mse_bwd_launch(out, target, pitch, t, loss_weight, nullptr, gloss, B, C, HW, Cpad, gout, stream);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

// The weighted MSE under a timestep sampler's plan (include/lgm_hip.h, "Timestep samplers"): the plain per-sample launch, then
// iw_mean_kernel in place of mean_kernel; the backward is the plain launch with the per-sample weights wb the forward left.
static int iw_mean_launch(const float* per, int n_terms, float vb_weight, const int64_t* t, const float* iw, int n_table, int B,
                          float* wb, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(iw_mean_kernel, dim3(1), dim3(256), 0, s, per, n_terms, vb_weight, (const long*)t, iw, n_table, B, wb, loss);
  return LGM_OK;
}
extern "C" int lgm_weighted_mse_fwd_iw(const float* out, const float* target, int64_t pitch, const int64_t* t,
                                       const float* loss_weight, const float* iw, int n_table, int B, int C, int HW, int Cpad,
                                       float* per_sample, float* wb, float* loss, void* stream) {
  LGM_REQUIRE(t && iw && wb && loss && n_table > 0, "weighted_mse_fwd_iw: bad arguments");
  const int rc = lgm_weighted_mse_fwd(out, target, pitch, t, loss_weight, B, C, HW, Cpad, per_sample, nullptr, stream);
  if (rc != LGM_OK) return rc;
  lgm_note_kernel("iw_mean_kernel");
  iw_mean_launch(per_sample, 1, 0.f, t, iw, n_table, B, wb, loss, (hipStream_t)stream);
  LGM_LAUNCH_CHECK_AS("weighted_mse_fwd_iw");
  return LGM_OK;
}
extern "C" int lgm_weighted_mse_bwd_iw(const float* out, const float* target, int64_t pitch, const int64_t* t,
                                       const float* loss_weight, const float* wb, const float* gloss, int B, int C, int HW,
                                       int Cpad, float* gout, void* stream) {
  LGM_REQUIRE(out && target && gloss && gout && wb && B > 0 && (!loss_weight || t), "weighted_mse_bwd_iw: bad arguments");
  mse_bwd_launch(out, target, pitch, t, loss_weight, wb, gloss, B, C, HW, Cpad, gout, stream);
  LGM_LAUNCH_CHECK_AS("weighted_mse_bwd_iw");
  return LGM_OK;
}

// ---------------------------------------------------------------------------------------
// Diffusion elementwise entry points: one launcher per op.  The *_slice forms take the network's input buffer as it is
// (pitch, x slice, optional self-conditioning slice); the plain and *_obj forms are the same launch on a buffer of one
// slice (x_off = 0, sc_off = -1, Cpad lanes), the plain ones at objective 2 (pred_v) without offset noise.
// ---------------------------------------------------------------------------------------
static bool objective_ok(int objective) { return objective >= 0 && objective <= 2; }
// The two slices lie inside the pitch and do not overlap; sc_off < 0 = no self-conditioning slice.
static bool slices_ok(int64_t pitch, int x_off, int sc_off, int C) {
  if (C <= 0 || x_off < 0 || x_off + C > pitch) return false;
  if (sc_off < 0) return true;
  return sc_off + C <= pitch && (sc_off + C <= x_off || x_off + C <= sc_off);
}

// Hybrid loss of a learned-variance network (hybrid_loss_*_kernel): out [B, HW, pitch] with 2 C lanes, target [B, HW,
// target_pitch], img NCHW (normalised here when `normalize`), x_t in the x slice of xin, tab [T][8] (ddpm.py learned_table),
// per [2][B] = (lw mse_b, vb_b), loss [1] (optional) = mean_b(per[0]) + vb_weight mean_b(per[1]).
static bool hybrid_ok(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                      const float* xin, int64_t x_pitch, int x_off, const int64_t* t, const HybridTables& T, int B, int C, int HW,
                      int objective) {
  if (!out || !target || !img || !xin || !t || !T.sa || !T.s1 || !T.r || !T.rm1 || !T.tab || T.n_table <= 0) return false;
  return B > 0 && C > 0 && HW > 0 && pitch >= 2 * (int64_t)C && target_pitch >= C && slices_ok(x_pitch, x_off, -1, C) &&
         objective_ok(objective) && (int64_t)B * HW * pitch < ((int64_t)1 << 40);
}
extern "C" int lgm_hybrid_loss_fwd(const float* out, int64_t pitch, const float* target, int64_t target_pitch,
                                   const float* img, int normalize, const float* xin, int64_t x_pitch, int x_off,
                                   const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip,
                                   const float* sqrt_recipm1, const float* loss_weight, const float* tab, int n_table,
                                   int objective, float vb_weight, int B, int C, int HW, float* per, float* loss,
                                   void* stream) {
  const HybridTables T = {sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, loss_weight, tab, n_table};
  LGM_REQUIRE(per && hybrid_ok(out, pitch, target, target_pitch, img, xin, x_pitch, x_off, t, T, B, C, HW, objective),
              "hybrid_loss_fwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  lgm_note_kernel("hybrid_loss_fwd_kernel");
  hipLaunchKernelGGL(hybrid_loss_fwd_kernel, dim3(B), dim3(256), 0, s, out, (long)pitch, target, (long)target_pitch, img,
                     normalize, xin, (long)x_pitch, x_off, (const long*)t, T, objective, C, HW, per, B);
  if (loss) hipLaunchKernelGGL(hybrid_mean_kernel, dim3(1), dim3(256), 0, s, (const float*)per, B, vb_weight, loss);
  LGM_LAUNCH_CHECK_AS("hybrid_loss_fwd");
  return LGM_OK;
}
static void hybrid_bwd_launch(const float* out, int64_t pitch, const float* target, int64_t target_pitch, const float* img,
                              int normalize, const float* xin, int64_t x_pitch, int x_off, const int64_t* t,
                              const HybridTables& T, int objective, float vb_weight, const float* wb, const float* gloss, int B,
                              int C, int HW, float* gout, void* stream) {
  lgm_note_kernel("hybrid_loss_bwd_kernel");
  hipLaunchKernelGGL(hybrid_loss_bwd_kernel, dim3(lgm_cdiv((long)B * HW * pitch, 256)), dim3(256), 0, (hipStream_t)stream, out,
                     (long)pitch, target, (long)target_pitch, img, normalize, xin, (long)x_pitch, x_off, (const long*)t, T,
                     objective, gloss, vb_weight, B, C, HW, gout, wb);
}
extern "C" int lgm_hybrid_loss_bwd(const float* out, int64_t pitch, const float* target, int64_t target_pitch,
                                   const float* img, int normalize, const float* xin, int64_t x_pitch, int x_off,
                                   const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip,
                                   const float* sqrt_recipm1, const float* loss_weight, const float* tab, int n_table,
                                   int objective, float vb_weight, const float* gloss, int B, int C, int HW, float* gout,
                                   void* stream) {
  const HybridTables T = {sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, loss_weight, tab, n_table};
  LGM_REQUIRE(gloss && gout && gout != out &&
                  hybrid_ok(out, pitch, target, target_pitch, img, xin, x_pitch, x_off, t, T, B, C, HW, objective),
              "hybrid_loss_bwd: bad arguments");
  hybrid_bwd_launch(out, pitch, target, target_pitch, img, normalize, xin, x_pitch, x_off, t, T, objective, vb_weight, nullptr,
                    gloss, B, C, HW, gout, stream);
  LGM_LAUNCH_CHECK_AS("hybrid_loss_bwd");
  return LGM_OK;
}
// The hybrid loss under a timestep sampler's plan: as lgm_weighted_mse_fwd_iw / _bwd_iw.
extern "C" int lgm_hybrid_loss_fwd_iw(const float* out, int64_t pitch, const float* target, int64_t target_pitch,
                                      const float* img, int normalize, const float* xin, int64_t x_pitch, int x_off,
                                      const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip,
                                      const float* sqrt_recipm1, const float* loss_weight, const float* tab, int n_table,
                                      int objective, float vb_weight, const float* iw, int B, int C, int HW, float* per,
                                      float* wb, float* loss, void* stream) {
  LGM_REQUIRE(iw && wb && loss, "hybrid_loss_fwd_iw: bad arguments");
  const int rc = lgm_hybrid_loss_fwd(out, pitch, target, target_pitch, img, normalize, xin, x_pitch, x_off, t, sqrt_ac, sqrt_1mac,
                                     sqrt_recip, sqrt_recipm1, loss_weight, tab, n_table, objective, vb_weight, B, C, HW, per,
                                     nullptr, stream);
  if (rc != LGM_OK) return rc;
  iw_mean_launch(per, 2, vb_weight, t, iw, n_table, B, wb, loss, (hipStream_t)stream);
  LGM_LAUNCH_CHECK_AS("hybrid_loss_fwd_iw");
  return LGM_OK;
}
extern "C" int lgm_hybrid_loss_bwd_iw(const float* out, int64_t pitch, const float* target, int64_t target_pitch,
                                      const float* img, int normalize, const float* xin, int64_t x_pitch, int x_off,
                                      const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* sqrt_recip,
                                      const float* sqrt_recipm1, const float* loss_weight, const float* tab, int n_table,
                                      int objective, float vb_weight, const float* wb, const float* gloss, int B, int C, int HW,
                                      float* gout, void* stream) {
  const HybridTables T = {sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, loss_weight, tab, n_table};
  LGM_REQUIRE(gloss && gout && gout != out && wb &&
                  hybrid_ok(out, pitch, target, target_pitch, img, xin, x_pitch, x_off, t, T, B, C, HW, objective),
              "hybrid_loss_bwd_iw: bad arguments");
  hybrid_bwd_launch(out, pitch, target, target_pitch, img, normalize, xin, x_pitch, x_off, t, T, objective, vb_weight, wb, gloss,
                    B, C, HW, gout, stream);
  LGM_LAUNCH_CHECK_AS("hybrid_loss_bwd_iw");
  return LGM_OK;
}

// Timestep samplers.  The names are noted without a registry entry (no LGM_KNAME), like dpm_step_kernel below: the ledger test
// lists every registry name with the test file that asserts it; tests/test_hip_tsampler.py asserts these two.
extern "C" int lgm_tsampler_draw(const float* u, const float* cdf, int T, int mode, int64_t* t_out, int B, void* stream) {
  LGM_REQUIRE(u && t_out && T > 0 && B > 0 && (mode == 0 || (mode == 1 && cdf)), "tsampler_draw: bad arguments");
  lgm_note_kernel("tsampler_draw_kernel");
  hipLaunchKernelGGL(tsampler_draw_kernel, dim3(lgm_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, u, cdf, T, mode,
                     (long*)t_out, B);
  LGM_LAUNCH_CHECK_AS("tsampler_draw");
  return LGM_OK;
}
extern "C" int lgm_tsampler_update(const int64_t* t, const float* per, int n_terms, float vb_weight, float* history,
                                   int32_t* counts, int H, float q, int T, int B, float* cdf, float* iw, void* stream) {
  LGM_REQUIRE(history && counts && cdf && iw && H >= 1 && T >= 1 && T <= (1 << 20) && B >= 0 && (B == 0 || (t && per)) &&
                  (n_terms == 1 || n_terms == 2) && q >= 0.f && q <= 1.f,
              "tsampler_update: bad arguments");
  LGM_REQUIRE(cdf != iw && cdf != history && (const void*)cdf != (const void*)counts && cdf != per,
              "tsampler_update: cdf must not alias another operand");
  // segments of the two-level prefix sum: about sqrt(T) long, and no more of them than the workgroup has threads
  int seg_len = 1;
  while ((long)seg_len * seg_len < T) ++seg_len;
  if (seg_len < lgm_cdiv(T, TS_THREADS)) seg_len = lgm_cdiv(T, TS_THREADS);
  lgm_note_kernel("tsampler_update_kernel");
  hipLaunchKernelGGL(tsampler_update_kernel, dim3(1), dim3(TS_THREADS), 0, (hipStream_t)stream, (const long*)t, per, n_terms,
                     vb_weight, history, (int*)counts, H, q, T, B, cdf, iw, seg_len);
  LGM_LAUNCH_CHECK_AS("tsampler_update");
  return LGM_OK;
}

static int qsample_slice_launch(const float* img, const float* noise, const float* offset, float strength, const int64_t* t,
                                const float* sqrt_ac, const float* sqrt_1mac, int normalize, int objective, float* xin,
                                int64_t pitch, int lanes, int x_off, int sc_off, float* target, int64_t target_pitch,
                                int B, int C, int HW, int Cpad, void* stream) {
  lgm_note_kernel(LGM_KNAME("qsample_slice_kernel"));
  hipLaunchKernelGGL(qsample_slice_kernel, dim3(lgm_cdiv((long)B * HW * lanes, 256)), dim3(256), 0, (hipStream_t)stream, img,
                     noise, offset, strength, t, sqrt_ac, sqrt_1mac, normalize, objective, xin, (long)pitch, lanes, x_off,
                     sc_off, target, (long)target_pitch, Cpad, B, C, HW);
  LGM_LAUNCH_CHECK_AS("qsample_target_slice");
  return LGM_OK;
}

extern "C" int lgm_qsample_target(const float* img, const float* noise, const int64_t* t, const float* sqrt_ac,
                                  const float* sqrt_1mac, int normalize, float* xt, float* target, int64_t pitch,
                                  int B, int C, int HW, int Cpad, void* stream) {
  LGM_REQUIRE(img && noise && t && sqrt_ac && sqrt_1mac && xt && B > 0 && C > 0 && HW > 0 && Cpad >= C && pitch >= Cpad,
              "qsample_target: bad arguments");
  return qsample_slice_launch(img, noise, nullptr, 0.f, t, sqrt_ac, sqrt_1mac, normalize, 2, xt, pitch, Cpad, 0, -1, target,
                              pitch, B, C, HW, Cpad, stream);
}

extern "C" int lgm_qsample_target_obj(const float* img, const float* noise, const float* offset, float strength,
                                      const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int normalize,
                                      int objective, float* xt, float* target, int64_t pitch, int B, int C, int HW,
                                      int Cpad, void* stream) {
  LGM_REQUIRE(img && noise && t && sqrt_ac && sqrt_1mac && xt && B > 0 && C > 0 && HW > 0 && Cpad >= C && pitch >= Cpad &&
                  objective_ok(objective),
              "qsample_target_obj: bad arguments");
  return qsample_slice_launch(img, noise, offset, strength, t, sqrt_ac, sqrt_1mac, normalize, objective, xt, pitch, Cpad, 0,
                              -1, target, pitch, B, C, HW, Cpad, stream);
}

extern "C" int lgm_qsample_target_slice(const float* img, const float* noise, const float* offset, float strength,
                                        const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int normalize,
                                        int objective, float* xin, int64_t pitch, int x_off, int sc_off, float* target,
                                        int64_t target_pitch, int B, int C, int HW, int Cpad, void* stream) {
  LGM_REQUIRE(img && noise && t && sqrt_ac && sqrt_1mac && xin && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) &&
                  Cpad >= C && Cpad <= pitch && target_pitch >= Cpad && objective_ok(objective),
              "qsample_target_slice: bad arguments");
  return qsample_slice_launch(img, noise, offset, strength, t, sqrt_ac, sqrt_1mac, normalize, objective, xin, pitch,
                              (int)pitch, x_off, sc_off, target, target_pitch, B, C, HW, Cpad, stream);
}

static int model_predictions_launch(const float* x, const float* out, const int64_t* t, const float* sqrt_ac,
                                    const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                                    int objective, int clip, int rederive, float* pred_noise, float* x_start, int B,
                                    int64_t per_sample, int n_table, void* stream, const float* thresh = nullptr) {
  const int gx = (int)(per_sample < 256L * 4096 ? lgm_cdiv(per_sample, 256) : 4096);
  hipLaunchKernelGGL(model_predictions_obj_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, out, (const long*)t,
                     sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, objective, clip, rederive, pred_noise, x_start,
                     (long)per_sample, n_table, thresh);
  LGM_LAUNCH_CHECK_AS("model_predictions_obj");
  return LGM_OK;
}

extern "C" int lgm_model_predictions(const float* x, const float* v, const int64_t* t, const float* sqrt_ac,
                                     const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1, int clip,
                                     float* pred_noise, float* x_start, int B, int64_t per_sample, int n_table,
                                     void* stream) {
  LGM_REQUIRE(x && v && t && sqrt_ac && sqrt_1mac && sqrt_recip && sqrt_recipm1 && pred_noise && x_start && B > 0 &&
                  B <= 65535 && per_sample > 0 && n_table > 0,
              "model_predictions: bad arguments");
  return model_predictions_launch(x, v, t, sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, 2, clip, 0, pred_noise, x_start, B,
                                  per_sample, n_table, stream);
}

extern "C" int lgm_model_predictions_obj(const float* x, const float* out, const int64_t* t, const float* sqrt_ac,
                                         const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                                         int objective, int clip, int rederive, float* pred_noise, float* x_start, int B,
                                         int64_t per_sample, int n_table, void* stream) {
  LGM_REQUIRE(x && out && t && sqrt_ac && sqrt_1mac && sqrt_recip && sqrt_recipm1 && pred_noise && x_start && B > 0 &&
                  B <= 65535 && per_sample > 0 && n_table > 0 && objective_ok(objective),
              "model_predictions_obj: bad arguments");
  return model_predictions_launch(x, out, t, sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, objective, clip, rederive,
                                  pred_noise, x_start, B, per_sample, n_table, stream);
}

extern "C" int lgm_model_predictions_thresh(const float* x, const float* out, const int64_t* t, const float* sqrt_ac,
                                            const float* sqrt_1mac, const float* sqrt_recip, const float* sqrt_recipm1,
                                            int objective, int rederive, float* pred_noise, float* x_start, int B,
                                            int64_t per_sample, int n_table, const float* thresh, void* stream) {
  LGM_REQUIRE(x && out && t && sqrt_ac && sqrt_1mac && sqrt_recip && sqrt_recipm1 && pred_noise && x_start && thresh &&
                  B > 0 && B <= 65535 && per_sample > 0 && n_table > 0 && objective_ok(objective),
              "model_predictions_thresh: bad arguments");
  return model_predictions_launch(x, out, t, sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, objective, 1, rederive,
                                  pred_noise, x_start, B, per_sample, n_table, stream, thresh);
}

extern "C" int lgm_selfcond_estimate(float* xin, int64_t pitch, int x_off, int sc_off, const float* out, int64_t out_pitch,
                                     const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                                     const float* sqrt_recip, const float* sqrt_recipm1, int objective, int B, int C, int HW,
                                     int n_table, void* stream) {
  LGM_REQUIRE(xin && out && t && sqrt_ac && sqrt_1mac && sqrt_recip && sqrt_recipm1 && B > 0 && HW > 0 && n_table > 0 &&
                  sc_off >= 0 && slices_ok(pitch, x_off, sc_off, C) && out_pitch >= C && objective_ok(objective),
              "selfcond_estimate: bad arguments");
  lgm_note_kernel(LGM_KNAME("selfcond_estimate_kernel"));
  hipLaunchKernelGGL(selfcond_estimate_kernel, dim3(lgm_cdiv((long)B * HW * C, 256)), dim3(256), 0, (hipStream_t)stream, xin,
                     (long)pitch, x_off, sc_off, out, (long)out_pitch, (const long*)t, sqrt_ac, sqrt_1mac, sqrt_recip,
                     sqrt_recipm1, objective, B, C, HW, n_table);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

// x0_out (optional, pitch x0_pitch >= pitch): only the one-slice forms hand one in.  table != null: row `counter` of it, and
// `advance` appends the counter's increment.
static int sample_step_slice_launch(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                    int64_t v_pitch, const float* noise, float* x0_out, int64_t x0_pitch, int B, int C,
                                    int HW, const SampleRow& row, const float* table, const int32_t* counter, int objective,
                                    int clip, int rederive, int advance, void* stream, const float* thresh = nullptr,
                                    const InpaintOps& ip = InpaintOps{}, int learned = 0, int lanes = 0) {
  lgm_note_kernel(LGM_KNAME("sample_step_slice_kernel"));
  if (lanes == 0) lanes = (int)pitch;                // the whole pitch; the *_extent entry points own fewer lanes
  hipLaunchKernelGGL(sample_step_slice_kernel, dim3(lgm_cdiv((long)B * HW * lanes, 256)), dim3(256), 0, (hipStream_t)stream,
                     xin, xout, (long)pitch, lanes, x_off, sc_off, v, (long)v_pitch, noise, B, C, HW, row, table,
                     (const int*)counter, objective, clip, rederive, x0_out, (long)x0_pitch, thresh, ip, learned);
  if (advance) hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)counter);
  LGM_LAUNCH_CHECK_AS("sample_step_slice");
  return LGM_OK;
}

extern "C" int lgm_sample_step(const float* x, const float* v, const float* noise, float* out, float* x0_out, int B,
                               int C, int HW, int Cpad, float A, float Bv, int clip, float R, float Rm1, float C0,
                               float C1, float C2, float C3, void* stream) {
  LGM_REQUIRE(x && v && out && B > 0 && C > 0 && HW > 0 && Cpad >= C, "sample_step: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  return sample_step_slice_launch(x, out, Cpad, 0, -1, v, Cpad, noise, x0_out, Cpad, B, C, HW, row, nullptr, nullptr, 2, clip,
                                  0, 0, stream);
}

extern "C" int lgm_sample_step_obj(const float* x, const float* v, const float* noise, float* out, float* x0_out, int B,
                                   int C, int HW, int Cpad, int objective, float A, float Bv, int clip, int rederive,
                                   float R, float Rm1, float C0, float C1, float C2, float C3, void* stream) {
  LGM_REQUIRE(x && v && out && B > 0 && C > 0 && HW > 0 && Cpad >= C && objective_ok(objective),
              "sample_step_obj: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  return sample_step_slice_launch(x, out, Cpad, 0, -1, v, Cpad, noise, x0_out, Cpad, B, C, HW, row, nullptr, nullptr,
                                  objective, clip, rederive, 0, stream);
}

extern "C" int lgm_sample_step_slice(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                     int64_t v_pitch, const float* noise, int B, int C, int HW, int objective, float A,
                                     float Bv, int clip, int rederive, float R, float Rm1, float C0, float C1, float C2,
                                     float C3, void* stream) {
  LGM_REQUIRE(xin && xout && v && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) && v_pitch >= C &&
                  objective_ok(objective),
              "sample_step_slice: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  return sample_step_slice_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, nullptr, 0, B, C, HW, row, nullptr,
                                  nullptr, objective, clip, rederive, 0, stream);
}

extern "C" int lgm_sample_step_table(float* x, const float* v, const float* noise, float* x0_out, int B, int C, int HW,
                                     int Cpad, const float* table, const int32_t* counter, int clip, int advance,
                                     void* stream) {
  LGM_REQUIRE(x && v && table && counter && B > 0 && C > 0 && HW > 0 && Cpad >= C, "sample_step_table: bad arguments");
  return sample_step_slice_launch(x, x, Cpad, 0, -1, v, Cpad, noise, x0_out, Cpad, B, C, HW, SampleRow{}, table, counter, 2,
                                  clip, 0, advance, stream);
}

extern "C" int lgm_sample_step_table_obj(float* x, const float* v, const float* noise, float* x0_out, int B, int C, int HW,
                                         int Cpad, const float* table, const int32_t* counter, int objective, int clip,
                                         int rederive, int advance, void* stream) {
  LGM_REQUIRE(x && v && table && counter && B > 0 && C > 0 && HW > 0 && Cpad >= C && objective_ok(objective),
              "sample_step_table_obj: bad arguments");
  return sample_step_slice_launch(x, x, Cpad, 0, -1, v, Cpad, noise, x0_out, Cpad, B, C, HW, SampleRow{}, table, counter,
                                  objective, clip, rederive, advance, stream);
}

extern "C" int lgm_sample_step_table_slice(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                                           const float* noise, int B, int C, int HW, const float* table,
                                           const int32_t* counter, int objective, int clip, int rederive, int advance,
                                           void* stream) {
  LGM_REQUIRE(x && v && table && counter && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) && v_pitch >= C &&
                  objective_ok(objective),
              "sample_step_table_slice: bad arguments");
  return sample_step_slice_launch(x, x, pitch, x_off, sc_off, v, v_pitch, noise, nullptr, 0, B, C, HW, SampleRow{}, table,
                                  counter, objective, clip, rederive, advance, stream);
}

// The ancestral step of a learned-variance network: v carries 2 C lanes, the row is (A, Bv, R, Rm1, P1, P2, log beta_t,
// log beta~_t) with log beta~_t = -inf on the step without noise; the same launch as every other update.
extern "C" int lgm_sample_step_learned(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                       int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW,
                                       int objective, float A, float Bv, float R, float Rm1, float P1, float P2,
                                       float log_beta, float log_tilde, void* stream) {
  LGM_REQUIRE(xin && xout && v && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) && v_pitch >= 2 * (int64_t)C &&
                  objective_ok(objective) && x0_out != xin && x0_out != xout,
              "sample_step_learned: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, P1, P2, log_beta, log_tilde}};
  return sample_step_slice_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, x0_out, pitch, B, C, HW, row, nullptr,
                                  nullptr, objective, 1, 0, 0, stream, nullptr, InpaintOps{}, 1);
}

extern "C" int lgm_sample_step_table_learned(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                                             const float* noise, int B, int C, int HW, const float* table,
                                             const int32_t* counter, int objective, int advance, void* stream) {
  LGM_REQUIRE(x && v && table && counter && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) &&
                  v_pitch >= 2 * (int64_t)C && objective_ok(objective),
              "sample_step_table_learned: bad arguments");
  return sample_step_slice_launch(x, x, pitch, x_off, sc_off, v, v_pitch, noise, nullptr, 0, B, C, HW, SampleRow{}, table,
                                  counter, objective, 1, 0, advance, stream, nullptr, InpaintOps{}, 1);
}

// The dynamically thresholded update (thresh [B] from lgm_dyn_thresh): both forms of the row behind one entry point - table
// != NULL takes row counter[0] of it, else the eight scalars.  x0_out (optional, pitch = `pitch`): a network without a
// self-conditioning slice hands one in for p_sample to return.
extern "C" int lgm_sample_step_thresh(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                      int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW,
                                      int objective, int rederive, float A, float Bv, float R, float Rm1, float C0, float C1,
                                      float C2, float C3, const float* table, const int32_t* counter, int advance,
                                      const float* thresh, void* stream) {
  LGM_REQUIRE(xin && xout && v && thresh && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) && v_pitch >= C &&
                  objective_ok(objective) && (table == nullptr) == (counter == nullptr) && (table || !advance) &&
                  (!table || xin == xout) && x0_out != xin && x0_out != xout,
              "sample_step_thresh: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  return sample_step_slice_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, x0_out, pitch, B, C, HW, row, table,
                                  counter, objective, 1, rederive, advance, stream, thresh);
}

// DPM-Solver++ step.  The name is noted without a registry entry (no LGM_KNAME): tests/test_hip_kernel_ledger.py keeps the
// list of every registry name with the test file that runs it, and tests/test_hip_dpmpp.py, which runs this kernel and
// asserts the noted name, is not on that list.  A memory-bound pass: at most 2048 workgroups, the rest by grid stride.
static int dpm_step_launch(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                           int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, const SampleRow& row,
                           const float* table, const int32_t* counter, int objective, int clip, int advance, void* stream,
                           const float* thresh = nullptr, const InpaintOps& ip = InpaintOps{}, int lanes = 0) {
  lgm_note_kernel("dpm_step_kernel");
  if (lanes == 0) lanes = (int)pitch;
  const long blocks = ((long)B * HW * lanes + 255) / 256;
  hipLaunchKernelGGL(dpm_step_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, xin,
                     xout, (long)pitch, lanes, x_off, sc_off, v, (long)v_pitch, noise, hist, B, C, HW, row, table,
                     (const int*)counter, objective, clip, thresh, ip);
  if (advance) hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)counter);
  LGM_LAUNCH_CHECK_AS("dpm_step");
  return LGM_OK;
}
// what both forms ask of the buffers: the slices inside a pitch that also covers the history's r4(C) lanes, the history a
// buffer of its own (the input buffer is rewritten by the same launch)
static bool dpm_buffers_ok(const float* xin, const float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                           int64_t v_pitch, const float* hist, int B, int C, int HW, int objective) {
  return xin && xout && v && hist && hist != xin && hist != xout && v != xout && B > 0 && HW > 0 &&
         slices_ok(pitch, x_off, sc_off, C) && pitch <= 4096 && pitch >= ((C + 3) & ~3) && v_pitch >= C &&
         objective_ok(objective);
}

extern "C" int lgm_dpm_step(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                            int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective, float A,
                            float Bv, int clip, float R, float Rm1, float Kx, float K0, float K1, float Kn, void* stream) {
  LGM_REQUIRE(dpm_buffers_ok(xin, xout, pitch, x_off, sc_off, v, v_pitch, hist, B, C, HW, objective),
              "dpm_step: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, Kx, K0, K1, Kn}};
  return dpm_step_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, hist, B, C, HW, row, nullptr, nullptr, objective,
                         clip, 0, stream);
}

extern "C" int lgm_dpm_step_table(float* x, int64_t pitch, int x_off, int sc_off, const float* v, int64_t v_pitch,
                                  const float* noise, float* hist, int B, int C, int HW, const float* table,
                                  const int32_t* counter, int objective, int clip, int advance, void* stream) {
  LGM_REQUIRE(table && counter && dpm_buffers_ok(x, x, pitch, x_off, sc_off, v, v_pitch, hist, B, C, HW, objective),
              "dpm_step_table: bad arguments");
  return dpm_step_launch(x, x, pitch, x_off, sc_off, v, v_pitch, noise, hist, B, C, HW, SampleRow{}, table, counter, objective,
                         clip, advance, stream);
}

// the dynamically thresholded DPM-Solver++ step: both forms of the row behind one entry point, like lgm_sample_step_thresh
extern "C" int lgm_dpm_step_thresh(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                   int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective,
                                   float A, float Bv, float R, float Rm1, float Kx, float K0, float K1, float Kn,
                                   const float* table, const int32_t* counter, int advance, const float* thresh,
                                   void* stream) {
  LGM_REQUIRE(thresh && dpm_buffers_ok(xin, xout, pitch, x_off, sc_off, v, v_pitch, hist, B, C, HW, objective) &&
                  (table == nullptr) == (counter == nullptr) && (table || !advance) && (!table || xin == xout),
              "dpm_step_thresh: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, Kx, K0, K1, Kn}};
  return dpm_step_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, hist, B, C, HW, row, table, counter, objective,
                         1, advance, stream, thresh);
}

// Inpainting: the update with the tail of inpaint_tail_one behind it, in the same launch.  One entry point per kernel for both
// forms of the rows (table != NULL: row counter[0] of table[n][8] and of itable[n][4], the scalars ignored) and with or
// without thresholds (thresh NULL: the static clamp).  known / mask / eps_k / eps_j as InpaintOps describes them; eps_k may
// be NULL only where M_n is zero by value, eps_j only where J_n is - a table step needs both.  known == NULL (then no mask, no
// draws, no itable): the update alone, the body the other entry points run.
static bool inpaint_ops_ok(const float* known, const float* mask, const float* eps_k, const float* eps_j, float Mn, float Jn,
                           const float* table, const float* itable, const void* xin, const void* xout) {
  if (!known) return !mask && !eps_k && !eps_j && !itable;
  if (!mask || known == xin || known == xout || mask == xin || mask == xout) return false;
  if ((table == nullptr) != (itable == nullptr)) return false;
  if (itable) return eps_k && eps_j;
  return (eps_k || Mn == 0.f) && (eps_j || Jn == 0.f);
}

extern "C" int lgm_sample_step_inpaint(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                       int64_t v_pitch, const float* noise, float* x0_out, int B, int C, int HW,
                                       int objective, int rederive, float A, float Bv, float R, float Rm1, float C0,
                                       float C1, float C2, float C3, const float* table, const int32_t* counter,
                                       int advance, const float* thresh, const float* known, const float* mask,
                                       const float* eps_k, const float* eps_j, float Ma, float Mn, float Jx, float Jn,
                                       const float* itable, void* stream) {
  LGM_REQUIRE(xin && xout && v && B > 0 && HW > 0 && slices_ok(pitch, x_off, sc_off, C) && v_pitch >= C &&
                  objective_ok(objective) && (table == nullptr) == (counter == nullptr) && (table || !advance) &&
                  (!table || xin == xout) && x0_out != xin && x0_out != xout &&
                  inpaint_ops_ok(known, mask, eps_k, eps_j, Mn, Jn, table, itable, xin, xout),
              "sample_step_inpaint: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  const InpaintOps ip = {known, mask, eps_k, eps_j, itable, {Ma, Mn, Jx, Jn}};
  return sample_step_slice_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, x0_out, pitch, B, C, HW, row, table,
                                  counter, objective, 1, rederive, advance, stream, thresh, ip);
}

extern "C" int lgm_dpm_step_inpaint(const float* xin, float* xout, int64_t pitch, int x_off, int sc_off, const float* v,
                                    int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW, int objective,
                                    float A, float Bv, float R, float Rm1, float Kx, float K0, float K1, float Kn,
                                    const float* table, const int32_t* counter, int advance, const float* thresh,
                                    const float* known, const float* mask, const float* eps_k, const float* eps_j, float Ma,
                                    float Mn, float Jx, float Jn, const float* itable, void* stream) {
  LGM_REQUIRE(dpm_buffers_ok(xin, xout, pitch, x_off, sc_off, v, v_pitch, hist, B, C, HW, objective) &&
                  (table == nullptr) == (counter == nullptr) && (table || !advance) && (!table || xin == xout) &&
                  known != hist && mask != hist &&
                  inpaint_ops_ok(known, mask, eps_k, eps_j, Mn, Jn, table, itable, xin, xout),
              "dpm_step_inpaint: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, Kx, K0, K1, Kn}};
  const InpaintOps ip = {known, mask, eps_k, eps_j, itable, {Ma, Mn, Jx, Jn}};
  return dpm_step_launch(xin, xout, pitch, x_off, sc_off, v, v_pitch, noise, hist, B, C, HW, row, table, counter, objective,
                         1, advance, stream, thresh, ip);
}

// The updates with an EXTENT: the launch owns lanes [lane0, lane0 + lanes) of the pitch - the x slice inside them, zeros in
// the rest of them - and touches no other lane, so a constant slice outside the extent (the low-resolution conditioning image
// of a cascaded stage, written once per chain by lgm_lowres_cond) is still there after the last step.  The kernels are the
// ones above, handed the buffers from lane0 on; no self-conditioning slice.  Both forms of the row (table != NULL: row
// counter[0]) and the thresholds (or NULL) behind one entry point each, like the *_inpaint ones.
static bool extent_ok(int64_t pitch, int lane0, int lanes, int x_off, int C) {
  return C > 0 && lane0 >= 0 && lanes > 0 && lane0 + (int64_t)lanes <= pitch && x_off >= lane0 && x_off + C <= lane0 + lanes;
}

extern "C" int lgm_sample_step_extent(const float* xin, float* xout, int64_t pitch, int lane0, int lanes, int x_off,
                                      const float* v, int64_t v_pitch, const float* noise, float* x0_out, int64_t x0_pitch,
                                      int B, int C, int HW, int objective, int rederive, float A, float Bv, float R, float Rm1,
                                      float C0, float C1, float C2, float C3, const float* table, const int32_t* counter,
                                      int advance, const float* thresh, int learned, void* stream) {
  LGM_REQUIRE(xin && xout && v && B > 0 && HW > 0 && extent_ok(pitch, lane0, lanes, x_off, C) &&
                  v_pitch >= (learned ? 2 : 1) * (int64_t)C && objective_ok(objective) &&
                  (table == nullptr) == (counter == nullptr) && (table || !advance) && (!table || xin == xout) &&
                  x0_out != xin && x0_out != xout && (!x0_out || x0_pitch >= lanes) && !(learned && thresh),
              "sample_step_extent: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, C0, C1, C2, C3}};
  return sample_step_slice_launch(xin + lane0, xout + lane0, pitch, x_off - lane0, -1, v, v_pitch, noise, x0_out, x0_pitch, B,
                                  C, HW, row, table, counter, objective, 1, learned ? 0 : rederive, advance, stream, thresh,
                                  InpaintOps{}, learned ? 1 : 0, lanes);
}

extern "C" int lgm_dpm_step_extent(const float* xin, float* xout, int64_t pitch, int lane0, int lanes, int x_off,
                                   const float* v, int64_t v_pitch, const float* noise, float* hist, int B, int C, int HW,
                                   int objective, float A, float Bv, float R, float Rm1, float Kx, float K0, float K1,
                                   float Kn, const float* table, const int32_t* counter, int advance, const float* thresh,
                                   void* stream) {
  LGM_REQUIRE(extent_ok(pitch, lane0, lanes, x_off, C) &&
                  dpm_buffers_ok(xin, xout, pitch, x_off, -1, v, v_pitch, hist, B, C, HW, objective) &&
                  (table == nullptr) == (counter == nullptr) && (table || !advance) && (!table || xin == xout),
              "dpm_step_extent: bad arguments");
  const SampleRow row = {{A, Bv, R, Rm1, Kx, K0, K1, Kn}};
  return dpm_step_launch(xin + lane0, xout + lane0, pitch, x_off - lane0, -1, v, v_pitch, noise, hist, B, C, HW, row, table,
                         counter, objective, 1, advance, stream, thresh, InpaintOps{}, lanes);
}

// Dynamic thresholding: thresh[b] = max(1, lo + w (hi - lo)) with lo, hi the k-th and (k+1)-th smallest |x0| of sample b
// ((k, w) = lgm_hip.sampler.dyn_rank(C * HW, p)), x0 the unclipped prediction from the x slice of xin and the network output
// v with the head (A, Bv, R, Rm1) by value or from row counter[0] of `table`.  One workgroup per sample.  The name is noted
// without a registry entry, like dpm_step_kernel's and for the same reason.
extern "C" int lgm_dyn_thresh(const float* xin, int64_t pitch, int x_off, const float* v, int64_t v_pitch, int B, int C,
                              int HW, int objective, float A, float Bv, float R, float Rm1, const float* table,
                              const int32_t* counter, int k, float w, float* thresh, void* stream) {
  LGM_REQUIRE(xin && v && thresh && B > 0 && HW > 0 && slices_ok(pitch, x_off, -1, C) && v_pitch >= C &&
                  objective_ok(objective) && (table == nullptr) == (counter == nullptr) &&
                  (int64_t)C * HW < ((int64_t)1 << 31) && k >= 0 && (int64_t)k < (int64_t)C * HW && w >= 0.f && w < 1.f,
              "dyn_thresh: bad arguments");
  lgm_note_kernel("dyn_thresh_kernel");
  const SampleRow row = {{A, Bv, R, Rm1, 0.f, 0.f, 0.f, 0.f}};
  hipLaunchKernelGGL(dyn_thresh_kernel, dim3(B), dim3(DT_THREADS), 0, (hipStream_t)stream, xin, (long)pitch, x_off, v,
                     (long)v_pitch, C, HW, row, table, (const int*)counter, objective, (unsigned)k, w, thresh);
  LGM_LAUNCH_CHECK_AS("dyn_thresh");
  return LGM_OK;
}

// Variational-bound terms (vlb_term_kernel): the row by value with an explicit output row, or row counter[0] of a table with
// `stride` floats per row, written to output row counter[0].  The name is noted without a registry entry, like
// dpm_step_kernel's and for the same reason.  A prior row (kind 2) reads img only.
static bool vlb_operands_ok(const float* img, const float* noise, const float* xin, int64_t pitch, int x_off, const float* v,
                            int64_t v_pitch, int B, int C, int HW, int objective, const float* out, int n_rows, bool prior) {
  if (!img || !out || out == img || B <= 0 || C <= 0 || HW <= 0 || n_rows <= 0 || !objective_ok(objective)) return false;
  if ((int64_t)n_rows * 3 * B >= ((int64_t)1 << 31)) return false;
  if (prior) return true;
  return noise && xin && v && out != noise && out != xin && out != v && slices_ok(pitch, x_off, -1, C) && v_pitch >= C;
}
static int vlb_term_launch(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch, int x_off,
                           const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip, const VlbRow& row,
                           const float* table, int stride, const int32_t* counter, int out_row, float* out, int n_rows,
                           int advance, void* stream) {
  const int v_lanes = v ? (int)(v_pitch < 2 * (int64_t)C ? C : 2 * C) : 0;
  lgm_note_kernel("vlb_term_kernel");
  hipLaunchKernelGGL(vlb_term_kernel, dim3(B), dim3(VLB_THREADS), 0, (hipStream_t)stream, img, noise, normalize, xin,
                     (long)pitch, x_off, v, (long)v_pitch, B, C, HW, row, table, stride, (const int*)counter, out_row,
                     objective, clip ? 1 : 0, out, n_rows, v_lanes);
  if (advance) hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)counter);
  LGM_LAUNCH_CHECK_AS("vlb_term");
  return LGM_OK;
}

extern "C" int lgm_vlb_term(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch, int x_off,
                            const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip, float A, float S,
                            float R, float Rm1, float P1, float P2, int kind, float KC, float KW, float inv_std, float* out,
                            int n_rows, int out_row, void* stream) {
  LGM_REQUIRE(kind >= 0 && kind <= 2 && out_row >= 0 && out_row < n_rows &&
                  vlb_operands_ok(img, noise, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, out, n_rows, kind == 2),
              "vlb_term: bad arguments");
  const VlbRow row = {{A, S, R, Rm1, P1, P2, (float)kind, KC, KW, inv_std, 0.f, 0.f}};
  return vlb_term_launch(img, noise, normalize, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, clip, row, nullptr, 0,
                         nullptr, out_row, out, n_rows, 0, stream);
}

extern "C" int lgm_vlb_term_table(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch,
                                  int x_off, const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip,
                                  const float* table, int stride, const int32_t* counter, float* out, int n_rows, int advance,
                                  void* stream) {
  LGM_REQUIRE(table && counter && stride >= VLB_ROW && out != table && (const void*)out != (const void*)counter &&
                  vlb_operands_ok(img, noise, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, out, n_rows, false),
              "vlb_term_table: bad arguments");
  return vlb_term_launch(img, noise, normalize, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, clip, VlbRow{}, table,
                         stride, counter, 0, out, n_rows, advance, stream);
}

// The term of a learned-variance network (kind 3: KL, 4: decoder; slots 10 / 11 = log beta_t, log beta~_t), both forms of the
// row behind one entry point like lgm_sample_step_thresh: table != NULL takes row counter[0] of it into output row counter[0].
// The network output carries 2 C lanes.
extern "C" int lgm_vlb_term_learned(const float* img, const float* noise, int normalize, const float* xin, int64_t pitch,
                                    int x_off, const float* v, int64_t v_pitch, int B, int C, int HW, int objective, int clip,
                                    float A, float S, float R, float Rm1, float P1, float P2, int kind, float log_beta,
                                    float log_tilde, const float* table, int stride, const int32_t* counter, float* out,
                                    int n_rows, int out_row, int advance, void* stream) {
  LGM_REQUIRE((table == nullptr) == (counter == nullptr) && (table || !advance) &&
                  (table ? stride >= VLB_ROW && out != table && (const void*)out != (const void*)counter
                         : (kind == 3 || kind == 4) && out_row >= 0 && out_row < n_rows) &&
                  v_pitch >= 2 * (int64_t)C &&
                  vlb_operands_ok(img, noise, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, out, n_rows, false),
              "vlb_term_learned: bad arguments");
  const VlbRow row = {{A, S, R, Rm1, P1, P2, (float)kind, 0.f, 0.f, 0.f, log_beta, log_tilde}};
  return vlb_term_launch(img, noise, normalize, xin, pitch, x_off, v, v_pitch, B, C, HW, objective, clip, row, table, stride,
                         counter, out_row, out, n_rows, advance, stream);
}

// ---------------------------------------------------------------------------------------
// WGAN-GP helpers (wgan.py:84-156)
// ---------------------------------------------------------------------------------------
namespace {

// interpolates: out[b] = alpha[b]*x[b] + (1-alpha[b])*y[b]   (dense rows of `rowlen` floats)
__global__ __launch_bounds__(256) void lerp_rows_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ alpha, float* __restrict__ out,
                                                        long B, long rowlen) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * rowlen) return;
  const float a = alpha[i / rowlen];
  out[i] = a * x[i] + (1.f - a) * y[i];
}

// gradient penalty with the reference's CHANNEL-ONLY norm (wgan.py:153-154):
//   r[p] = sqrt(sum_c g[p,c]^2);  partial[block] = sum_p (r-1)^2;  gbar[p,c] = coef*(r-1)/r * g[p,c],
//   coef = gscale * lambda * 2 / npix.  One thread per pixel, C <= 4 (padded to 4 floats).
__global__ __launch_bounds__(256) void gp_penalty_kernel(const float* __restrict__ g, long npix, int C, float lambda,
                                                         const float* __restrict__ gscale, float* __restrict__ partial,
                                                         float* __restrict__ gbar) {
  __shared__ float sh[16];
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float pen = 0.f;
  if (p < npix) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + p * 4);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) s += v[c] * v[c];
    const float r = sqrtf(s);
    pen = (r - 1.f) * (r - 1.f);
    if (gbar) {
      // r == 0 (a pixel whose channel gradient is exactly zero: dead / clipped critic): torch's backward of
      // norm(2, dim=1) uses the zero subgradient there (wgan.py:153-154), not (r-1)/r = -inf
      const float k = r > 0.f ? gscale[0] * lambda * 2.f / (float)npix * (r - 1.f) / r : 0.f;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) o[c] = k * v[c];
      *reinterpret_cast<f32x4*>(gbar + p * 4) = o;
    }
  }
  pen = lgm_block_sum(pen, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = pen;
}

// R1 penalty (r1gan.py:77): partial[block] = sum_p sum_c g[p,c]^2;  gbar = gscale / B * g.
__global__ __launch_bounds__(256) void r1_penalty_kernel(const float* __restrict__ g, long npix, float inv_b,
                                                         const float* __restrict__ gscale, float* __restrict__ partial,
                                                         float* __restrict__ gbar) {
  __shared__ float sh[16];
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float pen = 0.f;
  if (p < npix) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + p * 4);
    pen = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);   // the padding lane carries zeros
    if (gbar) *reinterpret_cast<f32x4*>(gbar + p * 4) = v * (gscale[0] * inv_b);
  }
  pen = lgm_block_sum(pen, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = pen;
}

// vals[slot] = scale * sum_i partial[i]   (single block, fixed order)
__global__ __launch_bounds__(256) void sum_scale_kernel(const float* __restrict__ partial, long n, long stride,
                                                        float scale, float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) s += partial[i * stride];
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// out[r][c] = (c == col) ? scale * (vptr ? vptr[0] : 1) : 0
__global__ void fill_col_kernel(float* __restrict__ out, long pitch, long n, int ncols, int col, float scale,
                                const float* __restrict__ vptr) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * ncols) return;
  const long r = i / ncols;
  const int c = (int)(i % ncols);
  out[r * pitch + c] = (c == col) ? scale * (vptr ? vptr[0] : 1.f) : 0.f;
}

// vals = (real, fake, gp, d_loss): d_loss = fake - real + gp
__global__ void wgan_dloss_kernel(float* __restrict__ vals) { vals[3] = vals[1] - vals[0] + vals[2]; }


// Device-side input pipeline of the reference DataModule (data/datamodule.py:41-53): ToTensor (u8 -> [0,1]),
// Normalize(0.5, 0.5), CenterCropMinXY (data/utils.py:7-35), Resize(S, bilinear, antialias=True),
// RandomHorizontalFlip (flags drawn by the caller).  The antialiased resize is the separable triangle
// filter of torch's _upsample_bilinear2d_aa: support = max(scale, 1), window [int(c - support + .5),
// int(c + support + .5)), weights max(0, 1 - |(j + .5 - c) / max(scale, 1)|) normalised to 1.
// One thread per output pixel, all (<= 4) channels; u8 HWC in, fp32 NCHW out.
__global__ __launch_bounds__(256) void image_transform_kernel(const unsigned char* __restrict__ src, int H, int W, int C,
                                                              const unsigned char* __restrict__ flip,
                                                              float* __restrict__ dst, int S, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % S), oy = (int)((i / S) % S);
  const long b = i / ((long)S * S);
  const int D = H < W ? H : W, top = (H - D) / 2, left = (W - D) / 2;
  const float scale = (float)D / (float)S;
  const float support = scale >= 1.f ? scale : 1.f;
  const float inv = 1.f / support;
  const int sx = (flip && flip[b]) ? S - 1 - ox : ox;     // flip after the resize == mirrored source column
  const float cy = scale * (oy + 0.5f), cx = scale * (sx + 0.5f);
  const int ymin = max(0, (int)(cy - support + 0.5f)), ymax = min(D, (int)(cy + support + 0.5f));
  const int xmin = max(0, (int)(cx - support + 0.5f)), xmax = min(D, (int)(cx + support + 0.5f));
  float wys = 0.f, wxs = 0.f;
  for (int y = ymin; y < ymax; ++y) wys += fmaxf(0.f, 1.f - fabsf((y - cy + 0.5f) * inv));
  for (int x = xmin; x < xmax; ++x) wxs += fmaxf(0.f, 1.f - fabsf((x - cx + 0.5f) * inv));
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const unsigned char* img = src + b * (long)H * W * C;
  for (int y = ymin; y < ymax; ++y) {
    const float wy = fmaxf(0.f, 1.f - fabsf((y - cy + 0.5f) * inv)) / wys;
    float row[4] = {0.f, 0.f, 0.f, 0.f};
    for (int x = xmin; x < xmax; ++x) {
      const float wx = fmaxf(0.f, 1.f - fabsf((x - cx + 0.5f) * inv)) / wxs;
      const unsigned char* px = img + ((long)(top + y) * W + left + x) * C;
      for (int c = 0; c < C; ++c) row[c] += wx * (float)px[c];
    }
    for (int c = 0; c < C; ++c) acc[c] += wy * row[c];
  }
  for (int c = 0; c < C; ++c)
    dst[((b * C + c) * S + oy) * (long)S + ox] = acc[c] * (2.f / 255.f) - 1.f;   // /255, (x - .5) / .5
}

}  // namespace

extern "C" int lgm_image_transform(const unsigned char* src, int64_t B, int H, int W, int C, const unsigned char* flip,
                                   float* dst, int S, void* stream) {
  LGM_REQUIRE(src && dst && B > 0 && H > 0 && W > 0 && C >= 1 && C <= 4 && S > 0, "image_transform: bad arguments");
  const long total = (long)B * S * S;
  hipLaunchKernelGGL(image_transform_kernel, dim3(lgm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, H, W, C,
                     flip, dst, S, total);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_lerp_rows(const float* x, const float* y, const float* alpha, float* out, int64_t B,
                             int64_t rowlen, void* stream) {
  LGM_REQUIRE(x && y && alpha && out && B > 0 && rowlen > 0, "lerp_rows: bad arguments");
  hipLaunchKernelGGL(lerp_rows_kernel, dim3(lgm_cdiv(B * rowlen, 256)), dim3(256), 0, (hipStream_t)stream, x, y, alpha,
                     out, (long)B, (long)rowlen);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int64_t lgm_gp_penalty_workspace(int64_t npix) { return (int64_t)lgm_cdiv(npix, 256) * 4 + 16; }

extern "C" int lgm_gp_penalty(const float* g, int64_t npix, int C, float lambda, const float* gscale, float* loss_out,
                              float* gbar, void* workspace, void* stream) {
  LGM_REQUIRE(g && loss_out && workspace && npix > 0 && C >= 1 && C <= 4 && (!gbar || gscale) && lgm_aligned16(g),
              "gp_penalty: bad arguments (dense NHWC4 gradient expected)");
  hipStream_t s = (hipStream_t)stream;
  const int nb = lgm_cdiv(npix, 256);
  hipLaunchKernelGGL(gp_penalty_kernel, dim3(nb), dim3(256), 0, s, g, (long)npix, C, lambda, gscale, (float*)workspace,
                     gbar);
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (long)nb, 1L,
                     lambda / (float)npix, loss_out);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_r1_penalty(const float* g, int64_t npix, int64_t B, const float* gscale, float* loss_out,
                              float* gbar, void* workspace, void* stream) {
  LGM_REQUIRE(g && loss_out && workspace && npix > 0 && B > 0 && (!gbar || gscale) && lgm_aligned16(g),
              "r1_penalty: bad arguments (dense NHWC4 gradient expected)");
  hipStream_t s = (hipStream_t)stream;
  const int nb = lgm_cdiv(npix, 256);
  hipLaunchKernelGGL(r1_penalty_kernel, dim3(nb), dim3(256), 0, s, g, (long)npix, 1.f / (float)B, gscale,
                     (float*)workspace, gbar);
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (long)nb, 1L, 0.5f / (float)B,
                     loss_out);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_mean_col(const float* v, int64_t pitch, int64_t n, float scale, float* out, void* stream) {
  LGM_REQUIRE(v && out && n > 0, "mean_col: bad arguments");
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, v, (long)n, (long)pitch,
                     scale / (float)n, out);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_fill_col(float* out, int64_t pitch, int64_t n, int ncols, int col, float scale, const float* vptr,
                            void* stream) {
  LGM_REQUIRE(out && n > 0 && ncols > 0 && col < ncols && pitch >= ncols, "fill_col: bad arguments");
  hipLaunchKernelGGL(fill_col_kernel, dim3(lgm_cdiv(n * ncols, 256)), dim3(256), 0, (hipStream_t)stream, out,
                     (long)pitch, (long)n, ncols, col, scale, vptr);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

namespace {
__global__ void vqvae_loss_kernel(const float* recon, const float* out3, float w_recon, float w_vq, float* vals4) {
  const float r = recon[0], v = out3[0];
  vals4[0] = r * w_recon + v * w_vq;
  vals4[1] = r;
  vals4[2] = v;
  vals4[3] = out3[1];
}
// the same with the reconstruction term still as per-sample values: their mean (mean_kernel's arithmetic) is taken here
__global__ __launch_bounds__(256) void vqvae_loss_mean_kernel(const float* per_sample, int n, const float* out3, float w_recon,
                                                              float w_vq, float* vals4) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += per_sample[i];
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float r = s / (float)n, v = out3[0];
    vals4[0] = r * w_recon + v * w_vq;
    vals4[1] = r;
    vals4[2] = v;
    vals4[3] = out3[1];
  }
}
__global__ void scale_pair_kernel(const float* g, float w0, float w1, float* out2) {
  out2[0] = g[0] * w0;
  out2[1] = g[0] * w1;
}
}  // namespace

extern "C" int lgm_vqvae_loss(const float* recon, const float* out3, float w_recon, float w_vq, float* vals4,
                              void* stream) {
  LGM_REQUIRE(recon && out3 && vals4, "vqvae_loss: null pointer");
  hipLaunchKernelGGL(vqvae_loss_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, recon, out3, w_recon, w_vq, vals4);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_vqvae_loss_samples(const float* per_sample, int n, const float* out3, float w_recon, float w_vq,
                                      float* vals4, void* stream) {
  LGM_REQUIRE(per_sample && out3 && vals4 && n > 0, "vqvae_loss_samples: bad arguments");
  hipLaunchKernelGGL(vqvae_loss_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, per_sample, n, out3, w_recon, w_vq,
                     vals4);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_scale_pair(const float* g, float w0, float w1, float* out2, void* stream) {
  LGM_REQUIRE(g && out2, "scale_pair: null pointer");
  hipLaunchKernelGGL(scale_pair_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, g, w0, w1, out2);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_wgan_dloss(float* vals4, void* stream) {
  LGM_REQUIRE(vals4, "wgan_dloss: null pointer");
  hipLaunchKernelGGL(wgan_dloss_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, vals4);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
