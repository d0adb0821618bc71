// BatchNorm1d over few rows (an MLP's batch: M = B from 1 to 512 rows, F features) in ONE launch per direction, and the
// binary-cross-entropy-with-logits head of the MLP GAN (reference models/generative/gan/gan.py:15-89, :258-308).  DESIGN
// section 6 has the definitions and the rounding counts.
//
// bn1d_fwd_kernel<R> / bn1d_bwd_kernel<R>   a workgroup of 512 threads owns a strip of 32 columns (one 128-byte line of every
//   row) and ALL B rows: thread (c, rg) holds rows rg, rg + 16, .. (at most R of them, R = 2 / 8 / 32 for B <= 32 / 128 / 512)
//   of column c in registers, so the batch is read once and stays on chip.  Column sums: every row group adds its rows in
//   ascending order, the 16 groups are added in index order through LDS (as dense_g_kernel does).  Forward, training: the
//   mean, then the CENTRED sum of squares of the rows in registers (never E[x^2] - E[x]^2), rstd = 1 / sqrt(var + eps) from
//   the biased variance, the running statistics (running_var with B / (B - 1)), y = act(gamma xhat + beta).  Forward, eval:
//   the same kernel normalises with the running statistics and writes none.  Backward: g = gy act'(y) with act' read from
//   the saved OUTPUT, s1 = sum g, s2 = sum g xhat, gbeta / ggamma = beta_acc . + s, ga = gamma rstd (g - s1 / B - xhat s2 / B).
// gan_bce_d_kernel / gan_bce_g_kernel / gan_bce_bwd_kernel   one wave: lane l sums samples l, l + 64, .. in order, then the
//   fixed shuffle tree.  bce(s, t) = max(s, 0) - s t + log1p(exp(-|s|)).
// Every grid and every summation order is a function of (B, F) alone - never of lgm_cu_margin() -, nothing is summed by an
// atomic and no workgroup waits for another: eager, replayed and repeated runs give equal bits.  Every access is guarded by
// (B, F): pad lanes of an input are never read, pad lanes [F, round_up(F, 4)) of an output are written 0, nothing beyond.
#include "lgm_common.h"

namespace {

constexpr int B1_COLS = 32, B1_GROUPS = 16, B1_THREADS = B1_COLS * B1_GROUPS;
constexpr int B1_MAX_ROWS = 512;              // 32 rows per thread
constexpr int B1_MAX_F = 1 << 20;

struct Bn1Fwd {
  const float* a; const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  float* y; float* mean; float* rstd;
  long a_pitch, y_pitch;
  int B, F, Fp, training, act;
  float eps, momentum, slope;
};

struct Bn1Bwd {
  const float* gy; const float* y; const float* a; const float* mean; const float* rstd; const float* gamma;
  float* ga; float* ggamma; float* gbeta;
  long gy_pitch, y_pitch, a_pitch, ga_pitch;
  int B, F, Fp, act;
  float slope, beta_acc;
};

// the 16 row groups' partial sums of column c, added in index order; every thread of the column gets the total
__device__ __forceinline__ float b1_groups_total(float (*sh)[B1_COLS], int rg, int c, float part) {
#pragma clang fp contract(off)
  sh[rg][c] = part;
  __syncthreads();
  float t = sh[0][c];
#pragma unroll
  for (int r = 1; r < B1_GROUPS; ++r) t = t + sh[r][c];
  __syncthreads();                            // sh may be written again
  return t;
}

template <int R>
__global__ __launch_bounds__(B1_THREADS) void bn1d_fwd_kernel(const Bn1Fwd p) {
#pragma clang fp contract(off)
  __shared__ float sh[B1_GROUPS][B1_COLS];
  const int c = threadIdx.x % B1_COLS, rg = threadIdx.x / B1_COLS;
  const int col = blockIdx.x * B1_COLS + c;
  const bool live = col < p.F;
  float v[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = rg + i * B1_GROUPS;
    v[i] = (live && m < p.B) ? p.a[(long)m * p.a_pitch + col] : 0.f;
  }
  float mean = 0.f, rstd = 0.f;
  if (p.training) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (rg + i * B1_GROUPS < p.B) s = s + v[i];
    mean = b1_groups_total(sh, rg, c, s) / (float)p.B;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (rg + i * B1_GROUPS < p.B) {
        const float d = v[i] - mean;
        q = q + d * d;
      }
    const float var = b1_groups_total(sh, rg, c, q) / (float)p.B;
    rstd = 1.f / sqrtf(var + p.eps);
    if (rg == 0 && live) {
      const float keep = 1.f - p.momentum;
      const float unbiased = var * ((float)p.B / (float)(p.B - 1));
      p.running_mean[col] = keep * p.running_mean[col] + p.momentum * mean;
      p.running_var[col] = keep * p.running_var[col] + p.momentum * unbiased;
    }
  } else if (live) {
    mean = p.running_mean[col];
    rstd = 1.f / sqrtf(p.running_var[col] + p.eps);
  }
  if (rg == 0 && live) {
    p.mean[col] = mean;
    p.rstd[col] = rstd;
  }
  if (col >= p.Fp) return;
  const float gm = live ? p.gamma[col] : 0.f, bt = live ? p.beta[col] : 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = rg + i * B1_GROUPS;
    if (m < p.B) {
      float o = 0.f;
      if (live) {
        o = gm * ((v[i] - mean) * rstd) + bt;
        if (p.act == LGM_ACT_LRELU) o = o > 0.f ? o : o * p.slope;
      }
      p.y[(long)m * p.y_pitch + col] = o;
    }
  }
}

template <int R>
__global__ __launch_bounds__(B1_THREADS) void bn1d_bwd_kernel(const Bn1Bwd p) {
#pragma clang fp contract(off)
  __shared__ float sh[B1_GROUPS][B1_COLS];
  const int c = threadIdx.x % B1_COLS, rg = threadIdx.x / B1_COLS;
  const int col = blockIdx.x * B1_COLS + c;
  const bool live = col < p.F;
  const float mean = live ? p.mean[col] : 0.f, rstd = live ? p.rstd[col] : 0.f;
  float g[R], xh[R];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = rg + i * B1_GROUPS;
    g[i] = 0.f;
    xh[i] = 0.f;
    if (live && m < p.B) {
      float gv = p.gy[(long)m * p.gy_pitch + col];
      if (p.act == LGM_ACT_LRELU) gv = gv * (p.y[(long)m * p.y_pitch + col] > 0.f ? 1.f : p.slope);
      g[i] = gv;
      xh[i] = (p.a[(long)m * p.a_pitch + col] - mean) * rstd;
      s1 = s1 + gv;
      s2 = s2 + gv * xh[i];
    }
  }
  s1 = b1_groups_total(sh, rg, c, s1);
  s2 = b1_groups_total(sh, rg, c, s2);
  if (rg == 0 && live) {
    p.gbeta[col] = p.beta_acc == 0.f ? s1 : p.beta_acc * p.gbeta[col] + s1;
    p.ggamma[col] = p.beta_acc == 0.f ? s2 : p.beta_acc * p.ggamma[col] + s2;
  }
  if (col >= p.Fp) return;
  const float c0 = live ? p.gamma[col] * rstd : 0.f;
  const float m1 = s1 / (float)p.B, m2 = s2 / (float)p.B;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = rg + i * B1_GROUPS;
    if (m < p.B) p.ga[(long)m * p.ga_pitch + col] = live ? c0 * ((g[i] - m1) - xh[i] * m2) : 0.f;
  }
}

// ---- binary cross entropy with logits ---------------------------------------------------------------------------------
__device__ __forceinline__ float bce_logits(float s, float t) {
#pragma clang fp contract(off)
  return (fmaxf(s, 0.f) - s * t) + log1pf(expf(-fabsf(s)));
}

// sigmoid(s) without cancellation at either end
__device__ __forceinline__ float bce_sigmoid(float s) {
#pragma clang fp contract(off)
  if (s >= 0.f) return 1.f / (1.f + expf(-s));
  const float e = expf(s);
  return e / (1.f + e);
}

// vals5 = (d_loss_real = mean bce(real, 1), d_loss_fake = mean bce(fake, 0), d_loss = (real + fake) / 2, mean real, mean fake)
__global__ __launch_bounds__(64) void gan_bce_d_kernel(const float* __restrict__ real, long real_pitch,
                                                       const float* __restrict__ fake, long fake_pitch, int B,
                                                       float* __restrict__ vals5) {
#pragma clang fp contract(off)
  float lr = 0.f, lf = 0.f, sr = 0.f, sf = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    const float r = real[(long)b * real_pitch], f = fake[(long)b * fake_pitch];
    lr = lr + bce_logits(r, 1.f);
    lf = lf + bce_logits(f, 0.f);
    sr = sr + r;
    sf = sf + f;
  }
  lr = lgm_wave_sum(lr);
  lf = lgm_wave_sum(lf);
  sr = lgm_wave_sum(sr);
  sf = lgm_wave_sum(sf);
  if (threadIdx.x == 0) {
    const float n = (float)B;
    const float a = lr / n, b = lf / n;
    vals5[0] = a;
    vals5[1] = b;
    vals5[2] = (a + b) * 0.5f;
    vals5[3] = sr / n;
    vals5[4] = sf / n;
  }
}

// vals2 = (g_loss, mean s): non-saturating (loss_type 0) mean bce(s, 1); min-max (1) -mean bce(s, 0)
__global__ __launch_bounds__(64) void gan_bce_g_kernel(const float* __restrict__ s, long pitch, int B, int loss_type,
                                                       float* __restrict__ vals2) {
#pragma clang fp contract(off)
  const float t = loss_type == 0 ? 1.f : 0.f;
  float l = 0.f, m = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    const float v = s[(long)b * pitch];
    l = l + bce_logits(v, t);
    m = m + v;
  }
  l = lgm_wave_sum(l);
  m = lgm_wave_sum(m);
  if (threadIdx.x == 0) {
    const float mean = l / (float)B;
    vals2[0] = loss_type == 0 ? mean : -mean;
    vals2[1] = m / (float)B;
  }
}

// g[b] = (gloss factor / B) (sigmoid(s[b]) - t), t in {0, 1}; lanes 1 .. 3 of a row of g are written 0.  Up to two vectors.
struct BceBwd {
  const float* s[2]; float* g[2];
  long s_pitch[2], g_pitch[2];
  float t[2], factor[2];
  const float* gloss;
  int B, n;
};

__global__ __launch_bounds__(256) void gan_bce_bwd_kernel(const BceBwd p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.B) return;
  const float gl = p.gloss[0];
  for (int k = 0; k < p.n; ++k) {
    const float c = (gl * p.factor[k]) / (float)p.B;
    const float v = p.s[k][(long)b * p.s_pitch[k]];
    const float d = p.t[k] == 1.f ? -bce_sigmoid(-v) : bce_sigmoid(v);
    float* o = p.g[k] + (long)b * p.g_pitch[k];
    o[0] = c * d;
    o[1] = 0.f;
    o[2] = 0.f;
    o[3] = 0.f;
  }
}

inline int r4(int n) { return (n + 3) / 4 * 4; }

bool b1_act_ok(int act) { return act == LGM_ACT_NONE || act == LGM_ACT_LRELU; }

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), as csrc/dense.hip's are and for the same reason:
// tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it; tests/test_hip_gan_mlp.py runs
// these.

extern "C" int64_t lgm_bn1d_supported(int B, int F) { return B >= 1 && B <= B1_MAX_ROWS && F >= 1 && F <= B1_MAX_F ? 1 : 0; }

extern "C" int lgm_bn1d_fwd(const float* a, int64_t a_pitch, int B, int F, const float* gamma, const float* beta, float eps,
                            float momentum, int training, int act, float slope, float* running_mean, float* running_var,
                            float* y, int64_t y_pitch, float* mean, float* rstd, void* stream) {
  LGM_REQUIRE(a && gamma && beta && running_mean && running_var && y && mean && rstd, "bn1d_fwd: null argument");
  LGM_REQUIRE(lgm_bn1d_supported(B, F), "bn1d_fwd: 1 <= B <= %d and F >= 1 required, got %d %d", B1_MAX_ROWS, B, F);
  LGM_REQUIRE(!training || B >= 2, "bn1d_fwd: batch statistics need more than one row");
  LGM_REQUIRE(a_pitch >= F && y_pitch >= r4(F), "bn1d_fwd: pitches below the feature count (a %ld < %d or y %ld < %d)",
              (long)a_pitch, F, (long)y_pitch, r4(F));
  LGM_REQUIRE(b1_act_ok(act), "bn1d_fwd: act must be none or LeakyReLU, got %d", act);
  LGM_REQUIRE((const void*)y != (const void*)a, "bn1d_fwd: y must not alias a");
  Bn1Fwd p{};
  p.a = a; p.gamma = gamma; p.beta = beta; p.running_mean = running_mean; p.running_var = running_var;
  p.y = y; p.mean = mean; p.rstd = rstd; p.a_pitch = (long)a_pitch; p.y_pitch = (long)y_pitch;
  p.B = B; p.F = F; p.Fp = r4(F); p.training = training ? 1 : 0; p.act = act;
  p.eps = eps; p.momentum = momentum; p.slope = slope;
  const dim3 grid(lgm_cdiv(p.Fp, B1_COLS));
  hipStream_t st = (hipStream_t)stream;
  lgm_note_kernel("bn1d_fwd_kernel");
  if (B <= 2 * B1_GROUPS) hipLaunchKernelGGL(bn1d_fwd_kernel<2>, grid, dim3(B1_THREADS), 0, st, p);
  else if (B <= 8 * B1_GROUPS) hipLaunchKernelGGL(bn1d_fwd_kernel<8>, grid, dim3(B1_THREADS), 0, st, p);
  else hipLaunchKernelGGL(bn1d_fwd_kernel<32>, grid, dim3(B1_THREADS), 0, st, p);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_bn1d_bwd(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* a,
                            int64_t a_pitch, const float* mean, const float* rstd, const float* gamma, int B, int F, int act,
                            float slope, float* ga, int64_t ga_pitch, float* ggamma, float* gbeta, float beta_acc,
                            void* stream) {
  LGM_REQUIRE(gy && a && mean && rstd && gamma && ga && ggamma && gbeta, "bn1d_bwd: null argument");
  LGM_REQUIRE(lgm_bn1d_supported(B, F), "bn1d_bwd: 1 <= B <= %d and F >= 1 required, got %d %d", B1_MAX_ROWS, B, F);
  LGM_REQUIRE(b1_act_ok(act), "bn1d_bwd: act must be none or LeakyReLU, got %d", act);
  LGM_REQUIRE(act == LGM_ACT_NONE || y, "bn1d_bwd: the saved output y is required with an activation");
  LGM_REQUIRE(gy_pitch >= F && a_pitch >= F && (!y || y_pitch >= F) && ga_pitch >= r4(F),
              "bn1d_bwd: pitches below the feature count %d", F);
  Bn1Bwd p{};
  p.gy = gy; p.y = y; p.a = a; p.mean = mean; p.rstd = rstd; p.gamma = gamma; p.ga = ga; p.ggamma = ggamma; p.gbeta = gbeta;
  p.gy_pitch = (long)gy_pitch; p.y_pitch = (long)y_pitch; p.a_pitch = (long)a_pitch; p.ga_pitch = (long)ga_pitch;
  p.B = B; p.F = F; p.Fp = r4(F); p.act = act; p.slope = slope; p.beta_acc = beta_acc;
  const dim3 grid(lgm_cdiv(p.Fp, B1_COLS));
  hipStream_t st = (hipStream_t)stream;
  lgm_note_kernel("bn1d_bwd_kernel");
  if (B <= 2 * B1_GROUPS) hipLaunchKernelGGL(bn1d_bwd_kernel<2>, grid, dim3(B1_THREADS), 0, st, p);
  else if (B <= 8 * B1_GROUPS) hipLaunchKernelGGL(bn1d_bwd_kernel<8>, grid, dim3(B1_THREADS), 0, st, p);
  else hipLaunchKernelGGL(bn1d_bwd_kernel<32>, grid, dim3(B1_THREADS), 0, st, p);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_gan_bce_d(const float* real, int64_t real_pitch, const float* fake, int64_t fake_pitch, int B, float* vals5,
                             void* stream) {
  LGM_REQUIRE(real && fake && vals5, "gan_bce_d: null argument");
  LGM_REQUIRE(B >= 1 && real_pitch >= 1 && fake_pitch >= 1, "gan_bce_d: B >= 1 and pitches >= 1 required, got %d", B);
  lgm_note_kernel("gan_bce_d_kernel");
  hipLaunchKernelGGL(gan_bce_d_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, real, (long)real_pitch, fake,
                     (long)fake_pitch, B, vals5);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_gan_bce_g(const float* s, int64_t pitch, int B, int loss_type, float* vals2, void* stream) {
  LGM_REQUIRE(s && vals2, "gan_bce_g: null argument");
  LGM_REQUIRE(B >= 1 && pitch >= 1, "gan_bce_g: B >= 1 and a pitch >= 1 required, got %d", B);
  LGM_REQUIRE(loss_type == 0 || loss_type == 1, "gan_bce_g: loss_type 0 (non-saturating) or 1 (min-max), got %d", loss_type);
  lgm_note_kernel("gan_bce_g_kernel");
  hipLaunchKernelGGL(gan_bce_g_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s, (long)pitch, B, loss_type, vals2);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_gan_bce_bwd(const float* s0, int64_t s0_pitch, float t0, float factor0, float* g0, int64_t g0_pitch,
                               const float* s1, int64_t s1_pitch, float t1, float factor1, float* g1, int64_t g1_pitch, int B,
                               const float* gloss, void* stream) {
  LGM_REQUIRE(s0 && g0 && gloss, "gan_bce_bwd: s0, g0 and gloss required");
  LGM_REQUIRE((s1 == nullptr) == (g1 == nullptr), "gan_bce_bwd: the second vector needs both s1 and g1");
  LGM_REQUIRE(B >= 1 && s0_pitch >= 1 && g0_pitch >= 4 && (!s1 || (s1_pitch >= 1 && g1_pitch >= 4)),
              "gan_bce_bwd: B >= 1, score pitches >= 1 and gradient pitches >= 4 required");
  LGM_REQUIRE((t0 == 0.f || t0 == 1.f) && (!s1 || t1 == 0.f || t1 == 1.f), "gan_bce_bwd: targets must be 0 or 1");
  BceBwd p{};
  p.s[0] = s0; p.g[0] = g0; p.s_pitch[0] = (long)s0_pitch; p.g_pitch[0] = (long)g0_pitch; p.t[0] = t0; p.factor[0] = factor0;
  p.s[1] = s1; p.g[1] = g1; p.s_pitch[1] = (long)s1_pitch; p.g_pitch[1] = (long)g1_pitch; p.t[1] = t1; p.factor[1] = factor1;
  p.gloss = gloss; p.B = B; p.n = s1 ? 2 : 1;
  lgm_note_kernel("gan_bce_bwd_kernel");
  hipLaunchKernelGGL(gan_bce_bwd_kernel, dim3(lgm_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, p);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
