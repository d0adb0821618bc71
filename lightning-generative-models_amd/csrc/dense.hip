// Fully connected layers with few rows (an MLP's batch: M = B from 1 to 512, K and N from 3 to about 1024), the MLP VAE's
// two latent heads with the reparameterisation and the KL terms, and its tanh + L1 reconstruction loss
// (reference models/generative/vae/vae.py:15-215).  DESIGN section 6 has the definitions and the rounding counts.
//
// dense_gemm_kernel<VECA>   C[M, No] = A[M, R] Bm[No, R]^T on v_mfma_f32_16x16x4_f32 (exact float32).  The forward pass calls
//   it with A = x, Bm = W [Np][Kp]; the input gradient with A = g, Bm = the transposed weight copy [Kp][Np] that
//   FlatParams.refresh_transposed keeps.  A workgroup (4 waves) owns 32 rows x 16 columns and one slice [r_lo, r_hi) of the
//   reduction; its waves deal the slice out in steps of 16 (wave w takes steps w, w + 4, ..), every lane loading 4
//   consecutive r of its row (one 16-byte load where the operand allows it, VECA, else 4 guarded scalar loads: the image
//   batch arrives as x.view(B, C S S), rows of 25 or 75 floats) which feed 4 MFMAs.  The weights are the traffic and are read
//   once per 32 rows; the chip is filled from N and from the reduction: grid = (No / 16, M / 32, splits).  The four waves'
//   accumulators are summed through LDS in wave order; a split launch leaves one plane per slice and dense_reduce_kernel sums
//   them in slice order and applies bias and activation.  The slice length depends on (M, No, R) alone - never on
//   lgm_cu_margin() - and nothing is summed by an atomic: eager, replayed and repeated runs give equal bits.
// dense_g_kernel            g = gy * act'(y) (act' read from the saved OUTPUT: LeakyReLU y > 0 ? 1 : slope, ReLU y > 0 ? 1 : 0,
//   tanh 1 - y^2) and
//   gb = beta gb + colsum(g): 16 columns x 16 row groups per workgroup, rows in ascending order inside a group, the groups in
//   order through LDS.
// dense_gw_kernel           gw[N, K] = beta gw + g^T x: one wave per 16 x 64 tile, the whole (short) reduction over the rows
//   in ascending order, 4 rows per MFMA.  Write-bound; no split.
// No workgroup waits for another one; every launch is bounds-guarded by (M, No, R) and reads neither a pad lane of an
// activation nor a padding row of a weight.
#include "lgm_common.h"

namespace {

constexpr int DN_BM = 32, DN_BN = 16, DN_STEP = 16, DN_SLICE = 64;    // DN_SLICE: 4 waves x one step
constexpr int DN_MAX_SPLITS = 32;
constexpr int DN_SLOTS = 256;                                         // workgroups the split plan aims at (a constant)

__device__ __forceinline__ float dn_act(float v, int act, float slope) {
  if (act == LGM_ACT_LRELU) return v > 0.f ? v : v * slope;
  if (act == LGM_ACT_TANH) return tanhf(v);
  if (act == LGM_ACT_RELU) return v > 0.f ? v : 0.f;
  return v;
}

__device__ __forceinline__ float dn_dact(float y, int act, float slope) {
#pragma clang fp contract(off)
  if (act == LGM_ACT_LRELU) return y > 0.f ? 1.f : slope;
  if (act == LGM_ACT_TANH) return 1.f - y * y;
  if (act == LGM_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  return 1.f;
}

struct GemmArgs {
  const float* a;      // [M, R], pitch a_pitch
  const float* bm;     // [No, R], pitch b_pitch (multiple of 4, 16-byte aligned base)
  const float* bias;   // [No] or null (unsplit launches only)
  float* out;          // unsplit: [M, out_pitch]; split: planes [splits][M][Nop]
  long a_pitch, b_pitch, out_pitch;
  int M, No, Nop, R, kper, splits, act;
  float slope;
};

// 4 consecutive reduction elements of one row, zero past r_hi
template <bool VEC>
__device__ __forceinline__ f32x4 dn_load4(const float* row, int r, int r_hi, bool row_ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok || r >= r_hi) return v;
  if (VEC) {
    v = *reinterpret_cast<const f32x4*>(row + r);
    if (r + 3 >= r_hi) {
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (r + i >= r_hi) v[i] = 0.f;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (r + i < r_hi) v[i] = row[r + i];
  }
  return v;
}

template <bool VECA>
__global__ __launch_bounds__(256) void dense_gemm_kernel(const GemmArgs p) {
  __shared__ float red[4][2][64][4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * DN_BN, m0 = blockIdx.y * DN_BM, s = blockIdx.z;
  const int r_lo = s * p.kper, r_hi = min(p.R, r_lo + p.kper);
  const bool two = m0 + 16 < p.M;                                     // wave-uniform: the second row tile holds rows
  const int ma = m0 + lr, mb = m0 + 16 + lr, n = n0 + lr;
  const bool a_ok = ma < p.M, b_ok = two && mb < p.M, n_ok = n < p.No;
  const float* arow = p.a + (long)ma * p.a_pitch;
  const float* brow = p.a + (long)mb * p.a_pitch;
  const float* wrow = p.bm + (long)n * p.b_pitch;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int r0 = r_lo + wid * DN_STEP; r0 < r_hi; r0 += 4 * DN_STEP) {
    const int r = r0 + 4 * lq;
    const f32x4 fw = dn_load4<true>(wrow, r, r_hi, n_ok);
    const f32x4 fa = dn_load4<VECA>(arow, r, r_hi, a_ok);
    f32x4 fb = {0.f, 0.f, 0.f, 0.f};
    if (two) fb = dn_load4<VECA>(brow, r, r_hi, b_ok);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fw[i], acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[i], fw[i], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[wid][0][lane][i] = acc0[i];
    red[wid][1][lane][i] = acc1[i];
  }
  __syncthreads();
  if (wid >= 2 || (wid == 1 && !two)) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v;
    {
#pragma clang fp contract(off)
      v = ((red[0][wid][lane][i] + red[1][wid][lane][i]) + red[2][wid][lane][i]) + red[3][wid][lane][i];
    }
    const int row = m0 + 16 * wid + 4 * lq + i, col = n0 + lr;
    if (row >= p.M || col >= p.Nop) continue;
    if (p.splits > 1) {
      p.out[((long)s * p.M + row) * p.Nop + col] = v;
    } else {
      float o = 0.f;
      if (col < p.No) o = dn_act(p.bias ? v + p.bias[col] : v, p.act, p.slope);
      p.out[(long)row * p.out_pitch + col] = o;
    }
  }
}

__global__ __launch_bounds__(256) void dense_reduce_kernel(const float* __restrict__ planes, const float* __restrict__ bias,
                                                           float* __restrict__ out, long out_pitch, int M, int No, int Nop,
                                                           int splits, int act, float slope) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long plane = (long)M * Nop;
  if (i >= plane) return;
  const int row = (int)(i / Nop), col = (int)(i - (long)row * Nop);
  float v = planes[i];
  for (int s = 1; s < splits; ++s) v = v + planes[s * plane + i];
  float o = 0.f;
  if (col < No) o = dn_act(bias ? v + bias[col] : v, act, slope);
  out[(long)row * out_pitch + col] = o;
}

// g (may be null) [M][Nop] = gy * act'(y), pad lanes 0;  gb (may be null) [Nop] = beta gb + colsum(g).  16 columns x 16 row
// groups per workgroup: group r sums rows r, r + 16, .. in ascending order, then the 16 groups are added in order
constexpr int DG_COLS = 16, DG_GROUPS = 16;
__global__ __launch_bounds__(256) void dense_g_kernel(const float* __restrict__ gy, long gy_pitch, const float* __restrict__ y,
                                                      long y_pitch, int M, int No, int Nop, int act, float slope,
                                                      float* __restrict__ g, float* __restrict__ gb, float beta) {
#pragma clang fp contract(off)
  __shared__ float sh[DG_GROUPS][DG_COLS];
  const int c = threadIdx.x % DG_COLS, rg = threadIdx.x / DG_COLS;
  const int col = blockIdx.x * DG_COLS + c;
  float sum = 0.f;
  if (col < Nop) {
#pragma unroll 4
    for (int m = rg; m < M; m += DG_GROUPS) {
      float v = 0.f;
      if (col < No) {
        v = gy[(long)m * gy_pitch + col];
        if (act != LGM_ACT_NONE) v = v * dn_dact(y[(long)m * y_pitch + col], act, slope);
      }
      if (g) g[(long)m * Nop + col] = v;
      sum = sum + v;
    }
  }
  sh[rg][c] = sum;
  __syncthreads();
  if (rg == 0 && gb && col < Nop) {
    float t = sh[0][c];
    for (int r = 1; r < DG_GROUPS; ++r) t = t + sh[r][c];
    gb[col] = beta == 0.f ? t : beta * gb[col] + t;
  }
}

// gw [Np][Kp] = beta gw + g^T x.  g [M, g_pitch] (N live columns), x [M, x_pitch] (K live columns).
__global__ __launch_bounds__(256) void dense_gw_kernel(const float* __restrict__ g, long g_pitch, const float* __restrict__ x,
                                                       long x_pitch, int M, int N, int Np, int K, int Kp, int tiles_k,
                                                       int tiles, float* __restrict__ gw, float beta) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tiles) return;                                             // whole waves leave; no barrier follows
  const int lr = lane & 15, lq = lane >> 4;
  const int n0 = (t / tiles_k) * 16, k0 = (t % tiles_k) * 64;
  const int n = n0 + lr;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // 16 rows per trip: the 20 loads of four MFMA steps are in flight together (one step per trip waited out a load's
  // latency 64 times at B = 256); the rows still enter the accumulators in ascending order
  for (int m0 = 0; m0 < M; m0 += 16) {
    float fa[4], fx[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + 4 * u + lq;
      const bool m_ok = m < M;
      fa[u] = (m_ok && n < N) ? g[(long)m * g_pitch + n] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 16 * j + lr;
        fx[u][j] = (m_ok && k < K) ? x[(long)m * x_pitch + k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u], fx[u][j], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = n0 + 4 * lq + i, k = k0 + 16 * j + lr;
      if (row >= Np || k >= Kp) continue;
      float* d = gw + (long)row * Kp + k;
      *d = beta == 0.f ? acc[j][i] : beta * *d + acc[j][i];
    }
}

// ---- the VAE's latent heads -------------------------------------------------------------------------------------------
constexpr int HEAD_MAX_L = 256;

// one workgroup per sample: 2 L dot products of length K (wave per output: lanes stride k, fixed shuffle tree), then
// z = mu + eps exp(log_var / 2) and the sample's sum of 1 + log_var - mu^2 - exp(log_var), latent index ascending
__global__ __launch_bounds__(256) void vae_head_fwd_kernel(const float* __restrict__ h, long h_pitch,
                                                           const float* __restrict__ w_mu, const float* __restrict__ b_mu,
                                                           const float* __restrict__ w_lv, const float* __restrict__ b_lv,
                                                           const float* __restrict__ eps, int K, int Kp, int L, int Lp,
                                                           float* __restrict__ mu, float* __restrict__ log_var,
                                                           float* __restrict__ z, float* __restrict__ kld_part) {
  __shared__ float pre[2 * HEAD_MAX_L];
  __shared__ float term[HEAD_MAX_L];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float* hr = h + (long)b * h_pitch;
  for (int j = wid; j < 2 * L; j += 4) {
    const float* wr = j < L ? w_mu + (long)j * Kp : w_lv + (long)(j - L) * Kp;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(hr[k], wr[k], acc);
    acc = lgm_wave_sum(acc);
    if (lane == 0) pre[j] = acc + (j < L ? b_mu[j] : b_lv[j - L]);
  }
  __syncthreads();
  const int t = threadIdx.x;
  for (int j = t; j < Lp; j += 256) {
#pragma clang fp contract(off)
    float m = 0.f, v = 0.f, zz = 0.f;
    if (j < L) {
      m = pre[j], v = pre[L + j];
      zz = m + eps[(long)b * L + j] * expf(0.5f * v);
      term[j] = ((1.f + v) - m * m) - expf(v);
    }
    mu[(long)b * Lp + j] = m;
    log_var[(long)b * Lp + j] = v;
    z[(long)b * Lp + j] = zz;
  }
  __syncthreads();
  if (t == 0) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int j = 0; j < L; ++j) s = s + term[j];
    kld_part[b] = s;
  }
}

// gmu = gz + c mu,  glv = gz eps 0.5 exp(log_var / 2) + c 0.5 (exp(log_var) - 1),  c = kld_weight gloss / (B L)
__global__ __launch_bounds__(256) void vae_head_g_kernel(const float* __restrict__ gz, const float* __restrict__ mu,
                                                         const float* __restrict__ log_var, const float* __restrict__ eps,
                                                         const float* __restrict__ gloss, float kld_weight, int B, int L,
                                                         int Lp, float* __restrict__ gmu, float* __restrict__ glv) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Lp) return;
  const int b = (int)(i / Lp), j = (int)(i - (long)b * Lp);
  float a = 0.f, c2 = 0.f;
  if (j < L) {
    const float c = kld_weight * gloss[0] / (float)((long)B * L);
    const float g = gz[i], v = log_var[i];
    a = g + c * mu[i];
    c2 = ((g * eps[(long)b * L + j]) * 0.5f) * expf(0.5f * v) + (c * 0.5f) * (expf(v) - 1.f);
  }
  gmu[i] = a;
  glv[i] = c2;
}

// gh[b, k] = sum_j gmu[b, j] Wmu[j, k] + sum_j glv[b, j] Wlv[j, k]: one fmaf chain, j ascending, the mu head first
__global__ __launch_bounds__(256) void vae_head_gh_kernel(const float* __restrict__ gmu, const float* __restrict__ glv,
                                                          const float* __restrict__ w_mu, const float* __restrict__ w_lv,
                                                          int B, int K, int Kp, int L, int Lp, float* __restrict__ gh,
                                                          long gh_pitch) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Kp) return;
  const int b = (int)(i / Kp), k = (int)(i - (long)b * Kp);
  float acc = 0.f;
  if (k < K) {
    for (int j = 0; j < L; ++j) acc = fmaf(gmu[(long)b * Lp + j], w_mu[(long)j * Kp + k], acc);
    for (int j = 0; j < L; ++j) acc = fmaf(glv[(long)b * Lp + j], w_lv[(long)j * Kp + k], acc);
  }
  gh[(long)b * gh_pitch + k] = acc;
}

// ---- tanh + L1 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tanh_l1_fwd_kernel(const float* __restrict__ pre, long pre_pitch,
                                                          const float* __restrict__ x, long x_pitch, int D, int Dp,
                                                          float* __restrict__ xh, long xh_pitch, float* __restrict__ row_part) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int d = threadIdx.x; d < Dp; d += 256) {
    float o = 0.f;
    if (d < D) {
      o = tanhf(pre[(long)b * pre_pitch + d]);
      s = s + fabsf(o - x[(long)b * x_pitch + d]);
    }
    xh[(long)b * xh_pitch + d] = o;
  }
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) row_part[b] = s;
}

__global__ __launch_bounds__(256) void tanh_l1_bwd_kernel(const float* __restrict__ xh, long xh_pitch,
                                                          const float* __restrict__ x, long x_pitch,
                                                          const float* __restrict__ gloss, int B, int D, int Dp,
                                                          float* __restrict__ gpre, long gpre_pitch) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Dp) return;
  const int b = (int)(i / Dp), d = (int)(i - (long)b * Dp);
  float o = 0.f;
  if (d < D) {
    const float c = gloss[0] / (float)((long)B * D);
    const float v = xh[(long)b * xh_pitch + d], df = v - x[(long)b * x_pitch + d];
    const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
    o = (sg * c) * (1.f - v * v);
  }
  gpre[(long)b * gpre_pitch + d] = o;
}

// vals3 = (recon + kld_weight kld, recon, kld): recon = sum(row_part) / (B D), kld = -0.5 sum(kld_part) / (B L); one wave,
// lane l sums samples l, l + 64, .. in order, then the fixed shuffle tree
__global__ __launch_bounds__(64) void vae_loss_kernel(const float* __restrict__ row_part, const float* __restrict__ kld_part,
                                                      int B, int D, int L, float kld_weight, float* __restrict__ vals3) {
#pragma clang fp contract(off)
  float r = 0.f, k = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    r = r + row_part[b];
    k = k + kld_part[b];
  }
  r = lgm_wave_sum(r);
  k = lgm_wave_sum(k);
  if (threadIdx.x == 0) {
    const float recon = r / (float)((long)B * D);
    const float kld = -0.5f * (k / (float)((long)B * L));
    vals3[0] = recon + kld_weight * kld;
    vals3[1] = recon;
    vals3[2] = kld;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
inline int r4(int n) { return (n + 3) / 4 * 4; }

// slices of the reduction: enough workgroups for DN_SLOTS, whole DN_SLICE units; a function of the shape alone
void split_plan(int M, int No, int R, int* kper, int* splits) {
  const long tiles = (long)lgm_cdiv(No, DN_BN) * lgm_cdiv(M, DN_BM);
  long want = DN_SLOTS / tiles;
  if (want < 1) want = 1;
  if (want > DN_MAX_SPLITS) want = DN_MAX_SPLITS;
  int per = lgm_cdiv(lgm_cdiv(R, want), DN_SLICE) * DN_SLICE;
  *kper = per;
  *splits = lgm_cdiv(R, per);
}

int64_t gemm_workspace(int M, int No, int R) {
  int kper, splits;
  split_plan(M, No, R, &kper, &splits);
  return splits > 1 ? (int64_t)splits * M * r4(No) * (int64_t)sizeof(float) : 0;
}

// C = act(A Bm^T + bias); `planes` holds gemm_workspace(M, No, R) bytes
int launch_gemm(const char* who, const float* a, long a_pitch, const float* bm, long b_pitch, const float* bias, int M, int No,
                int R, int act, float slope, float* out, long out_pitch, float* planes, hipStream_t st) {
  GemmArgs p{};
  p.a = a; p.bm = bm; p.a_pitch = a_pitch; p.b_pitch = b_pitch;
  p.M = M; p.No = No; p.Nop = r4(No); p.R = R; p.act = act; p.slope = slope;
  split_plan(M, No, R, &p.kper, &p.splits);
  if (p.splits > 1) {
    p.out = planes; p.bias = nullptr; p.out_pitch = p.Nop;
  } else {
    p.out = out; p.bias = bias; p.out_pitch = out_pitch;
  }
  const dim3 grid(lgm_cdiv(No, DN_BN), lgm_cdiv(M, DN_BM), p.splits);
  const bool vec = lgm_aligned16(a) && a_pitch % 4 == 0;
  lgm_note_kernel(vec ? "dense_gemm_kernel<true>" : "dense_gemm_kernel<false>");
  if (vec) hipLaunchKernelGGL(dense_gemm_kernel<true>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(dense_gemm_kernel<false>, grid, dim3(256), 0, st, p);
  LGM_LAUNCH_CHECK_AS(who);
  if (p.splits > 1) {
    hipLaunchKernelGGL(dense_reduce_kernel, dim3(lgm_cdiv((long)M * p.Nop, 256)), dim3(256), 0, st, planes, bias, out, out_pitch,
                       M, No, p.Nop, p.splits, act, slope);
    LGM_LAUNCH_CHECK_AS(who);
  }
  return LGM_OK;
}

int launch_g(const char* who, const float* gy, long gy_pitch, const float* y, long y_pitch, int M, int No, int act, float slope,
             float* g, float* gb, float beta, hipStream_t st) {
  hipLaunchKernelGGL(dense_g_kernel, dim3(lgm_cdiv(r4(No), DG_COLS)), dim3(256), 0, st, gy, gy_pitch, y, y_pitch, M, No, r4(No), act,
                     slope, g, gb, beta);
  LGM_LAUNCH_CHECK_AS(who);
  return LGM_OK;
}

int launch_gw(const char* who, const float* g, long g_pitch, const float* x, long x_pitch, int M, int N, int K, float* gw,
              float beta, hipStream_t st) {
  const int Np = r4(N), Kp = r4(K);
  const int tiles_k = lgm_cdiv(Kp, 64), tiles = lgm_cdiv(Np, 16) * tiles_k;
  hipLaunchKernelGGL(dense_gw_kernel, dim3(lgm_cdiv(tiles, 4)), dim3(256), 0, st, g, g_pitch, x, x_pitch, M, N, Np, K, Kp,
                     tiles_k, tiles, gw, beta);
  LGM_LAUNCH_CHECK_AS(who);
  return LGM_OK;
}

bool act_ok(int act) { return act == LGM_ACT_NONE || act == LGM_ACT_LRELU || act == LGM_ACT_TANH || act == LGM_ACT_RELU; }
constexpr int DN_MAX_DIM = 1 << 20;

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), like lowres_cond_kernel's and for the same reason:
// tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it; tests/test_hip_vae.py runs these.

extern "C" int64_t lgm_dense_fwd_workspace(int B, int K, int N) {
  if (B < 1 || K < 1 || N < 1 || B > DN_MAX_DIM || K > DN_MAX_DIM || N > DN_MAX_DIM) return -1;
  return gemm_workspace(B, N, K);
}

extern "C" int lgm_dense_fwd(const float* x, int64_t x_pitch, const float* w, const float* bias, int B, int K, int N, int act,
                             float slope, float* y, int64_t y_pitch, void* workspace, int64_t workspace_bytes, void* stream) {
  LGM_REQUIRE(x && w && y, "dense_fwd: x, w and y required");
  LGM_REQUIRE(B >= 1 && K >= 1 && N >= 1 && B <= DN_MAX_DIM && K <= DN_MAX_DIM && N <= DN_MAX_DIM, "dense_fwd: B, K, N >= 1 required, got %d %d %d", B, K, N);
  LGM_REQUIRE(x_pitch >= K && y_pitch >= r4(N), "dense_fwd: pitches below the channel counts (x %ld < %d or y %ld < %d)",
              (long)x_pitch, K, (long)y_pitch, r4(N));
  LGM_REQUIRE(act_ok(act), "dense_fwd: act must be none, ReLU, LeakyReLU or tanh, got %d", act);
  LGM_REQUIRE(lgm_aligned16(w), "dense_fwd: 16-byte aligned weights required");
  LGM_REQUIRE((const void*)y != (const void*)x, "dense_fwd: y must not alias x");
  const int64_t need = gemm_workspace(B, N, K);
  LGM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "dense_fwd: workspace of %ld bytes required", (long)need);
  return launch_gemm("dense_fwd", x, (long)x_pitch, w, r4(K), bias, B, N, K, act, slope, y, (long)y_pitch, (float*)workspace,
                     (hipStream_t)stream);
}

// workspace: g [B][Np], then the planes of the input gradient
extern "C" int64_t lgm_dense_bwd_workspace(int B, int K, int N, int need_gx) {
  if (B < 1 || K < 1 || N < 1 || B > DN_MAX_DIM || K > DN_MAX_DIM || N > DN_MAX_DIM) return -1;
  return (int64_t)B * r4(N) * (int64_t)sizeof(float) + (need_gx ? gemm_workspace(B, K, N) : 0);
}

extern "C" int lgm_dense_bwd(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* x, int64_t x_pitch,
                             const float* wt, int B, int K, int N, int act, float slope, float* gx, int64_t gx_pitch, float* gw,
                             float* gb, float beta, void* workspace, int64_t workspace_bytes, void* stream) {
  LGM_REQUIRE(gy && x && gw && workspace, "dense_bwd: gy, x, gw and a workspace required");
  LGM_REQUIRE(B >= 1 && K >= 1 && N >= 1 && B <= DN_MAX_DIM && K <= DN_MAX_DIM && N <= DN_MAX_DIM, "dense_bwd: B, K, N >= 1 required, got %d %d %d", B, K, N);
  LGM_REQUIRE(act_ok(act), "dense_bwd: act must be none, ReLU, LeakyReLU or tanh, got %d", act);
  LGM_REQUIRE(act == LGM_ACT_NONE || y, "dense_bwd: the saved output y is required with an activation");
  LGM_REQUIRE(gy_pitch >= N && x_pitch >= K && (!y || y_pitch >= N), "dense_bwd: pitches below the channel counts");
  LGM_REQUIRE(!gx || (wt && lgm_aligned16(wt) && gx_pitch >= r4(K)),
              "dense_bwd: the input gradient needs the 16-byte aligned transposed weights [Kp][Np] and gx_pitch >= %d", r4(K));
  const int64_t need = lgm_dense_bwd_workspace(B, K, N, gx != nullptr);
  LGM_REQUIRE(workspace_bytes >= need && lgm_aligned16(workspace), "dense_bwd: 16-byte aligned workspace of %ld bytes required",
              (long)need);
  hipStream_t st = (hipStream_t)stream;
  const int Np = r4(N);
  float* g = (float*)workspace;
  int rc = launch_g("dense_bwd", gy, (long)gy_pitch, y, (long)y_pitch, B, N, act, slope, g, gb, beta, st);
  if (rc) return rc;
  if (gx) {
    rc = launch_gemm("dense_bwd", g, Np, wt, Np, nullptr, B, K, N, LGM_ACT_NONE, 0.f, gx, (long)gx_pitch, g + (long)B * Np, st);
    if (rc) return rc;
  }
  lgm_note_kernel("dense_gw_kernel");
  return launch_gw("dense_bwd", g, Np, x, (long)x_pitch, B, N, K, gw, beta, st);
}

// the input gradient alone (a sweep through a network whose parameters are not being updated): dense_g_kernel and
// dense_gemm_kernel as lgm_dense_bwd launches them, the same bits in gx; workspace of lgm_dense_bwd_workspace(B, K, N, 1)
extern "C" int lgm_dense_dgrad(const float* gy, int64_t gy_pitch, const float* y, int64_t y_pitch, const float* wt, int B, int K,
                               int N, int act, float slope, float* gx, int64_t gx_pitch, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  LGM_REQUIRE(gy && gx && wt && workspace, "dense_dgrad: gy, gx, wt and a workspace required");
  LGM_REQUIRE(B >= 1 && K >= 1 && N >= 1 && B <= DN_MAX_DIM && K <= DN_MAX_DIM && N <= DN_MAX_DIM, "dense_dgrad: B, K, N >= 1 required, got %d %d %d", B, K, N);
  LGM_REQUIRE(act_ok(act), "dense_dgrad: act must be none, ReLU, LeakyReLU or tanh, got %d", act);
  LGM_REQUIRE(act == LGM_ACT_NONE || y, "dense_dgrad: the saved output y is required with an activation");
  LGM_REQUIRE(gy_pitch >= N && (!y || y_pitch >= N), "dense_dgrad: pitches below the channel count %d", N);
  LGM_REQUIRE(lgm_aligned16(wt) && gx_pitch >= r4(K),
              "dense_dgrad: 16-byte aligned transposed weights [Kp][Np] and gx_pitch >= %d required", r4(K));
  const int64_t need = lgm_dense_bwd_workspace(B, K, N, 1);
  LGM_REQUIRE(workspace_bytes >= need && lgm_aligned16(workspace), "dense_dgrad: 16-byte aligned workspace of %ld bytes required",
              (long)need);
  hipStream_t st = (hipStream_t)stream;
  const int Np = r4(N);
  float* g = (float*)workspace;
  const int rc = launch_g("dense_dgrad", gy, (long)gy_pitch, y, (long)y_pitch, B, N, act, slope, g, nullptr, 0.f, st);
  if (rc) return rc;
  return launch_gemm("dense_dgrad", g, Np, wt, Np, nullptr, B, K, N, LGM_ACT_NONE, 0.f, gx, (long)gx_pitch, g + (long)B * Np, st);
}

extern "C" int lgm_vae_head_fwd(const float* h, int64_t h_pitch, const float* w_mu, const float* b_mu, const float* w_lv,
                                const float* b_lv, const float* eps, int B, int K, int L, float* mu, float* log_var, float* z,
                                float* kld_part, void* stream) {
  LGM_REQUIRE(h && w_mu && b_mu && w_lv && b_lv && eps && mu && log_var && z && kld_part, "vae_head_fwd: null argument");
  LGM_REQUIRE(B >= 1 && B <= DN_MAX_DIM && K >= 1 && K <= DN_MAX_DIM && L >= 1 && L <= HEAD_MAX_L,
              "vae_head_fwd: B >= 1, K >= 1 and 1 <= L <= %d required, got %d %d %d", HEAD_MAX_L, B, K, L);
  LGM_REQUIRE(h_pitch >= K, "vae_head_fwd: pitch %ld below the channel count %d", (long)h_pitch, K);
  lgm_note_kernel("vae_head_fwd_kernel");
  hipLaunchKernelGGL(vae_head_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, h, (long)h_pitch, w_mu, b_mu, w_lv, b_lv,
                     eps, K, r4(K), L, r4(L), mu, log_var, z, kld_part);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int64_t lgm_vae_head_bwd_workspace(int B, int L) {
  if (B < 1 || L < 1 || B > DN_MAX_DIM || L > HEAD_MAX_L) return -1;
  return 2 * (int64_t)B * r4(L) * (int64_t)sizeof(float);
}

extern "C" int lgm_vae_head_bwd(const float* gz, const float* mu, const float* log_var, const float* eps, const float* gloss,
                                float kld_weight, const float* h, int64_t h_pitch, const float* w_mu, const float* w_lv, int B,
                                int K, int L, float* gh, int64_t gh_pitch, float* gw_mu, float* gb_mu, float* gw_lv,
                                float* gb_lv, float beta, void* workspace, int64_t workspace_bytes, void* stream) {
  LGM_REQUIRE(gz && mu && log_var && eps && gloss && h && w_mu && w_lv && gh && gw_mu && gb_mu && gw_lv && gb_lv && workspace,
              "vae_head_bwd: null argument");
  LGM_REQUIRE(B >= 1 && B <= DN_MAX_DIM && K >= 1 && K <= DN_MAX_DIM && L >= 1 && L <= HEAD_MAX_L,
              "vae_head_bwd: B >= 1, K >= 1 and 1 <= L <= %d required, got %d %d %d", HEAD_MAX_L, B, K, L);
  LGM_REQUIRE(h_pitch >= K && gh_pitch >= r4(K), "vae_head_bwd: pitches below the channel count %d", K);
  LGM_REQUIRE(workspace_bytes >= lgm_vae_head_bwd_workspace(B, L), "vae_head_bwd: workspace of %ld bytes required",
              (long)lgm_vae_head_bwd_workspace(B, L));
  hipStream_t st = (hipStream_t)stream;
  const int Lp = r4(L), Kp = r4(K);
  float* gmu = (float*)workspace;
  float* glv = gmu + (long)B * Lp;
  lgm_note_kernel("vae_head_g_kernel");
  hipLaunchKernelGGL(vae_head_g_kernel, dim3(lgm_cdiv((long)B * Lp, 256)), dim3(256), 0, st, gz, mu, log_var, eps, gloss,
                     kld_weight, B, L, Lp, gmu, glv);
  LGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(vae_head_gh_kernel, dim3(lgm_cdiv((long)B * Kp, 256)), dim3(256), 0, st, gmu, glv, w_mu, w_lv, B, K, Kp, L,
                     Lp, gh, (long)gh_pitch);
  LGM_LAUNCH_CHECK();
  int rc = launch_g("vae_head_bwd", gmu, Lp, nullptr, 0, B, L, LGM_ACT_NONE, 0.f, nullptr, gb_mu, beta, st);
  if (rc) return rc;
  rc = launch_g("vae_head_bwd", glv, Lp, nullptr, 0, B, L, LGM_ACT_NONE, 0.f, nullptr, gb_lv, beta, st);
  if (rc) return rc;
  rc = launch_gw("vae_head_bwd", gmu, Lp, h, (long)h_pitch, B, L, K, gw_mu, beta, st);
  if (rc) return rc;
  return launch_gw("vae_head_bwd", glv, Lp, h, (long)h_pitch, B, L, K, gw_lv, beta, st);
}

extern "C" int lgm_tanh_l1_fwd(const float* pre, int64_t pre_pitch, const float* x, int64_t x_pitch, int B, int D, float* xh,
                               int64_t xh_pitch, float* row_part, void* stream) {
  LGM_REQUIRE(pre && x && xh && row_part, "tanh_l1_fwd: null argument");
  LGM_REQUIRE(B >= 1 && B <= DN_MAX_DIM && D >= 1 && D <= DN_MAX_DIM, "tanh_l1_fwd: B >= 1 and D >= 1 required, got %d %d", B, D);
  LGM_REQUIRE(pre_pitch >= D && x_pitch >= D && xh_pitch >= r4(D), "tanh_l1_fwd: pitches below the channel count %d", D);
  lgm_note_kernel("tanh_l1_fwd_kernel");
  hipLaunchKernelGGL(tanh_l1_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pre, (long)pre_pitch, x, (long)x_pitch, D,
                     r4(D), xh, (long)xh_pitch, row_part);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_tanh_l1_bwd(const float* xh, int64_t xh_pitch, const float* x, int64_t x_pitch, const float* gloss, int B,
                               int D, float* gpre, int64_t gpre_pitch, void* stream) {
  LGM_REQUIRE(xh && x && gloss && gpre, "tanh_l1_bwd: null argument");
  LGM_REQUIRE(B >= 1 && B <= DN_MAX_DIM && D >= 1 && D <= DN_MAX_DIM, "tanh_l1_bwd: B >= 1 and D >= 1 required, got %d %d", B, D);
  LGM_REQUIRE(xh_pitch >= D && x_pitch >= D && gpre_pitch >= r4(D), "tanh_l1_bwd: pitches below the channel count %d", D);
  lgm_note_kernel("tanh_l1_bwd_kernel");
  hipLaunchKernelGGL(tanh_l1_bwd_kernel, dim3(lgm_cdiv((long)B * r4(D), 256)), dim3(256), 0, (hipStream_t)stream, xh,
                     (long)xh_pitch, x, (long)x_pitch, gloss, B, D, r4(D), gpre, (long)gpre_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_vae_loss(const float* row_part, const float* kld_part, int B, int D, int L, float kld_weight, float* vals3,
                            void* stream) {
  LGM_REQUIRE(row_part && kld_part && vals3, "vae_loss: null argument");
  LGM_REQUIRE(B >= 1 && D >= 1 && L >= 1, "vae_loss: B, D, L >= 1 required, got %d %d %d", B, D, L);
  lgm_note_kernel("vae_loss_kernel");
  hipLaunchKernelGGL(vae_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_part, kld_part, B, D, L, kld_weight, vals3);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
