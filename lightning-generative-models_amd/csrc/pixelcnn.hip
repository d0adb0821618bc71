// Gated PixelCNN prior over the VQ-VAE's codes (reference models/generative/autoregressive/pixelcnn.py): masked k x k
// convolutions that touch the LIVE taps only, the gate, the per-position cross-entropy, and the two kernels of incremental
// sampling (one layer at one position; the categorical draw).
//
// A type-A / type-B mask keeps the taps whose row-major index kh * k + kw is below L = (k / 2) * k + k / 2 + [type B]: the
// live taps are a PREFIX of the tap axis of the physical weight [Nw][k * k][Cw], so a kernel that stops at tap L - 1 never
// reads a dead tap and needs no mask.  All products run on v_mfma_f32_32x32x2_f32 (exact fp32, one rounding per product);
// one wave owns a 32 x 32 (or 32 x 64) output tile and walks its whole reduction alone, in a fixed order: no split, no
// atomics, nothing that depends on lgm_set_cu_margin.  Operands are read with 16-byte loads where the reduction axis is the
// contiguous one (the forward's x and w, the input gradient's gy), else with 4-byte loads that are contiguous across lanes.
// The order of the reduction inside a group of 8 channels is (c + 4 (lane / 32) + j), j = 0 .. 3: A and B use the same map.
#include "lgm_common.h"

namespace lgmpcnn {

struct MGeom {
  int B, H, W, C, N, K, pad, T, L;
  long M;      // B * H * W
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// accumulator register i of lane half lh holds tile row (i & 3) + 8 (i >> 2) + 4 lh, tile column lane & 31
__device__ __forceinline__ int acc_row(int i, int lh) { return (i & 3) + 8 * (i >> 2) + 4 * lh; }

// ---- forward: y[m, n] = bias[n] + sum_{t < L} sum_c x[m + d(t), c] w[n][t][c] ---------------------------------------------
// block = 4 waves as 2 (rows) x 2 (columns); a wave owns 32 positions x 32 NT output channels
template <int NT>
__global__ __launch_bounds__(256) void mconv_xy_kernel(MGeom g, const float* __restrict__ x, long x_pitch,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ y, long y_pitch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const long m0 = ((long)blockIdx.x * 2 + (wid & 1)) * 32;
  const int n0 = (blockIdx.y * 2 + (wid >> 1)) * 32 * NT;
  if (m0 >= g.M || n0 >= g.N) return;
  const long m = m0 + r;
  const bool vm = m < g.M;
  const int HW = g.H * g.W;
  const int b = vm ? (int)(m / HW) : 0, rem = vm ? (int)(m % HW) : 0, oh = rem / g.W, ow = rem % g.W;
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = zero16();
  for (int t = 0; t < g.L; ++t) {
    const int ih = oh + t / g.K - g.pad, iw = ow + t % g.K - g.pad;
    const bool ok = vm && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
    if (!__any(ok)) continue;
    const float* xp = x + (((long)b * g.H + (ok ? ih : 0)) * g.W + (ok ? iw : 0)) * x_pitch;
    for (int c0 = 0; c0 < g.C; c0 += 8) {
      const int cc = c0 + 4 * lh;
      const f32x4 a = (ok && cc < g.C) ? ld4(xp + cc) : zero4();
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + 32 * j + r;
        const f32x4 bv = (n < g.N && cc < g.C) ? ld4(w + ((long)n * g.T + t) * g.C + cc) : zero4();
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j] = mfma(a[e], bv[e], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + 32 * j + r;
    if (n >= g.N) continue;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long mr = m0 + acc_row(i, lh);
      if (mr < g.M) y[mr * y_pitch + n] = acc[j][i] + bn;
    }
  }
}

// ---- input gradient: gx[m, c] = res[m, c] + sum_{t < L} sum_n gy[m - d(t), n] w[n][t][c] -----------------------------------
template <int NT>
__global__ __launch_bounds__(256) void mconv_yx_kernel(MGeom g, const float* __restrict__ gy, long gy_pitch,
                                                       const float* __restrict__ w, const float* res, long res_pitch,
                                                       float* gx, long gx_pitch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const long m0 = ((long)blockIdx.x * 2 + (wid & 1)) * 32;
  const int c0 = (blockIdx.y * 2 + (wid >> 1)) * 32 * NT;
  if (m0 >= g.M || c0 >= g.C) return;
  const long m = m0 + r;
  const bool vm = m < g.M;
  const int HW = g.H * g.W;
  const int b = vm ? (int)(m / HW) : 0, rem = vm ? (int)(m % HW) : 0, ih = rem / g.W, iw = rem % g.W;
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = zero16();
  for (int t = 0; t < g.L; ++t) {
    const int oh = ih - t / g.K + g.pad, ow = iw - t % g.K + g.pad;
    const bool ok = vm && oh >= 0 && oh < g.H && ow >= 0 && ow < g.W;
    if (!__any(ok)) continue;
    const float* yp = gy + (((long)b * g.H + (ok ? oh : 0)) * g.W + (ok ? ow : 0)) * gy_pitch;
    for (int k0 = 0; k0 < g.N; k0 += 8) {
      const int nn = k0 + 4 * lh;
      const f32x4 a = (ok && nn < g.N) ? ld4(yp + nn) : zero4();
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int c = c0 + 32 * j + r;
        f32x4 bv = zero4();
        if (c < g.C && nn < g.N) {
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[e] = w[((long)(nn + e) * g.T + t) * g.C + c];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j] = mfma(a[e], bv[e], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = c0 + 32 * j + r;
    if (c >= g.C) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long mr = m0 + acc_row(i, lh);
      if (mr < g.M) gx[mr * gx_pitch + c] = res ? acc[j][i] + res[mr * res_pitch + c] : acc[j][i];
    }
  }
}

// ---- weight gradient: gw[n][t][c] = beta gw + sum_m gy[m, n] x[m + d(t), c], t < L; positions in ascending order ----------
// blockIdx.x = tap + L * split; a wave owns 32 output channels x 32 NT input channels of that tap over the split's run of
// positions.  The split count is a function of the geometry alone (mconv_wgrad_splits): slabs, added in ascending order.
template <int NT>
__global__ __launch_bounds__(256) void mconv_wgrad_kernel(MGeom g, const float* __restrict__ gy, long gy_pitch,
                                                          const float* __restrict__ x, long x_pitch, float* gw, float beta,
                                                          float* __restrict__ slabs, long chunk) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const int t = blockIdx.x % g.L, split = blockIdx.x / g.L;
  const int n0 = (blockIdx.y * 2 + (wid & 1)) * 32;
  const int c0 = (blockIdx.z * 2 + (wid >> 1)) * 32 * NT;
  if (n0 >= g.N || c0 >= g.C) return;
  const int dh = t / g.K - g.pad, dw = t % g.K - g.pad, HW = g.H * g.W;
  const int n = n0 + r;
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = zero16();
  const long m_lo = split * chunk, m_hi = m_lo + chunk < g.M ? m_lo + chunk : g.M;      // chunk % 8 == 0
  for (long k0 = m_lo; k0 < m_hi; k0 += 8) {
    const long mm = k0 + 4 * lh;
    float a[4];
    long xoff[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long me = mm + e;
      const bool vm = me < m_hi;
      a[e] = (vm && n < g.N) ? gy[me * gy_pitch + n] : 0.f;
      const int b = vm ? (int)(me / HW) : 0, rem = vm ? (int)(me % HW) : 0;
      const int ih = rem / g.W + dh, iw = rem % g.W + dw;
      xoff[e] = (vm && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) ? (((long)b * g.H + ih) * g.W + iw) * x_pitch : -1;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int c = c0 + 32 * j + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float bv = (xoff[e] >= 0 && c < g.C) ? x[xoff[e] + c] : 0.f;
        acc[j] = mfma(a[e], bv, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = c0 + 32 * j + r;
    if (c >= g.C) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int nr = n0 + acc_row(i, lh);
      if (nr >= g.N) continue;
      if (slabs) {
        slabs[(((long)split * g.N + nr) * g.L + t) * g.C + c] = acc[j][i];
        continue;
      }
      float* o = gw + ((long)nr * g.T + t) * g.C + c;
      *o = beta != 0.f ? __fadd_rn(__fmul_rn(beta, *o), acc[j][i]) : acc[j][i];
    }
  }
}

// gw[n][t][c] = beta gw + slab_0 + slab_1 + ... (ascending), t < L
__global__ __launch_bounds__(256) void mconv_wgrad_reduce_kernel(MGeom g, const float* __restrict__ slabs, int splits, float* gw,
                                                                 float beta) {
  const long per = (long)g.N * g.L * g.C;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float s = slabs[i];
  for (int k = 1; k < splits; ++k) s += slabs[k * per + i];
  const long n = i / ((long)g.L * g.C), rest = i % ((long)g.L * g.C);
  float* o = gw + n * g.T * g.C + rest;
  *o = beta != 0.f ? __fadd_rn(__fmul_rn(beta, *o), s) : s;
}

// bias gradient gb[n] = beta gb + sum_m gy[m, n]: 16 row groups x 16 columns a block, each group in ascending order, the
// 16 partial sums combined in ascending order
__global__ __launch_bounds__(256) void mconv_bias_grad_kernel(const float* __restrict__ gy, long gy_pitch, long M, int N,
                                                              float* gb, float beta) {
  __shared__ float sh[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + tx;
  float s = 0.f;
  if (n < N)
    for (long m = ty; m < M; m += 16) s += gy[m * gy_pitch + n];
  sh[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && n < N) {
    float tot = 0.f;
    for (int i = 0; i < 16; ++i) tot += sh[i][tx];
    gb[n] = beta != 0.f ? __fadd_rn(__fmul_rn(beta, gb[n]), tot) : tot;
  }
}

// beta == 0: the dead taps of the gradient are exact zeros
__global__ __launch_bounds__(256) void mconv_dead_zero_kernel(float* gw, int N, int T, int L, int C) {
  const long per = (long)(T - L) * C, total = (long)N * per;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / per, o = i % per;
  gw[(n * T + L) * C + o] = 0.f;
}

// ---- gate: y = x + tanh(a) sigmoid(b), (a, b) = lanes [0, H) and [H, 2H) of the convolution output -------------------------
__device__ __forceinline__ float sigmoidf_(float v) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-v))); }

__global__ __launch_bounds__(256) void gated_fwd_kernel(const float* __restrict__ x, long x_pitch, const float* __restrict__ pre,
                                                        long pre_pitch, long M, int H, float* __restrict__ y, long y_pitch) {
  const int H4 = H >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * H4) return;
  const long m = i / H4;
  const int h = (int)(i % H4) * 4;
  const f32x4 xv = ld4(x + m * x_pitch + h), a = ld4(pre + m * pre_pitch + h), b = ld4(pre + m * pre_pitch + H + h);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(xv[e], __fmul_rn(tanhf(a[e]), sigmoidf_(b[e])));
  *reinterpret_cast<f32x4*>(y + m * y_pitch + h) = o;
}

// ga = gy s (1 - t^2), gb = gy t (s (1 - s)) over (a, b) (gpre may be pre itself); gx += gy where gx is given
__global__ __launch_bounds__(256) void gated_bwd_kernel(const float* __restrict__ gy, long gy_pitch, const float* pre,
                                                        long pre_pitch, long M, int H, float* gx, long gx_pitch, float* gpre,
                                                        long gpre_pitch) {
  const int H4 = H >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * H4) return;
  const long m = i / H4;
  const int h = (int)(i % H4) * 4;
  const f32x4 g = ld4(gy + m * gy_pitch + h), a = ld4(pre + m * pre_pitch + h), b = ld4(pre + m * pre_pitch + H + h);
  f32x4 ga, gb;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = tanhf(a[e]), s = sigmoidf_(b[e]);
    ga[e] = __fmul_rn(__fmul_rn(g[e], s), __fsub_rn(1.f, __fmul_rn(t, t)));
    gb[e] = __fmul_rn(__fmul_rn(g[e], t), __fmul_rn(s, __fsub_rn(1.f, s)));
  }
  *reinterpret_cast<f32x4*>(gpre + m * gpre_pitch + h) = ga;
  *reinterpret_cast<f32x4*>(gpre + m * gpre_pitch + H + h) = gb;
  if (gx) {
    f32x4 o = ld4(gx + m * gx_pitch + h);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(o[e], g[e]);
    *reinterpret_cast<f32x4*>(gx + m * gx_pitch + h) = o;
  }
}

// ---- cross-entropy over K classes a row: one wave per row ---------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_xent_fwd_kernel(const float* __restrict__ logits, long pitch,
                                                               const int64_t* __restrict__ target, long M, int K,
                                                               float* __restrict__ loss_rows, float* __restrict__ lse_out) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* l = logits + m * pitch;
  float mx = -INFINITY;
  for (int k = lane; k < K; k += 64) mx = fmaxf(mx, l[k]);
  mx = lgm_wave_max(mx);
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += expf(l[k] - mx);
  s = lgm_wave_sum(s);
  const float lse = mx + logf(s);
  if (lane == 0) {
    const int64_t t = target[m];
    lse_out[m] = lse;
    loss_rows[m] = (t >= 0 && t < K) ? lse - l[t] : NAN;
  }
}

// mean of the per-row losses by one workgroup: thread i sums rows i, i + 1024, ... in ascending order, then the fixed tree
__global__ __launch_bounds__(1024) void xent_mean_kernel(const float* __restrict__ loss_rows, long M, float* __restrict__ mean) {
  __shared__ float sh[16];
  float s = 0.f;
  for (long m = threadIdx.x; m < M; m += 1024) s += loss_rows[m];
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) mean[0] = s / (float)M;
}

__global__ __launch_bounds__(256) void softmax_xent_bwd_kernel(const float* __restrict__ logits, long pitch,
                                                               const int64_t* __restrict__ target,
                                                               const float* __restrict__ lse, const float* __restrict__ gloss,
                                                               long M, int K, int lanes, float* __restrict__ out, long out_pitch) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* l = logits + m * pitch;
  const float g = gloss[0] / (float)M, ls = lse[m];
  const int64_t t = target[m];
  for (int k = lane; k < lanes; k += 64)
    out[m * out_pitch + k] = k < K ? __fmul_rn(expf(l[k] - ls) - (k == t ? 1.f : 0.f), g) : 0.f;
}

// ---- incremental step: one layer at the one position p = counter[0] ----------------------------------------------------------
// partial[t][b][n] = sum_c w[n][t][c] cache_in[b, p + d(t), c] for the taps whose source lies inside the map; the finishing
// kernel adds the planes of those taps in ascending order.  blockIdx.x = tap; a wave owns 32 samples x 32 output channels.
__global__ __launch_bounds__(256) void pixelcnn_step_partial_kernel(MGeom g, const float* __restrict__ cache, long pitch,
                                                                    const float* __restrict__ w,
                                                                    const int32_t* __restrict__ counter,
                                                                    float* __restrict__ partial) {
  const int p = counter[0], HW = g.H * g.W;
  if (p < 0 || p >= HW) return;
  const int t = blockIdx.x;
  const int ih = p / g.W + t / g.K - g.pad, iw = p % g.W + t % g.K - g.pad;
  if (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const int n0 = (blockIdx.y * 4 + wid) * 32, b0 = blockIdx.z * 32;
  if (n0 >= g.N) return;
  const int b = b0 + r, n = n0 + r;
  const float* xp = cache + ((long)(b < g.B ? b : 0) * HW + ih * g.W + iw) * pitch;
  const float* wp = w + ((long)(n < g.N ? n : 0) * g.T + t) * g.C;
  f32x16 acc = zero16();
  for (int c0 = 0; c0 < g.C; c0 += 8) {
    const int cc = c0 + 4 * lh;
    const f32x4 a = (b < g.B && cc < g.C) ? ld4(xp + cc) : zero4();
    const f32x4 bv = (n < g.N && cc < g.C) ? ld4(wp + cc) : zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma(a[e], bv[e], acc);
  }
  if (n >= g.N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int br = b0 + acc_row(i, lh);
    if (br < g.B) partial[((long)t * g.B + br) * g.N + n] = acc[i];
  }
}

__device__ __forceinline__ float step_sum(const MGeom& g, const float* partial, const float* bias, int p, int b, int n) {
  float s = 0.f;
  for (int t = 0; t < g.L; ++t) {
    const int ih = p / g.W + t / g.K - g.pad, iw = p % g.W + t % g.K - g.pad;
    if (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) continue;
    s += partial[((long)t * g.B + b) * g.N + n];
  }
  return bias ? s + bias[n] : s;
}

// out lanes: N (gate = 0) or N / 2 (gate: the residual is cache_in[b, p, h]); out is a [B, H, W, .] map written at p
// (at_p) or a [B, .] matrix
__global__ __launch_bounds__(256) void pixelcnn_step_finish_kernel(MGeom g, int gate, const float* __restrict__ cache, long pitch,
                                                                   const float* __restrict__ partial,
                                                                   const float* __restrict__ bias,
                                                                   const int32_t* __restrict__ counter, float* __restrict__ out,
                                                                   long out_pitch, int at_p) {
  const int p = counter[0], HW = g.H * g.W;
  if (p < 0 || p >= HW) return;
  const int lanes = gate ? g.N / 2 : g.N;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)g.B * lanes) return;
  const int b = (int)(i / lanes), h = (int)(i % lanes);
  float v = step_sum(g, partial, bias, p, b, h);
  if (gate) {
    const float sb = step_sum(g, partial, bias, p, b, lanes + h);
    v = __fadd_rn(cache[((long)b * HW + p) * pitch + h], __fmul_rn(tanhf(v), sigmoidf_(sb)));
  }
  out[(at_p ? (long)b * HW + p : (long)b) * out_pitch + h] = v;
}

// ---- categorical draw: one wave per sample -------------------------------------------------------------------------------
// e_k = exp(z_k - max z), z = logits / temperature; lane i owns the classes [i chunk, (i + 1) chunk); cumulative sums run in
// ascending class order inside a lane, the lanes' offsets come from a fixed shuffle scan.  The draw is the first class with
// e_k > 0 whose cumulative sum exceeds u * total, else the last class with e_k > 0.
__global__ __launch_bounds__(64) void categorical_draw_kernel(const float* __restrict__ logits, long pitch, int B, int K,
                                                              float temperature, const float* __restrict__ u,
                                                              const float* __restrict__ codebook, long cb_pitch, int C, int HW,
                                                              const int32_t* __restrict__ counter, int64_t* __restrict__ codes,
                                                              float* __restrict__ xin, long xin_pitch) {
  const int p = counter[0];
  if (p < 0 || p >= HW) return;
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* l = logits + (long)b * pitch;
  const int chunk = (K + 63) / 64, k0 = min(K, lane * chunk), k1 = min(K, k0 + chunk);
  float mx = -INFINITY;
  for (int k = k0; k < k1; ++k) mx = fmaxf(mx, __fdiv_rn(l[k], temperature));
  mx = lgm_wave_max(mx);
  float local = 0.f;
  for (int k = k0; k < k1; ++k) local += expf(__fdiv_rn(l[k], temperature) - mx);
  float incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  float c = __shfl_up(incl, 1, 64);
  if (lane == 0) c = 0.f;
  const float thresh = __fmul_rn(u[b], __shfl(incl, 63, 64));
  int first = -1, last = -1;
  for (int k = k0; k < k1; ++k) {
    const float e = expf(__fdiv_rn(l[k], temperature) - mx);
    c += e;
    if (first < 0 && e > 0.f && c > thresh) first = k;      // (a lane's offset comes from the scan: never a class with e = 0)
    if (e > 0.f) last = k;
  }
  int idx = 0;
  const unsigned long long hit = __ballot(first >= 0), pos = __ballot(last >= 0);
  if (hit)
    idx = __shfl(first, __ffsll((long long)hit) - 1, 64);
  else if (pos)
    idx = __shfl(last, 63 - __clzll((long long)pos), 64);
  if (lane == 0) codes[(long)b * HW + p] = idx;
  float* xo = xin + ((long)b * HW + p) * xin_pitch;
  for (int ch = lane; ch < C; ch += 64) xo[ch] = codebook ? codebook[(long)idx * cb_pitch + ch] : (float)idx;
}

__global__ void pixelcnn_advance_kernel(int32_t* counter) { counter[0] += 1; }

// ---- host ------------------------------------------------------------------------------------------------------------------
static int make_geom(const char* who, const LgmConvGeom* g, int taps_live, MGeom* o) {
  LGM_REQUIRE(g && g->B > 0 && g->H > 0 && g->W > 0 && g->Cw > 0 && g->Nw > 0, "%s: empty geometry", who);
  LGM_REQUIRE(g->stride == 1 && g->KH == g->KW && (g->KH & 1) && g->pad == g->KH / 2 && g->Ho == g->H && g->Wo == g->W,
              "%s: stride 1, odd KH = KW and pad = KH / 2 expected", who);
  LGM_REQUIRE(taps_live >= 1 && taps_live <= g->KH * g->KW, "%s: taps_live %d outside [1, %d]", who, taps_live, g->KH * g->KW);
  LGM_REQUIRE(g->Cw % 4 == 0 && g->Nw % 4 == 0, "%s: channel counts must be multiples of 4", who);
  LGM_REQUIRE((long)g->B * g->H * g->W < (1L << 31), "%s: too many positions", who);
  *o = MGeom{g->B, g->H, g->W, g->Cw, g->Nw, g->KH, g->pad, g->KH * g->KW, taps_live, (long)g->B * g->H * g->W};
  return LGM_OK;
}
// runs of 2048 positions, at most 16: from the geometry alone, never from the CU budget
static const long WGRAD_CHUNK = 2048;
static int mconv_wgrad_splits(const MGeom& m) { return (int)((m.M + WGRAD_CHUNK - 1) / WGRAD_CHUNK > 16 ? 16 : (m.M + WGRAD_CHUNK - 1) / WGRAD_CHUNK); }
static bool pitched(const void* p, long pitch, int lanes) { return lgm_aligned16(p) && pitch % 4 == 0 && pitch >= lanes; }

}  // namespace lgmpcnn

using namespace lgmpcnn;

extern "C" {

int lgm_mconv_xy(const LgmConvGeom* g, int taps_live, const float* x, int64_t x_pitch, const float* w, const float* bias,
                 float* y, int64_t y_pitch, void* stream) {
  MGeom m;
  if (int rc = make_geom(__func__, g, taps_live, &m)) return rc;
  LGM_REQUIRE(x && w && y && pitched(x, x_pitch, m.C) && pitched(y, y_pitch, m.N) && lgm_aligned16(w),
              "lgm_mconv_xy: 16-byte aligned operands with pitch %% 4 == 0 expected");
  hipStream_t s = (hipStream_t)stream;
  if (m.N > 32)
    mconv_xy_kernel<2><<<dim3(lgm_cdiv(m.M, 64), lgm_cdiv(m.N, 128)), 256, 0, s>>>(m, x, x_pitch, w, bias, y, y_pitch);
  else
    mconv_xy_kernel<1><<<dim3(lgm_cdiv(m.M, 64), lgm_cdiv(m.N, 64)), 256, 0, s>>>(m, x, x_pitch, w, bias, y, y_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int lgm_mconv_yx(const LgmConvGeom* g, int taps_live, const float* gy, int64_t gy_pitch, const float* w, const float* res,
                 int64_t res_pitch, float* gx, int64_t gx_pitch, void* stream) {
  MGeom m;
  if (int rc = make_geom(__func__, g, taps_live, &m)) return rc;
  LGM_REQUIRE(gy && w && gx && pitched(gy, gy_pitch, m.N) && pitched(gx, gx_pitch, m.C) && lgm_aligned16(w) &&
              (!res || pitched(res, res_pitch, m.C)), "lgm_mconv_yx: 16-byte aligned operands with pitch %% 4 == 0 expected");
  hipStream_t s = (hipStream_t)stream;
  if (m.C > 32)
    mconv_yx_kernel<2><<<dim3(lgm_cdiv(m.M, 64), lgm_cdiv(m.C, 128)), 256, 0, s>>>(m, gy, gy_pitch, w, res, res_pitch, gx, gx_pitch);
  else
    mconv_yx_kernel<1><<<dim3(lgm_cdiv(m.M, 64), lgm_cdiv(m.C, 64)), 256, 0, s>>>(m, gy, gy_pitch, w, res, res_pitch, gx, gx_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int64_t lgm_mconv_wgrad_workspace(const LgmConvGeom* g, int taps_live) {
  MGeom m;
  if (make_geom(__func__, g, taps_live, &m)) return 0;
  const int splits = mconv_wgrad_splits(m);
  return splits > 1 ? (int64_t)splits * m.N * m.L * m.C * (int64_t)sizeof(float) : 0;
}

int lgm_mconv_wgrad(const LgmConvGeom* g, int taps_live, const float* gy, int64_t gy_pitch, const float* x, int64_t x_pitch,
                    float* gw, float* gbias, float beta, void* workspace, int64_t workspace_bytes, void* stream) {
  MGeom m;
  if (int rc = make_geom(__func__, g, taps_live, &m)) return rc;
  LGM_REQUIRE(gy && x && gw && pitched(gy, gy_pitch, m.N) && pitched(x, x_pitch, m.C),
              "lgm_mconv_wgrad: 16-byte aligned operands with pitch %% 4 == 0 expected");
  const int splits = mconv_wgrad_splits(m);
  const long chunk = splits > 1 ? (lgm_cdiv(m.M, splits) + 7) / 8 * 8 : m.M;
  LGM_REQUIRE(splits == 1 || (workspace && workspace_bytes >= lgm_mconv_wgrad_workspace(g, taps_live)),
              "lgm_mconv_wgrad: workspace of lgm_mconv_wgrad_workspace() bytes expected");
  float* slabs = splits > 1 ? (float*)workspace : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (m.C > 32)
    mconv_wgrad_kernel<2><<<dim3(m.L * splits, lgm_cdiv(m.N, 64), lgm_cdiv(m.C, 128)), 256, 0, s>>>(m, gy, gy_pitch, x, x_pitch, gw,
                                                                                                  beta, slabs, chunk);
  else
    mconv_wgrad_kernel<1><<<dim3(m.L * splits, lgm_cdiv(m.N, 64), lgm_cdiv(m.C, 64)), 256, 0, s>>>(m, gy, gy_pitch, x, x_pitch, gw,
                                                                                                 beta, slabs, chunk);
  LGM_LAUNCH_CHECK();
  if (slabs) {
    mconv_wgrad_reduce_kernel<<<lgm_cdiv((long)m.N * m.L * m.C, 256), 256, 0, s>>>(m, slabs, splits, gw, beta);
    LGM_LAUNCH_CHECK();
  }
  if (beta == 0.f && m.L < m.T) {
    const long total = (long)m.N * (m.T - m.L) * m.C;
    mconv_dead_zero_kernel<<<lgm_cdiv(total, 256), 256, 0, s>>>(gw, m.N, m.T, m.L, m.C);
    LGM_LAUNCH_CHECK();
  }
  if (gbias) {
    mconv_bias_grad_kernel<<<lgm_cdiv(m.N, 16), 256, 0, s>>>(gy, gy_pitch, m.M, m.N, gbias, beta);
    LGM_LAUNCH_CHECK();
  }
  return LGM_OK;
}

int lgm_mconv_zero_dead(const LgmConvGeom* g, int taps_live, float* gw, void* stream) {
  MGeom m;
  if (int rc = make_geom(__func__, g, taps_live, &m)) return rc;
  LGM_REQUIRE(gw, "lgm_mconv_zero_dead: gw expected");
  if (m.L < m.T) {
    const long total = (long)m.N * (m.T - m.L) * m.C;
    mconv_dead_zero_kernel<<<lgm_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(gw, m.N, m.T, m.L, m.C);
    LGM_LAUNCH_CHECK();
  }
  return LGM_OK;
}

int lgm_gated_fwd(const float* x, int64_t x_pitch, const float* pre, int64_t pre_pitch, int64_t M, int H, float* y,
                  int64_t y_pitch, void* stream) {
  LGM_REQUIRE(M > 0 && H > 0 && H % 4 == 0 && M * (H / 4) < (1L << 39), "lgm_gated_fwd: M > 0 and H %% 4 == 0 expected");
  LGM_REQUIRE(x && pre && y && pitched(x, x_pitch, H) && pitched(pre, pre_pitch, 2 * H) && pitched(y, y_pitch, H),
              "lgm_gated_fwd: 16-byte aligned operands with pitch %% 4 == 0 expected");
  gated_fwd_kernel<<<lgm_cdiv(M * (H / 4), 256), 256, 0, (hipStream_t)stream>>>(x, x_pitch, pre, pre_pitch, M, H, y, y_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int lgm_gated_bwd(const float* gy, int64_t gy_pitch, const float* pre, int64_t pre_pitch, int64_t M, int H, float* gx,
                  int64_t gx_pitch, float* gpre, int64_t gpre_pitch, void* stream) {
  LGM_REQUIRE(M > 0 && H > 0 && H % 4 == 0 && M * (H / 4) < (1L << 39), "lgm_gated_bwd: M > 0 and H %% 4 == 0 expected");
  LGM_REQUIRE(gy && pre && gpre && pitched(gy, gy_pitch, H) && pitched(pre, pre_pitch, 2 * H) &&
              pitched(gpre, gpre_pitch, 2 * H) && (!gx || pitched(gx, gx_pitch, H)),
              "lgm_gated_bwd: 16-byte aligned operands with pitch %% 4 == 0 expected");
  gated_bwd_kernel<<<lgm_cdiv(M * (H / 4), 256), 256, 0, (hipStream_t)stream>>>(gy, gy_pitch, pre, pre_pitch, M, H, gx, gx_pitch,
                                                                                gpre, gpre_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int lgm_softmax_xent_fwd(const float* logits, int64_t pitch, const int64_t* target, int64_t M, int K, float* loss_rows,
                         float* lse, float* mean, void* stream) {
  LGM_REQUIRE(logits && target && loss_rows && lse && M > 0 && M < (1L << 31) && K > 0 && pitch >= K,
              "lgm_softmax_xent_fwd: M > 0, K > 0 and pitch >= K expected");
  hipStream_t s = (hipStream_t)stream;
  softmax_xent_fwd_kernel<<<lgm_cdiv(M, 4), 256, 0, s>>>(logits, pitch, target, M, K, loss_rows, lse);
  LGM_LAUNCH_CHECK();
  if (mean) {
    xent_mean_kernel<<<1, 1024, 0, s>>>(loss_rows, M, mean);
    LGM_LAUNCH_CHECK();
  }
  return LGM_OK;
}

int lgm_softmax_xent_bwd(const float* logits, int64_t pitch, const int64_t* target, const float* lse, const float* gloss,
                         int64_t M, int K, int lanes, float* glogits, int64_t g_pitch, void* stream) {
  LGM_REQUIRE(logits && target && lse && gloss && glogits && M > 0 && M < (1L << 31) && K > 0 && pitch >= K && lanes >= K &&
              g_pitch >= lanes, "lgm_softmax_xent_bwd: K <= lanes <= g_pitch and pitch >= K expected");
  softmax_xent_bwd_kernel<<<lgm_cdiv(M, 4), 256, 0, (hipStream_t)stream>>>(logits, pitch, target, lse, gloss, M, K, lanes,
                                                                           glogits, g_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int64_t lgm_pixelcnn_step_workspace(const LgmConvGeom* g, int taps_live) {
  if (!g || taps_live < 1 || g->B < 1 || g->Nw < 1) return 0;
  return (int64_t)taps_live * g->B * g->Nw * (int64_t)sizeof(float);
}

int lgm_pixelcnn_step(const LgmConvGeom* g, int taps_live, int gate, const float* cache_in, int64_t in_pitch, const float* w,
                      const float* bias, const int32_t* counter, float* out, int64_t out_pitch, int out_at_p, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  MGeom m;
  if (int rc = make_geom(__func__, g, taps_live, &m)) return rc;
  const int lanes = gate ? m.N / 2 : m.N;
  LGM_REQUIRE(cache_in && w && counter && out && pitched(cache_in, in_pitch, m.C) && lgm_aligned16(w) && out_pitch >= lanes,
              "lgm_pixelcnn_step: 16-byte aligned operands with pitch %% 4 == 0 expected");
  LGM_REQUIRE(!gate || (m.N % 2 == 0 && m.N / 2 <= m.C), "lgm_pixelcnn_step: the gate's residual needs Cw >= Nw / 2");
  LGM_REQUIRE(workspace && workspace_bytes >= lgm_pixelcnn_step_workspace(g, taps_live),
              "lgm_pixelcnn_step: workspace of lgm_pixelcnn_step_workspace() bytes expected");
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pixelcnn_step_partial_kernel<<<dim3(m.L, lgm_cdiv(m.N, 128), lgm_cdiv(m.B, 32)), 256, 0, s>>>(m, cache_in, in_pitch, w, counter,
                                                                                               partial);
  LGM_LAUNCH_CHECK();
  pixelcnn_step_finish_kernel<<<lgm_cdiv((long)m.B * lanes, 256), 256, 0, s>>>(m, gate, cache_in, in_pitch, partial, bias, counter,
                                                                               out, out_pitch, out_at_p);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int lgm_categorical_draw(const float* logits, int64_t pitch, int B, int K, float temperature, const float* u,
                         const float* codebook, int64_t cb_pitch, int C, int HW, int32_t* counter, int64_t* codes, float* xin,
                         int64_t xin_pitch, int advance, void* stream) {
  LGM_REQUIRE(logits && u && counter && codes && xin && B > 0 && K > 0 && C > 0 && HW > 0 && pitch >= K && xin_pitch >= C &&
              (!codebook || cb_pitch >= C), "lgm_categorical_draw: pitches must cover their lanes");
  LGM_REQUIRE(temperature > 0.f, "lgm_categorical_draw: temperature must be positive");
  hipStream_t s = (hipStream_t)stream;
  categorical_draw_kernel<<<B, 64, 0, s>>>(logits, pitch, B, K, temperature, u, codebook, cb_pitch, C, HW, counter, codes, xin,
                                           xin_pitch);
  LGM_LAUNCH_CHECK();
  if (advance) {
    pixelcnn_advance_kernel<<<1, 1, 0, s>>>(counter);
    LGM_LAUNCH_CHECK();
  }
  return LGM_OK;
}

}  // extern "C"
