// Tiled full softmax attention (flash-style) for maps of more than 128 query pixels: the 12 x 12 (n = 144), 16 x 16
// (n = 256) and 32 x 32 (n = 1024) maps of the DDPM UNet at 96, 128 and 256 pixels.  Same operands and results as the
// one-workgroup-per-(batch, head) kernels of attention.hip: qkv [B, n, pitch] with channel = which*hidden + head*32 + d,
// M <= 16 memory rows (mem_kv [2, heads, M, 32]) in front of the n pixel keys, lse[(b*heads + h)*n + i] = ln sum_j
// exp(scale q_i . k_j) over memory and pixel keys, and the memory rows' gradient per image in part [B][2][heads][M][32].
//
// Products on v_mfma_f32_16x16x4_f32 (exact fp32).  A wave owns 16 rows; a workgroup (4 waves) owns a 64-row tile and
// stages 64-row tiles of the other side through LDS.  Products are oriented so that an accumulator register is already
// the B operand of the next product (lane l, register r of a 16 x 16 tile holds row 4*(l>>4) + r, column l&15; a
// 16x16x4 step reads B[k = l>>4][column l&15]): the four registers of a lane are the four k-steps that follow.
//
//   forward        one workgroup per (b, h, 64 queries).  S^T = K Q^T per 64-key tile (memory rows first), online
//                  softmax per query (running max and sum; the query is on the lane), O^T += V^T P^T.
//   backward       one launch, two roles with disjoint outputs, no atomics (bitwise reproducible):
//     dQ role      workgroup per (b, h, 64 queries), sweeps the key tiles: S^T, dP^T = V dO^T, P = exp(S - lse),
//                  dS = P (dP - delta), dQ^T += K^T dS^T.
//     dK/dV role   workgroup per (b, h, 64 keys), sweeps the query tiles: S = Q K^T, dP = dO V^T, dK^T += Q^T dS,
//                  dV^T += dO^T P.
//                  delta_i = dO_i . O_i is recomputed (one fixed-order function for both roles).
// Tails in either direction are zero-filled in registers / LDS and masked; any row pitch (scalar global accesses).
#include "lgm_common.h"

namespace {

constexpr int DH = 32;          // dim_head
constexpr int TT = 64;          // rows per tile (queries or keys), 16 per wave
constexpr int LD = DH + 1;      // LDS row pitch

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// key row j of (b, h): memory rows first, then pixels; nullptr past the end
__device__ __forceinline__ const float* key_row(const float* qkv, long pitch, const float* mem_kv, int b, int h, int n,
                                                int heads, int M, int j, int which) {
  if (j < M) return mem_kv + ((long)(which * heads + h) * M + j) * DH;
  if (j < n + M) return qkv + ((long)b * n + (j - M)) * pitch + (which + 1) * heads * DH + h * DH;
  return nullptr;
}

// stage keys [j0, j0 + 64) of K and V into LDS (zeros past the end)
__device__ __forceinline__ void stage_kv(const float* qkv, long pitch, const float* mem_kv, int b, int h, int n, int heads,
                                         int M, int j0, float* Ks, float* Vs) {
  for (int e = threadIdx.x; e < TT * DH; e += blockDim.x) {
    const int r = e / DH, d = e % DH;
    const float* kr = key_row(qkv, pitch, mem_kv, b, h, n, heads, M, j0 + r, 0);
    const float* vr = key_row(qkv, pitch, mem_kv, b, h, n, heads, M, j0 + r, 1);
    Ks[r * LD + d] = kr ? kr[d] : 0.f;
    Vs[r * LD + d] = vr ? vr[d] : 0.f;
  }
}

// delta_i = dO_i . O_i in a fixed order (the same bits in both backward roles)
__device__ __forceinline__ float row_delta(const float* g, const float* o) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) s = fmaf(g[d], o[d], s);
  return s;
}

__global__ __launch_bounds__(256) void attn_tiled_fwd_kernel(const float* __restrict__ qkv, long pitch,
                                                             const float* __restrict__ mem_kv, int n, int heads, int M,
                                                             float scale, float* __restrict__ out, long out_pitch,
                                                             float* __restrict__ lse) {
  __shared__ float Ks[TT * LD], Vs[TT * LD];
  const int bh = blockIdx.x, b = bh / heads, h = bh % heads, nk = n + M;
  const int lane = threadIdx.x & 63, ql = lane & 15, kg = lane >> 4;
  const int i = blockIdx.y * TT + (threadIdx.x >> 6) * 16 + ql;     // this lane's query
  float qf[8];                                                        // B operand of S^T = K Q^T: Q[i][4s + kg] * scale
  {
    const float* qr = qkv + ((long)b * n + i) * pitch + h * DH;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = i < n ? qr[4 * s + kg] * scale : 0.f;
  }
  f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};        // O^T[d = 16e + 4kg + r][query ql]
  float mx = -INFINITY, den = 0.f;
  for (int j0 = 0; j0 < nk; j0 += TT) {
    __syncthreads();
    stage_kv(qkv, pitch, mem_kv, b, h, n, heads, M, j0, Ks, Vs);
    __syncthreads();
    f32x4 st[4];                                                      // S^T[key 16t + 4kg + r][query ql]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) st[t] = mfma4(Ks[(16 * t + ql) * LD + 4 * s + kg], qf[s], st[t]);
    }
    float tm = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (j0 + 16 * t + 4 * kg + r >= nk) st[t][r] = -INFINITY;
        tm = fmaxf(tm, st[t][r]);
      }
    tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float nm = fmaxf(mx, tm);                                   // finite: key j0 < nk is in every tile
    const float corr = __expf(mx - nm);
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = __expf(st[t][r] - nm);
        ps += st[t][r];
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    den = den * corr + ps;
    mx = nm;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      o[e] *= corr;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[e] = mfma4(Vs[(16 * t + 4 * kg + r) * LD + 16 * e + ql], st[t][r], o[e]);
    }
  }
  if (i >= n) return;
  const float inv = 1.f / den;
  float* orow = out + ((long)b * n + i) * out_pitch + h * DH;
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int r = 0; r < 4; ++r) orow[16 * e + 4 * kg + r] = o[e][r] * inv;
  if (kg == 0) lse[(long)bh * n + i] = mx + __logf(den);
}

__global__ __launch_bounds__(256) void attn_tiled_bwd_kernel(const float* __restrict__ qkv, long pitch,
                                                             const float* __restrict__ mem_kv,
                                                             const float* __restrict__ out, long out_pitch,
                                                             const float* __restrict__ gout, long gout_pitch,
                                                             const float* __restrict__ lse, int n, int heads, int M,
                                                             float scale, int n_qtiles, float* __restrict__ gqkv,
                                                             long gq_pitch, float* __restrict__ gmem_partial) {
  __shared__ float sm[2 * TT * LD + 2 * TT];
  const int bh = blockIdx.x, b = bh / heads, h = bh % heads, nk = n + M, hidden = heads * DH;
  const int lane = threadIdx.x & 63, cl = lane & 15, kg = lane >> 4, w16 = (threadIdx.x >> 6) * 16;
  f32x4 acc[2][2] = {};
  if ((int)blockIdx.y < n_qtiles) {
    // ---- dQ role: this lane's query i = column cl of the transposed products ----
    float* Ks = sm;
    float* Vs = sm + TT * LD;
    const int i = blockIdx.y * TT + w16 + cl;
    float qf[8], gf[8], li = 0.f, di = 0.f;
    {
      const long row = (long)b * n + i;
      const float* qr = qkv + row * pitch + h * DH;
      const float* gr = gout + row * gout_pitch + h * DH;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        qf[s] = i < n ? qr[4 * s + kg] * scale : 0.f;
        gf[s] = i < n ? gr[4 * s + kg] : 0.f;
      }
      if (i < n) {
        li = lse[(long)bh * n + i];
        di = row_delta(gr, out + row * out_pitch + h * DH);
      }
    }
    for (int j0 = 0; j0 < nk; j0 += TT) {
      __syncthreads();
      stage_kv(qkv, pitch, mem_kv, b, h, n, heads, M, j0, Ks, Vs);
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};  // [key 16t + 4kg + r][query cl]
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          st = mfma4(Ks[(16 * t + cl) * LD + 4 * s + kg], qf[s], st);
          dp = mfma4(Vs[(16 * t + cl) * LD + 4 * s + kg], gf[s], dp);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = j0 + 16 * t + 4 * kg + r < nk ? __expf(st[r] - li) : 0.f;
          const float ds = p * (dp[r] - di);
#pragma unroll
          for (int e = 0; e < 2; ++e) acc[0][e] = mfma4(Ks[(16 * t + 4 * kg + r) * LD + 16 * e + cl], ds, acc[0][e]);
        }
      }
    }
    if (i >= n) return;
    float* gq = gqkv + ((long)b * n + i) * gq_pitch + h * DH;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) gq[16 * e + 4 * kg + r] = acc[0][e][r] * scale;
    return;
  }
  // ---- dK/dV role: this lane's key j = column cl of S = Q K^T ----
  float* Qs = sm;                 // [64][33] queries, pre-scaled
  float* Gs = sm + TT * LD;       // [64][33] dO
  float* Ls = Gs + TT * LD;       // [64] lse (+inf past n: P = 0)
  float* Ds = Ls + TT;            // [64] delta
  const int j = (blockIdx.y - n_qtiles) * TT + w16 + cl;
  float kf[8], vf[8];             // B operands: K[j][4s + kg], V[j][4s + kg]
  {
    const float* kr = key_row(qkv, pitch, mem_kv, b, h, n, heads, M, j, 0);
    const float* vr = key_row(qkv, pitch, mem_kv, b, h, n, heads, M, j, 1);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      kf[s] = kr ? kr[4 * s + kg] : 0.f;
      vf[s] = vr ? vr[4 * s + kg] : 0.f;
    }
  }
  for (int i0 = 0; i0 < n; i0 += TT) {
    __syncthreads();
    for (int e = threadIdx.x; e < TT * DH; e += blockDim.x) {
      const int r = e / DH, d = e % DH, i = i0 + r;
      const long row = (long)b * n + i;
      Qs[r * LD + d] = i < n ? qkv[row * pitch + h * DH + d] * scale : 0.f;
      Gs[r * LD + d] = i < n ? gout[row * gout_pitch + h * DH + d] : 0.f;
    }
    if (threadIdx.x < TT) {
      const int i = i0 + threadIdx.x;
      const long row = (long)b * n + i;
      Ls[threadIdx.x] = i < n ? lse[(long)bh * n + i] : INFINITY;
      Ds[threadIdx.x] = i < n ? row_delta(gout + row * gout_pitch + h * DH, out + row * out_pitch + h * DH) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};    // [query 16t + 4kg + r][key cl]
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        st = mfma4(Qs[(16 * t + cl) * LD + 4 * s + kg], kf[s], st);
        dp = mfma4(Gs[(16 * t + cl) * LD + 4 * s + kg], vf[s], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * t + 4 * kg + r;
        const float p = __expf(st[r] - Ls[q]);
        const float ds = p * (dp[r] - Ds[q]);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          acc[0][e] = mfma4(Qs[q * LD + 16 * e + cl], ds, acc[0][e]);   // dK^T[d][key]
          acc[1][e] = mfma4(Gs[q * LD + 16 * e + cl], p, acc[1][e]);    // dV^T[d][key]
        }
      }
    }
  }
  if (j >= nk) return;
  float* dst[2];
  if (j < M) {
    float* gm = gmem_partial + (long)b * 2 * heads * M * DH;            // [B][2][heads][M][32]
    dst[0] = gm + ((long)(0 * heads + h) * M + j) * DH;
    dst[1] = gm + ((long)(1 * heads + h) * M + j) * DH;
  } else {
    float* g = gqkv + ((long)b * n + (j - M)) * gq_pitch + h * DH;
    dst[0] = g + hidden;
    dst[1] = g + 2 * hidden;
  }
#pragma unroll
  for (int which = 0; which < 2; ++which)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[which][16 * e + 4 * kg + r] = acc[which][e][r];
}

}  // namespace

int lgm_attn_tiled_fwd_launch(const float* qkv, long pitch, const float* mem_kv, int B, int n, int heads, int M,
                              float scale, float* out, long out_pitch, float* lse, hipStream_t s) {
  LGM_REQUIRE(lgm_cdiv(n, TT) <= 65535, "attn_fwd: n=%d too large", n);
  lgm_note_kernel(LGM_KNAME("attn_tiled_fwd_kernel"));
  hipLaunchKernelGGL(attn_tiled_fwd_kernel, dim3(B * heads, lgm_cdiv(n, TT)), dim3(256), 0, s, qkv, pitch, mem_kv, n,
                     heads, M, scale, out, out_pitch, lse);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

int lgm_attn_tiled_bwd_launch(const float* qkv, long pitch, const float* mem_kv, const float* out, long out_pitch,
                              const float* gout, long gout_pitch, const float* lse, int B, int n, int heads, int M,
                              float scale, float* gqkv, long gq_pitch, float* gmem_partial, hipStream_t s) {
  const int nqt = lgm_cdiv(n, TT), nkt = lgm_cdiv(n + M, TT);
  LGM_REQUIRE(nqt + nkt <= 65535, "attn_bwd: n=%d too large", n);
  lgm_note_kernel(LGM_KNAME("attn_tiled_bwd_kernel"));
  hipLaunchKernelGGL(attn_tiled_bwd_kernel, dim3(B * heads, nqt + nkt), dim3(256), 0, s, qkv, pitch, mem_kv, out,
                     out_pitch, gout, gout_pitch, lse, n, heads, M, scale, nqt, gqkv, gq_pitch, gmem_partial);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
