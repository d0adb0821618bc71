// Class conditioning and classifier-free guidance: the label embedding added to the time embedding (forward, weight
// gradient) and the mix of a conditional and a null-label network output.  Three row-local, float4-wide kernels; the only
// reduction (over the batch, per embedding row) runs in ascending sample order in one thread: no atomics, so an eager
// launch and a graph replay give the same bits.
#include "lgm_common.h"

namespace {

__device__ __forceinline__ int label_of(const long* __restrict__ y, int b, int K) {
  const long v = y[b];
  return v < 0 ? 0 : (v > K ? K : (int)v);           // labels live in [0, K]; K is the null label
}

// temb[b] += emb[y[b]];  st[b] = SiLU(temb[b])   (SiLU as lgm_act_fwd computes it)
__global__ __launch_bounds__(256) void label_emb_fwd_kernel(float* __restrict__ temb, float* __restrict__ st,
                                                            const float* __restrict__ emb, const long* __restrict__ y, int B,
                                                            int td4, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * td4) return;
  const int b = (int)(i / td4), c = (int)(i % td4);
  const f32x4 e = reinterpret_cast<const f32x4*>(emb)[(long)label_of(y, b, K) * td4 + c];
  f32x4 v = reinterpret_cast<f32x4*>(temb)[i];
  f32x4 s;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] += e[k];
    s[k] = v[k] / (1.f + expf(-v[k]));
  }
  reinterpret_cast<f32x4*>(temb)[i] = v;
  reinterpret_cast<f32x4*>(st)[i] = s;
}

// gemb[k] = beta * gemb[k] + sum_{b : y[b] = k} gtemb[b], b ascending.  One workgroup per embedding row k; the labels go
// through LDS once per chunk of LE_CHUNK samples, every thread owns float4 columns of the row.
constexpr int LE_CHUNK = 1024;
__global__ __launch_bounds__(256) void label_emb_wgrad_kernel(const float* __restrict__ gtemb, const long* __restrict__ y,
                                                              float* __restrict__ gemb, float beta, int B, int td4, int K) {
  __shared__ int ysh[LE_CHUNK];
  const int k = blockIdx.x;
  for (int c0 = 0; c0 < td4; c0 += blockDim.x) {
    const int c = c0 + threadIdx.x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += LE_CHUNK) {
      const int nb = B - b0 < LE_CHUNK ? B - b0 : LE_CHUNK;
      __syncthreads();
      for (int j = threadIdx.x; j < nb; j += blockDim.x) ysh[j] = label_of(y, b0 + j, K);
      __syncthreads();
      if (c < td4) {
        for (int j = 0; j < nb; ++j) {
          if (ysh[j] != k) continue;                 // uniform over the workgroup
          const f32x4 g = reinterpret_cast<const f32x4*>(gtemb)[(long)(b0 + j) * td4 + c];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], g[e]);
        }
      }
    }
    if (c < td4) {
      f32x4* o = reinterpret_cast<f32x4*>(gemb) + (long)k * td4 + c;
      if (beta != 0.f) {
        const f32x4 old = *o;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(__fmul_rn(beta, old[e]), acc[e]);
      }
      *o = acc;
    }
  }
}

// cond <- null + s (cond - null) on the first C lanes of every pixel; s == 1 keeps cond and s == 0 takes null, bit for bit.
// s comes from s_dev when given (a captured sampling step reads the scale of the current run from a static buffer).
__global__ __launch_bounds__(256) void cfg_mix_kernel(float* __restrict__ cond, long cond_pitch, const float* __restrict__ null_,
                                                      long null_pitch, float s, const float* __restrict__ s_dev, long rows,
                                                      int C) {
  const int c4 = (C + 3) >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * c4) return;
  if (s_dev) s = s_dev[0];
  if (s == 1.f) return;
  const long r = i / c4;
  const int q = (int)(i % c4);
  f32x4* pc = reinterpret_cast<f32x4*>(cond + r * cond_pitch) + q;
  const f32x4 n = reinterpret_cast<const f32x4*>(null_ + r * null_pitch)[q];
  f32x4 v = *pc;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * q + e < C) v[e] = s == 0.f ? n[e] : __fadd_rn(n[e], __fmul_rn(s, __fsub_rn(v[e], n[e])));
  *pc = v;                                            // pad lanes: their own value
}

}  // namespace

extern "C" int lgm_label_emb_fwd(float* temb, float* st, const float* emb, const int64_t* y, int B, int time_dim,
                                 int num_classes, void* stream) {
  LGM_REQUIRE(temb && st && emb && y && B > 0 && time_dim > 0 && num_classes > 0, "label_emb_fwd: bad arguments");
  LGM_REQUIRE(time_dim % 4 == 0 && lgm_aligned16(temb) && lgm_aligned16(st) && lgm_aligned16(emb),
              "label_emb_fwd: time_dim %% 4 == 0 and 16-byte aligned temb / st / emb required");
  lgm_note_kernel(LGM_KNAME("label_emb_fwd_kernel"));
  hipLaunchKernelGGL(label_emb_fwd_kernel, dim3(lgm_cdiv((long)B * (time_dim / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                     temb, st, emb, (const long*)y, B, time_dim / 4, num_classes);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_label_emb_wgrad(const float* gtemb, const int64_t* y, float* gemb, float beta, int B, int time_dim,
                                   int num_classes, void* stream) {
  LGM_REQUIRE(gtemb && y && gemb && B > 0 && time_dim > 0 && num_classes > 0, "label_emb_wgrad: bad arguments");
  LGM_REQUIRE(time_dim % 4 == 0 && lgm_aligned16(gtemb) && lgm_aligned16(gemb),
              "label_emb_wgrad: time_dim %% 4 == 0 and 16-byte aligned gtemb / gemb required");
  const int td4 = time_dim / 4;
  const int threads = td4 >= 256 ? 256 : (td4 + 63) / 64 * 64;
  lgm_note_kernel(LGM_KNAME("label_emb_wgrad_kernel"));
  hipLaunchKernelGGL(label_emb_wgrad_kernel, dim3(num_classes + 1), dim3(threads), 0, (hipStream_t)stream, gtemb,
                     (const long*)y, gemb, beta, B, td4, num_classes);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_cfg_mix(float* out_cond, int64_t cond_pitch, const float* out_null, int64_t null_pitch, float scale,
                           const float* scale_dev, int64_t rows, int C, void* stream) {
  LGM_REQUIRE(out_cond && out_null && out_cond != out_null && rows > 0 && C > 0, "cfg_mix: bad arguments");
  const int Cp = (C + 3) / 4 * 4;
  LGM_REQUIRE(cond_pitch >= Cp && null_pitch >= Cp && cond_pitch % 4 == 0 && null_pitch % 4 == 0 && lgm_aligned16(out_cond) &&
                  lgm_aligned16(out_null),
              "cfg_mix: 16-byte aligned outputs with pitch %% 4 == 0 and pitch >= r4(C) required");
  lgm_note_kernel(LGM_KNAME("cfg_mix_kernel"));
  hipLaunchKernelGGL(cfg_mix_kernel, dim3(lgm_cdiv(rows * (Cp / 4), 256)), dim3(256), 0, (hipStream_t)stream, out_cond,
                     (long)cond_pitch, out_null, (long)null_pitch, scale, scale_dev, (long)rows, C);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
