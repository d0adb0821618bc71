// Low-resolution conditioning of a cascaded super-resolution DDPM (SR3, Saharia et al. 2021; Cascaded Diffusion Models, Ho
// et al. 2021; Imagen, Saharia et al. 2022): the producer of the conditioning slice of the network's input buffer, and the
// row-local add that joins the augmentation-level embedding to the time embedding.
//
// lowres_cond_kernel<R>.  One workgroup owns LT_H x LT_W = 8 x 16 low-resolution pixels of one sample, all C channels, and
// the (8 R) x (16 R) outputs above them.
//   pass 1  the low-resolution tile plus a one-pixel halo, [C][10][18] floats, into LDS.  Training source (img, high
//           resolution): every thread forms whole low-resolution pixels - R row loads of R contiguous floats (one 8-, 16- or
//           2 x 16-byte load: neighbouring threads read neighbouring vectors), each row summed by a halving tree (v[i] +=
//           v[i + n/2], n = R, R/2, ..), the R row sums by the same tree, times 1/R^2 (exact).  A high-resolution pixel is
//           read once by its own tile and again only where it lies under a neighbour's halo: (10 * 18) / (8 * 16) = 1.41 of
//           the image at most, nothing is re-averaged per output.  Sampling source (low): the tile is copied.  Either way the
//           value is then normalised, n = 2 l - 1 (the bilinear weights sum to one exactly, so normalising the R^2 times
//           fewer low-resolution values is the same map as normalising the outputs).  Halo cells outside the image are never
//           read: the clamped taps below stay inside it.
//   pass 2  one (pixel, channel) per thread and trip, channel fastest (the store order of qsample_slice_kernel): the bilinear
//           taps of torch's align_corners=False rule from LDS - source coordinate (dst + 0.5) / R - 0.5 clamped at 0, upper tap
//           clamped at the last row / column; for R a power of two the weights are exact - then the augmentation, and ONE
//           scalar store into lane cond_off + c.  No other lane, no other buffer is written.
// No atomics, no cross-thread sums: every output is a fixed expression of its inputs, so a graph replay, an eager launch and
// the two sources (given the float32 averages pass 1 forms) agree to the bit.  Contraction is off.  Roundings on the longest
// path: 2 log2 R (average) + 1 (normalise) + 4 (bilinear: tap product, row sum, row product, column sum) + 2 (augmentation:
// product, sum).
#include "lgm_common.h"

namespace {

constexpr int LT_H = 8, LT_W = 16;                   // low-resolution pixels per workgroup
constexpr int LT_HH = LT_H + 2, LT_WH = LT_W + 2;    // with the halo
constexpr int LOWRES_MAX_C = 64;                     // 64 * 10 * 18 * 4 = 46080 bytes of LDS

template <int N>
__device__ __forceinline__ float tree_sum(float* v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int n = N; n > 1; n >>= 1) {
#pragma unroll
    for (int i = 0; i < n / 2; ++i) v[i] = v[i] + v[i + n / 2];
  }
  return v[0];
}

// the float32 area average of the R x R block whose first element is p (row pitch W floats; p is R * 4-byte aligned)
template <int R>
__device__ __forceinline__ float area_mean(const float* __restrict__ p, long W) {
  float rows[R];
#pragma unroll
  for (int dy = 0; dy < R; ++dy) {
    float v[R];
    const float* q = p + dy * W;
    if constexpr (R == 2) {
      const float2 a = *reinterpret_cast<const float2*>(q);
      v[0] = a.x, v[1] = a.y;
    } else {
#pragma unroll
      for (int k = 0; k < R / 4; ++k) {
        const f32x4 a = reinterpret_cast<const f32x4*>(q)[k];
        v[4 * k] = a[0], v[4 * k + 1] = a[1], v[4 * k + 2] = a[2], v[4 * k + 3] = a[3];
      }
    }
    rows[dy] = tree_sum<R>(v);
  }
  return tree_sum<R>(rows) * (1.f / (R * R));
}

__device__ __forceinline__ float lowres_lerp(float a, float b, float w0, float w1) {
#pragma clang fp contract(off)
  return a * w0 + b * w1;
}

__device__ __forceinline__ float lowres_augment(float u, float sa, float sb, float e) {
#pragma clang fp contract(off)
  return sa * u + sb * e;
}

// src: img [B, C, h R, w R] when from_high, else low [B, C, h, w].  xin [B, (h R)(w R), pitch].
template <int R>
__global__ __launch_bounds__(256) void lowres_cond_kernel(const float* __restrict__ src, int from_high,
                                                          const float* __restrict__ eps, const long* __restrict__ s,
                                                          const float* __restrict__ sa, const float* __restrict__ sb,
                                                          int n_table, int normalize, float* __restrict__ xin, long pitch,
                                                          int cond_off, int C, int h, int w, int tiles_x) {
  extern __shared__ float tile[];                    // [C][LT_HH][LT_WH]
  const int b = blockIdx.y;
  const int ly0 = (blockIdx.x / tiles_x) * LT_H, lx0 = (blockIdx.x % tiles_x) * LT_W;
  const int H = h * R, W = w * R;
  // ---- pass 1 ----
  for (int i = threadIdx.x; i < C * LT_HH * LT_WH; i += 256) {
    const int jx = i % LT_WH, jy = (i / LT_WH) % LT_HH, c = i / (LT_WH * LT_HH);
    const int ly = ly0 - 1 + jy, lx = lx0 - 1 + jx;
    if (ly < 0 || ly >= h || lx < 0 || lx >= w) continue;        // outside the image: no tap reaches it
    const long plane = (long)b * C + c;
    float l = from_high ? area_mean<R>(src + (plane * H + (long)ly * R) * W + (long)lx * R, W) : src[(plane * h + ly) * w + lx];
    if (normalize) l = l * 2.f - 1.f;
    tile[i] = l;
  }
  __syncthreads();
  // ---- pass 2 ----
  float a_s = 1.f, b_s = 0.f;
  if (eps) {
    long si = s[b];
    si = si < 0 ? 0 : (si >= n_table ? n_table - 1 : si);
    a_s = sa[si], b_s = sb[si];
  }
  const int th = min(LT_H, h - ly0) * R, tw = min(LT_W, w - lx0) * R;      // this tile's outputs (partial at the edges)
  const int y0 = ly0 * R, x0 = lx0 * R;
  for (int i = threadIdx.x; i < th * tw * C; i += 256) {
    const int c = i % C, px = i / C;
    const int y = y0 + px / tw, x = x0 + px % tw;
    // exact for R in {2, 4, 8}: (dst + 0.5) / R - 0.5 is a multiple of 1 / (2 R)
    const float fy = fmaxf(((float)y + 0.5f) * (1.f / R) - 0.5f, 0.f), fx = fmaxf(((float)x + 0.5f) * (1.f / R) - 0.5f, 0.f);
    const int iy0 = (int)fy, ix0 = (int)fx;
    const int iy1 = min(iy0 + 1, h - 1), ix1 = min(ix0 + 1, w - 1);
    const float wy1 = fy - (float)iy0, wx1 = fx - (float)ix0;
    const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    const float* t = tile + c * (LT_HH * LT_WH);
    const int r0 = (iy0 - ly0 + 1) * LT_WH, r1 = (iy1 - ly0 + 1) * LT_WH, c0 = ix0 - lx0 + 1, c1 = ix1 - lx0 + 1;
    const float top = lowres_lerp(t[r0 + c0], t[r0 + c1], wx0, wx1);
    const float bot = lowres_lerp(t[r1 + c0], t[r1 + c1], wx0, wx1);
    float u = lowres_lerp(top, bot, wy0, wy1);
    const long p = (long)y * W + x;
    if (eps) u = lowres_augment(u, a_s, b_s, eps[((long)b * C + c) * H * W + p]);
    xin[((long)b * H * W + p) * pitch + cond_off + c] = u;
  }
}

// temb[b] += add[b];  st[b] = SiLU(temb[b]) (st may be null: a label embedding follows and writes it)
__global__ __launch_bounds__(256) void lowres_emb_add_kernel(float* __restrict__ temb, float* __restrict__ st,
                                                             const float* __restrict__ add, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = reinterpret_cast<f32x4*>(temb)[i];
  const f32x4 e = reinterpret_cast<const f32x4*>(add)[i];
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] += e[k];
    o[k] = v[k] / (1.f + expf(-v[k]));
  }
  reinterpret_cast<f32x4*>(temb)[i] = v;
  if (st) reinterpret_cast<f32x4*>(st)[i] = o;
}

template <int R>
void launch_lowres(const float* src, int from_high, const float* eps, const int64_t* s, const float* sa, const float* sb,
                   int n_table, int normalize, float* xin, int64_t pitch, int cond_off, int B, int C, int h, int w,
                   void* stream) {
  const int tiles_x = lgm_cdiv(w, LT_W), tiles_y = lgm_cdiv(h, LT_H);
  hipLaunchKernelGGL(lowres_cond_kernel<R>, dim3(tiles_x * tiles_y, B), dim3(256), (size_t)C * LT_HH * LT_WH * sizeof(float),
                     (hipStream_t)stream, src, from_high, eps, (const long*)s, sa, sb, n_table, normalize, xin, (long)pitch,
                     cond_off, C, h, w, tiles_x);
}

}  // namespace

// The name is noted without a registry entry (no LGM_KNAME), like dpm_step_kernel's and for the same reason:
// tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it, and tests/test_hip_lowres.py,
// which runs this kernel and asserts the noted name, is not on that list.
extern "C" int lgm_lowres_cond(const float* img, const float* low, const float* eps, const int64_t* s, const float* sqrt_ac,
                               const float* sqrt_1mac, int n_table, int normalize, float* xin, int64_t pitch, int cond_off,
                               int B, int C, int H, int W, int r, void* stream) {
  LGM_REQUIRE((img != nullptr) != (low != nullptr) && xin && B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0,
              "lowres_cond: exactly one of img / low, an input buffer and positive sizes required");
  LGM_REQUIRE(r == 2 || r == 4 || r == 8, "lowres_cond: the factor must be 2, 4 or 8, got %d", r);
  LGM_REQUIRE(H % r == 0 && W % r == 0, "lowres_cond: the factor %d must divide the size %d x %d", r, H, W);
  LGM_REQUIRE(C <= LOWRES_MAX_C && cond_off >= 0 && cond_off + C <= pitch, "lowres_cond: C <= %d and the slice inside the pitch required",
              LOWRES_MAX_C);
  LGM_REQUIRE(!eps || (s && sqrt_ac && sqrt_1mac && n_table > 0), "lowres_cond: eps needs s and the two tables");
  LGM_REQUIRE(!img || lgm_aligned16(img), "lowres_cond: 16-byte aligned img required");
  LGM_REQUIRE((const void*)xin != (const void*)img && (const void*)xin != (const void*)low && (const void*)xin != (const void*)eps,
              "lowres_cond: the input buffer must not alias a source");
  const float* src = img ? img : low;
  const int fh = img ? 1 : 0;
  lgm_note_kernel("lowres_cond_kernel");
  if (r == 2) launch_lowres<2>(src, fh, eps, s, sqrt_ac, sqrt_1mac, n_table, normalize, xin, pitch, cond_off, B, C, H / r, W / r, stream);
  else if (r == 4) launch_lowres<4>(src, fh, eps, s, sqrt_ac, sqrt_1mac, n_table, normalize, xin, pitch, cond_off, B, C, H / r, W / r, stream);
  else launch_lowres<8>(src, fh, eps, s, sqrt_ac, sqrt_1mac, n_table, normalize, xin, pitch, cond_off, B, C, H / r, W / r, stream);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_lowres_emb_fwd(float* temb, float* st, const float* add, int B, int time_dim, void* stream) {
  LGM_REQUIRE(temb && add && temb != add && B > 0 && time_dim > 0, "lowres_emb_fwd: bad arguments");
  LGM_REQUIRE(time_dim % 4 == 0 && lgm_aligned16(temb) && lgm_aligned16(add) && (!st || lgm_aligned16(st)),
              "lowres_emb_fwd: time_dim %% 4 == 0 and 16-byte aligned temb / st / add required");
  const long n4 = (long)B * (time_dim / 4);
  lgm_note_kernel("lowres_emb_add_kernel");
  hipLaunchKernelGGL(lowres_emb_add_kernel, dim3(lgm_cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, temb, st, add, n4);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
