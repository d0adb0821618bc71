// The NICE flow's own kernels (reference models/generative/flow/nice.py): the additive coupling on a lane slice of the state
// buffer, the diagonal scaling layer with the Gaussian log-likelihood, its backward with the column-sum gradient of
// log_scale, and the loss.  The coupling nets' Linear layers run on csrc/dense.hip.  DESIGN section 6 has the definitions
// and the rounding counts.
//
// nice_couple_kernel<VEC>      out[b][d] = fl(x[b][d] + sign t[b][d - off]) on lanes [off, off + n), x's bits elsewhere: one
//   rounding.  A thread owns one quad of one row; it reads its quad of x before it writes its quad of out, and no other thread
//   touches those lanes, so out == x (same pitch) runs in place.
// nice_scale_fwd_kernel<VEC>   one workgroup per row: z = fl(h expf(+-log_scale[d])), row_part[b] = sum_d z^2.  Thread t adds
//   the elements of quads t, t + 256, .. in ascending order, then lgm_block_sum: the order depends on D alone and is the same
//   in both load forms.  Without row_part (the inverse) nothing is summed.
// nice_loss_kernel             one wave: lane l adds rows l, l + 64, .. of row_part, then the fixed shuffle tree; the same over
//   the D lanes of log_scale.
// nice_scale_bwd_kernel<VEC>   two roles, picked per workgroup (both only read z): the first ceil(Q / 64) workgroups own one
//   quad of columns per thread and walk the B rows in ascending order, adding (c z) z to four column sums, c = gloss[0] / B;
//   the others write gh = (c z) expf(log_scale[d]), one quad of one row per thread.  No row count is too large and no sum
//   depends on the grid.
// VEC: every operand starts at a 16-byte boundary with a pitch that is a multiple of 4 (and, for the coupling, off % 4 == 0)
// - whole quads inside [0, D) move as one 16-byte access; the quad that holds the row's end, a quad of t that straddles an
// end of the slice, and every quad of the other form, moves lane by lane under a guard.  Pad lanes of an input are never
// read; pad lanes [D, round_up(D, 4)) of an output are written +0, nothing beyond.  No atomics, no workgroup waits for
// another, every grid is a function of (B, D) alone.
#include "lgm_common.h"

namespace {

constexpr int NICE_MAX_DIM = 1 << 20;
constexpr int NICE_EW_THREADS = 64;           // elementwise: one quad per thread; B = 32, D = 784 spreads over 98 workgroups
constexpr long NICE_MAX_ELEMS = 1L << 31;     // B round_up(D, 4): the one-wave elementwise grids then hold at most 2^23 workgroups

inline int r4(int n) { return (n + 3) / 4 * 4; }

template <bool VEC>
__device__ __forceinline__ f32x4 nice_load4(const float* row, int d, int D) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC && d + 3 < D) return *reinterpret_cast<const f32x4*>(row + d);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) v[e] = row[d + e];
  return v;
}

// lanes [d, d + 4) lie below Dp = round_up(D, 4): the whole quad is the output's
template <bool VEC>
__device__ __forceinline__ void nice_store4(float* row, int d, f32x4 v) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(row + d) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) row[d + e] = v[e];
  }
}

// x and out may be the same buffer: no __restrict__ on them
template <bool VEC>
__global__ __launch_bounds__(NICE_EW_THREADS) void nice_couple_kernel(const float* x, long x_pitch, const float* __restrict__ t,
                                                                     long t_pitch, int B, int D, int Q, int off, int n,
                                                                     int sign, float* out, long out_pitch) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * NICE_EW_THREADS + threadIdx.x;
  if (i >= (long)B * Q) return;
  const int b = (int)(i / Q), d = 4 * (int)(i - (long)b * Q);
  f32x4 o = nice_load4<VEC>(x + (long)b * x_pitch, d, D);      // lanes >= D come back +0
  const float* trow = t + (long)b * t_pitch;
  const int j = d - off;                                       // the quad's first lane inside the slice
  if (j + 3 >= 0 && j < n) {
    f32x4 tv = {0.f, 0.f, 0.f, 0.f};
    if (VEC && j >= 0 && j + 3 < n) {
      tv = *reinterpret_cast<const f32x4*>(trow + j);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e >= 0 && j + e < n) tv[e] = trow[j + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e >= 0 && j + e < n) o[e] = sign > 0 ? o[e] + tv[e] : o[e] - tv[e];
  }
  nice_store4<VEC>(out + (long)b * out_pitch, d, o);
}

template <bool VEC>
__global__ __launch_bounds__(256) void nice_scale_fwd_kernel(const float* __restrict__ h, long h_pitch,
                                                             const float* __restrict__ log_scale, int D, int Dp, int reverse,
                                                             float* __restrict__ z, long z_pitch, float* __restrict__ row_part) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int d = 4 * threadIdx.x; d < Dp; d += 4 * 256) {
    const f32x4 hv = nice_load4<VEC>(h + (long)b * h_pitch, d, D);
    const f32x4 lv = nice_load4<VEC>(log_scale, d, D);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (d + e < D) {
        const float zz = hv[e] * expf(reverse ? -lv[e] : lv[e]);
        o[e] = zz;
        s = s + zz * zz;
      }
    nice_store4<VEC>(z + (long)b * z_pitch, d, o);
  }
  if (row_part == nullptr) return;             // the same for every thread of the launch
  s = lgm_block_sum(s, sh);
  if (threadIdx.x == 0) row_part[b] = s;
}

__global__ __launch_bounds__(64) void nice_loss_kernel(const float* __restrict__ row_part, const float* __restrict__ log_scale,
                                                       int B, int D, float half_d_log2pi, int exact, float* __restrict__ vals3) {
#pragma clang fp contract(off)
  float r = 0.f, s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) r = r + row_part[b];
  for (int d = threadIdx.x; d < D; d += 64) s = s + log_scale[d];
  r = lgm_wave_sum(r);
  s = lgm_wave_sum(s);
  if (threadIdx.x == 0) {
    const float mean_ll = (-0.5f * r) / (float)B - half_d_log2pi;
    vals3[0] = exact ? -(mean_ll + s) : -(mean_ll - s);
    vals3[1] = mean_ll;
    vals3[2] = s;
  }
}

constexpr int NICE_BWD_UNROLL = 16;            // rows in flight per column thread: its walk over b is bound by load latency

// Two roles in one launch, picked per workgroup; both only read z, so neither waits for the other.  Workgroups [0, col_blocks)
// sum columns: a thread owns one quad of columns and walks the B rows in ascending order with nothing but loads in its loop
// (a store between them would put its latency into every round of loads).  The others write gh, one quad of one row per
// thread, like the coupling.
template <bool VEC>
__global__ __launch_bounds__(NICE_EW_THREADS) void nice_scale_bwd_kernel(const float* __restrict__ z, long z_pitch,
                                                                        const float* __restrict__ log_scale,
                                                                        const float* __restrict__ gloss, int B, int D, int Q,
                                                                        int col_blocks, int exact, float* __restrict__ gh,
                                                                        long gh_pitch, float* __restrict__ gls, float beta) {
#pragma clang fp contract(off)
  const float gl = gloss[0];
  const float c = gl / (float)B;
  if ((int)blockIdx.x >= col_blocks) {
    const long i = (long)(blockIdx.x - col_blocks) * NICE_EW_THREADS + threadIdx.x;
    if (i >= (long)B * Q) return;
    const int b = (int)(i / Q), d = 4 * (int)(i - (long)b * Q);
    const f32x4 zv = nice_load4<VEC>(z + (long)b * z_pitch, d, D);
    const f32x4 lv = nice_load4<VEC>(log_scale, d, D);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (d + e < D) {
        const float cz = c * zv[e];
        o[e] = cz * expf(lv[e]);
      }
    nice_store4<VEC>(gh + (long)b * gh_pitch, d, o);
    return;
  }
  const int q = blockIdx.x * NICE_EW_THREADS + threadIdx.x;
  if (q >= Q) return;
  const int d = 4 * q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll NICE_BWD_UNROLL
  for (int b = 0; b < B; ++b) {
    const f32x4 zv = nice_load4<VEC>(z + (long)b * z_pitch, d, D);
#pragma unroll
    for (int e = 0; e < 4; ++e) {            // lanes past D hold +0 and add nothing
      const float cz = c * zv[e];
      acc[e] = acc[e] + cz * zv[e];
    }
  }
  const float k = exact ? -gl : gl;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) {
      const float r = acc[e] + k;
      gls[d + e] = beta == 0.f ? r : beta * gls[d + e] + r;      // beta = 0 overwrites whatever is there
    }
}

inline bool vec_ok(const void* p, long pitch) { return lgm_aligned16(p) && pitch % 4 == 0; }
inline bool dims_ok(int B, int D) {
  return B >= 1 && B <= NICE_MAX_DIM && D >= 1 && D <= NICE_MAX_DIM && (long)B * r4(D) <= NICE_MAX_ELEMS;
}
// do the B rows of `wa` floats at a (pitch ap) and of `wb` floats at b (pitch bp) share a byte?  Whole spans are compared: rows
// that interleave without touching are refused too
inline bool overlaps(const float* a, long ap, const float* b, long bp, int B, int wa, int wb) {
  const float* ae = a + (long)(B - 1) * ap + wa;
  const float* be = b + (long)(B - 1) * bp + wb;
  return a < be && b < ae;
}

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), like csrc/dense.hip's and csrc/dae.hip's and for the same
// reason: tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it; tests/test_hip_nice.py
// runs these.

extern "C" int lgm_nice_couple(const float* x, int64_t x_pitch, const float* t, int64_t t_pitch, int B, int D, int off, int n,
                               int sign, float* out, int64_t out_pitch, void* stream) {
  LGM_REQUIRE(x && t && out, "nice_couple: null argument");
  LGM_REQUIRE(dims_ok(B, D), "nice_couple: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(off >= 0 && n >= 1 && n <= D && off <= D - n, "nice_couple: the slice [off, off + n) must lie in [0, %d), got %d %d",
              D, off, n);
  LGM_REQUIRE(sign == 1 || sign == -1, "nice_couple: sign must be +1 or -1, got %d", sign);
  LGM_REQUIRE(x_pitch >= D && t_pitch >= n && out_pitch >= r4(D), "nice_couple: pitches below the lane counts %d, %d", D, n);
  const bool in_place = out == x && out_pitch == x_pitch;
  LGM_REQUIRE(in_place || !overlaps(out, (long)out_pitch, x, (long)x_pitch, B, r4(D), D),
              "nice_couple: out must be x itself (same pitch) or not overlap it");
  LGM_REQUIRE(!overlaps(out, (long)out_pitch, t, (long)t_pitch, B, r4(D), n), "nice_couple: out must not overlap t");
  const int Q = r4(D) / 4;
  const dim3 grid(lgm_cdiv((long)B * Q, NICE_EW_THREADS)), block(NICE_EW_THREADS);
  const bool vec = vec_ok(x, (long)x_pitch) && vec_ok(t, (long)t_pitch) && vec_ok(out, (long)out_pitch) && off % 4 == 0;
  lgm_note_kernel(vec ? "nice_couple_kernel<true>" : "nice_couple_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(nice_couple_kernel<true>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch, t, (long)t_pitch, B, D, Q,
                       off, n, sign, out, (long)out_pitch);
  else
    hipLaunchKernelGGL(nice_couple_kernel<false>, grid, block, 0, (hipStream_t)stream, x, (long)x_pitch, t, (long)t_pitch, B, D, Q,
                       off, n, sign, out, (long)out_pitch);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_nice_scale_fwd(const float* h, int64_t h_pitch, const float* log_scale, int B, int D, int reverse, float* z,
                                  int64_t z_pitch, float* row_part, void* stream) {
  LGM_REQUIRE(h && log_scale && z, "nice_scale_fwd: null argument");
  LGM_REQUIRE(dims_ok(B, D), "nice_scale_fwd: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(h_pitch >= D && z_pitch >= r4(D), "nice_scale_fwd: pitches below the lane count %d", D);
  // a vector is a span with pitch 0
  LGM_REQUIRE(!overlaps(z, (long)z_pitch, h, (long)h_pitch, B, r4(D), D) && !overlaps(z, (long)z_pitch, log_scale, 0, B, r4(D), D),
              "nice_scale_fwd: z must not overlap an input");
  LGM_REQUIRE(!row_part || (!overlaps(row_part, 0, h, (long)h_pitch, B, B, D) &&
                            !overlaps(row_part, 0, z, (long)z_pitch, B, B, r4(D)) && !overlaps(row_part, 0, log_scale, 0, B, B, D)),
              "nice_scale_fwd: row_part must not overlap h, z or log_scale");
  const bool vec = vec_ok(h, (long)h_pitch) && vec_ok(z, (long)z_pitch) && lgm_aligned16(log_scale);
  lgm_note_kernel(vec ? "nice_scale_fwd_kernel<true>" : "nice_scale_fwd_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(nice_scale_fwd_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, h, (long)h_pitch, log_scale, D,
                       r4(D), reverse ? 1 : 0, z, (long)z_pitch, row_part);
  else
    hipLaunchKernelGGL(nice_scale_fwd_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, h, (long)h_pitch, log_scale, D,
                       r4(D), reverse ? 1 : 0, z, (long)z_pitch, row_part);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_nice_loss(const float* row_part, const float* log_scale, int B, int D, int exact, float* vals3, void* stream) {
  LGM_REQUIRE(row_part && log_scale && vals3, "nice_loss: null argument");
  LGM_REQUIRE(dims_ok(B, D), "nice_loss: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(!overlaps(vals3, 0, row_part, 0, 1, 3, B) && !overlaps(vals3, 0, log_scale, 0, 1, 3, D),
              "nice_loss: vals3 must not overlap an input");
  const float half_d_log2pi = (float)(0.5 * (double)D * 1.8378770664093454835606594728112);      // log(2 pi), rounded once
  lgm_note_kernel("nice_loss_kernel");
  hipLaunchKernelGGL(nice_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_part, log_scale, B, D, half_d_log2pi,
                     exact ? 1 : 0, vals3);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_nice_scale_bwd(const float* z, int64_t z_pitch, const float* log_scale, const float* gloss, int B, int D,
                                  int exact, float* gh, int64_t gh_pitch, float* gls, float beta, void* stream) {
  LGM_REQUIRE(z && log_scale && gloss && gh && gls, "nice_scale_bwd: null argument");
  LGM_REQUIRE(dims_ok(B, D), "nice_scale_bwd: B >= 1, D >= 1 and B D <= 2^31 required, got %d %d", B, D);
  LGM_REQUIRE(z_pitch >= D && gh_pitch >= r4(D), "nice_scale_bwd: pitches below the lane count %d", D);
  LGM_REQUIRE(!overlaps(gh, (long)gh_pitch, z, (long)z_pitch, B, r4(D), D) &&
                  !overlaps(gh, (long)gh_pitch, log_scale, 0, B, r4(D), D) &&
                  !overlaps(gh, (long)gh_pitch, gloss, 0, B, r4(D), 1) && !overlaps(gh, (long)gh_pitch, gls, 0, B, r4(D), D),
              "nice_scale_bwd: gh must not overlap an input or gls");
  LGM_REQUIRE(!overlaps(gls, 0, z, (long)z_pitch, B, D, D) && !overlaps(gls, 0, log_scale, 0, B, D, D) &&
                  !overlaps(gls, 0, gloss, 0, B, D, 1),
              "nice_scale_bwd: gls must not overlap an input");
  const int Q = r4(D) / 4;
  const int col_blocks = lgm_cdiv(Q, NICE_EW_THREADS);
  const dim3 grid(col_blocks + lgm_cdiv((long)B * Q, NICE_EW_THREADS)), block(NICE_EW_THREADS);
  const bool vec = vec_ok(z, (long)z_pitch) && vec_ok(gh, (long)gh_pitch) && lgm_aligned16(log_scale);
  lgm_note_kernel(vec ? "nice_scale_bwd_kernel<true>" : "nice_scale_bwd_kernel<false>");
  if (vec)
    hipLaunchKernelGGL(nice_scale_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, z, (long)z_pitch, log_scale, gloss, B, D,
                       Q, col_blocks, exact ? 1 : 0, gh, (long)gh_pitch, gls, beta);
  else
    hipLaunchKernelGGL(nice_scale_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, z, (long)z_pitch, log_scale, gloss, B, D,
                       Q, col_blocks, exact ? 1 : 0, gh, (long)gh_pitch, gls, beta);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
