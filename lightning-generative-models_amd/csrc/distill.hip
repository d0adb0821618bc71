// Progressive distillation of the DDPM sampler (Salimans & Ho 2022, Algorithm 2): the two elementwise launches that stand
// between the teacher's two forwards and the student's loss.  One student DDIM step t -> t'' is trained to land where two
// teacher DDIM steps t -> t' -> t'' land (eta = 0; lgm_hip/distill.py plans the grids and the coefficient rows).
//
// The table has one row of DISTILL_K = 16 floats per timestep, read at t[b] (rows off the student's grid hold NaN):
//     0..3   A_t  S_t  R_t  Rm1_t      sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1 at t   (the head of the teacher's step at t)
//     4..7   A_m  S_m  R_m  Rm1_m      the same at t'
//     8..9   A_n  S_n                  alpha, sigma at t''   ((1, 0) when t'' = -1)
//     10..11 cX   cZ                   1 / den, -(S_n / S_t) / den with den = A_n - (S_n / S_t) A_t   ((1, 0) when t'' = -1)
//     12     iS_t                      1 / S_t
//     13     t'                        as a float (exact: T < 2^24)
//     14..15 den, t''                  not read here (the tests and the bound read them)
// every entry float64 on the host, rounded once.
//
// distill_half_step_kernel   (x1, e1) = the teacher's model_predictions at (z_t, t) from its output - x1 clamped to [-1, 1] when
//                            clip, e1 rederived from the clamped x1, exactly the pair ddim_sample forms - then
//                            z_t' = A_m x1 + S_m e1 into the x slice of the teacher's second input buffer, t_mid[b] = t'.
// distill_target_kernel      (x2, e2) the same at (z_t', t'), z_t'' = A_n x2 + S_n e2, x~ = cX z_t'' + cZ z_t, and the target in
//                            the student's objective: x~ | e~ = (z_t - A_t x~) iS_t | A_t e~ - S_t x~.
// Both are streaming: one thread per (pixel, four lanes) with 16-byte loads and stores where every pitch and offset is a
// multiple of four floats and the bases are 16-byte aligned, else one thread per (pixel, lane).  The row is read through
// wave-uniform addresses (blockIdx.y is the sample), once per wave.  No atomics, no cross-thread value: every output is a fixed
// expression of its own inputs, so an eager launch and a graph replay agree to the bit, and so do the two access forms.
// Contraction is off in every expression below: each product and each sum rounds once, nothing is fused.
#include "lgm_common.h"

namespace {

constexpr int DISTILL_K = 16;

struct DistillRow {
  f32x4 head_t, head_m, next, tail;      // the four 16-byte quarters of a row, in the order above
};

__device__ __forceinline__ DistillRow distill_row(const float* __restrict__ table, const long* __restrict__ t, int b, int n_table) {
  long ti = t[b];
  ti = ti < 0 ? 0 : (ti >= n_table ? n_table - 1 : ti);
  const f32x4* r = reinterpret_cast<const f32x4*>(table + ti * DISTILL_K);
  DistillRow row;
  row.head_t = r[0], row.head_m = r[1], row.next = r[2], row.tail = r[3];
  return row;
}

// model_predictions (reference ddpm.py:707-734) with rederive_pred_noise=True, as csrc/elementwise.hip's predictions_one spells
// it: objective 0 = pred_noise, 1 = pred_x0, 2 = pred_v; head = (A, S, R, Rm1)
__device__ __forceinline__ void distill_predictions(int objective, float xv, float ov, const f32x4 head, int clip, float& pn,
                                                    float& x0) {
#pragma clang fp contract(off)
  const float A = head[0], S = head[1], R = head[2], Rm1 = head[3];
  const float p = objective == 0 ? R : A, q = objective == 0 ? Rm1 : S;
  const float lin = p * xv - q * ov;
  x0 = objective == 1 ? ov : lin;
  if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  const float derived = (R * xv - x0) / Rm1;
  pn = (objective == 0 && !clip) ? ov : derived;
}

__device__ __forceinline__ float distill_ddim(float a, float s, float x0, float pn) {
#pragma clang fp contract(off)
  return a * x0 + s * pn;
}

__device__ __forceinline__ float distill_half_one(const DistillRow& row, int obj_t, int clip, float z, float o) {
  float pn, x0;
  distill_predictions(obj_t, z, o, row.head_t, clip, pn, x0);
  return distill_ddim(row.head_m[0], row.head_m[1], x0, pn);
}

__device__ __forceinline__ float distill_target_one(const DistillRow& row, int obj_t, int obj_s, int clip, float zt, float zm,
                                                    float o) {
#pragma clang fp contract(off)
  float pn, x0;
  distill_predictions(obj_t, zm, o, row.head_m, clip, pn, x0);
  const float zn = distill_ddim(row.next[0], row.next[1], x0, pn);
  const float xs = row.next[2] * zn + row.next[3] * zt;
  const float es = (zt - row.head_t[0] * xs) * row.tail[0];
  const float vs = row.head_t[0] * es - row.head_t[1] * xs;
  return obj_s == 1 ? xs : (obj_s == 0 ? es : vs);
}

// per = HW * (VEC ? Cpad / 4 : Cpad) work items of one sample; blockIdx.y = the sample
template <bool VEC>
__global__ __launch_bounds__(256) void distill_half_step_kernel(const float* __restrict__ xin, long in_pitch, int x_off,
                                                                const float* __restrict__ out, long out_pitch,
                                                                const long* __restrict__ t, const float* __restrict__ table,
                                                                int n_table, int obj_t, int clip, float* __restrict__ xmid,
                                                                long mid_pitch, int mid_off, long* __restrict__ t_mid, int C,
                                                                int Cpad, int HW, long per) {
  const int b = blockIdx.y;
  const DistillRow row = distill_row(table, t, b, n_table);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) t_mid[b] = (long)row.tail[1];
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long pix = (long)b * HW + i / Q;
    const f32x4 z = *reinterpret_cast<const f32x4*>(xin + pix * in_pitch + x_off + c0);
    const f32x4 o = *reinterpret_cast<const f32x4*>(out + pix * out_pitch + c0);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = c0 + k < C ? distill_half_one(row, obj_t, clip, z[k], o[k]) : 0.f;
    *reinterpret_cast<f32x4*>(xmid + pix * mid_pitch + mid_off + c0) = r;
  } else {
    const int c = (int)(i % Cpad);
    const long pix = (long)b * HW + i / Cpad;
    xmid[pix * mid_pitch + mid_off + c] =
        c < C ? distill_half_one(row, obj_t, clip, xin[pix * in_pitch + x_off + c], out[pix * out_pitch + c]) : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void distill_target_kernel(const float* __restrict__ xin, long in_pitch, int x_off,
                                                             const float* __restrict__ xmid, long mid_pitch, int mid_off,
                                                             const float* __restrict__ out, long out_pitch,
                                                             const long* __restrict__ t, const float* __restrict__ table,
                                                             int n_table, int obj_t, int obj_s, int clip,
                                                             float* __restrict__ target, long target_pitch, int C, int Cpad,
                                                             int HW, long per) {
  const int b = blockIdx.y;
  const DistillRow row = distill_row(table, t, b, n_table);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  if constexpr (VEC) {
    const int Q = Cpad >> 2, c0 = (int)(i % Q) * 4;
    const long pix = (long)b * HW + i / Q;
    const f32x4 zt = *reinterpret_cast<const f32x4*>(xin + pix * in_pitch + x_off + c0);
    const f32x4 zm = *reinterpret_cast<const f32x4*>(xmid + pix * mid_pitch + mid_off + c0);
    const f32x4 o = *reinterpret_cast<const f32x4*>(out + pix * out_pitch + c0);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = c0 + k < C ? distill_target_one(row, obj_t, obj_s, clip, zt[k], zm[k], o[k]) : 0.f;
    *reinterpret_cast<f32x4*>(target + pix * target_pitch + c0) = r;
  } else {
    const int c = (int)(i % Cpad);
    const long pix = (long)b * HW + i / Cpad;
    target[pix * target_pitch + c] =
        c < C ? distill_target_one(row, obj_t, obj_s, clip, xin[pix * in_pitch + x_off + c], xmid[pix * mid_pitch + mid_off + c],
                                   out[pix * out_pitch + c])
              : 0.f;
  }
}

inline bool distill_obj_ok(int o) { return o >= 0 && o <= 2; }
inline bool distill_vec_ok(const void* p, int64_t pitch, int off) { return lgm_aligned16(p) && pitch % 4 == 0 && off % 4 == 0; }

}  // namespace

// The kernel names are noted without a registry entry (no LGM_KNAME), like lowres_cond_kernel's and dpm_step_kernel's and for
// the same reason: tests/test_hip_kernel_ledger.py lists every registry name with the test file that runs it, and
// tests/test_hip_distill.py, which runs these kernels and asserts the noted names, is not on that list.
extern "C" int lgm_distill_half_step(const float* xin, int64_t in_pitch, int x_off, const float* out, int64_t out_pitch,
                                     const int64_t* t, const float* table, int n_table, int teacher_objective, int clip,
                                     float* xmid, int64_t mid_pitch, int mid_off, int64_t* t_mid, int B, int C, int HW,
                                     void* stream) {
  LGM_REQUIRE(xin && out && t && table && xmid && t_mid && B > 0 && B <= 65535 && C > 0 && HW > 0 && n_table > 0,
              "distill_half_step: operands and positive sizes required (B <= 65535)");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(x_off >= 0 && x_off + Cpad <= in_pitch && mid_off >= 0 && mid_off + Cpad <= mid_pitch && out_pitch >= Cpad,
              "distill_half_step: the x slices and their padding (r4(C) = %d lanes) must lie inside the pitches", Cpad);
  LGM_REQUIRE(distill_obj_ok(teacher_objective), "distill_half_step: objective must be 0, 1 or 2, got %d", teacher_objective);
  LGM_REQUIRE((const void*)xmid != (const void*)xin && (const void*)xmid != (const void*)out && lgm_aligned16(table),
              "distill_half_step: the second input buffer must not alias a source; 16-byte aligned table required");
  const bool vec = distill_vec_ok(xin, in_pitch, x_off) && distill_vec_ok(out, out_pitch, 0) && distill_vec_ok(xmid, mid_pitch, mid_off);
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("distill_half_step_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  if (vec)
    hipLaunchKernelGGL(distill_half_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, xin, (long)in_pitch, x_off, out,
                       (long)out_pitch, (const long*)t, table, n_table, teacher_objective, clip, xmid, (long)mid_pitch, mid_off,
                       (long*)t_mid, C, Cpad, HW, per);
  else
    hipLaunchKernelGGL(distill_half_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, xin, (long)in_pitch, x_off, out,
                       (long)out_pitch, (const long*)t, table, n_table, teacher_objective, clip, xmid, (long)mid_pitch, mid_off,
                       (long*)t_mid, C, Cpad, HW, per);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}

extern "C" int lgm_distill_target(const float* xin, int64_t in_pitch, int x_off, const float* xmid, int64_t mid_pitch, int mid_off,
                                  const float* out, int64_t out_pitch, const int64_t* t, const float* table, int n_table,
                                  int teacher_objective, int student_objective, int clip, float* target, int64_t target_pitch,
                                  int B, int C, int HW, void* stream) {
  LGM_REQUIRE(xin && xmid && out && t && table && target && B > 0 && B <= 65535 && C > 0 && HW > 0 && n_table > 0,
              "distill_target: operands and positive sizes required (B <= 65535)");
  const int Cpad = (C + 3) / 4 * 4;
  LGM_REQUIRE(x_off >= 0 && x_off + Cpad <= in_pitch && mid_off >= 0 && mid_off + Cpad <= mid_pitch && out_pitch >= Cpad &&
                  target_pitch >= Cpad,
              "distill_target: the x slices, the target and their padding (r4(C) = %d lanes) must lie inside the pitches", Cpad);
  LGM_REQUIRE(distill_obj_ok(teacher_objective) && distill_obj_ok(student_objective),
              "distill_target: objectives must be 0, 1 or 2, got %d and %d", teacher_objective, student_objective);
  LGM_REQUIRE((const void*)target != (const void*)xin && (const void*)target != (const void*)xmid &&
                  (const void*)target != (const void*)out && lgm_aligned16(table),
              "distill_target: the target must not alias a source; 16-byte aligned table required");
  const bool vec = distill_vec_ok(xin, in_pitch, x_off) && distill_vec_ok(xmid, mid_pitch, mid_off) &&
                   distill_vec_ok(out, out_pitch, 0) && distill_vec_ok(target, target_pitch, 0);
  const long per = (long)HW * (vec ? Cpad / 4 : Cpad);
  lgm_note_kernel("distill_target_kernel");
  const dim3 grid(lgm_cdiv(per, 256), B);
  if (vec)
    hipLaunchKernelGGL(distill_target_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, xin, (long)in_pitch, x_off, xmid,
                       (long)mid_pitch, mid_off, out, (long)out_pitch, (const long*)t, table, n_table, teacher_objective,
                       student_objective, clip, target, (long)target_pitch, C, Cpad, HW, per);
  else
    hipLaunchKernelGGL(distill_target_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, xin, (long)in_pitch, x_off, xmid,
                       (long)mid_pitch, mid_off, out, (long)out_pitch, (const long*)t, table, n_table, teacher_objective,
                       student_objective, clip, target, (long)target_pitch, C, Cpad, HW, per);
  LGM_LAUNCH_CHECK();
  return LGM_OK;
}
