// Counter-based dropout mask: Philox4x32-10 (Salmon et al., SC'11) evaluated in registers, never written to memory.
//
// For an activation [B, HW, C] (C % 4 == 0) the four channels c .. c + 3 of one 16-byte access share one Philox call:
//   n = (b * HW + pix) * C + c   (the LOGICAL element index: pitches and pad lanes play no part),  q = n >> 2 (64 bit),
//   counter = (q & 0xffffffff, q >> 32, layer, pass),  key = the two halves of the step's 64-bit key (read from the device),
//   element c + e is KEPT iff output word e >= thr,  thr = min(2^32 - 1, floor(p * 2^32)) (host),
//   kept values are multiplied by scale = float32(1 / (1 - p)) (host, division in double), dropped ones become +0.
// tests/dropout_ref.py restates this in numpy.
#pragma once

#include "lgm_common.h"

struct LgmDrop {
  const unsigned* key;   // device: key[0] = low half, key[1] = high half
  unsigned layer, pass, thr;
  float scale;
};

__device__ __forceinline__ void lgm_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                  unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    if (r < 9) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// v (channels c .. c + 3 of logical element index n, n % 4 == 0) -> kept ? fl32(v * scale) : +0
__device__ __forceinline__ f32x4 lgm_drop4(const LgmDrop& d, unsigned k0, unsigned k1, long n, f32x4 v) {
  const unsigned long q = (unsigned long)n >> 2;
  unsigned w[4];
  lgm_philox4x32_10((unsigned)(q & 0xffffffffu), (unsigned)(q >> 32), d.layer, d.pass, k0, k1, w);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = w[e] >= d.thr ? v[e] * d.scale : 0.f;
  return o;
}
