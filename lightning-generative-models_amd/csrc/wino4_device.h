// Device code the F(4x4, 3x3) Winograd kernels share: winograd4.hip (32-tile workgroups), winograd4l.hip (light workgroups)
// and winograd4_wgrad.hip (weight gradient) pull namespace lgmwino4dev into their own.  Only what is the same text in all
// of them lives here; the tile geometries, transforms, MFMA loops and epilogues stay with their kernels.
#pragma once
#include "lgm_common.h"

namespace lgmwino4dev {
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int KC = 8;              // reduction channels per phase
constexpr int NXI = 36;            // points of the 6 x 6 transform domain

__device__ __forceinline__ f32x4 add4(const f32x4 a, const f32x4 b) { return a + b; }
// hipcc emits four v_sub_f32 for a vector subtraction (the neg modifiers of v_pk_add_f32 are not selected)
__device__ __forceinline__ f32x4 sub4(const f32x4 a, const f32x4 b) {
  f32x2 lo, hi;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]"
      : "=v"(lo)
      : "v"(__builtin_shufflevector(a, a, 0, 1)), "v"(__builtin_shufflevector(b, b, 0, 1)));
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]"
      : "=v"(hi)
      : "v"(__builtin_shufflevector(a, a, 2, 3)), "v"(__builtin_shufflevector(b, b, 2, 3)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
__device__ __forceinline__ f32x4 fma4(const float c, const f32x4 a, const f32x4 b) {   // c * a + b
  return __builtin_elementwise_fma(f32x4{c, c, c, c}, a, b);
}
__device__ __forceinline__ f32x2 fma2(const float c, const f32x2 a, const f32x2 b) {
  return __builtin_elementwise_fma(f32x2{c, c}, a, b);
}

// Buffer resource over [ptr, ptr + bytes): loads past the end return zeros (the convolutions' padding).  Every word goes
// through readfirstlane: the descriptor is wave-uniform by construction, and the compiler must know it (SGPRs).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_buffer_rsrc(const float* ptr, unsigned bytes) {
  const unsigned long long ab = reinterpret_cast<unsigned long long>(ptr);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)ab);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(ab >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                           __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// Arguments both convolution kernels take (each appends its own: winograd4.hip, winograd4l.hip); the host fills them in
// wino4_host.h.
struct ConvArgs {
  const float* a;      // gathered activations, NHWC
  const float* u;      // transformed weights [N/64][C/8][36][2][2][32][4] (wino4_weights_kernel)
  const float* bias;
  const float* res;
  float* out;
  long a_pitch, res_pitch, out_pitch;
  int B, H, W;
  int C;               // reduction channels
  int N;               // produced channels
  int tb_h, tb_w, tiles_n, nbg;
  int splits, pps, units;
  int tn_slowest;      // unit order, see conv_unit
  int xcd_ranges;      // 1: an XCD takes a contiguous unit range (default); 0: unit = blockIdx (LGM_WINO4_NO_XCD_RANGES=1, A/B)
  float* ws;
  long ws_stride;
};

// The unit of this workgroup: 64-channel block tn, split of the reduction, tile block (thi, twi) of image group bg.
struct ConvUnit {
  int tn, split, twi, thi, bg;
};
__device__ __forceinline__ ConvUnit conv_unit(const ConvArgs& p) {
  // Hardware deals consecutive workgroup ids to the eight XCDs round-robin, each with its own 4 MB 16-way L2.  With
  // unit = blockIdx the 32 (64) workgroups an XCD runs together are units x, x + 8, ...: the same tile block of images
  // four apart, i.e. patches whose addresses differ by multiples of 1 MB and fall on the SAME L2 sets - they evict each
  // other between the four phases that share a 128-byte line (FETCH_SIZE 85 MB per launch for 33.5 MB of input at
  // 64 -> 64 @ 32 x 32, B = 128; the F(2x2) kernel, which always walked XCD-contiguous unit ranges: 38 MB).  An XCD takes a
  // CONTIGUOUS unit range instead: neighbouring tile blocks and images, addresses spread over all sets, halo rows and
  // the channel blocks of one tile block shared in one L2.
  int L = (p.xcd_ranges && (gridDim.x & 7) == 0) ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
  // Two unit orders (host: wino4_host.h): channel block fastest - the channel blocks and splits of one tile block sit in
  // one L2 and share its patch (large maps: the input is the big operand) - or channel block SLOWEST - an XCD works on
  // one or two (channel block, split) slices of U and streams the images past them (8 x 8 maps with hundreds of channels:
  // U is the big operand, 9 ... 19 MB, and every XCD would otherwise stream all of it)
  ConvUnit q;
  if (p.tn_slowest) {
    q.twi = L % p.tb_w;
    L /= p.tb_w;
    q.thi = L % p.tb_h;
    L /= p.tb_h;
    q.bg = L % p.nbg;
    L /= p.nbg;
    q.split = L % p.splits;
    q.tn = L / p.splits;
  } else {
    q.tn = L % p.tiles_n;
    L /= p.tiles_n;
    q.split = L % p.splits;
    L /= p.splits;
    q.twi = L % p.tb_w;
    L /= p.tb_w;
    q.thi = L % p.tb_h;
    q.bg = L / p.tb_h;
  }
  return q;
}

}  // namespace lgmwino4dev
