// OCP microscaling (MX) block quantiser arithmetic, shared by the activation and the weight quantiser of gemm_mxfp4.hip
// (contract: include/atom_hip.h, "MXFP4 W4A4"; restated in numpy by tests/mx_ref.py).
#pragma once
#include "common.h"

namespace atom {

// element formats: mantissa bits, exponent bias, largest finite code, emax = exponent of the largest finite value
struct MxE2M1 { static constexpr int MB = 1, BIAS = 1, MAXC = 7, EMAX = 2, SIGN = 8; };        // 0 .. 6
struct MxE4M3 { static constexpr int MB = 3, BIAS = 7, MAXC = 0x7E, EMAX = 8, SIGN = 0x80; };   // 0 .. 448 (0x7F is NaN)
struct MxE2M3 { static constexpr int MB = 3, BIAS = 1, MAXC = 31, EMAX = 2, SIGN = 0x20; };     // 0 .. 7.5 (the MXFP6 activation)

// E8M0 scale byte of a block whose absolute maximum is amax (finite, from fp16 values: a normal FP32 number or 0)
template <class F>
__device__ __forceinline__ int mx_scale_byte(float amax) {
  if (amax == 0.f) return 127;
  const int ex = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127;     // floor(log2(amax))
  return min(max(ex - F::EMAX, -127), 127) + 127;
}

// 2^-(byte - 127): the factor that takes a value onto the element grid (exact in FP32 for every byte a fp16 block can get)
__device__ __forceinline__ float mx_inv_scale(int byte) { return __uint_as_float((unsigned)(254 - byte) << 23); }

// code of v * inv: round to nearest even on the grid of F, saturate, sign bit where v < 0.  With ye the exponent of y (at least the
// smallest normal's), m = rint(y / 2^(ye - MB)) counts grid steps from 0 (subnormals) or 2^MB (normals); m = 2^(MB + 1) carries into
// the next exponent through the same sum.
template <class F>
__device__ __forceinline__ unsigned mx_code(float v, float inv) {
  const float y = fabsf(v) * inv;
  const int ye = max((int)((__float_as_uint(y) >> 23) & 0xff) - 127, 1 - F::BIAS);
  const float m = rintf(y * __uint_as_float((unsigned)(127 + F::MB - ye) << 23));
  const int c = min(((ye + F::BIAS) << F::MB) + (int)m - (1 << F::MB), (int)F::MAXC);
  return (unsigned)c | (v < 0.f ? (unsigned)F::SIGN : 0u);
}

}  // namespace atom
