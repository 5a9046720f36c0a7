// The RoPE angle of the table path of the INT4 paged-KV attention kernels (kv_i4.hip: decode, prefill_i4.hip: prefill and grouped-query
// attention).  The kernels work in REVOLUTIONS (v_sin_f32 / v_cos_f32 take revolutions): a frequency is revolutions per position, an
// angle the fractional part of position x frequency.  The theta path (rope_theta / rope_scale) forms that product in FP32, rounds it
// once and takes the fractional part (sincos_rev in either file): at position 131,072 and the fastest pair the product is ~2e4
// revolutions and its rounding ~1e-3 revolution.  The table path (rope_table: a frequency per pair, used as loaded) forms it exactly:
//   p = RN(pos * t), e = fma(pos, t, -p) is the product's rounding error EXACTLY, so (p - floor(p)) + e is the angle to the last bit
//   of the fraction -- two more VALU instructions per sine / cosine pair, whatever the position.  (p - floor(p) is exact; the sum may
//   leave [0, 1) by e: v_sin / v_cos take any argument within +-256 revolutions.)
#pragma once
#include "common.h"

namespace atom {

// The prefill kernel's K staging is VALU-bound, so it takes the exact product only for key tiles whose first position is at least this
// (a workgroup-uniform test per tile).  Below it the rounded product is off by at most 8192 * 0.16 * 2^-24 ~ 8e-5 revolution.
constexpr int kRopeExactFrom = 8192;

// sin / cos of 2*pi*pos*t, the product formed exactly
__device__ __forceinline__ void rope_sincos_exact(float pos, float t, float &s, float &c) {
  const float p = pos * t;
  const float e = __builtin_fmaf(pos, t, -p);
  const float turn = (p - floorf(p)) + e;
  s = __builtin_amdgcn_sinf(turn);
  c = __builtin_amdgcn_cosf(turn);
}

}  // namespace atom
