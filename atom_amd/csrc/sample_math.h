// The arithmetic of atom_sample_f16 (include/atom_hip.h), once: the canonical 16-bit key of a logit, the 2^40
// fixed-point weight, the top-p threshold, the Philox draw.  Every function is a pure function of its arguments, the same on the host
// and on the device; the library is built with -ffp-contract=off, so each FP32 operation below is rounded once, as written.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOM_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define ATOM_SAMPLE_HD inline
#endif

namespace atom {
namespace sample {

constexpr uint32_t kKeyNegInf = 0x03FFu;   // key of -inf: the smallest key a logit can have (0 marks "no element")
constexpr int kMaxVocab = 1 << 18;         // a row's weights sum below 2^59

// Step 1 + 2: fp16 bits -> order-preserving 16-bit key of the canonical logit.  NaN -> -inf, +inf -> 65504, -0 -> +0; a larger key
// is a larger logit, equal logits have equal keys.  Keys lie in 0x03FF .. 0xFBFF.
ATOM_SAMPLE_HD uint32_t canon_key(uint32_t u) {
  u &= 0xFFFFu;
  if ((u & 0x7FFFu) > 0x7C00u) u = 0xFC00u;
  else if (u == 0x7C00u) u = 0x7BFFu;
  else if (u == 0x8000u) u = 0u;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}

// the canonical logit of a key, as FP32
ATOM_SAMPLE_HD float key_value(uint32_t key) {
  const uint16_t u = (uint16_t)((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
  return (float)__builtin_bit_cast(_Float16, u);
}

// Step 3: T <= 0 or NaN is greedy (returns false); otherwise T is clamped to [2^-10, 2^10] and r = 1 / T
ATOM_SAMPLE_HD bool inv_temperature(float T, float &r) {
  if (!(T > 0.0f)) return false;
  T = T < 0x1p-10f ? 0x1p-10f : (T > 0x1p+10f ? 0x1p+10f : T);
  r = 1.0f / T;
  return true;
}

// Step 4: the weight of logit l under the row maximum m, 2^40 fixed point (the maximum's weight is exactly 2^40)
ATOM_SAMPLE_HD uint64_t weight(float l, float m, float r) {
  const float d = l - m;
  const float x = (d * r) * 0x1.715476p+0f;
  if (!(x >= -40.0f)) return 0;
  const float n = __builtin_floorf(x);
  const float f = x - n;
  float q = 0x1.f099a6p-10f * f;
  q = q + 0x1.24f70ap-7f;
  q = q * f;
  q = q + 0x1.c9bda2p-5f;
  q = q * f;
  q = q + 0x1.ebca2ap-3f;
  q = q * f;
  q = q + 0x1.62e572p-1f;
  q = q * f;
  q = q + 1.0f;
  const uint64_t mant = (uint32_t)(q * 8388608.0f);              // an integer below 2^25: one conversion instruction, not the 64-bit sequence
  const int sh = 17 + (int)n;
  return sh >= 0 ? mant << sh : mant >> -sh;
}

// atom_logprob_f16: the natural log of a row's weight sum Z (2^40 <= Z < 2^59) over 2^40, as FP32.  The conversion
// of Z rounds to nearest, the log is the double-precision libm's, 40 ln 2 is the double product 40 * 0x1.62e42fefa39efp-1.
ATOM_SAMPLE_HD float log_z(uint64_t Z) { return (float)(::log((double)Z) - 0x1.bb9d3beb8c86bp+4); }

// (a * b) >> 32 of the 96-bit product, a < 2^64, the result below 2^64 (a < 2^59 here)
ATOM_SAMPLE_HD uint64_t mul_shr32(uint64_t a, uint32_t b) { return (a >> 32) * b + (((a & 0xFFFFFFFFull) * b) >> 32); }

// Step 6: P of top_p; p >= 1 (top-p off) is the caller's test
ATOM_SAMPLE_HD uint32_t top_p_fixed(float p) { return p > 0.0f ? (uint32_t)(uint64_t)(p * 4294967296.0f) : 0u; }

// Step 7: word 0 of Philox4x32-10, key (seed lo, seed hi), counter (step lo, step hi, 0, 0)
ATOM_SAMPLE_HD uint32_t philox_word0(uint64_t seed, uint64_t step) {
  uint32_t c0 = (uint32_t)step, c1 = (uint32_t)(step >> 32), c2 = 0, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// The three boundary searches walk the order (key descending, index ascending) with a running token count c and weight sum w, and
// stop at the first token where the predicate holds: kCount  c >= val (top-k), kReach  w >= val (top-p, val >= 1), kPass  w > val (draw)
enum Mode : int { kCount = 0, kReach = 1, kPass = 2 };
ATOM_SAMPLE_HD bool holds(int mode, uint32_t c, uint64_t w, uint64_t val) {
  return mode == kCount ? (uint64_t)c >= val : (mode == kReach ? w >= val : w > val);
}
// ... inside a key of unit weight w1 that starts at (c0, w0) and is known to hold the stop: how many of its tokens the prefix takes (>= 1)
ATOM_SAMPLE_HD uint32_t take(int mode, uint32_t c0, uint64_t w0, uint64_t w1, uint64_t val) {
  if (mode == kCount) return (uint32_t)val - c0;
  if (mode == kReach) return (uint32_t)((val - w0 + w1 - 1) / w1);
  return (uint32_t)((val - w0) / w1) + 1u;
}

}  // namespace sample
}  // namespace atom
