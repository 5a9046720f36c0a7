// The arithmetic of atom_penalize_f16 (include/atom_hip.h), once: the state word of a (sequence, token), the neutral
// test of a row, the FP32 lines that penalise one logit, the final rounding.  Every function is a pure function of its arguments, the
// same on the host and on the device; the library is built with -ffp-contract=off, so each FP32 operation below is rounded once, as
// written (the product of line 3 and its difference are two operations).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOM_PENALTY_HD __host__ __device__ __forceinline__
#else
#define ATOM_PENALTY_HD inline
#endif

namespace atom {
namespace penalty {

constexpr int kMaxVocab = 1 << 18;
constexpr int kMaxBias = 512;              // bias entries per row
constexpr uint32_t kPromptFlag = 0x8000u;  // state word: the token occurs in the prompt
constexpr uint32_t kCountMask = 0x7FFFu;   //             how often it was fed back as a generated token, saturating
constexpr uint32_t kQuietNaN = 0x7E00u;

// the state word after one more occurrence: the count saturates at 32767, the prompt flag stays
ATOM_PENALTY_HD uint32_t count_up(uint32_t word) { return (word & kCountMask) == kCountMask ? word : word + 1u; }

// rep <= 0 or NaN: the repetition penalty is off (returns false); otherwise rep is clamped to [2^-10, 2^10], as the sampler's T
ATOM_PENALTY_HD bool repetition(float rep, float &r) {
  r = 1.0f;
  if (!(rep > 0.0f)) return false;
  r = rep < 0x1p-10f ? 0x1p-10f : (rep > 0x1p+10f ? 0x1p+10f : rep);
  return true;
}

// a row whose parameters change nothing (its bias list is the caller's half of the test): every word of it is copied
ATOM_PENALTY_HD bool neutral(bool rep_on, float r, float pres, float freq) { return (!rep_on || r == 1.0f) && pres == 0.0f && freq == 0.0f; }

// lines 1 .. 4 on one logit (fp16 bits) under its state word; r is the clamped repetition penalty
ATOM_PENALTY_HD float penalise(uint32_t bits, uint32_t word, bool rep_on, float r, float pres, float freq) {
  float l = (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
  const uint32_t count = word & kCountMask;
  if (word != 0 && rep_on) l = l > 0.0f ? l / r : l * r;
  const float t = freq * (float)count;
  l = l - t;
  if (count > 0) l = l - pres;
  return l;
}

// line 6: FP32 -> fp16 bits, round to nearest even.  IEEE leaves a NaN's payload open; a computed NaN is written as 0x7E00, so the
// result is one word on every machine (the sampler reads any NaN as -inf).
ATOM_PENALTY_HD uint32_t half_bits(float l) {
  if (l != l) return kQuietNaN;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(l));   // the value above is already rounded to FP32: no conversion fused into the operation that made it
#endif
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)l);
}

}  // namespace penalty
}  // namespace atom
