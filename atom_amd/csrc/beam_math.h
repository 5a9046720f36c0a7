// The arithmetic of atom_beam_select (include/atom_hip.h), once: a candidate's score, the order-preserving integer key
// of a score and the 64-bit word whose maximum is the next winner.  Pure functions of their arguments, the same on the host and on the
// device; the library is built with -ffp-contract=off, so the one FP32 addition is rounded once, as written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOM_BEAM_HD __host__ __device__ __forceinline__
#else
#define ATOM_BEAM_HD inline
#endif

namespace atom {
namespace beam {

constexpr int kMaxBeams = 16;   // w_out, w_in
constexpr int kMaxCand = 32;    // C: candidates per live row (the top-n limit of atom_logprob_f16)

// score of candidate c of a live row: one FP32 addition.  Log-probabilities and their sums are never +inf, so -inf + lp is -inf and
// no NaN arises.
ATOM_BEAM_HD float score(float cum, float lp) { return cum + lp; }

// order-preserving 32-bit key of a score: a larger key is a larger score, equal scores (IEEE ==) have equal keys.  -0 is +0; a NaN
// -- which only a corrupted input holds -- ranks as -inf.  Keys lie in 0x007FFFFF (-inf) .. 0xFF800000 (+inf): never 0.
ATOM_BEAM_HD uint32_t score_key(float s) {
  uint32_t u = __builtin_bit_cast(uint32_t, s);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0xFF800000u;
  else if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the word of candidate number idx = parent * C + c (below 2^16): its maximum over all candidates is the first of the order
// (score descending, parent ascending, c ascending).  0 marks "no candidate".
ATOM_BEAM_HD uint64_t order_word(uint32_t key, uint32_t idx) { return ((uint64_t)key << 32) | (0xFFFFFFFFu - idx); }
ATOM_BEAM_HD uint32_t word_index(uint64_t w) { return 0xFFFFFFFFu - (uint32_t)w; }

}  // namespace beam
}  // namespace atom
