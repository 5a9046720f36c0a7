// The rules of atom_guide_mask_f16 and atom_guide_advance (include/atom_hip.h), once: what a state value means for a
// row, whether a token's bit is set in a mask word, what a masked element becomes, and one step of the automaton over its CSR edges.
// Integer rules only; every function is a pure function of its arguments, the same on the host and on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOM_GUIDE_HD __host__ __device__ __forceinline__
#else
#define ATOM_GUIDE_HD inline
#endif

namespace atom {
namespace guide {

constexpr int kMaxVocab = 1 << 18;
constexpr int32_t kFree = -1;              // ATOM_GUIDE_FREE: the sequence is unconstrained
constexpr int32_t kDead = -2;              // ATOM_GUIDE_DEAD: the sequence left its language; unconstrained from then on
constexpr int32_t kRejected = 1;           // ATOM_GUIDE_REJECTED
constexpr int32_t kBadState = 2;           // ATOM_GUIDE_BAD_STATE
constexpr uint32_t kNegInf = 0xFC00u;      // fp16 -inf

enum RowKind : int { kMasked = 0, kCopied = 1, kCopiedBad = 2 };

// what the mask op does with a row in state s; s is compared here, before it is ever used as an index
ATOM_GUIDE_HD int row_kind(int32_t s, int64_t num_states) {
  if (s >= 0 && (int64_t)s < num_states) return kMasked;
  return (s == kFree || s == kDead) ? kCopied : kCopiedBad;
}

// token v's bit of its mask word (word v >> 5 of the state's mask row)
ATOM_GUIDE_HD bool allowed(uint32_t word, uint32_t v) { return ((word >> (v & 31u)) & 1u) != 0; }

// one element of a masked row: its own bits where allowed, -inf otherwise
ATOM_GUIDE_HD uint32_t select(uint32_t bits, bool allow) { return allow ? bits : kNegInf; }

ATOM_GUIDE_HD int32_t clamp_edge(int32_t x, int64_t num_edges) { return x < 0 ? 0 : ((int64_t)x > num_edges ? (int32_t)num_edges : x); }

// one step of sequence state s over token t (compared as int64); the bits to set in the status word are OR-ed into `bits`.  No index
// outside 0 .. num_states of indptr or 0 .. num_edges - 1 of the edge arrays is read, whatever the tables hold.
ATOM_GUIDE_HD int32_t advance(int32_t s, int64_t t, const int32_t *indptr, const int32_t *edge_tok, const int32_t *edge_next,
                              int64_t num_states, int64_t num_edges, int32_t &bits) {
  if (s == kFree || s == kDead) return s;
  if (s < 0 || (int64_t)s >= num_states) { bits |= kBadState; return kDead; }
  int32_t lo = clamp_edge(indptr[s], num_edges), hi = clamp_edge(indptr[s + 1], num_edges);
  if (hi < lo) hi = lo;
  const int32_t end = hi;
  while (lo < hi) {                                            // the first edge whose token is not below t
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)edge_tok[mid] < t) lo = mid + 1; else hi = mid;
  }
  if (lo >= end || (int64_t)edge_tok[lo] != t) { bits |= kRejected; return kDead; }
  const int32_t nxt = edge_next[lo];
  if (nxt < 0 || (int64_t)nxt >= num_states) { bits |= kBadState; return kDead; }
  return nxt;
}

}  // namespace guide
}  // namespace atom
