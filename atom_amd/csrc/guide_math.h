// The rules of atom_guide_mask_f16 and atom_guide_advance (include/atom_hip.h), once: what a state value means for a
// row, whether a token's bit is set in a mask word, what a masked element becomes, and one step of the automaton over its CSR edges.
// And of atom_guide_walk_rows: the state behind every verify row of a speculative step, and the drafts a state forces.
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

// ---- the verify rows of a speculative step (atom_guide_walk_rows) ----
constexpr int kMaxWalkRows = 9;            // Q = K + 1 with K <= 8 drafts

// advance, except that a token without an edge gives DEAD WITHOUT a status bit: a wrong draft is not an error
ATOM_GUIDE_HD int32_t step(int32_t s, int64_t t, const int32_t *indptr, const int32_t *edge_tok, const int32_t *edge_next,
                           int64_t num_states, int64_t num_edges, int32_t &bits) {
  int32_t b = 0;
  const int32_t s1 = advance(s, t, indptr, edge_tok, edge_next, num_states, num_edges, b);
  bits |= b & kBadState;
  return s1;
}

// true iff state s lies inside the table and its clamped edge range holds exactly one edge; `tok` is then that edge's token
ATOM_GUIDE_HD bool forced(int32_t s, const int32_t *indptr, const int32_t *edge_tok, int64_t num_states, int64_t num_edges, int64_t &tok) {
  if (s < 0 || (int64_t)s >= num_states) return false;
  const int32_t lo = clamp_edge(indptr[s], num_edges);
  int32_t hi = clamp_edge(indptr[s + 1], num_edges);
  if (hi < lo) hi = lo;
  if (hi - lo != 1) return false;
  tok = (int64_t)edge_tok[lo];
  return true;
}

// the committed state after the last step: `state` was the state before its ids[0], `add` the rows it committed, prev[j] the state
// behind its row j.  REJECTED is set here and nowhere else in the walk: a token without an edge has now been emitted.
ATOM_GUIDE_HD int32_t commit(int32_t state, int32_t add, const int32_t *prev, int Q, int32_t &bits) {
  int32_t s = state;
  if (add >= 1 && add <= Q) s = prev[add - 1];
  else if (add != 0) bits |= kBadState;
  if (state != kDead && s == kDead) bits |= kRejected;
  return s;
}

// One sequence's Q verify rows (1 <= Q <= kMaxWalkRows): returns the committed state; row[j] becomes the state behind ids[0 .. j], the
// one row j's logits are masked with.  With `force` a draft ids[j], j >= 1, that follows a state with a single edge is overwritten by
// that edge's token.  `prev` is read (one element) before `row` is written, so the two may be the same array.  ids == nullptr is the
// commit alone: nothing is walked and no row is written.
ATOM_GUIDE_HD int32_t walk(int32_t state, int32_t add, const int32_t *prev, int64_t *ids, int32_t *row, int Q, const int32_t *indptr,
                           const int32_t *edge_tok, const int32_t *edge_next, int64_t num_states, int64_t num_edges, bool force,
                           int32_t &bits) {
  const int32_t s = commit(state, add, prev, Q, bits);
  if (ids == nullptr) return s;
  int32_t r = s;
  for (int j = 0; j < Q; ++j) {
    int64_t t = ids[j];
    if (force && j >= 1) {
      int64_t only;
      if (forced(r, indptr, edge_tok, num_states, num_edges, only)) { t = only; ids[j] = only; }
    }
    r = step(r, t, indptr, edge_tok, edge_next, num_states, num_edges, bits);
    row[j] = r;
  }
  return s;
}

}  // namespace guide
}  // namespace atom
