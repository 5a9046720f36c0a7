// atom_guide_mask_f16 / atom_guide_advance: guided decoding over a token-level automaton (the rules are guide_math.h).
//
// Mask: one launch, a grid of (tile, row) workgroups of 256 threads as in penalize.hip; a tile is 2048 elements, thread t owns
// elements 8 t .. 8 t + 7 of it: one 16-byte load of logits, ONE BYTE of the state's mask row (bits 8 t .. 8 t + 7 of the tile: a
// wave reads 64 consecutive bytes, 16 mask words), one 16-byte store where the bases and leading dimensions allow; 2-byte accesses
// otherwise and in a row's tail.  The row's state is one scalar load, the same in every thread of the workgroup, and it is compared
// with 0 .. num_states - 1 before it scales the mask row's address.  A FREE / DEAD / bad row is copied (in place: nothing to do, the
// workgroup returns before it loads anything); a bad row's first workgroup sets ATOM_GUIDE_BAD_STATE.
// No workgroup reads what another writes and none waits: a row of 32,000 tokens is 16 workgroups.
//
// Advance: one launch, one thread per sequence: a binary search of tokens[b] in the sorted edge tokens of state[b], the state
// rewritten in place.  Every index is clamped into its array before it is used (guide_math.h advance).
//
// Walk rows (atom_guide_walk_rows): one launch, one thread per sequence as the advance: the commit of the last
// speculative step (one element of the thread's own row states), then Q chained searches over the step's input row, the row states
// and the forced drafts written with plain stores.  guide_math.h walk.
#include "common.h"
#include "guide_math.h"
#include "vocab_row.h"

namespace atom {

namespace gm = guide;

constexpr int kGuideThreads = 256;
constexpr int kGuideTile = 8 * kGuideThreads;
constexpr int kGuideMaxBatch = 65535;                          // rows are the grid's y
constexpr int kGuideAdvThreads = 64;

struct GuideMaskParams {
  const uint16_t *logits;
  int64_t ld;
  int vocab;
  const int32_t *state;
  const uint32_t *mask;
  int64_t mask_ld, num_states;
  uint16_t *out;
  int64_t out_ld;
  int32_t *status;
};

template <bool VEC>
__global__ __launch_bounds__(kGuideThreads) void guide_mask_kernel(GuideMaskParams p) {
  const int tid = threadIdx.x, row = blockIdx.y, vocab = p.vocab;
  const int e0 = blockIdx.x * kGuideTile + tid * 8;
  const int n = min(8, vocab - e0);                            // <= 0: a thread past the row's end
  const uint16_t *lrow = p.logits + (int64_t)row * p.ld;
  uint16_t *orow = p.out + (int64_t)row * p.out_ld;
  const int32_t s = p.state[row];                              // wave-uniform
  const int kind = gm::row_kind(s, p.num_states);
  if (kind == gm::kCopiedBad && blockIdx.x == 0 && tid == 0) atomicOr(p.status, gm::kBadState);
  if (n <= 0 || (kind != gm::kMasked && orow == lrow)) return;

  uint32_t lg[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) lg[c] = 0;
  // load8 / store8 of vocab_row.h written out: through the helpers this kernel compiles to other code (the masks of the 16-byte form are kept)
  if (VEC && n == 8) {
    const v4u x = *reinterpret_cast<const v4u *>(lrow + e0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { lg[2 * i] = x[i] & 0xFFFFu; lg[2 * i + 1] = x[i] >> 16; }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < n) lg[c] = lrow[e0 + c];
  }
  if (kind == gm::kMasked) {
    // byte e0 / 8 of the row (little endian: bits e0 .. e0 + 7 of word e0 / 32); e0 < vocab, so the word is below ceil(vocab / 32)
    const uint32_t byte = reinterpret_cast<const uint8_t *>(p.mask + (int64_t)s * p.mask_ld)[e0 >> 3];
#pragma unroll
    for (int c = 0; c < 8; ++c) lg[c] = gm::select(lg[c], gm::allowed(byte, (uint32_t)c));   // bits past n are computed, never stored
  }
  if (VEC && n == 8) {
    v4u x;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = (lg[2 * i] & 0xFFFFu) | (lg[2 * i + 1] << 16);
    *reinterpret_cast<v4u *>(orow + e0) = x;
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < n) orow[e0 + c] = (uint16_t)lg[c];
  }
}

__global__ __launch_bounds__(kGuideAdvThreads) void guide_advance_kernel(int32_t *state, const int64_t *tokens, int batch, const int32_t *indptr,
                                                                          const int32_t *edge_tok, const int32_t *edge_next, int64_t num_states,
                                                                          int64_t num_edges, int32_t *status) {
  const int b = blockIdx.x * kGuideAdvThreads + threadIdx.x;
  if (b >= batch) return;
  int32_t bits = 0;
  const int32_t s = state[b];
  const int32_t s1 = gm::advance(s, tokens[b], indptr, edge_tok, edge_next, num_states, num_edges, bits);
  if (s1 != s) state[b] = s1;
  if (bits) atomicOr(status, bits);
}

// one thread per sequence: the commit of the last step, then the walk over this step's rows.  Everything a thread reads or writes is
// its own sequence's: state[b], adds[b], row_state[b][.], input_ids[b][.]; the tables are read-only.
__global__ __launch_bounds__(kGuideAdvThreads) void guide_walk_rows_kernel(int32_t *state, const int32_t *adds, int32_t *row_state,
                                                                            int64_t *input_ids, int64_t ids_ld, int batch, int rows,
                                                                            const int32_t *indptr, const int32_t *edge_tok,
                                                                            const int32_t *edge_next, int64_t num_states, int64_t num_edges,
                                                                            int32_t force, int32_t *status) {
  const int b = blockIdx.x * kGuideAdvThreads + threadIdx.x;
  if (b >= batch) return;
  int32_t bits = 0;
  const int32_t s = state[b];
  int32_t *row = row_state + (int64_t)b * rows;
  int64_t *ids = input_ids ? input_ids + (int64_t)b * ids_ld : nullptr;
  const int32_t s1 = gm::walk(s, adds[b], row, ids, row, rows, indptr, edge_tok, edge_next, num_states, num_edges, force != 0, bits);
  if (s1 != s) state[b] = s1;
  if (bits) atomicOr(status, bits);
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_guide_mask_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const int32_t *state, const uint32_t *mask,
                        int64_t mask_ld, int64_t num_states, void *out, int64_t out_ld, int32_t *status, void *stream) {
  if (!logits || !state || !mask || !out || !status) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > kGuideMaxBatch || vocab < 1 || vocab > guide::kMaxVocab || ld < vocab || out_ld < vocab ||
      mask_ld < (vocab + 31) / 32 || num_states < 1 || num_states > INT32_MAX || mask_ld > INT32_MAX || num_states * mask_ld > INT32_MAX ||
      (out == logits && out_ld != ld))
    return ATOM_ERR_SHAPE;
  if (off_by(logits, 1u) || off_by(out, 1u) || off_by(state, 3u) || off_by(mask, 3u) || off_by(status, 3u)) return ATOM_ERR_ALIGN;
  GuideMaskParams p{static_cast<const uint16_t *>(logits), ld, (int)vocab, state, mask, mask_ld, num_states, static_cast<uint16_t *>(out), out_ld, status};
  // every row of both buffers starts on 16 bytes (the mask is read by the byte: it needs no more than its element's alignment)
  const bool vec = rows_aligned16(logits, ld) && rows_aligned16(out, out_ld);
  const dim3 grid((unsigned)((vocab + kGuideTile - 1) / kGuideTile), (unsigned)batch);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL((guide_mask_kernel<true>), grid, dim3(kGuideThreads), 0, s, p);
  else hipLaunchKernelGGL((guide_mask_kernel<false>), grid, dim3(kGuideThreads), 0, s, p);
  return check_launch();
}

int atom_guide_advance(int32_t *state, const int64_t *tokens, int64_t batch, const int32_t *indptr, const int32_t *edge_tok,
                       const int32_t *edge_next, int64_t num_states, int64_t num_edges, int32_t *status, void *stream) {
  if (!state || !tokens || !indptr || !status || (num_edges > 0 && (!edge_tok || !edge_next))) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > kGuideMaxBatch || num_states < 1 || num_states >= INT32_MAX || num_edges < 0 || num_edges > INT32_MAX) return ATOM_ERR_SHAPE;
  if (off_by(state, 3u) || off_by(tokens, 7u) || off_by(indptr, 3u) || off_by(edge_tok, 3u) || off_by(edge_next, 3u) ||
      off_by(status, 3u))
    return ATOM_ERR_ALIGN;
  const unsigned blocks = (unsigned)((batch + kGuideAdvThreads - 1) / kGuideAdvThreads);
  hipLaunchKernelGGL(guide_advance_kernel, dim3(blocks), dim3(kGuideAdvThreads), 0, reinterpret_cast<hipStream_t>(stream), state, tokens,
                     (int)batch, indptr, edge_tok, edge_next, num_states, num_edges, status);
  return check_launch();
}

int atom_guide_walk_rows(int32_t *state, const int32_t *adds, int32_t *row_state, int64_t *input_ids, int64_t ids_ld, int64_t batch,
                         int64_t rows, const int32_t *indptr, const int32_t *edge_tok, const int32_t *edge_next, int64_t num_states,
                         int64_t num_edges, int32_t force, int32_t *status, void *stream) {
  if (!state || !adds || !row_state || !indptr || !status || (num_edges > 0 && (!edge_tok || !edge_next))) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > kGuideMaxBatch || rows < 1 || rows > guide::kMaxWalkRows || ids_ld < rows || num_states < 1 ||
      num_states >= INT32_MAX || num_edges < 0 || num_edges > INT32_MAX)
    return ATOM_ERR_SHAPE;
  if (off_by(state, 3u) || off_by(adds, 3u) || off_by(row_state, 3u) || off_by(input_ids, 7u) || off_by(indptr, 3u) ||
      off_by(edge_tok, 3u) || off_by(edge_next, 3u) || off_by(status, 3u))
    return ATOM_ERR_ALIGN;
  const unsigned blocks = (unsigned)((batch + kGuideAdvThreads - 1) / kGuideAdvThreads);
  hipLaunchKernelGGL(guide_walk_rows_kernel, dim3(blocks), dim3(kGuideAdvThreads), 0, reinterpret_cast<hipStream_t>(stream), state, adds,
                     row_state, input_ids, ids_ld, (int)batch, (int)rows, indptr, edge_tok, edge_next, num_states, num_edges, force, status);
  return check_launch();
}

}  // extern "C"
