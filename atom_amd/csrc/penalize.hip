// atom_penalize_f16: repetition / presence / frequency penalties and a per-row logit bias on fp16 logits, with the per-(sequence,
// token) occurrence state advanced in the same launch (the arithmetic is penalty_math.h).
//
// One launch, a grid of (tile, row) workgroups of 256 threads; a tile is 2048 elements, thread t owns elements 8 t .. 8 t + 7 of it
// (one 16-byte load of logits, one of state, one 16-byte store where the bases and leading dimensions allow; 2-byte accesses
// otherwise and in a row's tail).  No workgroup reads what another writes and none waits: a row of 32,000 tokens is 16 workgroups.
//   count   the thread that owns element fed[b] of row b increments that state word itself (saturating, the prompt flag kept) and
//           penalises with the new word: no atomics, no second launch, no order between workgroups
//   neutral rows (parameters that change nothing, no bias id >= 0) copy their words and load no state but the owner's one word
//   bias    (max_bias > 0) the tile's FP32 results go to LDS, the workgroup's threads stride over the row's bias entries and add
//           those whose id lies inside the tile and below vocab (an LDS float add: duplicate ids give one of the addition orders),
//           mark them, and every thread converts and stores its own eight.  max_bias == 0 is a build without that stage.
// An element that is neither seen nor biased is stored with the bits it was loaded with.
// Safety: fed and the bias ids are COMPARED with element positions the thread already owns (below vocab, inside its tile); nothing
// read from device memory becomes a global address.
// atom_penalize_rows_f16 (further down) is the same arithmetic for the verify rows of a speculative step.
#include "common.h"
#include "penalty_math.h"
#include "vocab_row.h"

namespace atom {

namespace pm = penalty;

constexpr int kPenThreads = 256;
constexpr int kPenTile = 8 * kPenThreads;
constexpr int kPenBiasPerThread = pm::kMaxBias / kPenThreads;
constexpr int kPenMaxBatch = 65535;                            // rows are the grid's y

struct PenalizeParams {
  const uint16_t *logits;
  int64_t ld;
  int vocab;
  uint16_t *state;
  int64_t state_ld;
  const int64_t *fed;
  const float *rep, *pres, *freq;
  const int32_t *bias_ids;
  const float *bias_vals;
  int max_bias;
  uint16_t *out;
  int64_t out_ld;
};

template <bool BIAS, bool VEC>
__global__ __launch_bounds__(kPenThreads) void penalize_kernel(PenalizeParams p) {
  __shared__ float s_val[BIAS ? kPenTile : 1];                 // [element & 7][thread]: a thread's eight are 256 dwords apart
  __shared__ uint8_t s_hit[BIAS ? kPenTile : 1];
  const int tid = threadIdx.x, row = blockIdx.y, vocab = p.vocab;
  const int t0 = blockIdx.x * kPenTile, e0 = t0 + tid * 8;
  const int n = min(8, vocab - e0);                            // <= 0: a thread past the row's end (it still meets the barriers)
  const uint16_t *lrow = p.logits + (int64_t)row * p.ld;
  uint16_t *orow = p.out + (int64_t)row * p.out_ld;
  uint16_t *srow = p.state ? p.state + (int64_t)row * p.state_ld : nullptr;

  float r;
  const bool rep_on = pm::repetition(p.rep ? p.rep[row] : 1.0f, r);
  const float pres = p.pres ? p.pres[row] : 0.0f, freq = p.freq ? p.freq[row] : 0.0f;
  bool neutral = pm::neutral(rep_on, r, pres, freq);

  uint32_t lg[8], st[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) lg[c] = st[c] = 0;
  if (n > 0) load8<VEC>(lrow + e0, n, lg);                     // in flight while the bias list decides the row's neutrality

  int ids[BIAS ? kPenBiasPerThread : 1];
  float vals[BIAS ? kPenBiasPerThread : 1];
  if constexpr (BIAS) {
    int any = 0;
#pragma unroll
    for (int i = 0; i < kPenBiasPerThread; ++i) {
      const int j = i * kPenThreads + tid;
      ids[i] = -1;
      vals[i] = 0.0f;
      if (j < p.max_bias) {
        ids[i] = p.bias_ids[(int64_t)row * p.max_bias + j];
        vals[i] = p.bias_vals[(int64_t)row * p.max_bias + j];
      }
      any |= ids[i] >= 0;
    }
    neutral = !__syncthreads_or(any) && neutral;
  }

  if (srow) {
    if (!neutral && n > 0) load8<VEC>(srow + e0, n, st);
    if (p.fed) {
      const int64_t f = p.fed[row];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < n && f == (int64_t)(e0 + c)) {                 // at most one thread of the row, one of its own positions
          const uint32_t w = neutral ? (uint32_t)srow[e0 + c] : st[c];
          const uint32_t w1 = pm::count_up(w);
          if (w1 != w) srow[e0 + c] = (uint16_t)w1;
          st[c] = w1;
        }
    }
  }
  if (neutral) {                                               // the same in every thread of the workgroup
    if (n > 0) store8<VEC>(orow + e0, n, lg);
    return;
  }

  uint32_t res[8];
  if constexpr (BIAS) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      s_val[c * kPenThreads + tid] = pm::penalise(lg[c], st[c], rep_on, r, pres, freq);
      s_hit[c * kPenThreads + tid] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPenBiasPerThread; ++i) {
      const int id = ids[i];
      if (id >= t0 && id < t0 + kPenTile && id < vocab) {
        const int o = id - t0, slot = (o & 7) * kPenThreads + (o >> 3);
        atomicAdd(&s_val[slot], vals[i]);
        s_hit[slot] = 1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool touched = st[c] != 0 || s_hit[c * kPenThreads + tid] != 0;
      res[c] = touched ? pm::half_bits(s_val[c * kPenThreads + tid]) : lg[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) res[c] = st[c] != 0 ? pm::half_bits(pm::penalise(lg[c], st[c], rep_on, r, pres, freq)) : lg[c];
  }
  if (n > 0) store8<VEC>(orow + e0, n, res);
}

template <bool BIAS>
static int launch_penalize(const PenalizeParams &p, bool vec, int batch, hipStream_t s) {
  const dim3 grid((unsigned)((p.vocab + kPenTile - 1) / kPenTile), (unsigned)batch);
  if (vec) hipLaunchKernelGGL((penalize_kernel<BIAS, true>), grid, dim3(kPenThreads), 0, s, p);
  else hipLaunchKernelGGL((penalize_kernel<BIAS, false>), grid, dim3(kPenThreads), 0, s, p);
  return check_launch();
}

// atom_penalize_rows_f16: the verify rows of speculative decoding.  One workgroup per (tile, SEQUENCE): it counts the
// sequence's pending tokens into the state words it owns (the only workgroup that touches them: no atomics, no order between
// workgroups, no second launch), keeps the tile's words in registers and walks the sequence's rows, counting draft j in registers
// before row j is penalised as penalize_kernel does it.  The state is read once per sequence, drafts never reach it.  Row j + 1 is
// loaded while row j is worked on (two rows in flight, not all nine).  Pending tokens, drafts and bias ids are COMPARED with
// positions the thread owns; none becomes an address.
constexpr int kPenMaxRows = 9;

struct PenalizeRowsParams {
  const uint16_t *logits;                                      // null: the commit alone
  int64_t ld;
  int vocab, rows;
  uint16_t *state;
  int64_t state_ld;
  const int64_t *input_ids;
  int64_t ids_ld;
  const int64_t *commit_tokens;
  int64_t commit_ld;
  const int32_t *commit_counts;
  const float *rep, *pres, *freq;
  const int32_t *bias_ids;
  const float *bias_vals;
  int max_bias;
  uint16_t *out;
  int64_t out_ld;
};

template <bool BIAS, bool VEC>
__global__ __launch_bounds__(kPenThreads) void penalize_rows_kernel(PenalizeRowsParams p) {
  __shared__ float s_val[BIAS ? kPenTile : 1];
  __shared__ uint8_t s_hit[BIAS ? kPenTile : 1];
  const int tid = threadIdx.x, seq = blockIdx.y, vocab = p.vocab;
  const int t0 = blockIdx.x * kPenTile, e0 = t0 + tid * 8;
  const int n = min(8, vocab - e0);                            // <= 0: a thread past the row's end (it still meets the barriers)
  const int rows = p.logits ? p.rows : 0;
  const uint16_t *lrow = p.logits + (int64_t)seq * rows * p.ld;
  uint16_t *orow = p.out + (int64_t)seq * rows * p.out_ld;
  uint16_t *srow = p.state + (int64_t)seq * p.state_ld;

  float r;
  const bool rep_on = pm::repetition(p.rep ? p.rep[seq] : 1.0f, r);
  const float pres = p.pres ? p.pres[seq] : 0.0f, freq = p.freq ? p.freq[seq] : 0.0f;
  bool neutral = pm::neutral(rep_on, r, pres, freq);

  uint32_t lg[8], st[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) lg[c] = st[c] = 0;
  if (rows > 0 && n > 0) load8<VEC>(lrow + e0, n, lg);

  int ids[BIAS ? kPenBiasPerThread : 1];
  float vals[BIAS ? kPenBiasPerThread : 1];
  if constexpr (BIAS) {
    int any = 0;
#pragma unroll
    for (int i = 0; i < kPenBiasPerThread; ++i) {
      const int j = i * kPenThreads + tid;
      ids[i] = -1;
      vals[i] = 0.0f;
      if (j < p.max_bias) {
        ids[i] = p.bias_ids[(int64_t)seq * p.max_bias + j];
        vals[i] = p.bias_vals[(int64_t)seq * p.max_bias + j];
      }
      any |= ids[i] >= 0;
    }
    neutral = !__syncthreads_or(any) && neutral;
  }
  if (rows == 0) neutral = true;                               // the commit alone: only the owners load their words

  // 1. commit: the pending tokens, in order, once per occurrence, whatever the sequence's parameters are
  int pending = 0;
  if (p.commit_counts) pending = min(max(p.commit_counts[seq], 0), (int)min(p.commit_ld, (int64_t)kPenMaxRows));
  const int64_t *ctok = pending > 0 ? p.commit_tokens + (int64_t)seq * p.commit_ld : nullptr;
  bool mine = false;
  for (int i = 0; i < pending; ++i) mine |= ctok[i] >= (int64_t)e0 && ctok[i] < (int64_t)(e0 + n);
  if (n > 0 && (!neutral || mine)) load8<VEC>(srow + e0, n, st);
  if (mine) {
    uint32_t changed = 0;
    for (int i = 0; i < pending; ++i) {
      const int64_t t = ctok[i];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < n && t == (int64_t)(e0 + c)) {
          const uint32_t w1 = pm::count_up(st[c]);
          if (w1 != st[c]) changed |= 1u << c;
          st[c] = w1;
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (changed >> c & 1u) srow[e0 + c] = (uint16_t)st[c];
  }

  // 2., 3. the rows: draft j is counted in registers, then row j is penalised under those words
  for (int j = 0; j < rows; ++j) {
    uint32_t nxt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) nxt[c] = 0;
    if (j + 1 < rows && n > 0) load8<VEC>(lrow + (int64_t)(j + 1) * p.ld + e0, n, nxt);
    uint16_t *o = orow + (int64_t)j * p.out_ld + e0;
    if (neutral) {                                             // the same in every thread of the workgroup
      if (n > 0) store8<VEC>(o, n, lg);
    } else {
      if (j > 0) {
        const int64_t d = p.input_ids[(int64_t)seq * p.ids_ld + j];
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < n && d == (int64_t)(e0 + c)) st[c] = pm::count_up(st[c]);
      }
      uint32_t res[8];
      if constexpr (BIAS) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          s_val[c * kPenThreads + tid] = pm::penalise(lg[c], st[c], rep_on, r, pres, freq);
          s_hit[c * kPenThreads + tid] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPenBiasPerThread; ++i) {
          const int id = ids[i];
          if (id >= t0 && id < t0 + kPenTile && id < vocab) {
            const int o2 = id - t0, slot = (o2 & 7) * kPenThreads + (o2 >> 3);
            atomicAdd(&s_val[slot], vals[i]);
            s_hit[slot] = 1;
          }
        }
        __syncthreads();                                       // a thread reads its own slots only; the next row's first barrier orders them
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const bool touched = st[c] != 0 || s_hit[c * kPenThreads + tid] != 0;
          res[c] = touched ? pm::half_bits(s_val[c * kPenThreads + tid]) : lg[c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) res[c] = st[c] != 0 ? pm::half_bits(pm::penalise(lg[c], st[c], rep_on, r, pres, freq)) : lg[c];
      }
      if (n > 0) store8<VEC>(o, n, res);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) lg[c] = nxt[c];
  }
}

template <bool BIAS>
static int launch_penalize_rows(const PenalizeRowsParams &p, bool vec, int batch, hipStream_t s) {
  const dim3 grid((unsigned)((p.vocab + kPenTile - 1) / kPenTile), (unsigned)batch);
  if (vec) hipLaunchKernelGGL((penalize_rows_kernel<BIAS, true>), grid, dim3(kPenThreads), 0, s, p);
  else hipLaunchKernelGGL((penalize_rows_kernel<BIAS, false>), grid, dim3(kPenThreads), 0, s, p);
  return check_launch();
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_penalize_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, int16_t *state, int64_t state_ld, const int64_t *fed,
                      const float *rep, const float *pres, const float *freq, const int32_t *bias_ids, const float *bias_vals,
                      int64_t max_bias, void *out, int64_t out_ld, void *stream) {
  if (!logits || !out || (fed && !state) || (max_bias > 0 && (!bias_ids || !bias_vals))) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > kPenMaxBatch || vocab < 1 || vocab > penalty::kMaxVocab || ld < vocab || out_ld < vocab ||
      (state && state_ld < vocab) || max_bias < 0 || max_bias > penalty::kMaxBias || (out == logits && out_ld != ld))
    return ATOM_ERR_SHAPE;
  if (off_by(logits, 1u) || off_by(out, 1u) || off_by(state, 1u) || off_by(fed, 7u) || off_by(rep, 3u) || off_by(pres, 3u) || off_by(freq, 3u) ||
      (max_bias > 0 && (off_by(bias_ids, 3u) || off_by(bias_vals, 3u))))
    return ATOM_ERR_ALIGN;
  PenalizeParams p{static_cast<const uint16_t *>(logits), ld, (int)vocab, reinterpret_cast<uint16_t *>(state), state_ld, fed, rep, pres, freq,
                   bias_ids, bias_vals, (int)max_bias, static_cast<uint16_t *>(out), out_ld};
  const bool vec = rows_aligned16(logits, ld) && rows_aligned16(out, out_ld) && rows_aligned16(state, state_ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return max_bias > 0 ? launch_penalize<true>(p, vec, (int)batch, s) : launch_penalize<false>(p, vec, (int)batch, s);
}

int atom_penalize_rows_f16(const void *logits, int64_t ld, int64_t batch, int64_t rows, int64_t vocab, int16_t *state, int64_t state_ld,
                           const int64_t *input_ids, int64_t ids_ld, const int64_t *commit_tokens, int64_t commit_ld,
                           const int32_t *commit_counts, const float *rep, const float *pres, const float *freq, const int32_t *bias_ids,
                           const float *bias_vals, int64_t max_bias, void *out, int64_t out_ld, void *stream) {
  const bool scored = logits != nullptr;
  if ((logits == nullptr) != (out == nullptr) || (commit_tokens == nullptr) != (commit_counts == nullptr) || (!scored && !commit_tokens) ||
      !state || (scored && !input_ids) || (scored && max_bias > 0 && (!bias_ids || !bias_vals)))
    return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > kPenMaxBatch || rows < 1 || rows > kPenMaxRows || batch * rows > INT32_MAX || vocab < 1 ||
      vocab > penalty::kMaxVocab || state_ld < vocab || (commit_tokens && commit_ld < 1) || max_bias < 0 || max_bias > penalty::kMaxBias ||
      (scored && (ld < vocab || out_ld < vocab || ids_ld < rows || (out == logits && out_ld != ld))))
    return ATOM_ERR_SHAPE;
  if (off_by(logits, 1u) || off_by(out, 1u) || off_by(state, 1u) || off_by(input_ids, 7u) || off_by(commit_tokens, 7u) ||
      off_by(commit_counts, 3u) || off_by(rep, 3u) || off_by(pres, 3u) || off_by(freq, 3u) ||
      (max_bias > 0 && (off_by(bias_ids, 3u) || off_by(bias_vals, 3u))))
    return ATOM_ERR_ALIGN;
  PenalizeRowsParams p{static_cast<const uint16_t *>(logits), ld, (int)vocab, (int)rows, reinterpret_cast<uint16_t *>(state), state_ld,
                       input_ids, ids_ld, commit_tokens, commit_ld, commit_counts, rep, pres, freq, bias_ids, bias_vals,
                       scored ? (int)max_bias : 0, static_cast<uint16_t *>(out), out_ld};
  const bool vec = rows_aligned16(logits, ld) && rows_aligned16(out, out_ld) && rows_aligned16(state, state_ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return p.max_bias > 0 ? launch_penalize_rows<true>(p, vec, (int)batch, s) : launch_penalize_rows<false>(p, vec, (int)batch, s);
}

}  // extern "C"
