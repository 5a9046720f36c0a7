// Speculative decoding on the device: atom_spec_draft_ngram guesses K tokens per sequence from the sequence's own
// history, atom_spec_accept compares the guesses with the tokens the model chose at the K + 1 verify rows, commits the agreed prefix
// and prepares the next step.  Both are one launch, read nothing back and are capturable; the integer rules are spec_math.h.  (The third
// piece, the page-table step with per-sequence counts, is atom_kv_step_rows_i4 in kv_step.hip.)
//
// ---- atom_spec_draft_ngram: one workgroup of 512 threads per sequence, no workgroup reads what another writes.
// The last min(8, len) tokens go to LDS once.  Thread t then walks the candidate END positions e = t, t + 512, ... (0 .. len - 2), four
// per trip with their loads issued together: the token at e is compared with the history's last token first, and only an equal one
// is followed backwards (spec::match_len, at most ngram_max tokens).  Every end yields the word (match length, e); the winner -- the
// longest n-gram, then its most recent occurrence -- is the workgroup's maximum (wave64 shuffles, then 8 words in LDS), and threads
// 0 .. K - 1 write the drafts.  What bounds it: the latency of len / 2048 dependent trips through L2; a 128K history is 64 trips.
// Safety: every read is hist[i] with 0 <= i < len <= hist_cap inside the row; a length outside 1 .. hist_cap reads nothing.
//
// ---- atom_spec_accept: ONE workgroup of 256 threads, thread t takes rows t, t + 256, ...  A row's K + 1 targets and K drafts are
// loaded into registers before anything is written, so the row's own input_ids may be overwritten in place.  `done` is the AND over
// all rows of this launch (wave vote, 4 words in LDS): nothing is carried between launches and no other workgroup exists to wait for.
// Safety: the positions written into `tokens` and `hist` are compared with max_new and hist_cap; token values are copied, never used
// as an address.
#include "common.h"
#include "spec_math.h"
#include "vocab_row.h"

namespace atom {

constexpr int kDraftThreads = 512;
constexpr int kDraftUnroll = 4;
constexpr int kAcceptThreads = 256;

struct SpecDraftParams {
  const int32_t *hist, *hist_len;
  int64_t *out;
  int64_t out_ld;
  int hist_cap, nmin, nmax, K;
};

__global__ __launch_bounds__(kDraftThreads) void spec_draft_kernel(SpecDraftParams p) {
  __shared__ int32_t s_suf[spec::kMaxNgram];
  __shared__ unsigned long long s_best[kDraftThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int32_t *hist = p.hist + b * p.hist_cap;
  int64_t *out = p.out + b * p.out_ld;
  const int len = spec::clamp_len(p.hist_len[b], p.hist_cap);
  if (len == 0) {                                            // (uniform over the workgroup)
    if (tid < p.K) out[tid] = 0;
    return;
  }
  if (tid < spec::kMaxNgram) s_suf[tid] = tid < len ? hist[len - 1 - tid] : 0;
  __syncthreads();
  const int32_t last = s_suf[0];

  unsigned long long best = 0;
  for (int e0 = tid; e0 < len - 1; e0 += kDraftUnroll * kDraftThreads) {
    int32_t t[kDraftUnroll];
#pragma unroll
    for (int u = 0; u < kDraftUnroll; ++u) {
      const int e = e0 + u * kDraftThreads;
      t[u] = e < len - 1 ? hist[e] : 0;
    }
#pragma unroll
    for (int u = 0; u < kDraftUnroll; ++u) {
      const int e = e0 + u * kDraftThreads;
      if (e < len - 1 && t[u] == last) {
        const unsigned long long w = spec::draft_word(spec::match_len(hist, s_suf, e, p.nmax), e, p.nmin);
        best = w > best ? w : best;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(best >> 32), d, 64), lo = __shfl_xor((unsigned)best, d, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o > best ? o : best;
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kDraftThreads / 64; ++k) best = s_best[k] > best ? s_best[k] : best;
  if (tid < p.K) out[tid] = spec::draft_token(hist, len, best, tid);
}

struct SpecAcceptParams {
  const int64_t *targets;
  int64_t *input_ids;
  int32_t *n_out;
  const int32_t *budget;
  int64_t *tokens;
  int32_t *hist, *hist_len, *adds;
  int64_t *draw;
  int32_t *accepted, *steps, *done;
  int batch, K, max_new, hist_cap;
};

__global__ __launch_bounds__(kAcceptThreads) void spec_accept_kernel(SpecAcceptParams p) {
  __shared__ int s_all[kAcceptThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, Q = p.K + 1;
  int all = 1;
  for (int64_t b = tid; b < p.batch; b += kAcceptThreads) {
    int64_t tg[spec::kMaxDraft + 1], dr[spec::kMaxDraft];
#pragma unroll
    for (int j = 0; j <= spec::kMaxDraft; ++j) tg[j] = j < Q ? p.targets[b * Q + j] : 0;
#pragma unroll
    for (int j = 0; j < spec::kMaxDraft; ++j) dr[j] = j < K ? p.input_ids[b * Q + 1 + j] : 0;
    const int32_t n_out = p.n_out[b], budget = p.budget[b], hist_len = p.hist_len[b];
    const int e = spec::emit_count(spec::accept_count(dr, tg, K), budget, n_out);
    int64_t lastt = 0;
#pragma unroll
    for (int i = 0; i <= spec::kMaxDraft; ++i)
      if (i < e) {
        const int64_t at = (int64_t)n_out + i, ht = (int64_t)hist_len + i;
        if (at >= 0 && at < p.max_new) p.tokens[b * p.max_new + at] = tg[i];
        if (ht >= 0 && ht < p.hist_cap) p.hist[b * p.hist_cap + ht] = (int32_t)tg[i];
        lastt = tg[i];
      }
    p.adds[b] = e;
    if (e > 0) {                                             // (e > 0 implies n_out + e <= budget: no overflow)
      p.n_out[b] = n_out + e;
      p.hist_len[b] = (int32_t)((uint32_t)hist_len + (uint32_t)e);
      p.input_ids[b * Q] = lastt;
      p.draw[b] = (int64_t)n_out + e;
      p.accepted[b] += e - 1;
      p.steps[b] += 1;
    }
    all &= (int64_t)n_out + e >= (int64_t)budget;
  }
  all = __all(all);
  if (lane == 0) s_all[wave] = all;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < kAcceptThreads / 64; ++k) all &= s_all[k];
    p.done[0] = all;
  }
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_spec_draft_ngram(const int32_t *hist, const int32_t *hist_len, int64_t batch, int64_t hist_cap, int ngram_min, int ngram_max,
                          int K, int64_t *out, int64_t out_ld, void *stream) {
  if (!hist || !hist_len || !out) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > 0x7fffffff || hist_cap < 1 || hist_cap > 0x7fffffff) return ATOM_ERR_SHAPE;
  if (K < 1 || K > spec::kMaxDraft || ngram_min < 1 || ngram_max < ngram_min || ngram_max > spec::kMaxNgram || out_ld < K) return ATOM_ERR_SHAPE;
  if (off_by(hist, 3u) || off_by(hist_len, 3u) || off_by(out, 7u)) return ATOM_ERR_ALIGN;
  SpecDraftParams p{hist, hist_len, out, out_ld, (int)hist_cap, ngram_min, ngram_max, K};
  hipLaunchKernelGGL(spec_draft_kernel, dim3((unsigned)batch), dim3(kDraftThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  return check_launch();
}

int atom_spec_accept(const int64_t *targets, int64_t *input_ids, int32_t *n_out, const int32_t *budget, int64_t *tokens, int32_t *hist,
                     int32_t *hist_len, int32_t *adds, int64_t *draw, int32_t *accepted, int32_t *steps, int32_t *done, int64_t batch,
                     int K, int64_t max_new, int64_t hist_cap, void *stream) {
  if (!targets || !input_ids || !n_out || !budget || !tokens || !hist || !hist_len || !adds || !draw || !accepted || !steps || !done)
    return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > 0x7fffffff || K < 1 || K > spec::kMaxDraft) return ATOM_ERR_SHAPE;
  if (max_new < 1 || max_new > 0x7fffffff || hist_cap < 1 || hist_cap > 0x7fffffff) return ATOM_ERR_SHAPE;
  if (off_by(targets, 7u) || off_by(input_ids, 7u) || off_by(tokens, 7u) || off_by(draw, 7u)) return ATOM_ERR_ALIGN;
  for (const void *q : {(const void *)n_out, (const void *)budget, (const void *)hist, (const void *)hist_len, (const void *)adds,
                        (const void *)accepted, (const void *)steps, (const void *)done})
    if (off_by(q, 3u)) return ATOM_ERR_ALIGN;
  SpecAcceptParams p{targets, input_ids, n_out, budget, tokens, hist, hist_len, adds, draw, accepted, steps, done,
                     (int)batch, K, (int)max_new, (int)hist_cap};
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(kAcceptThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  return check_launch();
}

}  // extern "C"
