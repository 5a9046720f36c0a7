// The integer rules of speculative decoding (include/atom_hip.h), once: the n-gram drafter of atom_spec_draft_ngram
// and the accept / emit counts of atom_spec_accept.  Pure functions of their arguments, the same on the host and on the device;
// tests/spec_ref.py restates them line by line.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOM_SPEC_HD __host__ __device__ __forceinline__
#else
#define ATOM_SPEC_HD inline
#endif

namespace atom {
namespace spec {

constexpr int kMaxDraft = 8;    // K: draft tokens per sequence and step
constexpr int kMaxNgram = 8;    // ngram_max

// A row's usable length: a history that is empty or longer than its buffer (a corrupted length) counts as 0 -- its drafts are token 0.
ATOM_SPEC_HD int clamp_len(int len, int hist_cap) { return (len <= 0 || len > hist_cap) ? 0 : len; }

// How many tokens ending at position e equal the history's last tokens, compared LAST TOKEN FIRST, at most nmax:
//   m = the largest i <= min(nmax, e + 1) with hist[e - t] == hist[len - 1 - t] for every t < i.
// `suffix[t]` is hist[len - 1 - t] (t < min(nmax, len)).  The caller passes 0 <= e <= len - 2, so m <= e + 1 <= len - 1 and no index
// outside 0 .. len - 1 is read.
ATOM_SPEC_HD int match_len(const int32_t *hist, const int32_t *suffix, int e, int nmax) {
  const int lim = nmax < e + 1 ? nmax : e + 1;
  int m = 0;
  while (m < lim && hist[e - m] == suffix[m]) ++m;
  return m;
}

// The drafter's rule as ONE maximum.  An occurrence of the last n tokens at start s ends at e = s + n - 1 (0 <= s, s + n <= len - 1:
// n - 1 <= e <= len - 2) and exists exactly when match_len(e) >= n.  "The largest n of ngram_max .. ngram_min with an occurrence, then
// its largest s" is therefore: n* = max over e of min(match_len(e), ngram_max) if that is >= ngram_min, and e* = the largest e whose
// match_len reaches n* (s* = e* - n* + 1 is largest where e* is).  match_len is already capped, so the winner is the maximum of
// word(m, e) = m << 32 | e over the ends with m >= ngram_min; 0 says "no occurrence" (m >= 1 in every real word).
ATOM_SPEC_HD uint64_t draft_word(int m, int e, int ngram_min) { return m >= ngram_min ? ((uint64_t)m << 32) | (uint32_t)e : 0; }

// Draft j of a row of usable length len (> 0) whose winning word is w: the token behind the occurrence, hist[s + n + j] =
// hist[e + 1 + j], while that lies inside the history; otherwise -- and with no occurrence at all -- the last token.
ATOM_SPEC_HD int32_t draft_token(const int32_t *hist, int len, uint64_t w, int j) {
  if (w == 0) return hist[len - 1];
  const int64_t at = (int64_t)(uint32_t)w + 1 + j;
  return at < len ? hist[at] : hist[len - 1];
}

// atom_spec_accept: a = the leading drafts the model agrees with -- drafts[j] (input_ids[b][1 + j]) == targets[b][j], j < K
// (a fixed trip count, so that the device keeps both rows in registers; elements from K on are never read)
ATOM_SPEC_HD int accept_count(const int64_t *drafts, const int64_t *targets, int K) {
  int a = 0;
  bool agreed = true;
#pragma unroll
  for (int j = 0; j < kMaxDraft; ++j) {
    agreed = agreed && j < K && drafts[j] == targets[j];
    a += agreed ? 1 : 0;
  }
  return a;
}

// ... and e = the tokens the step emits: the a agreed drafts and the model's own next token, cut at the row's budget (64-bit: the
// buffers may hold anything)
ATOM_SPEC_HD int emit_count(int a, int32_t budget, int32_t n_out) {
  const int64_t room = (int64_t)budget - (int64_t)n_out;
  const int64_t e = a + 1 < room ? a + 1 : room;
  return e > 0 ? (int)e : 0;
}

}  // namespace spec
}  // namespace atom
