// atom_logprob_f16: log-probability and rank of a target token, and the top-n tokens with their log-probabilities, per row of fp16
// logits.  The arithmetic is the sampler's (sample_math.h): canonical keys, the 2^40 fixed-point weight at T = 1, an
// integer row sum Z, lz = log_z(Z), lp_i = (l_i - m) - lz.  Every sum is an integer sum and every choice a maximum of distinct
// integers, so a row's result is a function of its bits and its target alone: no atomics anywhere, no order of additions to depend on.
//
// One workgroup of 1024 threads per row; no workgroup reads what another writes, none waits.  Thread t holds elements
// 8 (1024 q + t) .. + 7 of "slab" q as 4 dwords of 16-bit keys.  Up to 32,768 tokens the row is read from memory once and kept in
// registers (4 slabs); longer rows are loaded again in every pass, from L2 (profiles/logprob/README.md has both timed).
//   pass A  maximum key m (wave shuffles, LDS)
//   pass B  per-thread u64 sum of the weights and the count of the tokens in front of the target (key above the target's, or equal
//           with a lower index), reduced by wave shuffles and LDS.  Either half is skipped when nothing asks for it.
//   top-n   n rounds of "the largest (key, ~index) below the previous winner": every thread holds the largest of its own elements
//           that has not won yet, a round is one 64-bit maximum over the workgroup, and only the winner's thread rescans its elements.
//           No histogram, no gather, no sort.
// Safety: a target is compared with 0 and vocab before it is used as an index; a top-n index is an element position below vocab.
#include "common.h"
#include "sample_math.h"
#include "vocab_row.h"

#include <type_traits>

namespace atom {

namespace sm = sample;

constexpr int kLogprobThreads = 1024;
constexpr int kLogprobWaves = kLogprobThreads / 64;
constexpr int kLogprobSlab = 8 * kLogprobThreads;   // elements per slab
constexpr int kLogprobRegSlabs = 4;                 // the register-resident form: 16 VGPRs of keys
constexpr int kLogprobMaxTop = 32;

struct LogprobParams {
  const uint16_t *logits;
  int64_t ld;
  int vocab;
  const int64_t *targets;
  float *logprob;
  int32_t *rank;
  int top_n;
  int64_t *top_ids;
  float *top_logprobs;
};

struct LogprobShared {
  uint32_t red_key[kLogprobWaves];
  uint32_t red_cnt[kLogprobWaves];
  unsigned long long red_z[kLogprobWaves];
  unsigned long long red_best[2][kLogprobWaves];   // top-n rounds alternate between the two, one barrier per round
  unsigned long long top[kLogprobMaxTop];
};

template <int NQ, bool VEC>
__global__ __launch_bounds__(kLogprobThreads) void logprob_kernel(LogprobParams p) {
  __shared__ LogprobShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_id = blockIdx.x, vocab = p.vocab;
  const uint16_t *row = p.logits + (int64_t)row_id * p.ld;
  const int nslab = (vocab + kLogprobSlab - 1) / kLogprobSlab;
  uint32_t v[NQ > 0 ? NQ * 4 : 4];

  // every pass over the row: f(first element of the thread's 8, their 4 dwords of keys) -- the registers, or (NQ == 0) loaded again
  auto slabs = [&](auto &&f) {
    if constexpr (NQ > 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q < nslab) f((q * kLogprobThreads + tid) * 8, &v[q * 4]);
    } else {
#pragma unroll 4
      for (int q = 0; q < nslab; ++q) {                        // unrolled: four slabs' loads in flight, not one
        uint32_t d[4];
        load_slab<VEC>(row, vocab, (q * kLogprobThreads + tid) * 8, d);
        f((q * kLogprobThreads + tid) * 8, d);
      }
    }
  };

  // ---- pass A: the maximum key
  if constexpr (NQ > 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) load_slab<VEC>(row, vocab, (q * kLogprobThreads + tid) * 8, &v[q * 4]);
  }
  uint32_t mx = 0;
  slabs([&](int, const uint32_t *d) {
#pragma unroll
    for (int c = 0; c < 8; ++c) mx = max(mx, key_at(d, c));
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
  if (lane == 0) S.red_key[wave] = mx;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kLogprobWaves; ++i) mx = max(mx, S.red_key[i]);
  const bool all_neg = mx <= sm::kKeyNegInf;                   // nothing but -inf / NaN: every lp is -inf
  const float mval = sm::key_value(mx);

  // the target: compared first, an address only when it is in range
  const int64_t t64 = p.targets ? p.targets[row_id] : -1;
  const bool in_range = p.targets && t64 >= 0 && t64 < (int64_t)vocab;
  const int t = in_range ? (int)t64 : 0;
  const uint32_t kt = in_range ? sm::canon_key(row[t]) : 0u;
  const bool want_rank = in_range && p.rank;
  const bool want_z = !all_neg && (p.top_n > 0 || (in_range && p.logprob));

  // ---- pass B: the weight sum and the tokens in front of the target
  uint64_t z = 0;
  uint32_t cnt = 0;
  auto pass_b = [&](auto with_z, auto with_rank) {
    slabs([&](int e0, const uint32_t *d) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t key = key_at(d, c);
        if (key != 0) {
          if constexpr (decltype(with_z)::value) z += sm::weight(sm::key_value(key), mval, 1.0f);
          if constexpr (decltype(with_rank)::value) cnt += (key > kt || (key == kt && e0 + c < t)) ? 1u : 0u;
        }
      }
    });
  };
  if (want_z && want_rank) pass_b(std::true_type{}, std::true_type{});
  else if (want_z) pass_b(std::true_type{}, std::false_type{});
  else if (want_rank) pass_b(std::false_type{}, std::true_type{});
  float lz = 0.0f;
  if (want_z || want_rank) {                                   // uniform over the workgroup
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      z += shfl_xor_u64(z, d);
      cnt += (uint32_t)__shfl_xor(cnt, d, 64);
    }
    if (lane == 0) { S.red_z[wave] = z; S.red_cnt[wave] = cnt; }
    __syncthreads();
    z = 0;
    cnt = 0;
    if (wave == 0) {                                           // the only wave that writes results
#pragma unroll
      for (int i = 0; i < kLogprobWaves; ++i) { z += S.red_z[i]; cnt += S.red_cnt[i]; }
      if (want_z) lz = sm::log_z(z);
    }
  }
  if (tid == 0 && p.targets) {
    if (p.logprob) p.logprob[row_id] = !in_range ? 0.0f : (all_neg ? -__builtin_inff() : (sm::key_value(kt) - mval) - lz);
    if (p.rank) p.rank[row_id] = in_range ? (int32_t)cnt : -1;
  }
  if (p.top_n <= 0) return;

  // ---- top-n: round j finds the j-th token of the order, the largest (key, ~index) below round j - 1's.  Every thread keeps the
  // largest of its own elements that has not won yet; a round is one 64-bit maximum over the workgroup, after which only the winner's
  // thread (the values are distinct) looks through its elements again.  0: the thread, or the row, has run out of tokens.
  auto largest_below = [&](uint64_t bound) {
    uint64_t best = 0;
    slabs([&](int e0, const uint32_t *d) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t key = key_at(d, c);
        const uint64_t comp = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)(e0 + c);
        if (key != 0 && comp < bound && comp > best) best = comp;
      }
    });
    return best;
  };
  uint64_t mine = largest_below(~0ull);
  for (int j = 0; j < p.top_n; ++j) {
    uint64_t best = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t o = shfl_xor_u64(best, d);
      best = o > best ? o : best;
    }
    if (lane == 0) S.red_best[j & 1][wave] = best;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLogprobWaves; ++i) {
      const uint64_t o = S.red_best[j & 1][i];
      best = o > best ? o : best;
    }
    if (tid == 0) S.top[j] = best;
    if (best != 0 && mine == best) mine = largest_below(best);
  }
  __syncthreads();
  if (tid < p.top_n) {
    const uint64_t comp = S.top[tid];
    const uint32_t key = (uint32_t)(comp >> 32);
    const int64_t o = (int64_t)row_id * p.top_n + tid;
    const bool none = comp == 0;
    p.top_ids[o] = none ? -1 : (int64_t)(uint32_t)~(uint32_t)comp;
    p.top_logprobs[o] = (none || all_neg) ? -__builtin_inff() : (sm::key_value(key) - mval) - lz;
  }
}

template <int NQ>
static int launch_logprob(const LogprobParams &p, bool vec, int rows, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((logprob_kernel<NQ, true>), dim3((unsigned)rows), dim3(kLogprobThreads), 0, s, p);
  else hipLaunchKernelGGL((logprob_kernel<NQ, false>), dim3((unsigned)rows), dim3(kLogprobThreads), 0, s, p);
  return check_launch();
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_logprob_f16(const void *logits, int64_t ld, int64_t rows, int64_t vocab, const int64_t *targets, float *logprob, int32_t *rank,
                     int64_t top_n, int64_t *top_ids, float *top_logprobs, void *stream) {
  if (!logits || (top_n >= 1 && (!top_ids || !top_logprobs))) return ATOM_ERR_INVALID_ARG;
  if (top_n == 0 && (!targets || (!logprob && !rank))) return ATOM_ERR_INVALID_ARG;   // nothing to do
  if (rows < 1 || rows > 0x7fffffff || vocab < 1 || vocab > sample::kMaxVocab || ld < vocab || top_n < 0 || top_n > kLogprobMaxTop)
    return ATOM_ERR_SHAPE;
  if (off_by(logits, 1u) || off_by(targets, 7u) || off_by(logprob, 3u) || off_by(rank, 3u) || off_by(top_ids, 7u) || off_by(top_logprobs, 3u))
    return ATOM_ERR_ALIGN;
  LogprobParams p{static_cast<const uint16_t *>(logits), ld, (int)vocab, targets, logprob, rank, (int)top_n, top_ids, top_logprobs};
  const bool vec = rows_aligned16(logits, ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vocab <= kLogprobRegSlabs * kLogprobSlab) return launch_logprob<kLogprobRegSlabs>(p, vec, (int)rows, s);
  return launch_logprob<0>(p, vec, (int)rows, s);
}

}  // extern "C"
