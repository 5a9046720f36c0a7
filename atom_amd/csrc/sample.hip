// atom_sample_f16: exact temperature / top-k / top-p sampling of one token per row of fp16 logits (the arithmetic is
// sample_math.h).  The token is a pure function of the row's bits, (T, k, p, seed) and the step number: every sum is an integer sum,
// so no order of additions or atomics can change it.
//
// One workgroup of 1024 threads per row; no workgroup reads what another writes, none waits.  The row is read from memory ONCE, turned
// into 16-bit order-preserving keys (canon_key) and kept on the CU, two keys per dword: thread t holds elements 8 (1024 q + t) .. + 7
// of "slab" q as 4 dwords.  Up to 32,768 tokens: 4 slabs in registers.  Up to 131,072: 8 slabs in registers (32 VGPRs of the 128 a
// 1024-thread workgroup has per lane) and 8 in LDS (128 KiB, each thread reads back only what it wrote).  Longer rows (up to 2^18)
// fit neither: the same code with every slab loaded again, from L2, in every pass.
// Tokens are ordered by key descending, index ascending; equal keys have equal weights.  So top-k, top-p and the draw are three
// searches for "the first token of the order at which (count, weight sum) passes a bound", each resolved by KEY and never by sorting:
//   pass A  maximum key m (wave shuffles).  m = -inf: token 0.  Greedy rows go straight to pass D with (m, first).
//   pass B  histogram over the key's high byte: token count and weight sum per bin, integer LDS atomics on 8 lane-private copies
//           (bank = copy, so equal keys in a wave collide 8-fold, not 64-fold)
//   search  256 threads scan the bins in descending order (count u32, weight u64); the bin where the bound is first passed is refined
//   pass C  by a count histogram over the low byte of the keys in that bin (its weight sums are count x weight(key)) and a second scan,
//           which yields the boundary key K, how many tokens J of key K the prefix takes, and the prefix's count and weight sum.
//           A prefix found by one search truncates the next (top-k, then top-p inside it, then the draw inside both).
//   pass D  the J-th index, ascending, among the elements with key K: per-slab counts, then a scan over the threads of one slab.
// What bounds it (profiles/sample/README.md): one CU's instruction issue, not the row's bytes -- pass B evaluates the weight function
// and issues one or two LDS atomics per element, 0.5 .. 0.75 ns per element in all, so 32,000 tokens take 21 .. 24 us.
// Safety: a token index is only ever an element position below vocab at which the resident key equals K; k, p, T, seed and step are
// compared and multiplied, never used as an address.
#include "common.h"
#include "sample_math.h"
#include "vocab_row.h"

namespace atom {

namespace sm = sample;

constexpr int kSampleThreads = 1024;
constexpr int kSampleSlab = 8 * kSampleThreads;   // elements per slab
constexpr int kSampleCopies = 8;                  // lane-private histogram copies
constexpr int kSampleLoCopies = 4;                // ... of pass C, where the keys of one bin spread over 256 counters
constexpr int kSampleMaxSlabs = sm::kMaxVocab / kSampleSlab;

struct SampleParams {
  const uint16_t *logits;
  int64_t ld;
  int vocab;
  const float *temperature;
  const int32_t *top_k;
  const float *top_p;
  const uint64_t *seeds;
  const int64_t *step;
  int64_t step_offset;
  int64_t *tokens;
  int rows_per_seq;                             // atom_sample_rows_f16: step is [batch / rows_per_seq]; 0: step is one element
};

struct SampleShared {
  unsigned long long hw[256 * kSampleCopies];   // pass B: weight sums [bin][copy]
  uint32_t hc[256 * kSampleCopies];             //         counts
  uint32_t lc[256 * kSampleLoCopies];           // pass C: counts [low byte][copy]
  unsigned long long scan_w[4];
  uint32_t scan_c[4];
  uint32_t red[kSampleThreads / 64];
  uint32_t slab_tot[kSampleMaxSlabs];
  uint32_t bin, bin_c;                          // search: the bin that holds the stop, the count and weight in front of it
  unsigned long long bin_w;
  uint32_t key, take, count;                    // ... the boundary key, its tokens taken, the prefix's count and weight
  unsigned long long sum;
  int token;
};

// a prefix of the order: every token of a key above `key`, the first `take` of `key` (count tokens, weight sum in all)
struct Prefix {
  int key;
  uint32_t take, count;
  uint64_t sum;
};

// inclusive scan of (c, w) over threads 0 .. 255 (the others pass zeros through); every thread of the workgroup calls it
__device__ __forceinline__ void scan256(uint32_t &c, uint64_t &w, SampleShared &S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < 4) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t tc = __shfl_up(c, d, 64);
      const uint64_t tw = shfl_up_u64(w, d);
      if (lane >= d) { c += tc; w += tw; }
    }
    if (lane == 63) { S.scan_c[wave] = c; S.scan_w[wave] = w; }
  }
  __syncthreads();
  if (wave < 4)
    for (int i = 0; i < wave; ++i) { c += S.scan_c[i]; w += S.scan_w[i]; }
  __syncthreads();
}

template <int NQ, int NL, bool VEC>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(SampleParams p) {
  __shared__ SampleShared S;
  extern __shared__ v4u s_keys[];                              // NL > 0: slabs NQ .. NQ + NL - 1, [slab][thread]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_id = blockIdx.x, vocab = p.vocab;
  const uint16_t *row = p.logits + (int64_t)row_id * p.ld;
  const int nslab = (vocab + kSampleSlab - 1) / kSampleSlab;
  const int copy = lane & (kSampleCopies - 1);
  uint32_t v[NQ > 0 ? NQ * 4 : 4];

  // every pass over the row: f(slab, its 4 dwords of keys) -- the registers, or (NQ == 0) the slab loaded again
  auto slabs = [&](auto &&f) {
    if constexpr (NQ > 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q < nslab) {
          // a copy the optimiser cannot see through: otherwise the 8 keys it unpacks from every slab are kept live ACROSS the passes
          // (common subexpressions), 4 more registers per slab than the packed form, and the 8-slab form spills
          uint32_t d[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            d[i] = v[q * 4 + i];
            asm volatile("" : "+v"(d[i]));
          }
          f(q, d);
        }
      if constexpr (NL > 0) {
        for (int q = NQ; q < nslab; ++q) {
          const v4u x = s_keys[(q - NQ) * kSampleThreads + tid];
          const uint32_t d[4] = {x[0], x[1], x[2], x[3]};
          f(q, d);
        }
      }
    } else {
      for (int q = 0; q < nslab; ++q) {
        uint32_t d[4];
        load_slab<VEC>(row, vocab, (q * kSampleThreads + tid) * 8, d);
        f(q, d);
      }
    }
  };

  for (int i = tid; i < 256 * kSampleCopies; i += kSampleThreads) { S.hw[i] = 0; S.hc[i] = 0; }
  if (tid < kSampleMaxSlabs) S.slab_tot[tid] = 0;
  if (tid == 0) S.token = -1;

  // ---- pass A: the row, once; its maximum key
  if constexpr (NQ > 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) load_slab<VEC>(row, vocab, (q * kSampleThreads + tid) * 8, &v[q * 4]);
    if constexpr (NL > 0) {
      for (int q = NQ; q < nslab; ++q) {
        uint32_t d[4];
        load_slab<VEC>(row, vocab, (q * kSampleThreads + tid) * 8, d);
        s_keys[(q - NQ) * kSampleThreads + tid] = v4u{d[0], d[1], d[2], d[3]};   // read back by this thread only
      }
    }
  }
  uint32_t mx = 0;
  slabs([&](int, const uint32_t *d) {
#pragma unroll
    for (int c = 0; c < 8; ++c) mx = max(mx, key_at(d, c));
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
  if (lane == 0) S.red[wave] = mx;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kSampleThreads / 64; ++i) mx = max(mx, S.red[i]);
  if (mx <= sm::kKeyNegInf) {                                  // nothing but -inf / NaN
    if (tid == 0) p.tokens[row_id] = 0;
    return;
  }

  float r = 1.0f;
  const bool sampled = sm::inv_temperature(p.temperature ? p.temperature[row_id] : 1.0f, r);
  Prefix kept{(int)mx, 1u, 1u, 0};                             // greedy: the first token of the order

  if (sampled) {
    const float mval = sm::key_value(mx);
    const int k = p.top_k ? p.top_k[row_id] : 0;
    const bool top_k_on = k > 0 && k < vocab;                  // off: nothing below needs a token COUNT per bin, half the atomics
    // ---- pass B: count and weight sum per high byte
    slabs([&](int, const uint32_t *d) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t key = key_at(d, c);
        if (key != 0) {
          const int slot = (int)(key >> 8) * kSampleCopies + copy;
          if (top_k_on) atomicAdd(&S.hc[slot], 1u);
          const uint64_t w = sm::weight(sm::key_value(key), mval, r);
          if (w != 0) atomicAdd(&S.hw[slot], (unsigned long long)w);
        }
      }
    });
    __syncthreads();
    uint32_t hcnt = 0;                                         // thread t < 256 owns bin 255 - t: descending order
    uint64_t hsum = 0;
    if (tid < 256)
      for (int i = 0; i < kSampleCopies; ++i) {
        hcnt += S.hc[(255 - tid) * kSampleCopies + i];
        hsum += S.hw[(255 - tid) * kSampleCopies + i];
      }
    int lo_bin = -1;                                           // the bin S.lc describes

    // the first token of `lim` at which holds(mode, count, weight, val); the caller guarantees there is one
    auto search = [&](int mode, uint64_t val, const Prefix &lim) -> Prefix {
      const int lim_bin = lim.key >> 8;
      if (tid == 0) { S.bin = mx >> 8; S.bin_c = 0; S.bin_w = 0; S.key = mx; S.take = 1; S.count = 1; S.sum = 1ull << 40; }
      uint32_t ic = hcnt;
      uint64_t iw = hsum;
      scan256(ic, iw, S);
      if (tid < 256) {
        const int bin = 255 - tid;
        const uint32_t ec = min(ic - hcnt, lim.count);
        const uint64_t ew = bin >= lim_bin ? iw - hsum : lim.sum;
        ic = min(ic, lim.count);
        iw = bin > lim_bin ? iw : lim.sum;
        if (sm::holds(mode, ic, iw, val) && !sm::holds(mode, ec, ew, val)) { S.bin = bin; S.bin_c = ec; S.bin_w = ew; }
      }
      __syncthreads();
      const int bin = S.bin;
      const uint32_t c0 = S.bin_c;
      const uint64_t w0 = S.bin_w;
      // ---- pass C: counts per low byte inside `bin`
      if (bin != lo_bin) {
        for (int i = tid; i < 256 * kSampleLoCopies; i += kSampleThreads) S.lc[i] = 0;
        __syncthreads();
        slabs([&](int, const uint32_t *d) {
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t key = key_at(d, c);
            if ((int)(key >> 8) == bin && key != 0) atomicAdd(&S.lc[(key & 255u) * kSampleLoCopies + (lane & (kSampleLoCopies - 1))], 1u);
          }
        });
        __syncthreads();
        lo_bin = bin;
      }
      uint32_t cnt = 0;
      uint64_t w1 = 0;
      const uint32_t key = ((uint32_t)bin << 8) | (uint32_t)(255 - (tid & 255));
      if (tid < 256) {
        for (int i = 0; i < kSampleLoCopies; ++i) cnt += S.lc[(255 - tid) * kSampleLoCopies + i];
        if (cnt != 0) w1 = sm::weight(sm::key_value(key), mval, r);
      }
      ic = cnt;
      iw = cnt * w1;
      scan256(ic, iw, S);
      if (tid < 256) {
        const int lim_key = bin == lim_bin ? lim.key : -1;
        const uint32_t ec = min(c0 + ic - cnt, lim.count);
        const uint64_t ew = (int)key >= lim_key ? w0 + iw - cnt * w1 : lim.sum;
        ic = min(c0 + ic, lim.count);
        iw = (int)key > lim_key ? w0 + iw : lim.sum;
        if (sm::holds(mode, ic, iw, val) && !sm::holds(mode, ec, ew, val)) {
          const uint32_t j = sm::take(mode, ec, ew, w1, val);
          S.key = key; S.take = j; S.count = ec + j; S.sum = ew + j * w1;
        }
      }
      __syncthreads();
      const Prefix res{(int)S.key, S.take, top_k_on ? S.count : lim.count, S.sum};
      __syncthreads();
      return res;
    };

    // top-k (off: the whole row, Z_k = the sum over the bins), top-p inside it, the draw inside both: one copy of the search's code,
    // up to three trips
    const float top_p = p.top_p ? p.top_p[row_id] : 1.0f;
    const uint64_t seed = p.seeds ? p.seeds[row_id] : 0;
    // the draw number: *step, or (atom_sample_rows_f16) the sequence's base + the row's place inside the sequence
    const int64_t step0 = !p.step ? 0 : (p.rows_per_seq > 0 ? p.step[row_id / p.rows_per_seq] + row_id % p.rows_per_seq : *p.step);
    const uint64_t step = (uint64_t)(step0 + p.step_offset);
    kept = Prefix{-1, 0u, (uint32_t)vocab, 0};
    if (!top_k_on) {
      uint32_t c = 0;
      uint64_t w = hsum;
      scan256(c, w, S);
      if (tid == 255) S.sum = w;
      __syncthreads();
      kept.sum = S.sum;
      __syncthreads();
    }
#pragma nounroll
    for (int mode = top_k_on ? sm::kCount : sm::kReach; mode <= sm::kPass; ++mode) {
      uint64_t val;
      if (mode == sm::kCount) {
        val = (uint64_t)k;
      } else if (mode == sm::kReach) {
        if (top_p >= 1.0f) continue;
        val = sm::mul_shr32(kept.sum, sm::top_p_fixed(top_p));
        val = val > 0 ? val : 1;                               // the prefix is never empty, and the first token's weight is 2^40
      } else {
        val = sm::mul_shr32(kept.sum, sm::philox_word0(seed, step));
      }
      kept = search(mode, val, kept);
    }
  }

  // ---- pass D: the kept.take-th index (ascending) with key kept.key
  const uint32_t K = (uint32_t)kept.key;
  slabs([&](int q, const uint32_t *d) {
    uint32_t n = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) n += key_at(d, c) == K;
    if (n != 0) atomicAdd(&S.slab_tot[q], n);
  });
  __syncthreads();
  int qs = -1;
  uint32_t want = kept.take;                                   // 1-based rank inside slab qs
  for (int q = 0; q < nslab; ++q) {
    const uint32_t t = S.slab_tot[q];
    if (want <= t) { qs = q; break; }
    want -= t;
  }
  if (qs >= 0) {
    uint32_t d[4] = {0, 0, 0, 0};
    if constexpr (NQ > 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (q == qs) { d[0] = v[q * 4]; d[1] = v[q * 4 + 1]; d[2] = v[q * 4 + 2]; d[3] = v[q * 4 + 3]; }
      if constexpr (NL > 0) {
        if (qs >= NQ) {
          const v4u x = s_keys[(qs - NQ) * kSampleThreads + tid];
          d[0] = x[0]; d[1] = x[1]; d[2] = x[2]; d[3] = x[3];
        }
      }
    } else {
      load_slab<VEC>(row, vocab, (qs * kSampleThreads + tid) * 8, d);
    }
    uint32_t n = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) n += key_at(d, c) == K;
    uint32_t inc = n;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t t = __shfl_up(inc, s, 64);
      if (lane >= s) inc += t;
    }
    __syncthreads();                                           // S.red: the maximum's partials have been read by everyone
    if (lane == 63) S.red[wave] = inc;
    __syncthreads();
    for (int i = 0; i < wave; ++i) inc += S.red[i];
    if (inc - n < want && want <= inc) {                       // exactly one thread
      uint32_t left = want - (inc - n);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (key_at(d, c) == K && --left == 0) S.token = (qs * kSampleThreads + tid) * 8 + c;
    }
  }
  __syncthreads();
  if (tid == 0) p.tokens[row_id] = S.token >= 0 ? S.token : 0;
}

constexpr int kSampleRegSlabs = 8, kSampleLdsSlabs = 8;       // the middle form: 32 VGPRs + 128 KiB of LDS
static std::atomic<uint64_t> g_sample_lds_vec{0}, g_sample_lds_scalar{0};

template <int NQ, int NL, bool VEC>
static int launch_sample_as(const SampleParams &p, int batch, hipStream_t s) {
  const int lds = NL * kSampleThreads * 16;
  if (NL > 0) {
    const int st = ensure_max_lds(reinterpret_cast<const void *>(&sample_kernel<NQ, NL, VEC>), lds, VEC ? g_sample_lds_vec : g_sample_lds_scalar);
    if (st != ATOM_OK) return st;
  }
  hipLaunchKernelGGL((sample_kernel<NQ, NL, VEC>), dim3((unsigned)batch), dim3(kSampleThreads), lds, s, p);
  return check_launch();
}

template <int NQ, int NL>
static int launch_sample(const SampleParams &p, bool vec, int batch, hipStream_t s) {
  return vec ? launch_sample_as<NQ, NL, true>(p, batch, s) : launch_sample_as<NQ, NL, false>(p, batch, s);
}

// both entries: rows_per_seq 0 is atom_sample_f16 (step of one element)
static int sample_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const float *temperature, const int32_t *top_k,
                      const float *top_p, const uint64_t *seeds, const int64_t *step, int rows_per_seq, int64_t step_offset,
                      int64_t *tokens, void *stream) {
  if (!logits || !tokens) return ATOM_ERR_INVALID_ARG;
  if (batch < 1 || batch > 0x7fffffff || vocab < 1 || vocab > sample::kMaxVocab || ld < vocab) return ATOM_ERR_SHAPE;
  if (off_by(logits, 1u) || off_by(temperature, 3u) || off_by(top_k, 3u) || off_by(top_p, 3u) || off_by(seeds, 7u) || off_by(step, 7u) || off_by(tokens, 7u))
    return ATOM_ERR_ALIGN;
  SampleParams p{static_cast<const uint16_t *>(logits), ld, (int)vocab, temperature, top_k, top_p, seeds, step, step_offset, tokens, rows_per_seq};
  const bool vec = rows_aligned16(logits, ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vocab <= 4 * kSampleSlab) return launch_sample<4, 0>(p, vec, (int)batch, s);
  if (vocab <= (kSampleRegSlabs + kSampleLdsSlabs) * kSampleSlab) return launch_sample<kSampleRegSlabs, kSampleLdsSlabs>(p, vec, (int)batch, s);
  return launch_sample<0, 0>(p, vec, (int)batch, s);
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_sample_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const float *temperature, const int32_t *top_k,
                    const float *top_p, const uint64_t *seeds, const int64_t *step, int64_t step_offset, int64_t *tokens, void *stream) {
  return sample_f16(logits, ld, batch, vocab, temperature, top_k, top_p, seeds, step, 0, step_offset, tokens, stream);
}

int atom_sample_rows_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const float *temperature, const int32_t *top_k,
                         const float *top_p, const uint64_t *seeds, const int64_t *step, int64_t rows_per_seq, int64_t step_offset,
                         int64_t *tokens, void *stream) {
  if (!step) return ATOM_ERR_INVALID_ARG;
  if (rows_per_seq < 1 || rows_per_seq > 0x7fffffff || (batch >= 1 && batch % rows_per_seq != 0)) return ATOM_ERR_SHAPE;
  return sample_f16(logits, ld, batch, vocab, temperature, top_k, top_p, seeds, step, (int)rows_per_seq, step_offset, tokens, stream);
}

}  // extern "C"
