// Shared by the INT4 paged-KV attention ops (kv_i4.hip: decode, prefill_i4.hip: prefill): the head size, the argument check of
// the cache tables, and the merge of KV-split partial states float [rows][heads][splits][130] (128 un-normalised values, running
// maximum in base 2, denominator).
#pragma once
#include "common.h"

namespace atom {

constexpr int kHeadDim = 128;
constexpr float kLog2e = 1.4426950408889634f;

// out[b,h,:] = sum_s o_s * 2^(m_s - M) / sum_s d_s * 2^(m_s - M)
// Round 6: every split's (value, m, d) is requested before the first one is used -- in batches of 8 splits with compile-time bounds.
// The partial states were written by waves on other XCDs, so each request is a trip to memory (~1.5 us): the two run-time loops of
// rounds 1-5 (one for the maximum, one for the sums, their loads inside) paid it 2 x splits times in sequence on a 130-thread kernel
// (4.7 us per decode step for 133 KB).  Same operations in the same order: same bits.
// SB = splits handled in one batch of loads: 8 or 16 by the launcher.  (Round 6 lowered the KV-split size to 4 tiles: a batch-1 step at
// context 1024 has 16 splits, and with SB = 8 that took the run-time loops below -- four dependent trips to memory instead of one.)
template <int SB>
__global__ __launch_bounds__(128) void decode_merge_kernel(const float *ws, half_t *o, int splits) {
  const int64_t bh = blockIdx.x;
  const int dim = threadIdx.x;
  const float *wp = ws + bh * splits * (kHeadDim + 2);
  float M = -INFINITY;
  if (splits <= SB) {
    float ov[SB], mv[SB], dv[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const int sc = min(s, splits - 1);
      ov[s] = wp[sc * (kHeadDim + 2) + dim];
      mv[s] = wp[sc * (kHeadDim + 2) + kHeadDim];
      dv[s] = wp[sc * (kHeadDim + 2) + kHeadDim + 1];
    }
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s < splits) M = fmaxf(M, mv[s]);
    float acc = 0.f, den = 0.f;
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s < splits) {
        const float w = mv[s] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mv[s] - M);
        acc = __builtin_fmaf(ov[s], w, acc);
        den = __builtin_fmaf(dv[s], w, den);
      }
    o[bh * kHeadDim + dim] = (half_t)(den > 0.f ? acc / den : 0.f);
    return;
  }
  for (int s0 = 0; s0 < splits; s0 += SB) {
    float mv[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) mv[s] = wp[min(s0 + s, splits - 1) * (kHeadDim + 2) + kHeadDim];
#pragma unroll
    for (int s = 0; s < SB; ++s) M = fmaxf(M, mv[s]);        // (a clamped repeat of the last split changes no maximum)
  }
  float acc = 0.f, den = 0.f;
  for (int s0 = 0; s0 < splits; s0 += SB) {
    float ov[SB], mv[SB], dv[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const int sc = min(s0 + s, splits - 1);
      ov[s] = wp[sc * (kHeadDim + 2) + dim];
      mv[s] = wp[sc * (kHeadDim + 2) + kHeadDim];
      dv[s] = wp[sc * (kHeadDim + 2) + kHeadDim + 1];
    }
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s0 + s < splits) {
        const float w = mv[s] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mv[s] - M);
        acc = __builtin_fmaf(ov[s], w, acc);
        den = __builtin_fmaf(dv[s], w, den);
      }
  }
  o[bh * kHeadDim + dim] = (half_t)(den > 0.f ? acc / den : 0.f);
}

static int check_kv(const void *kv_data, const void *kv_param, const int32_t *indptr, const int32_t *indices,
                    const int32_t *lpo, int batch, int L, int layer, int N, int P, int D) {
  if (!kv_data || !kv_param || !indptr || !indices || !lpo) return ATOM_ERR_INVALID_ARG;
  if (D != kHeadDim || batch < 1 || L < 1 || layer < 0 || layer >= L || N < 1 || P < 16 || (P % 16) != 0) return ATOM_ERR_SHAPE;
  if (!aligned16(kv_data) || (reinterpret_cast<uintptr_t>(kv_param) & 3u)) return ATOM_ERR_ALIGN;
  return ATOM_OK;
}

}  // namespace atom
