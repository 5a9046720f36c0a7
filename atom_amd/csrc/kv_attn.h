// Shared by the INT4 paged-KV attention ops (kv_i4.hip: append and decode, prefill_i4.hip: prefill and grouped-query attention): the
// head size; the cache's arguments, their check and their kernel-argument form; and the KV-split partial states float
// [rows][heads][splits][130] (128 un-normalised values, running maximum in base 2, denominator) -- their size, the rule for a
// workspace that cannot hold them, the merge kernel and its ONLY launch (launch_merge).  Each file keeps its own plan (DecodePlan,
// PrefillPlan: splits and launch geometry), computed by one function that its queries and its launcher both call.
#pragma once
#include "common.h"

namespace atom {

constexpr int kHeadDim = 128;
constexpr float kLog2e = 1.4426950408889634f;

// the u4 epilogue on one 128-value head vector held by 32 lanes (4 values each; both halves of a wave at once): returns the lane's four
// codes as 16 bits and the vector's (scale, zero) as a half2 bit pattern -- what the cache stores
__device__ __forceinline__ unsigned short quant_head_u4(const v4f &x, unsigned &sz) {
  float lo = fminf(fminf(x[0], x[1]), fminf(x[2], x[3])), hi = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
#pragma unroll
  for (int k = 16; k >= 1; k >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, k));
    hi = fmaxf(hi, __shfl_xor(hi, k));
  }
  const float scale = (hi - lo) / 15.f, zero = -lo, rs = 1.0f / scale;
  unsigned w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t = (x[k] + zero) * rs;
    float tr = truncf(t);
    if (fabsf(t - tr) >= 0.5f) tr += copysignf(1.0f, t);
    tr = fminf(fmaxf(tr, 0.f), 15.f);
    if (scale == 0.f) tr = 0.f;
    w |= (unsigned)(int)tr << (4 * k);
  }
  sz = (unsigned)__builtin_bit_cast(unsigned short, f2h(scale)) | ((unsigned)__builtin_bit_cast(unsigned short, f2h(zero)) << 16);
  return (unsigned short)w;
}

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

// ---- host side
struct KvParams {     // the cache as the append and decode kernels take it
  uint8_t *data;
  half_t *param;
  const int32_t *indptr, *indices, *last_page_offset;
  int batch, L, layer, N, P;
};

static KvParams kv_params(const void *kv_data, const void *kv_param, const int32_t *indptr, const int32_t *indices, const int32_t *lpo,
                          int batch, int L, int layer, int N, int P) {
  KvParams kv;
  kv.data = (uint8_t *)kv_data, kv.param = (half_t *)kv_param;
  kv.indptr = indptr, kv.indices = indices, kv.last_page_offset = lpo;
  kv.batch = batch, kv.L = L, kv.layer = layer, kv.N = N, kv.P = P;
  return kv;
}

static int check_kv(const void *kv_data, const void *kv_param, const int32_t *indptr, const int32_t *indices,
                    const int32_t *lpo, int batch, int L, int layer, int N, int P, int D) {
  if (!kv_data || !kv_param || !indptr || !indices || !lpo) return ATOM_ERR_INVALID_ARG;
  if (D != kHeadDim || batch < 1 || L < 1 || layer < 0 || layer >= L || N < 1 || P < 16 || (P % 16) != 0) return ATOM_ERR_SHAPE;
  if (!aligned16(kv_data) || (reinterpret_cast<uintptr_t>(kv_param) & 3u)) return ATOM_ERR_ALIGN;
  return ATOM_OK;
}

// the two arguments of the _rope entry points: a per-pair frequency table (NULL: the theta path) and a factor on the logits
static int check_rope_table(const float *rope_table, float attn_scale) {
  if (!(attn_scale > 0.f)) return ATOM_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(rope_table) & 3u) return ATOM_ERR_ALIGN;
  return ATOM_OK;
}

// kv_i4.hip: the MHA decode op with the _rope arguments (no C entry point of its own: atom_batch_decode_gqa_i4_rope forwards to it)
int batch_decode_rope(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                      const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_heads, int page_size, int head_dim,
                      float rope_theta, float rope_scale, const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                      size_t workspace_bytes, void *stream);

static size_t partial_state_bytes(int64_t rows_times_heads, int splits) {
  return (size_t)rows_times_heads * splits * (kHeadDim + 2) * sizeof(float);
}

// splits > 1 leave their partial states in the caller's workspace; where it is missing, too small or misaligned the op runs unsplit
static bool workspace_holds(const void *ws, size_t ws_bytes, int64_t rows_times_heads, int splits) {
  return ws && ws_bytes >= partial_state_bytes(rows_times_heads, splits) && aligned16(ws);
}

static void launch_merge(const void *ws, void *o, int64_t rows_times_heads, int splits, hipStream_t s) {
  const dim3 grid((unsigned)rows_times_heads), block(128);
  if (splits <= 8)
    hipLaunchKernelGGL(decode_merge_kernel<8>, grid, block, 0, s, (const float *)ws, (half_t *)o, splits);
  else if (splits <= 16)
    hipLaunchKernelGGL(decode_merge_kernel<16>, grid, block, 0, s, (const float *)ws, (half_t *)o, splits);
  else
    hipLaunchKernelGGL(decode_merge_kernel<32>, grid, block, 0, s, (const float *)ws, (half_t *)o, splits);
}

}  // namespace atom
