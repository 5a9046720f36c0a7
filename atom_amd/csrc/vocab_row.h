// What the vocabulary-row kernels share (sample, logprob, penalize, guide; the 64-bit shuffles and the host predicates also serve
// beam, spec and kv_step): a thread's 8 consecutive fp16 elements of a row, loaded as canonical keys or as raw words, and the checks
// an entry point makes on its pointers.
#pragma once
#include "common.h"
#include "sample_math.h"

namespace atom {

// canonical keys of the 8 elements from e0 on (0 where there is none): one 16-byte load where the row allows it and all 8 exist
template <bool VEC>
__device__ __forceinline__ void load_slab(const uint16_t *row, int vocab, int e0, uint32_t *d) {
  d[0] = d[1] = d[2] = d[3] = 0;
  if (e0 >= vocab) return;
  if (VEC && e0 + 8 <= vocab) {
    const v4u x = *reinterpret_cast<const v4u *>(row + e0);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = sample::canon_key(x[i] & 0xFFFFu) | (sample::canon_key(x[i] >> 16) << 16);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (e0 + c < vocab) d[c >> 1] |= sample::canon_key(row[e0 + c]) << ((c & 1) * 16);
  }
}

__device__ __forceinline__ uint32_t key_at(const uint32_t *d, int c) { return (d[c >> 1] >> ((c & 1) * 16)) & 0xFFFFu; }

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t x, int d) {
  const uint32_t lo = __shfl_up((uint32_t)x, d, 64), hi = __shfl_up((uint32_t)(x >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)x, d, 64), hi = __shfl_xor((uint32_t)(x >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

// n (1 .. 8) 16-bit words from src, one per dword of d: one 16-byte load where the row allows it and all 8 exist
template <bool VEC>
__device__ __forceinline__ void load8(const uint16_t *src, int n, uint32_t *d) {
  if (VEC && n == 8) {
    const v4u x = *reinterpret_cast<const v4u *>(src);
#pragma unroll
    for (int i = 0; i < 4; ++i) { d[2 * i] = x[i] & 0xFFFFu; d[2 * i + 1] = x[i] >> 16; }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < n) d[c] = src[c];
  }
}

template <bool VEC>
__device__ __forceinline__ void store8(uint16_t *dst, int n, const uint32_t *d) {
  if (VEC && n == 8) {
    v4u x;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = (d[2 * i] & 0xFFFFu) | (d[2 * i + 1] << 16);
    *reinterpret_cast<v4u *>(dst) = x;
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < n) dst[c] = (uint16_t)d[c];
  }
}

// host: q is not a multiple of mask + 1 (a null pointer, an optional buffer left out, is)
inline bool off_by(const void *q, unsigned mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

// host: every row of the fp16 / int16 buffer q starts on 16 bytes, so the VEC forms above apply to it (a buffer left out does not object)
inline bool rows_aligned16(const void *q, int64_t ld) { return !q || (aligned16(q) && (ld % 8) == 0); }

}  // namespace atom
