// Multi-adapter LoRA on fp16 activations beside the W4A4 base (the reference's punica.ops bgmv / add_lora, whose kernels it no longer
// builds: e2e/punica-atom/setup.py:40-48; arithmetic as e2e/punica-atom/tests/test_bgmv.py states it), generalised from rows to row
// SEGMENTS, plus the fp16 form of the per-head KV quantiser.
//
//   for every segment s (rows seg_indptr[s] .. seg_indptr[s+1]-1; seg_indptr == NULL: segment s is row s), a = seg_adapter[s]:
//     a < 0 or a >= capacity:  the rows are not touched
//     else:  y[i, n] = half( float(y[i, n]) + scale * SUM_h float(x[i, h]) * float(W[a, layer_idx, n, h]) )
//
// W fp16 [capacity, L, H2, H1]: the sum index is contiguous in x and in W ("NT"), so both operands of every kernel below come straight
// from global memory in 16-byte pieces and nothing is staged in LDS.  One of H1, H2 is the adapter rank (8 .. 64):
//   "shrink"  H1 > 64 (a multiple of 64), H2 <= 64: few outputs, long sums -- bound by reading x and A once
//   "expand"  H1 <= 64: short sums, many outputs    -- bound by the read-modify-write of y
// Two regimes, each with both forms:
//   seg_indptr given (prefill: a request is a segment): 16-row tiles of ONE segment on v_mfma_f32_16x16x32_f16.  The grid holds
//     rows / 16 + S row tiles (a bound of sum ceil(len / 16), sized on the host from rows and S alone); a workgroup finds its
//     segment in the device table with a wave-wide prefix sum and leaves before touching x, y or W when it has none.  The MFMA
//     takes W's rows as A (row = lane & 15, k = 8 (lane >> 4) + j) and x's rows as B (col = lane & 15, same k), so a lane's four
//     results are four consecutive features of one row: one 8-byte read and write of y.  A tile that crosses its segment's end
//     loads zeros for the missing rows and does not store them.  Shrink: the four waves take every fourth 64-wide K step and the
//     partial tiles are added through LDS in wave order (a fixed order inside ONE workgroup).  Expand: a wave per 64 features.
//   seg_indptr NULL (decode: one row per segment): no MFMA.  Shrink: a workgroup per row, a wave per output, lanes over h, the
//     butterfly sum.  Expand: a thread per output.  add_lora runs both in ONE launch there, t (rounded to fp16) in LDS.
// Exactly one thread writes an output element, the h sum is never split across workgroups, there are no atomics: a result does not
// depend on timing, and a row's result does not depend on the other rows of its batch.  Nothing is read back and nothing
// synchronises, so the ops can be captured.
#include <type_traits>

#include "common.h"
#include "kv_attn.h"

namespace atom {

typedef _Float16 lr_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 lr_h4 __attribute__((ext_vector_type(4)));

struct LoraParams {
  half_t *y;
  const half_t *x, *w;           // w: the layer's slice of adapter 0, W + layer_idx * H2 * H1
  const int32_t *seg_adapter, *seg_indptr;
  int rows, S, H1, H2, capacity;
  int64_t w_stride;              // halves between adapters: L * H2 * H1
  float scale;
  int overwrite;                 // y = half(scale * sum): add_lora's shrink pass into its (then never read before written) t
};

__device__ __forceinline__ lr_h8 ld8(const half_t *p) { return *reinterpret_cast<const lr_h8 *>(p); }

__device__ __forceinline__ int lora_adapter(const LoraParams &p, int seg) {
  const int a = p.seg_adapter[seg];
  return (a < 0 || a >= p.capacity) ? -1 : a;
}

// y <- half(y + scale * acc) for four consecutive features of one row
__device__ __forceinline__ void lora_store4(const LoraParams &p, half_t *yp, const v4f &acc) {
  lr_h4 o;
  lr_h4 y0 = {0, 0, 0, 0};
  if (!p.overwrite) y0 = *reinterpret_cast<const lr_h4 *>(yp);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = f2h((float)y0[i] + p.scale * acc[i]);
  *reinterpret_cast<lr_h4 *>(yp) = o;
}

// The 16-row tile `t` of the segment table: its segment, first row and the segment's end; false when the table has fewer tiles.
// Every wave runs this on its own (the loads are the same addresses in all four: one trip, no barrier).
__device__ __forceinline__ bool lora_find_tile(const LoraParams &p, int t, int lane, int &seg, int &row0, int &rend) {
  int base = 0;
  for (int s0 = 0; s0 < p.S; s0 += 64) {
    const int s = s0 + lane;
    int b = 0, e = 0;
    if (s < p.S) {
      b = max(p.seg_indptr[s], 0);
      e = min(p.seg_indptr[s + 1], p.rows);
    }
    const int nt = e > b ? (e - b + 15) >> 4 : 0;
    int inc = nt;                                              // inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d);
      if (lane >= d) inc += v;
    }
    const int first = base + inc - nt;
    const unsigned long long hit = __ballot(nt > 0 && t >= first && t < first + nt);
    if (hit) {
      const int src = __ffsll((long long)hit) - 1;
      seg = s0 + src;
      row0 = __shfl(b, src) + 16 * (t - __shfl(first, src));
      rend = __shfl(e, src);
      return true;
    }
    base += __shfl(inc, 63);
  }
  return false;
}

// ------------------------------------------------------------------------------------------------ segments, shrink (H1 % 64 == 0, H2 <= 64)
// NT = the 16-feature tiles of H2 (1 .. 4).  A K step of a wave is 64 wide: two x pieces and 2 NT weight pieces per lane, all requested
// before the first MFMA, and the loop over a wave's K steps is unrolled so that several steps' requests are in flight (the op is a
// stream of x: what it needs is bytes in flight, not arithmetic).
template <int NT>
__global__ __launch_bounds__(256) void lora_tile_shrink_kernel(LoraParams p) {
  __shared__ v4f red[4][NT][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  int seg, row0, rend;
  if (!lora_find_tile(p, blockIdx.x, lane, seg, row0, rend)) return;      // (workgroup-uniform)
  const int a = lora_adapter(p, seg);
  if (a < 0) return;
  const int H1 = p.H1, H2 = p.H2;
  const bool row_ok = row0 + r < rend;
  const half_t *xp = p.x + (int64_t)(row_ok ? row0 + r : row0) * H1 + 8 * kq;   // (a missing row reads the tile's first row and is masked)
  const half_t *wp[NT];
  bool n_ok[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    n_ok[ct] = ct * 16 + r < H2;
    wp[ct] = p.w + (int64_t)a * p.w_stride + (int64_t)(n_ok[ct] ? ct * 16 + r : 0) * H1 + 8 * kq;
  }
  const lr_h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  v4f acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) acc[ct] = v4f{0.f, 0.f, 0.f, 0.f};
  // UN K steps at a time: 2 UN x pieces and 2 UN NT weight pieces requested, then their MFMAs in ascending k
  auto steps = [&](auto un, int k0) {
    constexpr int UN = decltype(un)::value;
    lr_h8 xb[UN][2], wa[UN][2][NT];
#pragma unroll
    for (int i = 0; i < UN; ++i)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        xb[i][u] = ld8(xp + k0 + 256 * i + 32 * u);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) wa[i][u][ct] = ld8(wp[ct] + k0 + 256 * i + 32 * u);
      }
#pragma unroll
    for (int i = 0; i < UN; ++i)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!row_ok) xb[i][u] = zero8;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          if (!n_ok[ct]) wa[i][u][ct] = zero8;
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[i][u][ct], xb[i][u], acc[ct], 0, 0, 0);
        }
      }
  };
  constexpr int kUn = NT <= 2 ? 4 : 2;
  int k0 = wv * 64;
  for (; k0 + 256 * (kUn - 1) < H1; k0 += 256 * kUn) steps(std::integral_constant<int, kUn>{}, k0);
  for (; k0 < H1; k0 += 256) steps(std::integral_constant<int, 1>{}, k0);
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) red[wv][ct][lane] = acc[ct];
  __syncthreads();
  const int ct = wv;                                                        // wave w finishes feature tile w
  if (ct >= NT) return;
  v4f s = red[0][ct][lane];
#pragma unroll
  for (int w2 = 1; w2 < 4; ++w2) {
    const v4f q = red[w2][ct][lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += q[i];
  }
  const int n = ct * 16 + 4 * kq;                                           // lane: row r of the tile, features n .. n + 3
  if (row_ok && n < H2) lora_store4(p, p.y + (int64_t)(row0 + r) * H2 + n, s);
}

// ------------------------------------------------------------------------------------------------ segments, expand (H1 <= 64)
__global__ __launch_bounds__(256) void lora_tile_expand_kernel(LoraParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int H1 = p.H1, H2 = p.H2;
  const int nw = (blockIdx.y * 4 + wv) * 64;                                // this wave's 64 features
  if (nw >= H2) return;
  int seg, row0, rend;
  if (!lora_find_tile(p, blockIdx.x, lane, seg, row0, rend)) return;
  const int a = lora_adapter(p, seg);
  if (a < 0) return;
  const bool row_ok = row0 + r < rend;
  const half_t *xp = p.x + (int64_t)(row_ok ? row0 + r : row0) * H1;
  const half_t *wp = p.w + (int64_t)a * p.w_stride;
  const lr_h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int k_lo = 8 * kq, k_hi = 32 + 8 * kq;                              // the lane's pieces of K steps 0 and 1 (H1 % 8 == 0)
  const lr_h8 xb0 = (row_ok && k_lo < H1) ? ld8(xp + k_lo) : zero8;
  const lr_h8 xb1 = (row_ok && k_hi < H1) ? ld8(xp + k_hi) : zero8;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int n0 = nw + ct * 16;
    if (n0 >= H2) break;                                                    // (uniform)
    const int n = n0 + r;
    const bool n_ok = n < H2;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    const lr_h8 wa0 = (n_ok && k_lo < H1) ? ld8(wp + (int64_t)n * H1 + k_lo) : zero8;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa0, xb0, acc, 0, 0, 0);
    if (H1 > 32) {
      const lr_h8 wa1 = (n_ok && k_hi < H1) ? ld8(wp + (int64_t)n * H1 + k_hi) : zero8;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa1, xb1, acc, 0, 0, 0);
    }
    const int nn = n0 + 4 * kq;
    if (row_ok && nn < H2) lora_store4(p, p.y + (int64_t)(row0 + r) * H2 + nn, acc);
  }
}

// ------------------------------------------------------------------------------------------------ one-row segments
// The shrink sums of one row: wave wv takes the outputs n = wv + 4 j, j < H2 / 4 (H2 % 8 == 0: every wave has the same even count),
// its lanes every 64th 16-byte piece of the row, in passes of 4 (or 2) outputs whose loads carry no branch, so that the unrolled loop
// keeps two steps' requests in flight; emit(n, total) gets each total (butterfly order, the same value in every lane).
template <int U, class F>
__device__ __forceinline__ void row_shrink_pass(const half_t *xp, const half_t *wp, int H1, int lane, int n0, F emit) {
  float acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0.f;
#pragma unroll 2
  for (int h = 8 * lane; h < H1; h += 512) {
    const lr_h8 xv = ld8(xp + h);
    lr_h8 wv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) wv[u] = ld8(wp + (int64_t)(n0 + 4 * u) * H1 + h);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[u] = __builtin_fmaf((float)xv[i], (float)wv[u][i], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) emit(n0 + 4 * u, wave_sum_butterfly(acc[u]));
}

template <class F>
__device__ __forceinline__ void row_shrink_sums(const half_t *xp, const half_t *wp, int H1, int H2, int lane, int wv, F emit) {
  int n0 = wv;
  for (; n0 + 12 < H2; n0 += 16) row_shrink_pass<4>(xp, wp, H1, lane, n0, emit);
  if (n0 + 4 < H2) row_shrink_pass<2>(xp, wp, H1, lane, n0, emit);
}

// The expand sum of one output: h ascending, one FMA chain (xp: global memory or LDS).
__device__ __forceinline__ float row_expand_sum(const half_t *xp, const half_t *wp, int H1) {
  float acc = 0.f;
  for (int h = 0; h < H1; h += 8) {
    const lr_h8 xv = ld8(xp + h), wv = ld8(wp + h);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_fmaf((float)xv[i], (float)wv[i], acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void lora_row_shrink_kernel(LoraParams p) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int a = lora_adapter(p, row);
  if (a < 0) return;
  half_t *yrow = p.y + (int64_t)row * p.H2;
  row_shrink_sums(p.x + (int64_t)row * p.H1, p.w + (int64_t)a * p.w_stride, p.H1, p.H2, lane, wv, [&](int n, float s) {
    if (lane == 0) {
      const float y0 = p.overwrite ? 0.f : (float)yrow[n];
      yrow[n] = f2h(y0 + p.scale * s);
    }
  });
}

__global__ __launch_bounds__(256) void lora_row_expand_kernel(LoraParams p) {
  const int row = blockIdx.x;
  const int n = blockIdx.y * 256 + threadIdx.x;
  const int a = lora_adapter(p, row);
  if (a < 0 || n >= p.H2) return;
  const float acc = row_expand_sum(p.x + (int64_t)row * p.H1, p.w + (int64_t)a * p.w_stride + (int64_t)n * p.H1, p.H1);
  half_t *yp = p.y + (int64_t)row * p.H2 + n;
  const float y0 = p.overwrite ? 0.f : (float)*yp;
  *yp = f2h(y0 + p.scale * acc);
}

// add_lora for one-row segments in ONE launch: a workgroup per (row, kFusedCols features) computes the row's t with the shrink sums
// above, rounds it to fp16 into LDS, and expands its features from there -- the same operations in the same order as the two row
// kernels, so the same bits as the two passes.  Every feature block of a row repeats the shrink (x and A come from L2 after the first):
// at decode sizes the launch and the latency of one pass through A bound the op, not those bytes.
constexpr int kFusedCols = 1024;

struct LoraFusedParams {
  half_t *y;
  const half_t *x, *wa, *wb;     // the layer's slices of adapter 0
  const int32_t *seg_adapter;
  int H1, H2, rank, capacity;
  int64_t wa_stride, wb_stride;
  float scale;
};

__global__ __launch_bounds__(256) void lora_row_fused_kernel(LoraFusedParams p) {
  __shared__ __attribute__((aligned(16))) half_t t[64];
  const int row = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int a = p.seg_adapter[row];
  if (a < 0 || a >= p.capacity) return;
  row_shrink_sums(p.x + (int64_t)row * p.H1, p.wa + (int64_t)a * p.wa_stride, p.H1, p.rank, lane, wv, [&](int n, float s) {
    if (lane == 0) t[n] = f2h(0.f + 1.0f * s);
  });
  __syncthreads();
  const half_t *wb = p.wb + (int64_t)a * p.wb_stride;
  half_t *yrow = p.y + (int64_t)row * p.H2;
  constexpr int kPer = kFusedCols / 256;                                    // a thread's features: requests first, stores last
  float s[kPer], y0[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int n = blockIdx.y * kFusedCols + threadIdx.x + 256 * i;
    if (n < p.H2) {
      y0[i] = (float)yrow[n];
      s[i] = row_expand_sum(t, wb + (int64_t)n * p.rank, p.rank);
    }
  }
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int n = blockIdx.y * kFusedCols + threadIdx.x + 256 * i;
    if (n < p.H2) yrow[n] = f2h(y0[i] + p.scale * s[i]);
  }
}

// ------------------------------------------------------------------------------------------------ fp16 k / v -> cache form
// Half a wave per (token, head) vector of 128 values, 4 per lane: quant_head_u4 (kv_attn.h) on float(k), i.e. what
// kv_quant_append_kernel computes from FP32 sums, written to plain [T, heads, 64] + [T, heads, 2] tensors instead of a cache slot.
__global__ __launch_bounds__(256) void kv_quant_u4_f16_kernel(const half_t *k, uint8_t *packed, half_t *param, int64_t vecs) {
  const int l = threadIdx.x & 31;
  const int64_t vec = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (vec >= vecs) return;
  const lr_h4 h = *reinterpret_cast<const lr_h4 *>(k + vec * kHeadDim + 4 * l);
  const v4f x = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  unsigned sz;
  const unsigned short w = quant_head_u4(x, sz);
  *reinterpret_cast<unsigned short *>(packed + vec * 64 + 2 * l) = w;
  if (l == 0) *reinterpret_cast<unsigned *>(param + vec * 2) = sz;
}

// ------------------------------------------------------------------------------------------------ host side
static int lora_check_shape(int64_t rows, int64_t S, bool have_indptr, int64_t capacity, int64_t L, int64_t layer_idx) {
  if (rows < 1 || rows > 0x7fffffff || S < 1 || S > rows || (!have_indptr && S != rows)) return ATOM_ERR_SHAPE;
  if (capacity < 1 || capacity > 0x7fffffff || L < 1 || layer_idx < 0 || layer_idx >= L) return ATOM_ERR_SHAPE;
  return ATOM_OK;
}

// one of (H1, H2) is a rank (a multiple of 8 in 8 .. 64), the other a multiple of 64 (or a rank as well)
static bool lora_pass_shape(int64_t H1, int64_t H2) {
  if (H1 < 8 || H2 < 8 || H1 % 8 || H2 % 8 || H1 > (1 << 20) || H2 > (1 << 20)) return false;
  return H1 <= 64 ? (H2 <= 64 || H2 % 64 == 0) : (H2 <= 64 && H1 % 64 == 0);
}

// one pass (all arguments checked by the caller): the kernel by regime (segment table or rows) and form (shrink or expand)
static int lora_launch(half_t *y, const half_t *x, const half_t *w, const int32_t *seg_adapter, const int32_t *seg_indptr, int64_t rows,
                       int64_t S, int64_t H1, int64_t H2, int64_t capacity, int64_t L, int64_t layer_idx, float scale, int overwrite,
                       hipStream_t s) {
  LoraParams p{y, x, w + layer_idx * H2 * H1, seg_adapter, seg_indptr, (int)rows, (int)S, (int)H1, (int)H2, (int)capacity, L * H2 * H1,
               scale, overwrite};
  const bool shrink = H1 > 64;
  if (seg_indptr) {
    const unsigned tiles = (unsigned)(rows / 16 + S);
    if (shrink) {
      switch ((H2 + 15) / 16) {
        case 1: hipLaunchKernelGGL(lora_tile_shrink_kernel<1>, dim3(tiles), dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL(lora_tile_shrink_kernel<2>, dim3(tiles), dim3(256), 0, s, p); break;
        case 3: hipLaunchKernelGGL(lora_tile_shrink_kernel<3>, dim3(tiles), dim3(256), 0, s, p); break;
        default: hipLaunchKernelGGL(lora_tile_shrink_kernel<4>, dim3(tiles), dim3(256), 0, s, p); break;
      }
    }
    else hipLaunchKernelGGL(lora_tile_expand_kernel, dim3(tiles, (unsigned)((H2 + 255) / 256)), dim3(256), 0, s, p);
  } else {
    if (shrink) hipLaunchKernelGGL(lora_row_shrink_kernel, dim3((unsigned)rows), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(lora_row_expand_kernel, dim3((unsigned)rows, (unsigned)((H2 + 255) / 256)), dim3(256), 0, s, p);
  }
  return check_launch();
}

static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace atom

using namespace atom;

extern "C" {

int atom_bgmv_f16(void *y, const void *x, const void *w, const int32_t *seg_adapter, const int32_t *seg_indptr, int64_t rows, int64_t S,
                  int64_t H1, int64_t H2, int64_t capacity, int64_t L, int64_t layer_idx, float scale, void *stream) {
  if (!y || !x || !w || !seg_adapter) return ATOM_ERR_INVALID_ARG;
  const int st = lora_check_shape(rows, S, seg_indptr != nullptr, capacity, L, layer_idx);
  if (st != ATOM_OK) return st;
  if (!lora_pass_shape(H1, H2) || rows * (H1 > H2 ? H1 : H2) > 0x7fffffffll * 16) return ATOM_ERR_SHAPE;
  if (!aligned16(y) || !aligned16(x) || !aligned16(w) || !aligned4(seg_adapter) || !aligned4(seg_indptr)) return ATOM_ERR_ALIGN;
  return lora_launch((half_t *)y, (const half_t *)x, (const half_t *)w, seg_adapter, seg_indptr, rows, S, H1, H2, capacity, L, layer_idx,
                     scale, 0, reinterpret_cast<hipStream_t>(stream));
}

int atom_add_lora_f16(void *y, const void *x, const void *wa, const void *wb, const int32_t *seg_adapter, const int32_t *seg_indptr,
                      void *t, int64_t rows, int64_t S, int64_t H1, int64_t H2, int64_t rank, int64_t capacity, int64_t L,
                      int64_t layer_idx, float scale, void *stream) {
  if (!y || !x || !wa || !wb || !seg_adapter || !t) return ATOM_ERR_INVALID_ARG;
  const int st = lora_check_shape(rows, S, seg_indptr != nullptr, capacity, L, layer_idx);
  if (st != ATOM_OK) return st;
  if (H1 < 64 || H2 < 64 || H1 % 64 || H2 % 64 || H1 > (1 << 20) || H2 > (1 << 20) || rank < 8 || rank > 64 || rank % 8)
    return ATOM_ERR_SHAPE;
  if (rows * (H1 > H2 ? H1 : H2) > 0x7fffffffll * 16) return ATOM_ERR_SHAPE;
  if (!aligned16(y) || !aligned16(x) || !aligned16(wa) || !aligned16(wb) || !aligned16(t) || !aligned4(seg_adapter) ||
      !aligned4(seg_indptr))
    return ATOM_ERR_ALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!seg_indptr) {                                   // one-row segments: one launch, t in LDS (the caller's t is not touched)
    LoraFusedParams p{(half_t *)y, (const half_t *)x, (const half_t *)wa + layer_idx * rank * H1, (const half_t *)wb + layer_idx * H2 * rank,
                      seg_adapter, (int)H1, (int)H2, (int)rank, (int)capacity, L * rank * H1, L * H2 * rank, scale};
    hipLaunchKernelGGL(lora_row_fused_kernel, dim3((unsigned)rows, (unsigned)((H2 + kFusedCols - 1) / kFusedCols)), dim3(256), 0, s, p);
    return check_launch();
  }
  // shrink: t = half(x A^T) -- "a zeroed t, scale 1", written instead of added to (the rows of segments without an adapter keep
  // whatever t held, and the expand pass skips the same rows); expand: y += scale * t B^T
  const int st1 = lora_launch((half_t *)t, (const half_t *)x, (const half_t *)wa, seg_adapter, seg_indptr, rows, S, H1, rank, capacity, L,
                              layer_idx, 1.0f, 1, s);
  if (st1 != ATOM_OK) return st1;
  return lora_launch((half_t *)y, (const half_t *)t, (const half_t *)wb, seg_adapter, seg_indptr, rows, S, rank, H2, capacity, L,
                     layer_idx, scale, 0, s);
}

int atom_kv_quant_u4_f16(const void *k, void *packed, void *param, int64_t T, int kv_heads, int head_dim, void *stream) {
  if (!k || !packed || !param) return ATOM_ERR_INVALID_ARG;
  if (T < 1 || kv_heads < 1 || head_dim != kHeadDim || T * kv_heads > 0x7fffffffll) return ATOM_ERR_SHAPE;
  if (!aligned16(k) || !aligned16(packed) || !aligned4(param)) return ATOM_ERR_ALIGN;
  const int64_t vecs = T * kv_heads;
  hipLaunchKernelGGL(kv_quant_u4_f16_kernel, dim3((unsigned)((vecs + 7) / 8)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const half_t *)k, (uint8_t *)packed, (half_t *)param, vecs);
  return check_launch();
}

}  // extern "C"
