// MXFP4 W4A4 on the block-scaled MFMA with its own scales (contract: include/atom_hip.h "MXFP4 W4A4"; design: DESIGN.md 4.26).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 takes, per lane, 32 codes of one row and ONE E8M0 scale byte: lane l supplies the scale of row
// l % 16, block l / 16 of the step's four 32-channel blocks.  For E2M1 the lane's 16 bytes are exactly that block; for E4M3 its 32
// bytes are channels 16 (l / 16) .. + 15 and 64 + 16 (l / 16) .. + 15 (two half blocks, scaled by the lanes that own their blocks).
// Operands are stored in that order (one 1 KiB fragment per 16 rows and K step, one scale byte per lane beside it) and
// nothing stands between a fragment read and the MFMA: no unpack, no scale multiply, no VALU.  The keeper (MXFP8) is the same
// instruction with format code 0: one more K step.  Weights are the first operand, activations the second, so that a lane ends up
// with 4 consecutive output features of one token (one 8-byte store).
//
//   mx_quant_kernel         the quantisers: one wave per row, 8 channels per lane and trip, block maximum across 4 lanes; the 8 values
//                           are the row's own (gathered by the reorder index or not) or silu(gate) * up of two rows, kept in FP32
//   gemm_mxfp4_tile_kernel  128 x 128 tiles, 4 waves of 64 x 64, operands and scale bytes through a 3-stage LDS ring by LDS-DMA
//   gemm_mxfp4_dec_kernel   M <= 16: one 16-feature tile per workgroup, weight fragments straight into registers, the K steps dealt
//                           to 8 waves and summed through LDS in wave order
// Every kernel is templated on the format of the activation's bulk codes: MxE2M1 (W4A4) or MxE2M3 (W4A6, DESIGN.md 4.29: the MXFP6
// activation in 6 registers per lane against the same E2M1 weight, at the same MFMA rate); the GEMM kernels also on the weight's
// (W6A4 / W6A6, DESIGN.md 4.30: a 1536-byte weight fragment through its own ring arithmetic, 1.5 x the weight stream at decode).
#include "mx_gemm.h"
#include "quant_math.h"

namespace atom {
namespace {

struct MxGemmParams {
  MxOperand a, w;
  half_t *out;
  const half_t *add;   // ADD kernels: the residual fp16 [M, N] summed into the store
  int M, N, S;   // S = FP4 K steps; step S is the keeper
};

// the store of 4 consecutive features of one token: half(acc), or half(acc + float(residual)) in FP32
template <bool ADD>
__device__ __forceinline__ void mx_store4(const MxGemmParams &p, int64_t off, v4f s) {
  if constexpr (ADD) {
    const v2u rv = *reinterpret_cast<const v2u *>(p.add + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += h2f(__builtin_bit_cast(half_t, (unsigned short)((rv[e >> 1] >> (16 * (e & 1))) & 0xffffu)));
  }
  const half_t h[4] = {(half_t)s[0], (half_t)s[1], (half_t)s[2], (half_t)s[3]};
  *reinterpret_cast<v2u *>(p.out + off) = __builtin_bit_cast(v2u, h);
}

// ------------------------------------------------------------------------------------------------------------------ quantiser
// Row `row` of the padded operand (rows >= M are written as zero blocks), every lane 8 channels of a block per trip: lanes 4 b .. 4 b + 3
// share block b of the trip's 16.  The lane's codes go to its 4 (E2M1) or 8 (E4M3) bytes of the MFMA lane that holds those channels.
// SILU: the values are silu_mul<false>(x, up) of quant_math.h (x = gate; no reorder: the producer's rows are stored in channel order).
template <bool SILU, class AF>
__global__ __launch_bounds__(256) void mx_quant_kernel(const half_t *__restrict__ x, const half_t *__restrict__ up, const int16_t *__restrict__ idx,
                                                       int M, int rows_pad, int K, uint8_t *__restrict__ q4, uint8_t *__restrict__ sc,
                                                       uint8_t *__restrict__ q8) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows_pad) return;
  const int S = K / 128 - 1, rt = row >> 4, r = row & 15;
  const half_t *xr = x + (int64_t)row * K;
  for (int c0 = lane * 8; c0 < K; c0 += 512) {
    float v[8];
    if (row < M) {
      if constexpr (SILU) {
        const v4u gv = *reinterpret_cast<const v4u *>(xr + c0), uv = *reinterpret_cast<const v4u *>(up + (int64_t)row * K + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = silu_mul<false>(h2f(__builtin_bit_cast(half_t, (unsigned short)((gv[i >> 1] >> (16 * (i & 1))) & 0xffffu))),
                                 h2f(__builtin_bit_cast(half_t, (unsigned short)((uv[i >> 1] >> (16 * (i & 1))) & 0xffffu))));
      } else if (idx) {
        const v4u iv = *reinterpret_cast<const v4u *>(idx + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const unsigned ch = (iv[i >> 1] >> (16 * (i & 1))) & 0xffffu;
          v[i] = h2f(xr[min(ch, (unsigned)(K - 1))]);
        }
      } else {
        const v4u xv = *reinterpret_cast<const v4u *>(xr + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = h2f(__builtin_bit_cast(half_t, (unsigned short)((xv[i >> 1] >> (16 * (i & 1))) & 0xffffu)));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
    mx_quant_store8<AF>(v, c0, rt, r, S, q4, sc, q8);
  }
}

// ------------------------------------------------------------------------------------------------------------- 128 x 128 tiles
// (ring and K loop: mx_tile_accumulate of mx_gemm.h)
template <bool ADD, class AF, class WF>
__global__ __launch_bounds__(256) void gemm_mxfp4_tile_kernel(MxGemmParams p) {
  __shared__ __attribute__((aligned(16))) char lds[MxRing<AF, WF>::LDS];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int wt0 = blockIdx.x * 8, at0 = blockIdx.y * 8;     // first fragment (16 features / 16 tokens) of the tile
  const int wn = w & 1, wm = w >> 1;
  v4f acc[4][4];
  mx_tile_accumulate<AF, WF>(p.a, p.w, p.S, wt0, at0, lds, acc);
  // lane l: token l % 16 of activation fragment i, features 4 (l / 16) .. + 3 of weight fragment j
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (at0 + wm * 4 + i) * 16 + (l & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = (wt0 + wn * 4 + j) * 16 + (l >> 4) * 4;
      if (m < p.M && n < p.N) mx_store4<ADD>(p, (int64_t)m * p.N + n, acc[i][j]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ decode
// M <= 16: the activation is one fragment per K step (it stays in L2), the weight is read once.  Workgroup = one weight fragment column
// (16 features), wave w = K steps w, w + 8, ... (the keeper counts as step S); the 8 partial tiles are summed in wave order.
constexpr int MXD_WAVES = 8;

template <bool ADD, class AF, class WF>
__global__ __launch_bounds__(64 * MXD_WAVES) void gemm_mxfp4_dec_kernel(MxGemmParams p) {
  __shared__ v4f part[MXD_WAVES][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t ct = blockIdx.x;
  v4f acc1[1];
  mx_dec_accumulate<AF, 1, MXD_WAVES, WF>(p.a, p.w, p.S, ct, w, l, acc1);
  const v4f acc = acc1[0];
  part[w][l] = acc;
  __syncthreads();
  if (w == 0) {
    v4f s = part[0][l];
#pragma unroll
    for (int i = 1; i < MXD_WAVES; ++i) s += part[i][l];
    const int m = l & 15;
    if (m < p.M) mx_store4<ADD>(p, (int64_t)m * p.N + ct * 16 + (l >> 4) * 4, s);
  }
}

template <bool SILU, class AF = MxE2M1>
int launch_mx_quant(const void *x, const void *up, const int16_t *idx, int64_t rows, int64_t K, void *q4, void *sc, void *q8, void *stream) {
  if (!x || (SILU && !up) || !q4 || !sc || !q8) return ATOM_ERR_INVALID_ARG;
  if (!mx_shape_ok(rows, K)) return ATOM_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(up) || !aligned16(idx) || !aligned16(q4) || !aligned16(sc) || !aligned16(q8)) return ATOM_ERR_ALIGN;
  const int64_t pad = (rows + 15) / 16 * 16;
  hipLaunchKernelGGL((mx_quant_kernel<SILU, AF>), dim3((unsigned)(pad / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const half_t *)x,
                     (const half_t *)up, idx, (int)rows, (int)pad, (int)K, (uint8_t *)q4, (uint8_t *)sc, (uint8_t *)q8);
  return check_launch();
}

}  // namespace
}  // namespace atom

using namespace atom;

namespace {
template <bool ADD, class AF = MxE2M1, class WF = MxE2M1>
int launch_mx_gemm(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8, const void *add,
                   void *out_f16, int64_t M, int64_t N, int64_t K, void *stream) {
  if (!a_q4 || !a_sc || !a_q8 || !w_q4 || !w_sc || !w_q8 || !out_f16 || (ADD && !add)) return ATOM_ERR_INVALID_ARG;
  const int route = atom_gemm_mxfp4_route(M, N, K);
  if (!route) return ATOM_ERR_SHAPE;
  if (!aligned16(a_q4) || !aligned16(a_sc) || !aligned16(a_q8) || !aligned16(w_q4) || !aligned16(w_sc) || !aligned16(w_q8) ||
      !aligned16(out_f16) || !aligned16(add))
    return ATOM_ERR_ALIGN;
  MxGemmParams p{{(const uint8_t *)a_q4, (const uint8_t *)a_sc, (const uint8_t *)a_q8, (int)((M + 15) / 16)},
                 {(const uint8_t *)w_q4, (const uint8_t *)w_sc, (const uint8_t *)w_q8, (int)(N / 16)},
                 (half_t *)out_f16, (const half_t *)add, (int)M, (int)N, (int)(K / 128 - 1)};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (route == 1) {
    hipLaunchKernelGGL((gemm_mxfp4_dec_kernel<ADD, AF, WF>), dim3((unsigned)(N / 16)), dim3(64 * MXD_WAVES), 0, s, p);
  } else {
    hipLaunchKernelGGL((gemm_mxfp4_tile_kernel<ADD, AF, WF>),dim3((unsigned)((N + 127) / 128), (unsigned)((M + 127) / 128)), dim3(256), 0, s, p);
  }
  return check_launch();
}

template <class AF, class WF>
int launch_mx_gemm_add(const void *a_q, const void *a_sc, const void *a_q8, const void *w_q, const void *w_sc, const void *w_q8, const void *add,
                       void *out_f16, int64_t M, int64_t N, int64_t K, void *stream) {
  return add ? launch_mx_gemm<true, AF, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, add, out_f16, M, N, K, stream)
             : launch_mx_gemm<false, AF, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, nullptr, out_f16, M, N, K, stream);
}
}  // namespace

extern "C" {

int atom_reorder_quant_mx_f16(const void *x_f16, const int16_t *reorder_index, int64_t M, int64_t K, void *q4, void *sc, void *q8,
                              void *stream) {
  if (K > 32768 && reorder_index) return ATOM_ERR_SHAPE;   // int16 indices
  return launch_mx_quant<false>(x_f16, nullptr, reorder_index, M, K, q4, sc, q8, stream);
}

int atom_silu_mul_quant_mx_f16(const void *gate_f16, const void *up_f16, int64_t rows, int64_t K, void *q4, void *sc, void *q8, void *stream) {
  return launch_mx_quant<true>(gate_f16, up_f16, nullptr, rows, K, q4, sc, q8, stream);
}

int atom_quant_weight_mx_f16(const void *w_f16, int64_t N, int64_t K, void *q4, void *sc, void *q8, void *stream) {
  if (w_f16 && q4 && sc && q8 && (N < 64 || (N % 64) != 0)) return ATOM_ERR_SHAPE;
  return launch_mx_quant<false>(w_f16, nullptr, nullptr, N, K, q4, sc, q8, stream);
}

// 0: not a shape of the GEMM; 1: the decode geometry; 2: 128 x 128 tiles
int atom_gemm_mxfp4_route(int64_t M, int64_t N, int64_t K) {
  if (!mx_shape_ok(M, K) || N < 64 || (N % 64) != 0 || N >= (1ll << 31)) return 0;
  if (M <= 16) return 1;
  return (M + 127) / 128 <= 65535 ? 2 : 0;
}

int atom_gemm_mxfp4_f16(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                        void *out_f16, int64_t M, int64_t N, int64_t K, void *stream) {
  return launch_mx_gemm<false>(a_q4, a_sc, a_q8, w_q4, w_sc, w_q8, nullptr, out_f16, M, N, K, stream);
}

// out = half(acc + float(residual)): the residual stream kept by the projection's own store (residual may be out: a lane reads its
// 4 halves before it writes them)
int atom_gemm_mxfp4_add_f16(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                            const void *residual_f16, void *out_f16, int64_t M, int64_t N, int64_t K, void *stream) {
  return launch_mx_gemm<true>(a_q4, a_sc, a_q8, w_q4, w_sc, w_q8, residual_f16, out_f16, M, N, K, stream);
}

// ---- W4A6: the same launches on an MXFP6 (E2M3) activation operand, q6 [R][S][96][16]
int atom_reorder_quant_mx6_f16(const void *x_f16, const int16_t *reorder_index, int64_t M, int64_t K, void *q6, void *sc, void *q8,
                               void *stream) {
  if (K > 32768 && reorder_index) return ATOM_ERR_SHAPE;   // int16 indices
  return launch_mx_quant<false, MxE2M3>(x_f16, nullptr, reorder_index, M, K, q6, sc, q8, stream);
}

int atom_gemm_mxfp4_a6_f16(const void *a_q6, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                           const void *add_f16, void *out_f16, int64_t M, int64_t N, int64_t K, void *stream) {
  return add_f16 ? launch_mx_gemm<true, MxE2M3>(a_q6, a_sc, a_q8, w_q4, w_sc, w_q8, add_f16, out_f16, M, N, K, stream)
                 : launch_mx_gemm<false, MxE2M3>(a_q6, a_sc, a_q8, w_q4, w_sc, w_q8, nullptr, out_f16, M, N, K, stream);
}

// ---- MXFP6 weights, W6A4 / W6A6: the weight operand's bulk codes as E2M3, wq [N/16][S][96][16]
// (any N >= 1: rows beyond N in the last 16-row tile are zero blocks, as in an activation operand; the GEMMs ask for N % 64 == 0)
int atom_quant_weight_mx6_f16(const void *w_f16, int64_t N, int64_t K, void *q6, void *sc, void *q8, void *stream) {
  return launch_mx_quant<false, MxE2M3>(w_f16, nullptr, nullptr, N, K, q6, sc, q8, stream);
}

// the one entry for every pair of bulk formats: act_bits / w_bits 4 (E2M1) or 6 (E2M3); add_f16 null or the residual
int atom_gemm_mx_f16(const void *a_q, const void *a_sc, const void *a_q8, const void *w_q, const void *w_sc, const void *w_q8, const void *add_f16,
                     void *out_f16, int64_t M, int64_t N, int64_t K, int act_bits, int w_bits, void *stream) {
  if ((act_bits != 4 && act_bits != 6) || (w_bits != 4 && w_bits != 6)) return ATOM_ERR_INVALID_ARG;
  if (w_bits == 6)
    return act_bits == 6 ? launch_mx_gemm_add<MxE2M3, MxE2M3>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, add_f16, out_f16, M, N, K, stream)
                         : launch_mx_gemm_add<MxE2M1, MxE2M3>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, add_f16, out_f16, M, N, K, stream);
  return act_bits == 6 ? launch_mx_gemm_add<MxE2M3, MxE2M1>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, add_f16, out_f16, M, N, K, stream)
                       : launch_mx_gemm_add<MxE2M1, MxE2M1>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, add_f16, out_f16, M, N, K, stream);
}

}  // extern "C"
