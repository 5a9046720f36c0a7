// The dense Llama layer on MX operands (contract: include/atom_hip.h "Dense Llama on MXFP4"; design: DESIGN.md 4.28): the kernels between
// the MXFP4 GEMMs of gemm_mxfp4.hip that keep fp16 intermediates out of memory.
//
//   gu_mxfp4_tile_kernel / gu_mxfp4_dec_kernel   gate_proj + up_proj + SiLU x up + MX quantiser in one launch.  The weight operand is the
//     two projections interleaved in pairs of 16-row fragments, [g0 g1 u0 u1 g2 g3 u2 u3 ...]: fused fragments 4 q .. 4 q + 3 are gate
//     and up of output channels 32 q .. 32 q + 31, ONE MX block of the output.  In the accumulator layout of the scaled MFMA a lane holds
//     4 consecutive features of one token per weight fragment, so a wave that owns four consecutive fused fragments has g and u of whole
//     output blocks in its own registers: 8 values of one (token, block) per lane, the other 24 in the lanes l ^ 16, l ^ 32, l ^ 48.
//     Block maximum = 7 maxima in registers + 2 exchanges; no LDS, no barrier.  The codes are then gathered to ONE lane per (token, block)
//     (4 ds_bpermute per operand register), which writes the block's 16 bytes (E2M1) or 2 x 16 bytes (E4M3, the keeper's lane layout)
//     with full-width stores, and the scale byte.
//       tile  (M > 16)   the 128 x 128 geometry of gemm_mxfp4.hip on the fused operand (mx_tile_accumulate: same ring, same chain): a
//                        workgroup = 128 fused features = 2 output blocks x 128 tokens; wave (wn, wm) owns block 2 bx + wn of 64 tokens:
//                        its acc[i][0 .. 3] ARE g0 g1 u0 u1.  The lanes of group i store activation fragment i's rows.
//       decode (M <= 16) a workgroup owns four consecutive fused fragments (one output block); 8 waves take K steps w, w + 8, ... with
//                        the weights streamed straight into registers (mx_dec_accumulate<4>), the 8 x 4 partial tiles are summed through
//                        LDS in wave order by wave 0, which runs the epilogue on the sums.
//     Either launch reads an E2M1 or an E2M3 activation (AF) and writes E2M1 or E2M3 bulk blocks (OF): an E2M3 block is
//     the lane's two 24-bit code quartets gathered the same way and written as the 16-byte head and 8-byte tail of its MFMA lane.
//     WF is the format of the fused weight's bulk codes (E2M3: DESIGN.md 4.30; the decode launch then holds four 6-register weight
//     fragments per K step); the epilogue does not depend on it.
//   rmsnorm_quant_mx_kernel<ADD, AF>   RMSNorm (optionally x + residual first, written back) + channel reorder + MX quantiser: one workgroup
//     of 256 per row; the row goes to LDS once while its squares are summed in quant_math.h's fixed shape, the gather reads LDS.
#include "mx_gemm.h"
#include "quant_math.h"

namespace atom {
namespace {

struct MxGuParams {
  MxOperand a, w;            // w: the fused gate / up operand, 2 F rows
  uint8_t *q4, *sc, *q8;     // the output operand [M, F]
  int M, S, Sp;              // S = FP4 K steps of the GEMM, Sp = F / 128 - 1 those of the output
};

// Output block q (channels 32 q .. + 31) of the 16 tokens of output row tile rt.  g0 g1 u0 u1: the sums of fused fragments 4 q .. 4 q + 3;
// lane l holds token l % 16, block channels 4 (l / 16) .. + 3 (g0, u0) and 16 + 4 (l / 16) .. + 3 (g1, u1).  row_live: the lane's token
// exists (a padding row is a zero block); store: rt is a tile of the output (wave-uniform); owner: the lane group that writes.
// Every lane of the wave must be here (exchanges).  OF: the format of the output's bulk blocks.
template <class OF>
__device__ __forceinline__ void gu_block_store(const v4f &g0, const v4f &g1, const v4f &u0, const v4f &u1, bool row_live, bool store, int owner,
                                               int rt, int q, int l, const MxGuParams &p) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = row_live ? silu_mul<false>(g0[e], u0[e]) : 0.f;
    v[4 + e] = row_live ? silu_mul<false>(g1[e], u1[e]) : 0.f;
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 16));
  amax = fmaxf(amax, __shfl_xor(amax, 32));
  const int r = l & 15, Sp = p.Sp, step = q >> 2;
  const bool mine = store && (l >> 4) == owner;
  const int64_t scrow = (int64_t)rt * (Sp + 1);
  if (step < Sp) {                                           // (uniform over the workgroup: F - 128 is a multiple of 128)
    if constexpr (std::is_same_v<OF, MxE2M3>) {
      const int sb = mx_scale_byte<MxE2M3>(amax);
      const float inv = mx_inv_scale(sb);
      unsigned pa = 0, pb = 0;                               // 24 bits each: block channels 4 g .. 4 g + 3 and 16 + 4 g .. + 3
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pa |= mx_code<MxE2M3>(v[e], inv) << (6 * e);
        pb |= mx_code<MxE2M3>(v[4 + e], inv) << (6 * e);
      }
      const unsigned a0 = __shfl(pa, r), a1 = __shfl(pa, r + 16), a2 = __shfl(pa, r + 32), a3 = __shfl(pa, r + 48);
      const unsigned b0 = __shfl(pb, r), b1 = __shfl(pb, r + 16), b2 = __shfl(pb, r + 32), b3 = __shfl(pb, r + 48);
      if (mine) {
        // the block's 192 bits = the four groups' low quartets (channels 0 .. 15), then their high quartets: head 16 bytes, tail 8
        const int ml = r + 16 * (q & 3);
        uint8_t *o = p.q4 + ((int64_t)rt * Sp + step) * 1536;
        *reinterpret_cast<v4u *>(o + ml * 16) = v4u{a0 | (a1 << 24), (a1 >> 8) | (a2 << 16), (a2 >> 16) | (a3 << 8), b0 | (b1 << 24)};
        *reinterpret_cast<v2u *>(o + 1024 + ml * 8) = v2u{(b1 >> 8) | (b2 << 16), (b2 >> 16) | (b3 << 8)};
        p.sc[(scrow + step) * 64 + ml] = (uint8_t)sb;
      }
    } else {
      const int sb = mx_scale_byte<MxE2M1>(amax);
      const float inv = mx_inv_scale(sb);
      unsigned pk = 0;                                       // low half: codes of g0 / u0, high half: of g1 / u1
#pragma unroll
      for (int i = 0; i < 8; ++i) pk |= mx_code<MxE2M1>(v[i], inv) << (4 * i);
      const unsigned p0 = __shfl(pk, r), p1 = __shfl(pk, r + 16), p2 = __shfl(pk, r + 32), p3 = __shfl(pk, r + 48);
      if (mine) {
        // byte c / 2 of the block's 16 holds channels c, c + 1: lane group g's halves are bytes 2 g, 2 g + 1 and 8 + 2 g, 9 + 2 g
        const v4u d = {(p0 & 0xffffu) | (p1 << 16), (p2 & 0xffffu) | (p3 << 16), (p0 >> 16) | (p1 & 0xffff0000u), (p2 >> 16) | (p3 & 0xffff0000u)};
        const int ml = r + 16 * (q & 3);
        *reinterpret_cast<v4u *>(p.q4 + (((int64_t)rt * Sp + step) * 64 + ml) * 16) = d;
        p.sc[(scrow + step) * 64 + ml] = (uint8_t)sb;
      }
    }
  } else {
    const int sb = mx_scale_byte<MxE4M3>(amax);
    const float inv = mx_inv_scale(sb);
    unsigned pa = 0, pb = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pa |= mx_code<MxE4M3>(v[e], inv) << (8 * e);
      pb |= mx_code<MxE4M3>(v[4 + e], inv) << (8 * e);
    }
    const v4u da = {__shfl(pa, r), __shfl(pa, r + 16), __shfl(pa, r + 32), __shfl(pa, r + 48)};
    const v4u db = {__shfl(pb, r), __shfl(pb, r + 16), __shfl(pb, r + 32), __shfl(pb, r + 48)};
    if (mine) {
      // keeper channel kc = 32 (q & 3) + c: half kc / 64, lane group (kc / 16) % 4 = 2 (q & 1) + c / 16, byte kc % 16 (mx_quant_store8's lines)
      uint8_t *o = p.q8 + (((int64_t)rt * 2 + ((q & 3) >> 1)) * 64 + r + 32 * (q & 1)) * 16;
      *reinterpret_cast<v4u *>(o) = da;
      *reinterpret_cast<v4u *>(o + 256) = db;
      p.sc[(scrow + Sp) * 64 + r + 16 * (q & 3)] = (uint8_t)sb;
    }
  }
}

template <class AF, class OF, class WF>
__global__ __launch_bounds__(256) void gu_mxfp4_tile_kernel(MxGuParams p) {
  __shared__ __attribute__((aligned(16))) char lds[MxRing<AF, WF>::LDS];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int wt0 = blockIdx.x * 8, at0 = blockIdx.y * 8;
  v4f acc[4][4];
  mx_tile_accumulate<AF, WF>(p.a, p.w, p.S, wt0, at0, lds, acc);
  const int q = blockIdx.x * 2 + (w & 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rt = at0 + (w >> 1) * 4 + i;
    gu_block_store<OF>(acc[i][0], acc[i][1], acc[i][2], acc[i][3], rt * 16 + (l & 15) < p.M, rt < p.a.tiles, i, rt, q, l, p);
  }
}

constexpr int GUD_WAVES = 8;

template <class AF, class OF, class WF>
__global__ __launch_bounds__(64 * GUD_WAVES) void gu_mxfp4_dec_kernel(MxGuParams p) {
  __shared__ v4f part[GUD_WAVES][4][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int q = blockIdx.x;
  v4f acc[4];
  mx_dec_accumulate<AF, 4, GUD_WAVES, WF>(p.a, p.w, p.S, (int64_t)q * 4, w, l, acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) part[w][j][l] = acc[j];
  __syncthreads();
  if (w == 0) {
    v4f s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = part[0][j][l];
#pragma unroll
      for (int i = 1; i < GUD_WAVES; ++i) s[j] += part[i][j][l];
    }
    gu_block_store<OF>(s[0], s[1], s[2], s[3], (l & 15) < p.M, true, 0, 0, q, l, p);
  }
}

// ------------------------------------------------------------------------------------------------------- RMSNorm quantisers
// Workgroup = one row of the padded operand (rows >= M: zero blocks).  Pass 1: 16-byte chunk c of the row in memory order belongs to
// thread c % 256 (quant_math.h's fixed shape); ADD: s = half(x + residual) first, written back to the residual stream.  The row (s)
// is parked in LDS.  Pass 2: thread t quantises reordered channels 8 t .. 8 t + 7 (+ 2048 per trip) of (s[idx[c]] w[idx[c]]) rinv,
// FP32 throughout, by mx_quant_kernel's lines (mx_quant_store8).
constexpr int RQ_MAX_K = 16384;                              // the row in LDS: 32 KiB

template <bool ADD, class AF>
__global__ __launch_bounds__(256) void rmsnorm_quant_mx_kernel(const half_t *__restrict__ x, half_t *__restrict__ res, const half_t *__restrict__ wgt,
                                                               const int16_t *__restrict__ idx, int M, int K, float eps, uint8_t *__restrict__ q4,
                                                               uint8_t *__restrict__ sc, uint8_t *__restrict__ q8) {
  __shared__ __attribute__((aligned(16))) half_t rowh[RQ_MAX_K];
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const bool live = row < M;                                 // (uniform over the workgroup)
  float rinv = 0.f;
  if (live) {
    const int64_t base = (int64_t)row * K;
    float ss = 0.f;
    for (int c = tid; c < K / 8; c += 256) {
      h8 a = *reinterpret_cast<const h8 *>(x + base + c * 8);
      if constexpr (ADD) {
        a = a + *reinterpret_cast<const h8 *>(res + base + c * 8);
        *reinterpret_cast<h8 *>(res + base + c * 8) = a;
      }
      *reinterpret_cast<h8 *>(rowh + c * 8) = a;
      ss = sumsq8(a, ss);
    }
    ss = wave_sum_butterfly(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    rinv = rms_rinv(red, K, eps);
  }
  const int S = K / 128 - 1;
  for (int c0 = tid * 8; c0 < K; c0 += 2048) {
    float v[8];
    if (live) {
      unsigned ch[8];
      if (idx) {
        const v4u iv = *reinterpret_cast<const v4u *>(idx + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) ch[i] = min((iv[i >> 1] >> (16 * (i & 1))) & 0xffffu, (unsigned)(K - 1));
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) ch[i] = c0 + i;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (h2f(rowh[ch[i]]) * h2f(wgt[ch[i]])) * rinv;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
    mx_quant_store8<AF>(v, c0, row >> 4, row & 15, S, q4, sc, q8);
  }
}

template <bool ADD, class AF = MxE2M1>
int launch_rmsnorm_quant_mx(const void *x, void *res, const void *wgt, const int16_t *idx, int64_t M, int64_t K, float eps, void *q4, void *sc,
                            void *q8, void *stream) {
  if (!x || (ADD && !res) || !wgt || !q4 || !sc || !q8) return ATOM_ERR_INVALID_ARG;
  if (!mx_shape_ok(M, K) || K > RQ_MAX_K || !(eps >= 0.f)) return ATOM_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(res) || !aligned16(wgt) || !aligned16(idx) || !aligned16(q4) || !aligned16(sc) || !aligned16(q8))
    return ATOM_ERR_ALIGN;
  const int64_t pad = (M + 15) / 16 * 16;
  hipLaunchKernelGGL((rmsnorm_quant_mx_kernel<ADD, AF>), dim3((unsigned)pad), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const half_t *)x,
                     (half_t *)res, (const half_t *)wgt, idx, (int)M, (int)K, eps, (uint8_t *)q4, (uint8_t *)sc, (uint8_t *)q8);
  return check_launch();
}

}  // namespace
}  // namespace atom

using namespace atom;

namespace {
template <class AF, class OF, class WF = MxE2M1>
int launch_gu(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8, void *out_q4, void *out_sc,
              void *out_q8, int64_t M, int64_t F, int64_t K, void *stream) {
  if (!a_q4 || !a_sc || !a_q8 || !w_q4 || !w_sc || !w_q8 || !out_q4 || !out_sc || !out_q8) return ATOM_ERR_INVALID_ARG;
  const int route = atom_gemm_mxfp4_silu_mul_quant_route(M, F, K);
  if (!route) return ATOM_ERR_SHAPE;
  if (!aligned16(a_q4) || !aligned16(a_sc) || !aligned16(a_q8) || !aligned16(w_q4) || !aligned16(w_sc) || !aligned16(w_q8) ||
      !aligned16(out_q4) || !aligned16(out_sc) || !aligned16(out_q8))
    return ATOM_ERR_ALIGN;
  MxGuParams p{{(const uint8_t *)a_q4, (const uint8_t *)a_sc, (const uint8_t *)a_q8, (int)((M + 15) / 16)},
               {(const uint8_t *)w_q4, (const uint8_t *)w_sc, (const uint8_t *)w_q8, (int)(F / 8)},
               (uint8_t *)out_q4, (uint8_t *)out_sc, (uint8_t *)out_q8, (int)M, (int)(K / 128 - 1), (int)(F / 128 - 1)};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (route == 1) {
    hipLaunchKernelGGL((gu_mxfp4_dec_kernel<AF, OF, WF>), dim3((unsigned)(F / 32)), dim3(64 * GUD_WAVES), 0, s, p);
  } else {
    hipLaunchKernelGGL((gu_mxfp4_tile_kernel<AF, OF, WF>), dim3((unsigned)(F / 64), (unsigned)((M + 127) / 128)), dim3(256), 0, s, p);
  }
  return check_launch();
}

template <class WF>
int launch_gu_bits(const void *a_q, const void *a_sc, const void *a_q8, const void *w_q, const void *w_sc, const void *w_q8, void *out_q, void *out_sc,
                   void *out_q8, int64_t M, int64_t F, int64_t K, int act_bits, int out_bits, void *stream) {
  if (act_bits == 6)
    return out_bits == 6 ? launch_gu<MxE2M3, MxE2M3, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream)
                         : launch_gu<MxE2M3, MxE2M1, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream);
  return out_bits == 6 ? launch_gu<MxE2M1, MxE2M3, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream)
                       : launch_gu<MxE2M1, MxE2M1, WF>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream);
}
}  // namespace

extern "C" {

// 0: not a shape of the fused launch; 1: the decode geometry (M <= 16); 2: 128 x 128 tiles of the fused operand
int atom_gemm_mxfp4_silu_mul_quant_route(int64_t M, int64_t F, int64_t K) {
  if (!mx_shape_ok(M, K) || F < 256 || (F % 128) != 0 || F > (1 << 20)) return 0;
  if (M <= 16) return 1;
  return (M + 127) / 128 <= 65535 ? 2 : 0;
}

int atom_gemm_mxfp4_silu_mul_quant(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                                   void *out_q4, void *out_sc, void *out_q8, int64_t M, int64_t F, int64_t K, void *stream) {
  return launch_gu<MxE2M1, MxE2M1>(a_q4, a_sc, a_q8, w_q4, w_sc, w_q8, out_q4, out_sc, out_q8, M, F, K, stream);
}

// act_bits / out_bits: 4 (E2M1 bulk codes, [R][S][64][16]) or 6 (E2M3, [R][S][96][16]) for the activation read and the operand written
int atom_gemm_mxfp4_a6_silu_mul_quant(const void *a_q, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                                      void *out_q, void *out_sc, void *out_q8, int64_t M, int64_t F, int64_t K, int act_bits, int out_bits,
                                      void *stream) {
  if ((act_bits != 4 && act_bits != 6) || (out_bits != 4 && out_bits != 6)) return ATOM_ERR_INVALID_ARG;
  if (act_bits == 6)
    return out_bits == 6 ? launch_gu<MxE2M3, MxE2M3>(a_q, a_sc, a_q8, w_q4, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream)
                         : launch_gu<MxE2M3, MxE2M1>(a_q, a_sc, a_q8, w_q4, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream);
  return out_bits == 6 ? launch_gu<MxE2M1, MxE2M3>(a_q, a_sc, a_q8, w_q4, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream)
                       : launch_gu<MxE2M1, MxE2M1>(a_q, a_sc, a_q8, w_q4, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, stream);
}

// the one fused entry for every format triple: w_bits 6 reads the fused operand of two MXFP6 weights, [F/8][S][96][16]
int atom_gemm_mx_silu_mul_quant(const void *a_q, const void *a_sc, const void *a_q8, const void *w_q, const void *w_sc, const void *w_q8, void *out_q,
                                void *out_sc, void *out_q8, int64_t M, int64_t F, int64_t K, int act_bits, int w_bits, int out_bits, void *stream) {
  if ((act_bits != 4 && act_bits != 6) || (w_bits != 4 && w_bits != 6) || (out_bits != 4 && out_bits != 6)) return ATOM_ERR_INVALID_ARG;
  return w_bits == 6 ? launch_gu_bits<MxE2M3>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, act_bits, out_bits, stream)
                     : launch_gu_bits<MxE2M1>(a_q, a_sc, a_q8, w_q, w_sc, w_q8, out_q, out_sc, out_q8, M, F, K, act_bits, out_bits, stream);
}

int atom_rmsnorm_quant_mx_f16(const void *x_f16, const void *weight_f16, const int16_t *reorder_index, int64_t M, int64_t K, float eps, void *q4,
                              void *sc, void *q8, void *stream) {
  return launch_rmsnorm_quant_mx<false>(x_f16, nullptr, weight_f16, reorder_index, M, K, eps, q4, sc, q8, stream);
}

int atom_add_rmsnorm_quant_mx_f16(const void *x_f16, void *residual_inout_f16, const void *weight_f16, const int16_t *reorder_index, int64_t M,
                                  int64_t K, float eps, void *q4, void *sc, void *q8, void *stream) {
  return launch_rmsnorm_quant_mx<true>(x_f16, residual_inout_f16, weight_f16, reorder_index, M, K, eps, q4, sc, q8, stream);
}

int atom_rmsnorm_quant_mx6_f16(const void *x_f16, const void *weight_f16, const int16_t *reorder_index, int64_t M, int64_t K, float eps, void *q6,
                               void *sc, void *q8, void *stream) {
  return launch_rmsnorm_quant_mx<false, MxE2M3>(x_f16, nullptr, weight_f16, reorder_index, M, K, eps, q6, sc, q8, stream);
}

int atom_add_rmsnorm_quant_mx6_f16(const void *x_f16, void *residual_inout_f16, const void *weight_f16, const int16_t *reorder_index, int64_t M,
                                   int64_t K, float eps, void *q6, void *sc, void *q8, void *stream) {
  return launch_rmsnorm_quant_mx<true, MxE2M3>(x_f16, residual_inout_f16, weight_f16, reorder_index, M, K, eps, q6, sc, q8, stream);
}

}  // extern "C"
