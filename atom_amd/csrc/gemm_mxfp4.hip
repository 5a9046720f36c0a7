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
#include "mx_math.h"
#include "quant_math.h"

namespace atom {
namespace {

typedef int v8i_t __attribute__((ext_vector_type(8)));

struct MxOperand {
  const uint8_t *q4, *sc, *q8;
  int tiles;   // row tiles of 16
};
struct MxGemmParams {
  MxOperand a, w;
  half_t *out;
  int M, N, S;   // S = FP4 K steps; step S is the keeper
};

constexpr int FMT_E2M1 = 4, FMT_E4M3 = 0;

// ------------------------------------------------------------------------------------------------------------------ quantiser
// Row `row` of the padded operand (rows >= M are written as zero blocks), every lane 8 channels of a block per trip: lanes 4 b .. 4 b + 3
// share block b of the trip's 16.  The lane's codes go to its 4 (E2M1) or 8 (E4M3) bytes of the MFMA lane that holds those channels.
// SILU: the values are silu_mul<false>(x, up) of quant_math.h (x = gate; no reorder: the producer's rows are stored in channel order).
template <bool SILU>
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
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const int kb = c0 >> 5, j = (c0 >> 3) & 3;          // block of the row, the lane's quarter of it
    const int step = kb >> 2, ml = r + 16 * (kb & 3);   // K step, MFMA lane
    if (step < S) {
      const int sb = mx_scale_byte<MxE2M1>(amax);
      const float inv = mx_inv_scale(sb);
      unsigned pk = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) pk |= mx_code<MxE2M1>(v[i], inv) << (4 * i);
      *reinterpret_cast<unsigned *>(q4 + (((int64_t)rt * S + step) * 64 + ml) * 16 + 4 * j) = pk;
      if (j == 0) sc[((int64_t)rt * (S + 1) + step) * 64 + ml] = (uint8_t)sb;
    } else {
      const int sb = mx_scale_byte<MxE4M3>(amax);
      const float inv = mx_inv_scale(sb);
      v2u pk = {0u, 0u};
#pragma unroll
      for (int i = 0; i < 8; ++i) pk[i >> 2] |= mx_code<MxE4M3>(v[i], inv) << (8 * (i & 3));
      // E4M3 operands sit differently from E2M1 ones (measured): registers 0 .. 3 of lane group g hold channels
      // 16 g .. 16 g + 15 of the step, registers 4 .. 7 channels 64 + 16 g ..; the scale of block b still comes from lane group b
      const int kc = c0 - S * 128;
      *reinterpret_cast<v2u *>(q8 + (((int64_t)rt * 2 + (kc >> 6)) * 64 + r + 16 * ((kc >> 4) & 3)) * 16 + (kc & 15)) = pk;
      if (j == 0) sc[((int64_t)rt * (S + 1) + S) * 64 + ml] = (uint8_t)sb;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- 128 x 128 tiles
// A ring slot: 8 weight fragments, 8 activation fragments (1 KiB each), their scale bytes (8 x 64 + 8 x 64).  A stage is one FP4 K step
// or one half of the keeper step (stages S and S + 1, consumed together); every wave requests 5 pieces of every stage (fragments w and
// w + 4 of either operand with 16 bytes per lane, a quarter of the scale bytes with 4), so the waits count stages.
constexpr int MXT_NS = 3, MXT_FRAG = 1024, MXT_A = 8 * MXT_FRAG, MXT_SC = 16 * MXT_FRAG, MXT_STAGE = MXT_SC + 1024, MXT_PPW = 5;

__device__ __forceinline__ v8i_t mx_frag4(const char *p) {
  const v4i f = *reinterpret_cast<const v4i *>(p);
  return v8i_t{f.x, f.y, f.z, f.w, 0, 0, 0, 0};
}
__device__ __forceinline__ v8i_t mx_frag8(const char *p0, const char *p1) {
  const v4i f = *reinterpret_cast<const v4i *>(p0), g = *reinterpret_cast<const v4i *>(p1);
  return v8i_t{f.x, f.y, f.z, f.w, g.x, g.y, g.z, g.w};
}

__global__ __launch_bounds__(256) void gemm_mxfp4_tile_kernel(MxGemmParams p) {
  __shared__ __attribute__((aligned(16))) char lds[MXT_NS * MXT_STAGE];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int S = p.S, T = S + 1;
  const int wt0 = blockIdx.x * 8, at0 = blockIdx.y * 8;     // first fragment (16 features / 16 tokens) of the tile
  const unsigned lds0 = lds_addr(lds);
  // a tile may hang over the operand's last row tile: the fragments beyond are read from the last one and their results never stored
  const int wf0 = min(wt0 + w, p.w.tiles - 1), wf1 = min(wt0 + w + 4, p.w.tiles - 1);
  const int af0 = min(at0 + w, p.a.tiles - 1), af1 = min(at0 + w + 4, p.a.tiles - 1);
  // the wave's quarter of the stage's scale bytes: 4 bytes per lane, bytes 256 w .. 256 w + 255 of [weights 8 x 64][activations 8 x 64]
  const int so = w * 256 + l * 4, sfrag = (so & 511) >> 6;
  const MxOperand &sop = so < 512 ? p.w : p.a;
  const uint8_t *ssrc = sop.sc + (int64_t)min((so < 512 ? wt0 : at0) + sfrag, sop.tiles - 1) * T * 64 + (so & 63);

  auto issue = [&](int st) {
    const unsigned dst = lds0 + (st % MXT_NS) * MXT_STAGE;
    const bool k8 = st >= S;
    const int64_t per = k8 ? 2 : S, at = k8 ? st - S : st;
    const uint8_t *wb = k8 ? p.w.q8 : p.w.q4, *ab = k8 ? p.a.q8 : p.a.q4;
    lds_dma_at<16>(wb + ((int64_t)wf0 * per + at) * MXT_FRAG + l * 16, dst + w * MXT_FRAG);
    lds_dma_at<16>(wb + ((int64_t)wf1 * per + at) * MXT_FRAG + l * 16, dst + (w + 4) * MXT_FRAG);
    lds_dma_at<16>(ab + ((int64_t)af0 * per + at) * MXT_FRAG + l * 16, dst + MXT_A + w * MXT_FRAG);
    lds_dma_at<16>(ab + ((int64_t)af1 * per + at) * MXT_FRAG + l * 16, dst + MXT_A + (w + 4) * MXT_FRAG);
    lds_dma_at<4>(ssrc + min(st, S) * 64, dst + MXT_SC + w * 256);
  };

  const int wn = w & 1, wm = w >> 1;                         // the wave's 64 features x 64 tokens of the tile
  v4f acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  issue(0);
  issue(1);                                                  // S + 2 >= 3 stages
  for (int st = 0; st < S; ++st) {
    // stage st has landed (one younger stage may be in flight), this wave's reads of the slot about to be refilled are done
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MXT_PPW) : "memory");
    __builtin_amdgcn_s_barrier();
    issue(st + 2);                                           // st + 2 <= S + 1: always a stage
    const char *slot = lds + (st % MXT_NS) * MXT_STAGE;
    v8i_t fa[4];
    int sa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa[i] = mx_frag4(slot + MXT_A + (wm * 4 + i) * MXT_FRAG + l * 16);
      sa[i] = *reinterpret_cast<const uint8_t *>(slot + MXT_SC + 512 + (wm * 4 + i) * 64 + l);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const v8i_t fw = mx_frag4(slot + (wn * 4 + j) * MXT_FRAG + l * 16);
      const int sw = *reinterpret_cast<const uint8_t *>(slot + MXT_SC + (wn * 4 + j) * 64 + l);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[i][j], FMT_E2M1, FMT_E2M1, 0, sw, 0, sa[i]);
    }
  }
  // the keeper: both halves have been requested; MXFP8 fragments are 32 bytes per lane, 16 from either slot
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  {
    const char *s0 = lds + (S % MXT_NS) * MXT_STAGE, *s1 = lds + ((S + 1) % MXT_NS) * MXT_STAGE;
    v8i_t fa[4];
    int sa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = MXT_A + (wm * 4 + i) * MXT_FRAG + l * 16;
      fa[i] = mx_frag8(s0 + o, s1 + o);
      sa[i] = *reinterpret_cast<const uint8_t *>(s0 + MXT_SC + 512 + (wm * 4 + i) * 64 + l);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = (wn * 4 + j) * MXT_FRAG + l * 16;
      const v8i_t fw = mx_frag8(s0 + o, s1 + o);
      const int sw = *reinterpret_cast<const uint8_t *>(s0 + MXT_SC + (wn * 4 + j) * 64 + l);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[i][j], FMT_E4M3, FMT_E4M3, 0, sw, 0, sa[i]);
    }
  }
  // lane l: token l % 16 of activation fragment i, features 4 (l / 16) .. + 3 of weight fragment j
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (at0 + wm * 4 + i) * 16 + (l & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = (wt0 + wn * 4 + j) * 16 + (l >> 4) * 4;
      if (m < p.M && n < p.N) {
        const half_t h[4] = {(half_t)acc[i][j][0], (half_t)acc[i][j][1], (half_t)acc[i][j][2], (half_t)acc[i][j][3]};
        *reinterpret_cast<v2u *>(p.out + (int64_t)m * p.N + n) = __builtin_bit_cast(v2u, h);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ decode
// M <= 16: the activation is one fragment per K step (it stays in L2), the weight is read once.  Workgroup = one weight fragment column
// (16 features), wave w = K steps w, w + 8, ... (the keeper counts as step S); the 8 partial tiles are summed in wave order.
constexpr int MXD_WAVES = 8;

__global__ __launch_bounds__(64 * MXD_WAVES) void gemm_mxfp4_dec_kernel(MxGemmParams p) {
  __shared__ v4f part[MXD_WAVES][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int S = p.S, T = S + 1;
  const int64_t ct = blockIdx.x;
  const uint8_t *wq = p.w.q4 + ct * S * 1024 + l * 16, *wsc = p.w.sc + ct * T * 64 + l;
  const uint8_t *aq = p.a.q4 + l * 16, *asc = p.a.sc + l;
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  for (int st = w; st < S; st += MXD_WAVES) {
    const v4i fw = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(wq + (int64_t)st * 1024));
    const v4i fa = *reinterpret_cast<const v4i *>(aq + (int64_t)st * 1024);
    const int sw = wsc[st * 64], sa = asc[st * 64];
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(v8i_t{fw.x, fw.y, fw.z, fw.w, 0, 0, 0, 0}, v8i_t{fa.x, fa.y, fa.z, fa.w, 0, 0, 0, 0},
                                                           acc, FMT_E2M1, FMT_E2M1, 0, sw, 0, sa);
  }
  if (w == S % MXD_WAVES) {
    const uint8_t *w8 = p.w.q8 + ct * 2048 + l * 16, *a8 = p.a.q8 + l * 16;
    const v4i f0 = *reinterpret_cast<const v4i *>(w8), f1 = *reinterpret_cast<const v4i *>(w8 + 1024);
    const v4i g0 = *reinterpret_cast<const v4i *>(a8), g1 = *reinterpret_cast<const v4i *>(a8 + 1024);
    const int sw = wsc[S * 64], sa = asc[S * 64];
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(v8i_t{f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w},
                                                           v8i_t{g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, acc, FMT_E4M3, FMT_E4M3, 0, sw, 0, sa);
  }
  part[w][l] = acc;
  __syncthreads();
  if (w == 0) {
    v4f s = part[0][l];
#pragma unroll
    for (int i = 1; i < MXD_WAVES; ++i) s += part[i][l];
    const int m = l & 15;
    if (m < p.M) {
      const half_t h[4] = {(half_t)s[0], (half_t)s[1], (half_t)s[2], (half_t)s[3]};
      *reinterpret_cast<v2u *>(p.out + (int64_t)m * p.N + ct * 16 + (l >> 4) * 4) = __builtin_bit_cast(v2u, h);
    }
  }
}

bool mx_shape_ok(int64_t rows, int64_t K) { return rows >= 1 && rows < (1ll << 31) - 16 && K >= 256 && (K % 128) == 0 && K <= (1 << 20); }

template <bool SILU>
int launch_mx_quant(const void *x, const void *up, const int16_t *idx, int64_t rows, int64_t K, void *q4, void *sc, void *q8, void *stream) {
  if (!x || (SILU && !up) || !q4 || !sc || !q8) return ATOM_ERR_INVALID_ARG;
  if (!mx_shape_ok(rows, K)) return ATOM_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(up) || !aligned16(idx) || !aligned16(q4) || !aligned16(sc) || !aligned16(q8)) return ATOM_ERR_ALIGN;
  const int64_t pad = (rows + 15) / 16 * 16;
  hipLaunchKernelGGL(mx_quant_kernel<SILU>, dim3((unsigned)(pad / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const half_t *)x,
                     (const half_t *)up, idx, (int)rows, (int)pad, (int)K, (uint8_t *)q4, (uint8_t *)sc, (uint8_t *)q8);
  return check_launch();
}

}  // namespace
}  // namespace atom

using namespace atom;

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
  if (!a_q4 || !a_sc || !a_q8 || !w_q4 || !w_sc || !w_q8 || !out_f16) return ATOM_ERR_INVALID_ARG;
  const int route = atom_gemm_mxfp4_route(M, N, K);
  if (!route) return ATOM_ERR_SHAPE;
  if (!aligned16(a_q4) || !aligned16(a_sc) || !aligned16(a_q8) || !aligned16(w_q4) || !aligned16(w_sc) || !aligned16(w_q8) ||
      !aligned16(out_f16))
    return ATOM_ERR_ALIGN;
  MxGemmParams p{{(const uint8_t *)a_q4, (const uint8_t *)a_sc, (const uint8_t *)a_q8, (int)((M + 15) / 16)},
                 {(const uint8_t *)w_q4, (const uint8_t *)w_sc, (const uint8_t *)w_q8, (int)(N / 16)},
                 (half_t *)out_f16, (int)M, (int)N, (int)(K / 128 - 1)};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (route == 1) {
    hipLaunchKernelGGL(gemm_mxfp4_dec_kernel, dim3((unsigned)(N / 16)), dim3(64 * MXD_WAVES), 0, s, p);
  } else {
    hipLaunchKernelGGL(gemm_mxfp4_tile_kernel, dim3((unsigned)((N + 127) / 128), (unsigned)((M + 127) / 128)), dim3(256), 0, s, p);
  }
  return check_launch();
}

}  // extern "C"
