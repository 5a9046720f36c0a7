// What the MX kernels share (gemm_mxfp4.hip, llama_mxfp4.hip; design: DESIGN.md 4.26, 4.28): the operand descriptors, the quantiser's
// block step (maximum, scale byte, codes, stores in fragment order) and the K loop of the 128 x 128 tile geometry.  A kernel is one of
// these plus its own value source or epilogue; the arithmetic and the accumulation chain exist once.
#pragma once
#include "mx_math.h"
#include <type_traits>

namespace atom {

typedef int v8i_t __attribute__((ext_vector_type(8)));

struct MxOperand {
  const uint8_t *q4, *sc, *q8;
  int tiles;   // row tiles of 16
};

constexpr int FMT_E2M1 = 4, FMT_E4M3 = 0, FMT_E2M3 = 2;   // the instruction's cbsz / blgp codes

// The bulk-code fragment (16 rows x one K step) of an operand, activation or weight, by format.  E2M1: [64 lanes][16 bytes].  E2M3: a lane's 32
// codes are 24 bytes = 6 registers, stored as a head [64 lanes][16 bytes] (registers 0 .. 3) and a tail [64 lanes][8 bytes] (registers
// 4, 5): 1024 + 512 bytes, every access a whole 16- or 8-byte piece at its natural alignment.  (A 12-byte LDS-DMA piece lands at a
// 16-byte lane stride -- measured, DESIGN.md 4.29 -- so planes of 12 bytes would cost 2 KiB of LDS per fragment.)  The instruction reads
// an E2M3 first operand (cbsz = 2) in the same lane and bit order as a second one (blgp = 2): measured, DESIGN.md 4.30.
template <class AF> struct MxAct;
template <> struct MxAct<MxE2M1> { static constexpr int FMT = FMT_E2M1, FRAG = 1024, TAIL = 0; };
template <> struct MxAct<MxE2M3> { static constexpr int FMT = FMT_E2M3, FRAG = 1536, TAIL = 512; };

inline bool mx_shape_ok(int64_t rows, int64_t K) { return rows >= 1 && rows < (1ll << 31) - 16 && K >= 256 && (K % 128) == 0 && K <= (1 << 20); }

// ------------------------------------------------------------------------------------------------------------------ quantiser
// The 8 values of channels c0 .. c0 + 7 of row 16 rt + r (S = the operand's FP4 steps): lanes 4 b .. 4 b + 3 of the wave hold block b of
// the trip, so the block maximum is two exchanges; the lane's codes go to its 4 (E2M1) or 8 (E4M3) bytes of the MFMA lane that holds
// those channels.  Every lane of such a group of 4 must be here.
// AF = MxE2M3: the lane's 8 bulk codes are bits 48 j .. 48 j + 47 of the block's 192; after three exchanges lane 0 of the group
// writes the head's 16 bytes and lane 2 the tail's 8.
template <class AF = MxE2M1>
__device__ __forceinline__ void mx_quant_store8(const float (&v)[8], int c0, int rt, int r, int S, uint8_t *__restrict__ q4,
                                                uint8_t *__restrict__ sc, uint8_t *__restrict__ q8) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  const int kb = c0 >> 5, j = (c0 >> 3) & 3;          // block of the row, the lane's quarter of it
  const int step = kb >> 2, ml = r + 16 * (kb & 3);   // K step, MFMA lane
  if (step < S) {
    const int sb = mx_scale_byte<AF>(amax);
    const float inv = mx_inv_scale(sb);
    if constexpr (std::is_same_v<AF, MxE2M3>) {
      unsigned lo = 0, hi = 0;                                // codes 0 .. 4 and the low 2 bits of code 5; the rest of 5, codes 6, 7
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned c = mx_code<MxE2M3>(v[i], inv);
        if (6 * i < 32) lo |= c << (6 * i);
        if (6 * i + 6 > 32) hi |= 6 * i >= 32 ? c << (6 * i - 32) : c >> (32 - 6 * i);
      }
      const unsigned olo = __shfl_xor(lo, 1), ohi = __shfl_xor(hi, 1), lo2 = __shfl_xor(lo, 2);
      uint8_t *frag = q4 + ((int64_t)rt * S + step) * 1536;
      const unsigned mid = hi | (olo << 16), top = (olo >> 16) | (ohi << 16);   // bits 32 .. 95 of the lane pair's 96
      if (j == 0) *reinterpret_cast<v4u *>(frag + ml * 16) = v4u{lo, mid, top, lo2};
      if (j == 2) *reinterpret_cast<v2u *>(frag + 1024 + ml * 8) = v2u{mid, top};
    } else {
      unsigned pk = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) pk |= mx_code<MxE2M1>(v[i], inv) << (4 * i);
      *reinterpret_cast<unsigned *>(q4 + (((int64_t)rt * S + step) * 64 + ml) * 16 + 4 * j) = pk;
    }
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

// ------------------------------------------------------------------------------------------------------------- 128 x 128 tiles
// A ring slot: 8 weight fragments, 8 activation fragments, their scale bytes (8 x 64 + 8 x 64).  A stage is one bulk K step or one half of
// the keeper step (stages S and S + 1, consumed together; their fragments are 1 KiB whatever the bulk formats are).  Either operand's
// region is the 8 fragments' first KiB (heads) at 1 KiB strides, then (E2M3) their 512-byte tails in the order 0 4 1 5 2 6 3 7; the
// activation's region follows the weight's (WA), the scale bytes follow both (SC).  Every wave requests PPW pieces of a bulk stage --
// per operand the heads of fragments w and w + 4 with 16 bytes per lane and (E2M3) the tails of fragments w and w + 4 as ONE 16-byte
// piece (lanes 0 .. 31 / 32 .. 63: they are neighbours in the tail order), then a quarter of the scale bytes with 4 -- and PPW8 = 5
// of a keeper stage; the waits count stages.  Stage / ring / workgroups per CU (160 KiB) by activation x weight format:
//   E2M1 x E2M1  17 KiB  51 KiB  3        E2M1 x E2M3  21 KiB  63 KiB  2
//   E2M3 x E2M1  21 KiB  63 KiB  2        E2M3 x E2M3  25 KiB  75 KiB  2   (static LDS beyond 64 KiB: the runtime launches it, 4.30)
// (three workgroups of 21 KiB stages would need 189 KiB; a 2-stage ring would fit more but cannot keep a stage in flight while one
// is read).
constexpr int MXT_NS = 3, MXT_FRAG = 1024;
template <class AF, class WF = MxE2M1>
struct MxRing {
  static constexpr int WA = 8 * MxAct<WF>::FRAG, SC = WA + 8 * MxAct<AF>::FRAG, STAGE = SC + 1024, LDS = MXT_NS * STAGE;
  static constexpr int PPW = 5 + (MxAct<AF>::TAIL ? 1 : 0) + (MxAct<WF>::TAIL ? 1 : 0), PPW8 = 5;
};

__device__ __forceinline__ v8i_t mx_frag4(const char *p) {
  const v4i f = *reinterpret_cast<const v4i *>(p);
  return v8i_t{f.x, f.y, f.z, f.w, 0, 0, 0, 0};
}
__device__ __forceinline__ v8i_t mx_frag8(const char *p0, const char *p1) {
  const v4i f = *reinterpret_cast<const v4i *>(p0), g = *reinterpret_cast<const v4i *>(p1);
  return v8i_t{f.x, f.y, f.z, f.w, g.x, g.y, g.z, g.w};
}
// a lane's registers of a bulk fragment of either operand (LDS or memory): its 16 bytes of the head (at head + 16 l) and, E2M3, its 8
// of the tail (at tail + 8 l)
template <class AF>
__device__ __forceinline__ v8i_t mx_frag_act(const char *head_l, const char *tail_l) {
  if constexpr (std::is_same_v<AF, MxE2M3>) {
    const v4i a = *reinterpret_cast<const v4i *>(head_l);
    const v2u b = *reinterpret_cast<const v2u *>(tail_l);
    return v8i_t{a.x, a.y, a.z, a.w, (int)b.x, (int)b.y, 0, 0};
  } else {
    return mx_frag4(head_l);
  }
}

// The tile's sums: weight fragments wt0 .. wt0 + 7 times activation fragments at0 .. at0 + 7, 4 waves of 64 x 64 (wave w: features
// 64 (w & 1) .., tokens 64 (w >> 1) ..).  acc[i][j], lane l: token l % 16 of the wave's activation fragment i, features 4 (l / 16) .. + 3
// of its weight fragment j.  Every element is one chain: K steps 0 .. S - 1 in order, then the keeper.  `lds`: MxRing<AF, WF>::LDS bytes,
// 16-aligned.  AF / WF: the formats of the activation's and the weight's bulk codes.
template <class AF, class WF = MxE2M1>
__device__ __forceinline__ void mx_tile_accumulate(const MxOperand &pa, const MxOperand &pw, int S, int wt0, int at0, char *lds, v4f (&acc)[4][4]) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int T = S + 1;
  using Ring = MxRing<AF, WF>;
  constexpr int AFRAG = MxAct<AF>::FRAG, WFRAG = MxAct<WF>::FRAG, MXT_A = Ring::WA, MXT_SC = Ring::SC, MXT_STAGE = Ring::STAGE, PPW = Ring::PPW,
                PPW8 = Ring::PPW8;
  const unsigned lds0 = lds_addr(lds);
  // a tile may hang over the operand's last row tile: the fragments beyond are read from the last one and their results never stored
  const int wf0 = min(wt0 + w, pw.tiles - 1), wf1 = min(wt0 + w + 4, pw.tiles - 1);
  const int af0 = min(at0 + w, pa.tiles - 1), af1 = min(at0 + w + 4, pa.tiles - 1);
  // the wave's quarter of the stage's scale bytes: 4 bytes per lane, bytes 256 w .. 256 w + 255 of [weights 8 x 64][activations 8 x 64]
  const int so = w * 256 + l * 4, sfrag = (so & 511) >> 6;
  const MxOperand &sop = so < 512 ? pw : pa;
  const uint8_t *ssrc = sop.sc + (int64_t)min((so < 512 ? wt0 : at0) + sfrag, sop.tiles - 1) * T * 64 + (so & 63);

  auto issue = [&](int st) {
    const unsigned dst = lds0 + (st % MXT_NS) * MXT_STAGE;
    const bool k8 = st >= S;
    const int64_t per = k8 ? 2 : S, at = k8 ? st - S : st;
    const uint8_t *wb = k8 ? pw.q8 : pw.q4, *ab = k8 ? pa.q8 : pa.q4;
    if (std::is_same_v<WF, MxE2M3> && !k8) {
      const uint8_t *w0 = wb + ((int64_t)wf0 * per + at) * WFRAG, *w1 = wb + ((int64_t)wf1 * per + at) * WFRAG;
      lds_dma_at<16>(w0 + l * 16, dst + w * MXT_FRAG);
      lds_dma_at<16>(w1 + l * 16, dst + (w + 4) * MXT_FRAG);
      lds_dma_at<16>((l < 32 ? w0 : w1) + MXT_FRAG + (l & 31) * 16, dst + 8 * MXT_FRAG + w * 1024);            // tails 2 w, 2 w + 1
    } else {
      lds_dma_at<16>(wb + ((int64_t)wf0 * per + at) * MXT_FRAG + l * 16, dst + w * MXT_FRAG);
      lds_dma_at<16>(wb + ((int64_t)wf1 * per + at) * MXT_FRAG + l * 16, dst + (w + 4) * MXT_FRAG);
    }
    if (std::is_same_v<AF, MxE2M3> && !k8) {
      const uint8_t *a0 = ab + ((int64_t)af0 * per + at) * AFRAG, *a1 = ab + ((int64_t)af1 * per + at) * AFRAG;
      lds_dma_at<16>(a0 + l * 16, dst + MXT_A + w * MXT_FRAG);
      lds_dma_at<16>(a1 + l * 16, dst + MXT_A + (w + 4) * MXT_FRAG);
      lds_dma_at<16>((l < 32 ? a0 : a1) + MXT_FRAG + (l & 31) * 16, dst + MXT_A + 8 * MXT_FRAG + w * 1024);   // tails 2 w, 2 w + 1
    } else {
      lds_dma_at<16>(ab + ((int64_t)af0 * per + at) * MXT_FRAG + l * 16, dst + MXT_A + w * MXT_FRAG);
      lds_dma_at<16>(ab + ((int64_t)af1 * per + at) * MXT_FRAG + l * 16, dst + MXT_A + (w + 4) * MXT_FRAG);
    }
    lds_dma_at<4>(ssrc + min(st, S) * 64, dst + MXT_SC + w * 256);
  };

  const int wn = w & 1, wm = w >> 1;                         // the wave's 64 features x 64 tokens of the tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  issue(0);
  issue(1);                                                  // S + 2 >= 3 stages
  for (int st = 0; st < S; ++st) {
    // stage st has landed (one younger stage may be in flight: stage st + 1, a keeper half when st = S - 1), this wave's reads of
    // the slot about to be refilled are done
    if (PPW == PPW8 || st + 1 < S) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PPW8) : "memory");
    __builtin_amdgcn_s_barrier();
    issue(st + 2);                                           // st + 2 <= S + 1: always a stage
    const char *slot = lds + (st % MXT_NS) * MXT_STAGE;
    v8i_t fa[4];
    int sa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa[i] = mx_frag_act<AF>(slot + MXT_A + (wm * 4 + i) * MXT_FRAG + l * 16, slot + MXT_A + 8 * MXT_FRAG + (2 * i + wm) * 512 + l * 8);
      sa[i] = *reinterpret_cast<const uint8_t *>(slot + MXT_SC + 512 + (wm * 4 + i) * 64 + l);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const v8i_t fw = mx_frag_act<WF>(slot + (wn * 4 + j) * MXT_FRAG + l * 16, slot + 8 * MXT_FRAG + (2 * j + wn) * 512 + l * 8);
      const int sw = *reinterpret_cast<const uint8_t *>(slot + MXT_SC + (wn * 4 + j) * 64 + l);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[i][j], MxAct<WF>::FMT, MxAct<AF>::FMT, 0, sw, 0, sa[i]);
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
}

// One K-step share of the decode geometry (M <= 16: a single activation fragment per step, the weight read once): the sums of the NF
// consecutive weight fragments from ct0 on, over this wave's K steps w, w + WAVES, ... (the keeper counts as step S), weights straight
// into registers, non-temporal.  The caller sums the waves' tiles in wave order.  AF / WF: the formats of the activation's and the
// weight's bulk codes; either fragment is 4 or 6 registers per lane, loaded straight from memory (E2M3 weight: one dwordx4 of the head
// and one dwordx2 of the tail per lane and fragment, both non-temporal: 1.5 x the weight stream).
template <class AF, int NF, int WAVES, class WF = MxE2M1>
__device__ __forceinline__ void mx_dec_accumulate(const MxOperand &pa, const MxOperand &pw, int S, int64_t ct0, int w, int l, v4f (&acc)[NF]) {
  const int T = S + 1;
  constexpr int WFRAG = MxAct<WF>::FRAG;
  const uint8_t *wq = pw.q4 + ct0 * S * WFRAG + l * 16, *wsc = pw.sc + ct0 * T * 64 + l;
  const uint8_t *aq = pa.q4 + l * 16, *at = pa.q4 + 1024 + l * 8, *asc = pa.sc + l;
#pragma unroll
  for (int j = 0; j < NF; ++j) acc[j] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int st = w; st < S; st += WAVES) {
    const int64_t ao = (int64_t)st * MxAct<AF>::FRAG;
    const v8i_t fa = mx_frag_act<AF>(reinterpret_cast<const char *>(aq) + ao, reinterpret_cast<const char *>(at) + ao);
    const int sa = asc[st * 64];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const uint8_t *wf = wq + ((int64_t)j * S + st) * WFRAG;
      const v4i fw = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(wf));
      v2u ft = {0u, 0u};
      if constexpr (std::is_same_v<WF, MxE2M3>) ft = __builtin_nontemporal_load(reinterpret_cast<const v2u *>(wf + 1024 - l * 8));
      const int sw = wsc[(j * T + st) * 64];
      acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(v8i_t{fw.x, fw.y, fw.z, fw.w, (int)ft.x, (int)ft.y, 0, 0}, fa, acc[j],
                                                                MxAct<WF>::FMT, MxAct<AF>::FMT, 0, sw, 0, sa);
    }
  }
  if (w == S % WAVES) {
    const uint8_t *a8 = pa.q8 + l * 16;
    const v4i g0 = *reinterpret_cast<const v4i *>(a8), g1 = *reinterpret_cast<const v4i *>(a8 + 1024);
    const int sa = asc[S * 64];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const uint8_t *w8 = pw.q8 + (ct0 + j) * 2048 + l * 16;
      const v4i f0 = *reinterpret_cast<const v4i *>(w8), f1 = *reinterpret_cast<const v4i *>(w8 + 1024);
      const int sw = wsc[(j * T + S) * 64];
      acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(v8i_t{f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w},
                                                                v8i_t{g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, acc[j], FMT_E4M3, FMT_E4M3, 0, sw,
                                                                0, sa);
    }
  }
}

}  // namespace atom
