// THE statement of the activation quantisers' arithmetic: every step between a row of fp16 values and the codes, scales and records
// that leave a quantiser is written here once, as a pure device function (the only memory traffic: the steps that ARE stores).  The
// kernels that contain a quantiser -- quant_kernels.hip (stand-alone launches, re-coding), gemvq_w4a4.hip and gemm_w4a4_skinny.hip
// (quantiser in front of a decode GEMM), gemm_w4a4_f6.hip (SiLU x up -> quant behind gate_proj / up_proj) -- differ only in how the
// values reach these functions and where the codes go.  Two modes, specified op by op and restated in oracle/:
//   SIM     the simulated path (model/quant.py:134-181): FP16 opmath -- amax.clamp(1e-5) * clip, scale = amax / qmax, every step
//           rounded to half; code = clamp(round_half_even(x / scale))
//   kernel  the CUDA kernels (Reorder.cuh:137-178 == Activate.cuh:112-167): FP32, scale = amax * clip / qmax,
//           code = clamp(round_half_away(x * (1 / scale)))
#pragma once
#include "common.h"

namespace atom {

struct GroupScale {
  float s_store;     // the scale as stored (SIM: already a half value; kernel: FP32, rounded to half by the store)
  float s_dq;        // the scale the de-quantised output uses
  float so, rs;      // SIM: scale (opaque copy) and RN(1 / scale); kernel: rs = 1 / scale (0 for an all-zero group)
  float qlo, qmax;
};

template <bool SIM>
__device__ __forceinline__ GroupScale group_scale(float amax, bool keeper, float clip) {
  GroupScale g;
  g.qmax = keeper ? 127.f : 7.f;
  g.qlo = keeper ? -128.f : -8.f;
  const float c = keeper ? 1.0f : clip;
  if constexpr (SIM) {
    amax = fmaxf(amax, (float)(half_t)1e-5f);               // quant.py:141-142
    if (c < 1.0f) amax = round_h(amax * c);                 // :168-169
    // amax / qmax and w / scales: correctly rounded FP32 quotients from  q1 = fma(fma(-q0,d,n), r, q0), q0 = n*r,
    // r = RN(1/d) -- exact for every finite fp16 n and positive fp16 d (tools/probes/div_probe.cpp; 7 and 127 are fp16)
    const float rq = keeper ? (1.0f / 127.0f) : (1.0f / 7.0f);
    const float a0 = opaque(amax);
    const float d0 = a0 * rq;
    const float s = round_h(__builtin_fmaf(__builtin_fmaf(-d0, g.qmax, a0), rq, d0));   // :170
    g.so = opaque(s);
    // RN(1/s) from v_rcp_f32 + one Newton step: equal to the IEEE quotient for every positive fp16 s (round_probe.cpp)
    const float r0 = __builtin_amdgcn_rcpf(g.so);
    g.rs = __builtin_fmaf(__builtin_fmaf(-r0, g.so, 1.0f), r0, r0);
    g.s_store = s;
    g.s_dq = s;
  } else {
    // Reorder.cuh:137-178
    if (c < 1.0f) amax = amax * c;
    const float sf = amax / g.qmax;
    g.so = sf;
    g.rs = sf != 0.f ? 1.0f / sf : 0.f;                     // all-zero group: codes 0 (0*inf = NaN in the reference)
    g.s_store = sf;
    g.s_dq = round_h(sf);
  }
  return g;
}

// the code of one value, as an integer-valued float
template <bool SIM>
__device__ __forceinline__ float group_code(float v, const GroupScale &g) {
  if constexpr (SIM) {
    const float q0 = v * g.rs;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-q0, g.so, v), g.rs, q0);
    // :181 clamp(round(w / scales)): clamp first (bounds are integers), then round half-to-even
    return rintf(__builtin_amdgcn_fmed3f(round_h(q1), g.qlo, g.qmax));
  } else {
    const float t = __builtin_amdgcn_fmed3f(v * g.rs, g.qlo, g.qmax);
    // round half away from zero (CUDA round()) = sign(t) * floor(|t| + 0.5): v_cvt_rpi_i32_f32 computes
    // floor(x + 0.5) exactly (checked for every fp32 in [0, 300), tools/probes/round_probe.cpp)
    int ri;
    asm("v_cvt_rpi_i32_f32 %0, |%1|" : "=v"(ri) : "v"(t));
    return __builtin_copysignf((float)ri, t);
  }
}

// Codes (integer-valued floats) -> packed words, exact integer arithmetic in FP32 (bias folded into the initial value, two's complement
// restored with one XOR per word): 4 codes -> one word of INT8 keeper bytes, code k at byte k; 8 codes -> one word of INT4 nibbles,
// code k at bits 4 k
__device__ __forceinline__ unsigned pack_bytes4(const float *tr) {
  const float lo = __builtin_fmaf(tr[1], 256.f, tr[0] + 32896.f);                        // (c0+128) + (c1+128)*256
  const float hi = __builtin_fmaf(tr[3], 256.f, tr[2] + 32896.f);
  return ((unsigned)lo | ((unsigned)hi << 16)) ^ 0x80808080u;
}
__device__ __forceinline__ unsigned pack_nibbles8(const float *tr) {
  float lo = 34952.f, hi = 34952.f;                                                      // sum 8*16^i, i<4
  lo = __builtin_fmaf(tr[0], 1.f, lo);
  lo = __builtin_fmaf(tr[1], 16.f, lo);
  lo = __builtin_fmaf(tr[2], 256.f, lo);
  lo = __builtin_fmaf(tr[3], 4096.f, lo);
  hi = __builtin_fmaf(tr[4], 1.f, hi);
  hi = __builtin_fmaf(tr[5], 16.f, hi);
  hi = __builtin_fmaf(tr[6], 256.f, hi);
  hi = __builtin_fmaf(tr[7], 4096.f, hi);
  return ((unsigned)lo | ((unsigned)hi << 16)) ^ 0x88888888u;
}
// 8 codes: the nibble word (in [0]) or the two keeper words
__device__ __forceinline__ v2u pack_codes8(const float *tr, bool keeper) {
  if (keeper) return v2u{pack_bytes4(tr), pack_bytes4(tr + 4)};
  return v2u{pack_nibbles8(tr), 0u};
}
// the 16 codes of one slot: channel k at nibble k % 8 of word k / 8 (2 words), or at keeper byte k % 4 of word k / 4 (4 words)
__device__ __forceinline__ v4u pack_codes16(const float (&tr)[16], bool keeper) {
  if (keeper) {
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = pack_bytes4(tr + 4 * k);
    return v4u{w[0], w[1], w[2], w[3]};
  }
  unsigned w[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) w[k] = pack_nibbles8(tr + 8 * k);
  return v4u{w[0], w[1], 0u, 0u};
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float max8(float a) {   // max over the aligned 8 lanes this lane belongs to
  a = fmaxf(a, dpp_f<0xB1>(a));                      // quad_perm [1,0,3,2]
  a = fmaxf(a, dpp_f<0x4E>(a));                      // quad_perm [2,3,0,1]
  a = fmaxf(a, dpp_f<0x141>(a));                     // row_half_mirror
  return a;
}

// ... and over the aligned 16 lanes (one DPP row): exact, order-free
__device__ __forceinline__ float max16(float a) {
  a = max8(a);
  a = fmaxf(a, dpp_f<0x140>(a));                      // row_mirror: lanes 8-15 <-> 7-0 of the row
  return a;
}

// One thread's N values of a quantisation group -> their codes tr (integer-valued floats) and the group's scale: amax over the values,
// `reduce` over the lanes that share the group (max8: 16 values per lane, max16: 8), group_scale, group_code
template <bool SIM, float (&reduce)(float), int N>
__device__ __forceinline__ GroupScale group_codes(const float (&v)[N], bool keeper, float clip, float (&tr)[N]) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = reduce(amax);
  const GroupScale gs = group_scale<SIM>(amax, keeper, clip);
#pragma unroll
  for (int i = 0; i < N; ++i) tr[i] = group_code<SIM>(v[i], gs);
  return gs;
}

// The de-quantised value of a code: code * scale is exact in FP32 (8 x 11 significant bits), so one rounding to half == the reference's
// half multiply; "+ 0" turns the -0 of a negative value that rounded to code 0 into the reference's +0
__device__ __forceinline__ half_t dequant_half(float code, const GroupScale &gs) { return (half_t)__builtin_fmaf(code, gs.s_dq, 0.0f); }

// N <= 32 codes -> the first N 6-bit fields of one BF6 conversion (the rest zero).  BF6 (E3M2) holds every INT4 code exactly;
// v_cvt_scalef32_2xpk16_bf6_f32 converts AND packs 32 floats, interleaving its two sources (field 2i = a[i], 2i+1 = b[i]; tools/probes)
template <int N>
__device__ __forceinline__ v6u_t bf6_fields(const float (&tr)[N]) {
  v16f_t ea, eb;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ea[i] = 2 * i < N ? tr[2 * i] : 0.f;
    eb[i] = 2 * i < N ? tr[2 * i + 1] : 0.f;
  }
  return cvt_2xpk16_bf6(ea, eb);
}
// 16 packed bytes = 32 INT4 codes -> the two sources of that conversion: byte i = fields 2i (low nibble) and 2i+1, sign-extended
__device__ __forceinline__ void nibbles16_to_f32x32(v4u raw, v16f_t &ea, v16f_t &eb) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned byte = (raw[i >> 2] >> (8 * (i & 3))) & 0xFF;
    ea[i] = (float)((int)(byte << 28) >> 28);
    eb[i] = (float)((int)(byte << 24) >> 28);
  }
}
// the scale words of a BF6 record: the GEMM reads the token scale from the row itself, fp16 at byte 96, the same value as fp32 at byte 100
__device__ __forceinline__ v2u f6_scale_words(unsigned sh) {
  return v2u{sh, __builtin_bit_cast(unsigned, (float)__builtin_bit_cast(half_t, (unsigned short)sh))};
}
// a token's scale into a per-group scale vector: plain [rows], or the reference layout's four replicas (Reorder.cuh:39-44)
__device__ __forceinline__ void store_token_scale(half_t *dst, int64_t row, half_t s, int ref_layout) {
  if (ref_layout) {
    const int base = ref_scale_index((int)row);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[base + 2 * k] = s;
  } else {
    dst[row] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// RMSNorm in front of the codes.  Sum of squares: a FIXED-SHAPE FP32 tree over the row in memory order (not over the gathered channels,
// so the reorder index does not enter): 16-byte chunk c belongs to thread (wave (c / 64) % 4, lane c % 64) of 256; a thread folds its
// chunks in order with s = fma(x, x, s); lanes combine by the butterfly xor 32, 16, .., 1 (wave_sum_butterfly); the four waves as
// ((w0 + w1) + w2) + w3.  Deterministic, restated step by step in oracle/ (r01 used an FP64 sum rounded once: two half-rate
// instructions per element).
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float sumsq8(h8 v, float ss) {
#pragma unroll
  for (int k = 0; k < 8; ++k) ss = __builtin_fmaf((float)v[k], (float)v[k], ss);
  return ss;
}
// 1.0f / sqrtf(x), BOTH operations correctly rounded (what hipcc's default expansion delivers and the oracle restates), without the
// range handling of that expansion: for 2^-64 <= x <= 2^64 -- every RMSNorm statistic `mean(x^2) + eps` of fp16 data with a sane eps --
// v_sqrt_f32's result is off by at most one ulp and the two residual tests below pick the correctly rounded neighbour (the compiler's
// own fix-up minus its 2^32 pre-scaling for tiny arguments), and the reciprocal is the compiler's Newton / residual sequence with the
// v_div_scale / v_div_fmas / v_div_fixup wrappers dropped (they are identities for a numerator of 1 and a denominator in [2^-32, 2^32]).
// 17 instructions instead of 45 per wave and row of the RMSNorm quantisers; outside the range the generic expression runs.  Checked
// against the generic expression for 1.5e9 arguments on the hardware (tools/probes/rinv_probe.cpp, profiles/r05/rinv_probe.txt).
__device__ __forceinline__ float rinv_sqrt_exact(float x) {
  if (!(x >= 0x1p-64f && x <= 0x1p+64f)) return 1.0f / sqrtf(x);   // (wave-uniform in the kernels: x is a row statistic)
  float y = __builtin_amdgcn_sqrtf(x);
  const float ym = __int_as_float(__float_as_int(y) - 1), yp = __int_as_float(__float_as_int(y) + 1);
  const float em = __builtin_fmaf(-ym, y, x), ep = __builtin_fmaf(-yp, y, x);
  y = em <= 0.f ? ym : y;
  y = ep > 0.f ? yp : y;
  float r = __builtin_amdgcn_rcpf(y);
  r = __builtin_fmaf(__builtin_fmaf(-y, r, 1.0f), r, r);
  float q = r;                                              // 1.0f * r
  q = __builtin_fmaf(__builtin_fmaf(-y, q, 1.0f), r, q);
  return __builtin_fmaf(__builtin_fmaf(-y, q, 1.0f), r, q);
}

// the four waves' partial sums -> 1 / sqrt(mean + eps): correctly rounded divide, sqrt and divide (hipcc default); a power-of-two H
// divides exactly by multiplying
__device__ __forceinline__ float rms_rinv(const float *red4, int H, float eps) {
  const float tot = ((red4[0] + red4[1]) + red4[2]) + red4[3];
  const float var = (H & (H - 1)) == 0 ? tot * (1.0f / (float)H) : tot / (float)H;
  return rinv_sqrt_exact(var + eps);
}
// One normalised value.  kernel: RMSNorm.cuh:145-151, (x * w) * rinv in FP32, then half -- TWO roundings.  SIM: HF LlamaRMSNorm in
// half opmath, half(x * rinv) from the FP32 product (two roundings again), then a half multiply by the weight (the exact product of
// two halves rounded once).  round_h / f2h keep hipcc from fusing product and conversion into v_fma_mixlo_f16, which rounds the exact
// product ONCE: a different half wherever the FP32 rounding lands on the midpoint of two halves, ~6e-5 of all values, one code or scale
// in a million (rounds 4-6 had it; found by the row-loop tests at 6181 rows).  sim_scale1 below is the SIM form on half pairs.
template <bool SIM>
__device__ __forceinline__ float rmsnorm_value(half_t x, half_t w, float rinv) {
  if constexpr (SIM) {
    const half_t y = f2h((float)x * rinv);
    return (float)(half_t)(w * y);
  } else {
    return round_h(((float)x * (float)w) * rinv);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// SIM mode in the FP16 domain (round 4).  The simulated path's values ARE halves (model/quant.py:134-181 runs in fp16), yet round 1-3
// carried them as floats: per value 3 FP32 ops for the exact quotient + 2 conversions to round it to half + clamp + rint = 7, after
// 3 for the RMSNorm product -- 112 + 48 of the 360 VALU a wave spends on a row (profiles/r04/pmc_quantisers.txt: the kernels are
// VALU-bound).  Here a slot's 16 values are 8 HALF PAIRS and the work that can be packed is:
//   pair i of a slot = channels (L, L + 4), L = 8 (i / 4) + i % 4   -- the nibble order of the packed word falls out of the pairing
//   q0 = half(v * RN(1/s))                      v_fma_mixlo/hi_f16   (any faithful estimate will do)
//   e  = v - s * q0          exactly, in FP32   v_fma_mix_f32        (22-bit product, cancellation: fits 24 bits)
//   q  = half(q0 + e * RN(1/s))                 v_fma_mixlo/hi_f16   == RN_half(v / s): q0 + e r = (v / s)(1 + 2^-25), and a quotient of
//        two halves that is not itself a half or a midpoint is >= 2^-23 (relative) away from the nearest midpoint of two halves
//   clamp, then + 1536                          v_pk_max/min/add_f16 (half(q + 1536) IS round-half-even to an integer; the code sits in
//        the low bits of the half's bit pattern, two's complement: 0x6600 + c)
// = 4.5 per value and the result is already packed pairwise.  Bit-identical to group_code<true> for every half v and every scale a
// group can have with clip >= 1/64 (smaller clips could overflow q0 in FP16: the callers take the FP32 form then); checked against
// the oracle by the same tests as before.  The sequences are inline asm: hipcc turns the C form into packed FP32 + conversions, and
// dependent 16-bit partial writes need a wait state it cannot see inside asm -- every block keeps dependent instructions >= 2 apart.
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__host__ __device__ constexpr int pair_lo(int i) { return 8 * (i >> 2) + (i & 3); }          // pair i = channels (pair_lo, pair_lo + 4)
constexpr float kSimHalfMinClip = 1.0f / 64.0f;

#define ATOM_Q0LO(i) "v_fma_mixlo_f16 %[q" #i "], %[z" #i "], %[rs], 0 op_sel_hi:[1,0,0]\n\t"
#define ATOM_Q0HI(i) "v_fma_mixhi_f16 %[q" #i "], %[z" #i "], %[rs], 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
#define ATOM_ELO(i) "v_fma_mix_f32 %[a" #i "], -%[s], %[q" #i "], %[z" #i "] op_sel_hi:[1,1,1]\n\t"
#define ATOM_EHI(i) "v_fma_mix_f32 %[b" #i "], -%[s], %[q" #i "], %[z" #i "] op_sel:[0,1,1] op_sel_hi:[1,1,1]\n\t"
#define ATOM_Q1LO(i) "v_fma_mixlo_f16 %[t" #i "], %[a" #i "], %[rs], %[q" #i "] op_sel_hi:[0,0,1]\n\t"
#define ATOM_Q1HI(i) "v_fma_mixhi_f16 %[t" #i "], %[b" #i "], %[rs], %[q" #i "] op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
#define ATOM_CMAX(i) "v_pk_max_f16 %[t" #i "], %[t" #i "], %[lo]\n\t"
#define ATOM_CMIN(i) "v_pk_min_f16 %[t" #i "], %[t" #i "], %[hi]\n\t"
#define ATOM_CADD(i) "v_pk_add_f16 %[t" #i "], %[t" #i "], %[mg]\n\t"
#define ATOM_X4(M) M(0) M(1) M(2) M(3)
// four pairs: t = half pairs (1536 + code).  s2 = the scale (half) in the low 16 bits; lo2 / hi2 = the clamp bounds in both halves
__device__ __forceinline__ void sim_codes4(unsigned z0, unsigned z1, unsigned z2, unsigned z3, float rs, unsigned s2, unsigned lo2,
                                           unsigned hi2, unsigned &t0, unsigned &t1, unsigned &t2, unsigned &t3) {
  unsigned q0, q1, q2, q3;
  float a0, a1, a2, a3, b0, b1, b2, b3;
  const unsigned mg2 = 0x66006600u;                                    // (1536, 1536)
  asm(ATOM_X4(ATOM_Q0LO) ATOM_X4(ATOM_Q0HI) ATOM_X4(ATOM_ELO) ATOM_X4(ATOM_EHI) ATOM_X4(ATOM_Q1LO) ATOM_X4(ATOM_Q1HI)
      ATOM_X4(ATOM_CMAX) ATOM_X4(ATOM_CMIN) ATOM_X4(ATOM_CADD)
      : [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3), [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3),
        [b0] "=&v"(b0), [b1] "=&v"(b1), [b2] "=&v"(b2), [b3] "=&v"(b3), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
      : [z0] "v"(z0), [z1] "v"(z1), [z2] "v"(z2), [z3] "v"(z3), [rs] "v"(rs), [s] "v"(s2), [lo] "v"(lo2), [hi] "v"(hi2), [mg] "v"(mg2));
}
#undef ATOM_Q0LO
#undef ATOM_Q0HI
#undef ATOM_ELO
#undef ATOM_EHI
#undef ATOM_Q1LO
#undef ATOM_Q1HI
#undef ATOM_CMAX
#undef ATOM_CMIN
#undef ATOM_CADD

// max |.| over the 16 halves of 8 pairs, as a float (two interleaved v_max3_f16 chains: |.| is a free source modifier there)
__device__ __forceinline__ float amax16_h(const unsigned (&z)[8]) {
  unsigned ma, mb;
  float r;
  asm("v_max3_f16 %[ma], |%[z0]|, |%[z0]|, |%[z1]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[mb], |%[z4]|, |%[z4]|, |%[z5]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[ma], %[ma], |%[z1]|, |%[z2]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[mb], %[mb], |%[z5]|, |%[z6]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[ma], %[ma], |%[z2]|, |%[z3]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[mb], %[mb], |%[z6]|, |%[z7]| op_sel:[0,1,0,0]\n\t"
      "v_max3_f16 %[ma], %[ma], |%[z3]|, |%[z7]| op_sel:[0,1,1,0]\n\t"
      "s_nop 0\n\t"
      "v_max_f16 %[ma], %[ma], %[mb]\n\t"
      "s_nop 0\n\t"
      "v_cvt_f32_f16 %[r], %[ma]\n\t"
      : [ma] "=&v"(ma), [mb] "=&v"(mb), [r] "=v"(r)
      : [z0] "v"(z[0]), [z1] "v"(z[1]), [z2] "v"(z[2]), [z3] "v"(z[3]), [z4] "v"(z[4]), [z5] "v"(z[5]), [z6] "v"(z[6]), [z7] "v"(z[7]));
  return r;
}

// max over the aligned 8 lanes, one v_max_f32 with a DPP operand per stage (fmaxf() around a DPP move costs a move and a
// canonicalising max more per stage); a DPP read of a just-written register needs two wait states
__device__ __forceinline__ float max8_dpp(float a) {
  asm("s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      : "+v"(a));
  return a;
}

// y = half(float(x) * rinv) for four pairs: pair i takes the low (HI = 0) or high (HI = 1) halves of xl[i] and xh[i].  Two roundings,
// as in rmsnorm_value<true>: opaque() keeps the compiler from fusing the FP32 product and the conversion.
template <int HI>
__device__ __forceinline__ unsigned sim_scale1(unsigned xl, unsigned xh, float rinv) {
  const h2v a = __builtin_bit_cast(h2v, xl), b = __builtin_bit_cast(h2v, xh);
  const float pa = opaque((float)(HI ? a.y : a.x) * rinv), pb = opaque((float)(HI ? b.y : b.x) * rinv);
  const h2v y = {(_Float16)pa, (_Float16)pb};
  return __builtin_bit_cast(unsigned, y);
}
template <int HI0, int HI1, int HI2, int HI3>
__device__ __forceinline__ void sim_scale4(unsigned xl0, unsigned xl1, unsigned xl2, unsigned xl3, unsigned xh0, unsigned xh1,
                                           unsigned xh2, unsigned xh3, float rinv, unsigned &y0, unsigned &y1, unsigned &y2,
                                           unsigned &y3) {
  y0 = sim_scale1<HI0>(xl0, xh0, rinv);
  y1 = sim_scale1<HI1>(xl1, xh1, rinv);
  y2 = sim_scale1<HI2>(xl2, xh2, rinv);
  y3 = sim_scale1<HI3>(xl3, xh3, rinv);
}

// silu(a) * b for fp16 inputs given as floats.  Activate.cuh:28  x / (1 + expf(-x)) with the hardware exp2 / rcp (1 ulp each):
// 5 instructions instead of ~20; expf differs by ulps between libraries anyway (the parity tests allow codes +-1 on < 0.2 %)
__device__ __forceinline__ float silu_f32(float a) {
  const float e = __builtin_amdgcn_exp2f(a * -1.4426950408889634f);
  return a * __builtin_amdgcn_rcpf(1.0f + e);
}
template <bool SIM>
__device__ __forceinline__ float silu_mul(float a, float b) {
  const float s = silu_f32(a);
  if constexpr (SIM) return round_h(round_h(s) * b);        // act_fn(gate) * up, both in half
  else return s * b;                                        // kept in FP32 (Activate.cuh:103-106)
}

}  // namespace atom
