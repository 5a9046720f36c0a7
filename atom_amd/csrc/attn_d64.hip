// Head size 64 in the INT4 paged-KV attention path on gfx950 (Llama-3.2-1B, TinyLlama, SmolLM2: 64-wide heads): the fp16 per-head
// quantiser, the append, and causal grouped-query attention (prefill, chunked prefill and decode are one kernel) with RoPE fused.
//
// Cache layout (utils.KvPoolInt4 with head_dim 64): kv_data u8 [pages, L, 2, N, P, 32], kv_param f16 [pages, L, 2, N, P, 2]; dim d of
// a head vector in byte d / 2, low nibble first; value = nibble * scale - zero with the (scale, zero) of quant_head_u4 taken over the
// 64 values.  RoPE pairs are (i, i + 32), frequency theta^(-2 i / 64) / rope_scale; the logits are scaled by attn_scale / sqrt(64).
//
//   atom_kv_quant_u4_f16_d64      16 lanes x 4 values per vector, four vectors per wave
//   atom_kv_append_i4_d64         one workgroup per token: 32 bytes + one (scale, zero) word per (K|V, head)
//   atom_batch_prefill_gqa_i4_d64 / atom_batch_decode_gqa_i4_d64 (the _rope arguments; rope_table float32 [32])
//
// The attention kernel is built for 64, not the 128 kernel with half its loops.  The 128 kernel is bound by staging between two
// barriers with the matrix pipe idle: 256 threads de-quantise and rotate a 64-key tile, wait, and 4 waves multiply.  At
// head 64 a key is half the bytes, so the same 32 KiB of LDS and the same per-thread staging work (16 RoPE pairs of K, 32 values of V,
// one (scale, zero) word each) cover a tile of 128 KEYS: half the barriers per key, and twice the MFMA work between a barrier pair.
//
// Geometry: one workgroup of 4 waves per (query block of 64 rows, sequence, K/V head, KV split); wave w owns rows 16 w .. 16 w + 15.
// A row is query r / G of query head h G + r % G (G = 1: MHA).  Staging thread = (key kk = tid >> 1, half u = tid & 1): K as two
// 8-byte loads, dims [16u, 16u + 16) and [32 + 16u, 32 + 16u + 16) -- the two halves of its 16 RoPE pairs, one sin / cos each -- and
// V as one 16-byte load, dims [32u, 32u + 32).  A wave's loads cover 32 keys x 32 bytes: 1 KiB contiguous within a page.
// LDS images [128 keys][64 dims] f16 for K and for V: 128-byte rows, 8 chunks of 16 bytes.  Two rows share the 256 bytes of one pass
// over the 64 banks, so the XOR swizzles of the 256-byte-row kernel would put keys k and k + 2 on the same banks here; re-derived:
//   K  chunk ^ fk(key), fk = key bits (1, 3, 2) -> bits (0, 1, 2).  Reads (ds_read_b128, 16 keys x one chunk): fk is a bijection of
//      (key >> 1) & 7, and the key's parity picks the 128-byte half: 16 distinct 16-byte slots.  Writes (8 keys x chunks {c, c ^ 2}):
//      bits (0, 2) of fk separate the 4 keys of a parity, bit 1 is free for the half u.
//   V  chunk ^ fv(key), fv = key bit 1 -> bit 1, key bit 2 -> bits 0 and 2.  Reads (ds_read_b64_tr_b16: 8 keys x chunks {c, c ^ 1}):
//      bits (1, 2) separate the 4 keys of a parity.  Writes (8 keys x chunks {c, c ^ 4}): bits (0, 1) do.
// Products per wave on v_mfma_f32_16x16x32_f16, FP32 accumulation:
//   S^T[key][q] = K . Q^T   2 k-steps per 16-key tile, 8 tiles: 16 MFMAs; A from LDS, B = the rotated q in registers (2 x 8 halves).
//   O^T[d][q]  = V^T . P^T  4 dim tiles x 4 k-steps: 16 MFMAs; B = P straight from the S accumulator (k-step s takes key tiles 2s,
//                           2s + 1 in the order the registers hold them), A = V read column-wise in the same key order.
// 16 accumulator registers for O (32 at head 128), 32 for S.  Softmax: online, FP32, base 2, one maximum reduction per 128 keys.
// Carried over from the 128 kernel: keys past a sequence's end are never loaded and staged as exact zeros; a fully masked row stays
// NaN-free (m_use); the cache is read-only; no host synchronisation (capturable).
//
// KV splits write partial states float [rows][heads][splits][66] (64 un-normalised values, the running maximum in base 2, the
// denominator), merged by the 64-thread form of decode_merge_kernel below: the same operations in the same order.
// Host side: d64_plan() decides rows, query blocks and splits for the plan queries and for launch_d64().
#include <math.h>

#include <algorithm>
#include <type_traits>
#include "common.h"
#include "kv_attn.h"
#include "rope_math.h"

namespace atom {

constexpr int kD64 = 64;          // the head size of this file
constexpr int kD64Rows = 64;      // query rows per workgroup (4 waves x 16)
constexpr int kD64Keys = 128;     // keys per tile
constexpr int kD64Threads = 256;
constexpr int kD64State = kD64 + 2;

typedef _Float16 d64_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 d64_h4 __attribute__((ext_vector_type(4)));
typedef short d64_s4 __attribute__((ext_vector_type(4)));
typedef float d64_f2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ quantiser and append
// quant_head_u4 (kv_attn.h) on a 64-value vector held by 16 lanes: the same arithmetic, the extrema over 16 lanes
__device__ __forceinline__ unsigned short quant_head64_u4(const v4f &x, unsigned &sz) {
  float lo = fminf(fminf(x[0], x[1]), fminf(x[2], x[3])), hi = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
#pragma unroll
  for (int k = 8; k >= 1; k >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, k));
    hi = fmaxf(hi, __shfl_xor(hi, k));
  }
  const float scale = (hi - lo) / 15.f, zero = -lo, rs = 1.0f / scale;
  unsigned w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) w |= o4_code<false>(x[k], zero, rs, scale) << (4 * k);
  sz = (unsigned)__builtin_bit_cast(unsigned short, f2h(scale)) | ((unsigned)__builtin_bit_cast(unsigned short, f2h(zero)) << 16);
  return (unsigned short)w;
}

__global__ __launch_bounds__(256) void kv_quant_u4_f16_d64_kernel(const half_t *k, uint8_t *packed, half_t *param, int64_t vecs) {
  const int l = threadIdx.x & 15;
  const int64_t vec = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (vec >= vecs) return;
  const d64_h4 h = *reinterpret_cast<const d64_h4 *>(k + vec * kD64 + 4 * l);
  const v4f x = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  unsigned sz;
  const unsigned short w = quant_head64_u4(x, sz);
  *reinterpret_cast<unsigned short *>(packed + vec * (kD64 / 2) + 2 * l) = w;
  if (l == 0) *reinterpret_cast<unsigned *>(param + vec * 2) = sz;
}

struct AppendD64Params {
  KvParams kv;
  const uint8_t *k, *v;
  const half_t *k_param, *v_param;
  const int32_t *append_indptr;   // NULL: one token per sequence
};

// kv_append_kernel (kv_i4.hip) for 32-byte head vectors: every token is one workgroup, 16-byte chunks per thread
__global__ __launch_bounds__(128) void kv_append_d64_kernel(AppendD64Params p) {
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x;
  int b, j, n;
  if (p.append_indptr) {
    int lo = 0, hi = p.kv.batch;                       // largest b with append_indptr[b] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.append_indptr[mid] <= t) lo = mid; else hi = mid;
    }
    b = lo;
    j = (int)(t - p.append_indptr[b]);
    n = p.append_indptr[b + 1] - p.append_indptr[b];
  } else {
    b = (int)t; j = 0; n = 1;
  }
  const int P = p.kv.P, N = p.kv.N;
  const int npages = p.kv.indptr[b + 1] - p.kv.indptr[b];
  const int seq_len = (npages - 1) * P + p.kv.last_page_offset[b];
  const int pos = seq_len - n + j;
  if (pos < 0 || pos / P >= npages) return;
  const int64_t page = p.kv.indices[p.kv.indptr[b] + pos / P];
  const int e = pos % P;
  const int64_t base = (page * p.kv.L + p.kv.layer) * 2;             // [.., 2, N, P, ..]
  for (int i = tid; i < 2 * N * 2; i += 128) {                       // (k|v, head, 16-byte chunk)
    const int kv = i / (N * 2), h = (i >> 1) % N, ch = i & 1;
    const uint8_t *src = (kv ? p.v : p.k) + ((int64_t)t * N + h) * 32 + ch * 16;
    uint8_t *dst = p.kv.data + (((base + kv) * N + h) * P + e) * 32 + ch * 16;
    *reinterpret_cast<v4u *>(dst) = *reinterpret_cast<const v4u *>(src);
  }
  for (int i = tid; i < 2 * N; i += 128) {                           // (scale, zero) half2 per (k|v, head)
    const int kv = i / N, h = i % N;
    const unsigned *src = reinterpret_cast<const unsigned *>((kv ? p.v_param : p.k_param) + ((int64_t)t * N + h) * 2);
    unsigned *dst = reinterpret_cast<unsigned *>(p.kv.param + (((base + kv) * N + h) * P + e) * 2);
    *dst = *src;
  }
}

// ------------------------------------------------------------------------------------------------ attention
struct AttnD64Params {
  const uint8_t *data;
  const half_t *param;
  const int32_t *kv_indptr, *kv_indices, *last_page_offset, *qo_indptr;   // qo_indptr NULL: one query per sequence (decode)
  const half_t *q;   // [T, Nq, 64]
  half_t *o;         // [T, Nq, 64] (splits == 1)
  float *ws;         // splits > 1: [T, Nq, splits, 66]
  int batch, L, layer, N, P;   // N: K/V heads
  int nqb;           // query blocks per (sequence, K/V head)
  int splits;
  float qk_scale, log2_theta, rope_inv_scale;
  int G, Nq;
  const float *rope_table;   // kTable: float[32], revolutions per position of pair i
};

__device__ __forceinline__ void d64_sincos_rev(float rev, float &s, float &c) {
  const float fr = rev - floorf(rev);
  s = __builtin_amdgcn_sinf(fr);
  c = __builtin_amdgcn_cosf(fr);
}

struct D64TileRegs {  // one thread's share of a 128-key tile, as loaded
  v2u k1, k2;         // K dims [16u, 16u + 16) and [32 + 16u, 32 + 16u + 16)
  v4u v;              // V dims [32u, 32u + 32)
  unsigned kq, vq;    // (scale, zero) half2 of the key
};

// byte offsets into the LDS images: 128-byte rows, chunk = 8 dims (16 bytes); the swizzles are derived in the file's head
__device__ __forceinline__ int d64_k_off(int key, int ch) {
  const int f = ((key >> 1) & 1) | (((key >> 3) & 1) << 1) | (((key >> 2) & 1) << 2);
  return key * 128 + 16 * (ch ^ f);
}
__device__ __forceinline__ int d64_v_off(int key, int ch) {
  const int f = (((key >> 1) & 1) << 1) | (((key >> 2) & 1) * 5);
  return key * 128 + 16 * (ch ^ f);
}

// kTable (a rope_table is given): the frequency of pair i is p.rope_table[i] as loaded; the query's angle is formed exactly
// (rope_math.h), a key's from position kRopeExactFrom on, chosen per key tile (workgroup-uniform).
template <bool kTable>
__global__ __launch_bounds__(kD64Threads) void attn_d64_kernel(AttnD64Params p) {
  __shared__ __attribute__((aligned(16))) half_t Ks[kD64Keys * kD64];
  __shared__ __attribute__((aligned(16))) half_t Vs[kD64Keys * kD64];
  __shared__ float rope_fr[32];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, P = p.P, G = p.G, Nq = p.Nq;
  // heavy-first order: the last query blocks (the most key tiles) get the lowest workgroup ids
  const int per_qb = p.batch * N * p.splits;
  const int idx = blockIdx.x;
  const int qb = p.nqb - 1 - idx / per_qb;
  const int rem = idx - (idx / per_qb) * per_qb;
  const int bh = rem / p.splits, sp = rem - bh * p.splits;
  const int b = bh / N, h = bh - b * N;

  const bool one_q = !p.qo_indptr;
  const int qbeg = one_q ? b : p.qo_indptr[b], q_b = one_q ? 1 : p.qo_indptr[b + 1] - qbeg;
  const int nrows = q_b * G;
  const int q0 = qb * kD64Rows;
  if (q0 >= nrows) return;                                // (uniform over the workgroup: before any barrier)
  const int pg0 = p.kv_indptr[b];
  const int len = (p.kv_indptr[b + 1] - pg0 - 1) * P + p.last_page_offset[b];
  const int prefix = len - q_b;                           // position of query 0
  const int kend = prefix + (min(q0 + kD64Rows, nrows) + G - 1) / G;   // keys this block sees: 0 .. kend-1
  const int ntiles = kend > 0 ? (kend + kD64Keys - 1) / kD64Keys : 0;
  const int chunk = (ntiles + p.splits - 1) / p.splits;
  const int t0 = sp * chunk, t1 = min(ntiles, t0 + chunk);

  if (tid < 32) {                                         // revolutions per position of pair (tid, tid + 32)
    if constexpr (kTable)
      rope_fr[tid] = p.rope_table[tid];
    else
      rope_fr[tid] = p.rope_inv_scale * 0.15915494309189535f * __builtin_amdgcn_exp2f(-p.log2_theta * (float)(2 * tid) * (1.0f / kD64));
  }
  __syncthreads();

  // ---- my query row: lane (li, g) = (row 16 w + li of the block, k-group); B operand of S^T: q[row][32 ks + 8 g .. + 7], ks = 0, 1:
  // the two halves of the RoPE pairs (i, i + 32) with i = 8 g + j
  const int li = lane & 15, g = lane >> 4;
  const int ri = q0 + 16 * w + li;
  const bool row_ok = ri < nrows;
  const int qi = ri / G, hq = h * G + (ri - qi * G);
  const int pos = prefix + qi;
  const bool wave_live = q0 + 16 * w < nrows;             // (wave-uniform)
  const int pmin_w = prefix + (q0 + 16 * w) / G, pmax_w = prefix + (q0 + 16 * w + 15) / G;
  d64_h8 qf[2];
  {
    v4u raw[2];
    const half_t *qp = p.q + ((int64_t)(qbeg + (row_ok ? qi : 0)) * Nq + hq) * kD64 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) raw[ks] = row_ok ? *reinterpret_cast<const v4u *>(qp + 32 * ks) : v4u{0u, 0u, 0u, 0u};
    const d64_h8 *x = reinterpret_cast<const d64_h8 *>(raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s, c;
      if constexpr (kTable)
        rope_sincos_exact((float)pos, rope_fr[8 * g + j], s, c);
      else
        d64_sincos_rev((float)pos * rope_fr[8 * g + j], s, c);
      const float x1 = (float)x[0][j], x2 = (float)x[1][j];
      qf[0][j] = (half_t)(x1 * c - x2 * s);
      qf[1][j] = (half_t)(x2 * c + x1 * s);
    }
  }

  // ---- staging: thread (key kk, half u)
  const int kk = tid >> 1, u = tid & 1;
  const int64_t blk = (int64_t)N * P;                     // tokens x heads of one (page, layer, K|V) block
  const uint8_t *kbase = p.data + ((int64_t)p.layer * 2 * N + h) * P * 32;
  const half_t *qpbase = p.param + ((int64_t)p.layer * 2 * N + h) * P * 2;
  const int64_t page_bytes = (int64_t)p.L * 2 * blk * 32, page_halves = (int64_t)p.L * 2 * blk * 2;
  auto load = [&](int tile) -> D64TileRegs {
    D64TileRegs r;
    const int j = tile * kD64Keys + kk;
    if (j < len) {                                        // (j < len: page j / P is one of the sequence's)
      const int pg = j / P, e = j - pg * P;
      const int64_t page = p.kv_indices[pg0 + pg];
      const uint8_t *kp = kbase + page * page_bytes + e * 32;
      const half_t *pp = qpbase + page * page_halves + e * 2;
      r.k1 = *reinterpret_cast<const v2u *>(kp + 8 * u);
      r.k2 = *reinterpret_cast<const v2u *>(kp + 16 + 8 * u);
      r.v = *reinterpret_cast<const v4u *>(kp + blk * 32 + 16 * u);
      r.kq = *reinterpret_cast<const unsigned *>(pp);
      r.vq = *reinterpret_cast<const unsigned *>(pp + blk * 2);
    } else {
      r.k1 = v2u{0u, 0u};
      r.k2 = v2u{0u, 0u};
      r.v = v4u{0u, 0u, 0u, 0u};
      r.kq = r.vq = 0u;
    }
    return r;
  };
  auto stage = [&](int tile, const D64TileRegs &r, auto exact) {
    const int j = tile * kD64Keys + kk;
    const bool ok = j < len;                              // past the end: zeros (the loaded registers are zeros too, see load)
    const float ks = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.kq & 0xFFFF)) : 0.f;
    const float kz = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.kq >> 16)) : 0.f;
    const float vs = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.vq & 0xFFFF)) : 0.f;
    const float vz = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.vq >> 16)) : 0.f;
    // K: pair m = dims (16u + m, 32 + 16u + m); word hw of k1 / k2 holds m = 8 hw .. 8 hw + 7, nibble e at bits 4e
    d64_h8 klo[2], khi[2];
#pragma unroll
    for (int hw = 0; hw < 2; ++hw)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = 8 * hw + e;
        const float x1 = __builtin_fmaf((float)((r.k1[hw] >> (4 * e)) & 0xF), ks, -kz);
        const float x2 = __builtin_fmaf((float)((r.k2[hw] >> (4 * e)) & 0xF), ks, -kz);
        float s, c;
        if constexpr (decltype(exact)::value)
          rope_sincos_exact((float)j, rope_fr[16 * u + m], s, c);
        else
          d64_sincos_rev((float)j * rope_fr[16 * u + m], s, c);
        klo[hw][e] = (half_t)(x1 * c - x2 * s);
        khi[hw][e] = (half_t)(x2 * c + x1 * s);
      }
    char *kl = reinterpret_cast<char *>(Ks);
    *reinterpret_cast<d64_h8 *>(kl + d64_k_off(kk, 2 * u)) = klo[0];
    *reinterpret_cast<d64_h8 *>(kl + d64_k_off(kk, 2 * u + 1)) = klo[1];
    *reinterpret_cast<d64_h8 *>(kl + d64_k_off(kk, 4 + 2 * u)) = khi[0];
    *reinterpret_cast<d64_h8 *>(kl + d64_k_off(kk, 4 + 2 * u + 1)) = khi[1];
    // V: word vw holds dims 32u + 8 vw .. + 7
    char *vl = reinterpret_cast<char *>(Vs);
#pragma unroll
    for (int vw = 0; vw < 4; ++vw) {
      d64_h8 vv;
#pragma unroll
      for (int e = 0; e < 8; ++e) vv[e] = (half_t)__builtin_fmaf((float)((r.v[vw] >> (4 * e)) & 0xF), vs, -vz);
      *reinterpret_cast<d64_h8 *>(vl + d64_v_off(kk, 4 * u + vw)) = vv;
    }
  };

  v4f O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) O[dt] = v4f{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;                   // row state (m reduced over the row's 4 lanes; l: this lane's keys only)

  D64TileRegs regs;
  if (t0 < t1) regs = load(t0);
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();                                      // the previous tile's LDS reads are done
    if constexpr (kTable) {
      if (tile * kD64Keys >= kRopeExactFrom)              // (workgroup-uniform)
        stage(tile, regs, std::true_type{});
      else
        stage(tile, regs, std::false_type{});
    } else {
      stage(tile, regs, std::false_type{});
    }
    __syncthreads();
    if (tile + 1 < t1) regs = load(tile + 1);             // in flight during this tile's products
    const int kt0 = tile * kD64Keys;
    if (!wave_live || kt0 > pmax_w) continue;             // (wave-uniform) no row of this wave sees a key of this tile
    // ---- S^T = K . Q^T; 16-key tiles wholly past the wave's last row are left out (their P is zero)
    const int nkt = min(8, (pmax_w - kt0) / 16 + 1);      // (wave-uniform) 1 .. 8
    v4f S[8];
    const char *kl = reinterpret_cast<const char *>(Ks);
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      S[kt] = v4f{0.f, 0.f, 0.f, 0.f};
      if (kt < nkt) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const d64_h8 a = *reinterpret_cast<const d64_h8 *>(kl + d64_k_off(16 * kt + li, 4 * ks + g));
          S[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], S[kt], 0, 0, 0);
        }
      }
    }
    // ---- online softmax; lane holds row li's scores of keys kt0 + 16 kt + 4 g + r
    const bool masked = kt0 + kD64Keys - 1 > pmin_w;      // (wave-uniform) some key of the tile is past some row's position
    float mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = S[kt][r] * p.qk_scale;
        if (masked && kt0 + 16 * kt + 4 * g + r > pos) s = -INFINITY;
        S[kt][r] = s;
        mt = fmaxf(mt, s);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m_run, mt);
    const float m_use = m_new == -INFINITY ? 0.f : m_new; // (a row with every key masked so far: exp2(-inf - 0) = 0, no NaN)
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    m_run = m_new;
    float ls = 0.f;
    d64_h8 pf[4];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __builtin_amdgcn_exp2f(S[kt][r] - m_use);
        ls += pr;
        pf[kt >> 1][4 * (kt & 1) + r] = (half_t)pr;
      }
    l_run = __builtin_fmaf(l_run, alpha, ls);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) O[dt] *= alpha;
    // ---- O^T += V^T . P^T; k-step s: element j of lane group g is key 32 s + 16 (j >> 2) + 4 g + (j & 3)
    const char *vl = reinterpret_cast<const char *>(Vs);
    const int tq = li >> 2, tp = li & 3;                  // transposed read: lane 4 tq + tp addresses row tq, dims 4 tp .. 4 tp + 3
    const int nks = (nkt + 1) >> 1;                       // (wave-uniform) k-steps with a key some row sees
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < nks) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          d64_h4 half2x[2];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const int row = 32 * s + 16 * hh + 4 * g + tq;
            const int off = d64_v_off(row, 2 * dt + (tp >> 1)) + 8 * (tp & 1);
            const d64_s4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) d64_s4 *)(const_cast<char *>(vl) + off));
            half2x[hh] = __builtin_bit_cast(d64_h4, t);
          }
          const d64_h8 a = {half2x[0][0], half2x[0][1], half2x[0][2], half2x[0][3], half2x[1][0], half2x[1][1], half2x[1][2], half2x[1][3]};
          O[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[s], O[dt], 0, 0, 0);
        }
      }
    }
  }

  // ---- the row's denominator over its 4 lanes; lane holds O[row][16 dt + 4 g + r]
  float l_all = l_run + __shfl_xor(l_run, 16);
  l_all += __shfl_xor(l_all, 32);
  if (!row_ok) return;
  const int64_t orow = (int64_t)(qbeg + qi) * Nq + hq;
  if (p.splits == 1) {
    const float rl = l_all > 0.f ? 1.0f / l_all : 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const d64_h4 hv = {(half_t)(O[dt][0] * rl), (half_t)(O[dt][1] * rl), (half_t)(O[dt][2] * rl), (half_t)(O[dt][3] * rl)};
      *reinterpret_cast<d64_h4 *>(p.o + orow * kD64 + 16 * dt + 4 * g) = hv;
    }
  } else {
    float *wp = p.ws + (orow * p.splits + sp) * kD64State;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *reinterpret_cast<d64_f2 *>(wp + 16 * dt + 4 * g) = d64_f2{O[dt][0], O[dt][1]};
      *reinterpret_cast<d64_f2 *>(wp + 16 * dt + 4 * g + 2) = d64_f2{O[dt][2], O[dt][3]};
    }
    if (g == 0) {
      wp[kD64] = m_run;
      wp[kD64 + 1] = l_all;
    }
  }
}

// decode_merge_kernel (kv_attn.h) on 66-float states, one thread per dim: out = sum_s o_s 2^(m_s - M) / sum_s d_s 2^(m_s - M), every
// split's (value, m, d) requested before the first is used, in batches of SB splits -- the same operations in the same order
template <int SB>
__global__ __launch_bounds__(64) void merge_d64_kernel(const float *ws, half_t *o, int splits) {
  const int64_t bh = blockIdx.x;
  const int dim = threadIdx.x;
  const float *wp = ws + bh * splits * kD64State;
  float M = -INFINITY;
  for (int s0 = 0; s0 < splits; s0 += SB) {
    float mv[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) mv[s] = wp[min(s0 + s, splits - 1) * kD64State + kD64];
#pragma unroll
    for (int s = 0; s < SB; ++s) M = fmaxf(M, mv[s]);        // (a clamped repeat of the last split changes no maximum)
  }
  float acc = 0.f, den = 0.f;
  for (int s0 = 0; s0 < splits; s0 += SB) {
    float ov[SB], mv[SB], dv[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const int sc = min(s0 + s, splits - 1);
      ov[s] = wp[sc * kD64State + dim];
      mv[s] = wp[sc * kD64State + kD64];
      dv[s] = wp[sc * kD64State + kD64 + 1];
    }
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s0 + s < splits) {
        const float w = mv[s] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mv[s] - M);
        acc = __builtin_fmaf(ov[s], w, acc);
        den = __builtin_fmaf(dv[s], w, den);
      }
  }
  o[bh * kD64 + dim] = (half_t)(den > 0.f ? acc / den : 0.f);
}

// ------------------------------------------------------------------------------------------------ host side
// check_kv (kv_attn.h) refuses every head size but 128; this file's entries take 64 and nothing else
static int check_kv_d64(const void *kv_data, const void *kv_param, const int32_t *indptr, const int32_t *indices, const int32_t *lpo,
                        int batch, int L, int layer, int N, int P, int D) {
  return check_kv(kv_data, kv_param, indptr, indices, lpo, batch, L, layer, N, P, D == kD64 ? kHeadDim : 0);
}

static int d64_group(int num_qo_heads, int num_kv_heads) {   // G, or 0 for a rejected pair of head counts
  if (num_kv_heads < 1 || num_qo_heads < 1 || num_qo_heads % num_kv_heads != 0) return 0;
  return num_qo_heads / num_kv_heads;
}

// The plan of a call: query rows of a (sequence, K/V head) at most, the query blocks they make, and the KV splits.  Decode (one query
// per sequence, every G): the grouped-query decode policy of prefill_i4.hip -- a unit is (sequence, K/V head), 512 resident
// workgroups, at least 2 key tiles per split -- on 128-key tiles.  Prefill: splits only where the query blocks leave the chip short of
// work (short chunks on long prefixes), ~2 workgroups per CU, at least 2 key tiles per split.
struct D64Plan {
  int rows, nqb, splits;
};
static D64Plan d64_plan(bool decode, int64_t total_q, int max_q_len, int batch, int G, int num_kv_heads, int P, int max_pages) {
  D64Plan pl;
  pl.rows = decode ? G : (int)std::min<int64_t>(std::min<int64_t>(max_q_len, total_q) * G, 0x7fffffff);
  pl.nqb = (int)(((int64_t)pl.rows + kD64Rows - 1) / kD64Rows);
  pl.splits = 1;
  if (max_pages <= 0) return pl;
  const int64_t tiles = ((int64_t)max_pages * P + kD64Keys - 1) / kD64Keys;
  if (decode) {
    const int64_t units = (int64_t)batch * num_kv_heads;
    const int64_t smax = std::max<int64_t>(std::min<int64_t>(tiles / 2, 32), 1);
    double best_cost = 1e30;
    for (int64_t s = 1; s <= smax; ++s) {
      const int64_t rounds = (units * s + 511) / 512;
      const double cost = (double)rounds * ((double)tiles / (double)s + 2.0) + 0.15 * (double)s;
      if (cost < best_cost - 1e-9) { best_cost = cost; pl.splits = (int)s; }
    }
  } else {
    const int64_t blocks = (int64_t)batch * num_kv_heads * pl.nqb;
    if (blocks >= 512 || tiles < 4) return pl;
    int64_t s = (512 + blocks - 1) / blocks;
    s = std::min<int64_t>(std::min<int64_t>(s, tiles / 2), 32);
    pl.splits = (int)std::max<int64_t>(s, 1);
  }
  return pl;
}

static size_t d64_state_bytes(int64_t rows_times_heads, int splits) {
  return (size_t)rows_times_heads * splits * kD64State * sizeof(float);
}

static size_t d64_workspace_bytes(bool decode, int64_t total_q, int max_q_len, int batch, int G, int num_kv_heads, int P, int max_pages) {
  if (G == 0 || total_q < 1 || batch < 1 || num_kv_heads < 1 || P < 16 || max_q_len < 1) return 0;
  const int s = d64_plan(decode, total_q, max_q_len, batch, G, num_kv_heads, P, max_pages).splits;
  return s > 1 ? d64_state_bytes(total_q * num_kv_heads * G, s) : 0;
}

// The one host path of attn_d64_kernel, in the order of launch_prefill's checks (prefill_i4.hip).  decode: one query per sequence (no
// qo_indptr, total_q = batch).  A workspace that cannot hold the partial states runs the call unsplit.
static int launch_d64(bool decode, void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                      const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset, int batch,
                      int num_layers, int layer_idx, int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta,
                      float rope_scale, const float *rope_table, float attn_scale, int max_pages, void *workspace, size_t workspace_bytes,
                      void *stream) {
  const int G = d64_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  const int st = check_kv_d64(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx, num_kv_heads,
                              page_size, head_dim);
  if (st != ATOM_OK) return st;
  if (!q || !o || !(rope_theta > 0.f) || !(rope_scale > 0.f) || (!decode && !qo_indptr)) return ATOM_ERR_INVALID_ARG;
  if (!decode && (total_q < 1 || total_q > 0x7fffffff || max_q_len < 1)) return ATOM_ERR_SHAPE;
  if (!aligned16(o) || !aligned16(q) || (reinterpret_cast<uintptr_t>(qo_indptr) & 3u)) return ATOM_ERR_ALIGN;
  D64Plan pl = d64_plan(decode, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages);
  const int64_t rows_heads = total_q * num_qo_heads;
  if (pl.splits > 1 && !(workspace && workspace_bytes >= d64_state_bytes(rows_heads, pl.splits) && aligned16(workspace))) pl.splits = 1;
  const int64_t grid = (int64_t)pl.nqb * batch * num_kv_heads * pl.splits;
  if (grid > 0x7fffffff || rows_heads > 0x7fffffff) return ATOM_ERR_SHAPE;
  if (const int rs = check_rope_table(rope_table, attn_scale)) return rs;
  AttnD64Params p;
  p.data = (const uint8_t *)kv_data, p.param = (const half_t *)kv_param;
  p.kv_indptr = kv_indptr, p.kv_indices = kv_indices, p.last_page_offset = last_page_offset, p.qo_indptr = qo_indptr;
  p.q = (const half_t *)q, p.o = (half_t *)o, p.ws = (float *)workspace;
  p.batch = batch, p.L = num_layers, p.layer = layer_idx, p.N = num_kv_heads, p.P = page_size;
  p.nqb = pl.nqb, p.splits = pl.splits;
  p.qk_scale = kLog2e / sqrtf((float)kD64) * attn_scale, p.log2_theta = log2f(rope_theta), p.rope_inv_scale = 1.0f / rope_scale;
  p.G = G, p.Nq = num_qo_heads;
  p.rope_table = rope_table;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (rope_table)
    hipLaunchKernelGGL(attn_d64_kernel<true>, dim3((unsigned)grid), dim3(kD64Threads), 0, s, p);
  else
    hipLaunchKernelGGL(attn_d64_kernel<false>, dim3((unsigned)grid), dim3(kD64Threads), 0, s, p);
  if (pl.splits > 1) {
    const dim3 mgrid((unsigned)rows_heads), mblock(64);
    if (pl.splits <= 8)
      hipLaunchKernelGGL(merge_d64_kernel<8>, mgrid, mblock, 0, s, (const float *)workspace, (half_t *)o, pl.splits);
    else if (pl.splits <= 16)
      hipLaunchKernelGGL(merge_d64_kernel<16>, mgrid, mblock, 0, s, (const float *)workspace, (half_t *)o, pl.splits);
    else
      hipLaunchKernelGGL(merge_d64_kernel<32>, mgrid, mblock, 0, s, (const float *)workspace, (half_t *)o, pl.splits);
  }
  return check_launch();
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_kv_quant_u4_f16_d64(const void *k, void *packed, void *param, int64_t T, int kv_heads, int head_dim, void *stream) {
  if (!k || !packed || !param) return ATOM_ERR_INVALID_ARG;
  if (T < 1 || kv_heads < 1 || head_dim != kD64 || T * kv_heads > 0x7fffffffll) return ATOM_ERR_SHAPE;
  if (!aligned16(k) || !aligned16(packed) || (reinterpret_cast<uintptr_t>(param) & 3u)) return ATOM_ERR_ALIGN;
  const int64_t vecs = T * kv_heads;
  hipLaunchKernelGGL(kv_quant_u4_f16_d64_kernel, dim3((unsigned)((vecs + 15) / 16)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const half_t *)k, (uint8_t *)packed, (half_t *)param, vecs);
  return check_launch();
}

int atom_kv_append_i4_d64(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                          const int32_t *last_page_offset, const void *k, const void *v, const void *k_param, const void *v_param,
                          const int32_t *append_indptr, int64_t total_tokens, int batch, int num_layers, int layer_idx, int num_heads,
                          int page_size, int head_dim, void *stream) {
  const int st = check_kv_d64(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx, num_heads,
                              page_size, head_dim);
  if (st != ATOM_OK) return st;
  if (!k || !v || !k_param || !v_param) return ATOM_ERR_INVALID_ARG;
  if (total_tokens < 1 || total_tokens > 0x7fffffff || (!append_indptr && total_tokens != batch)) return ATOM_ERR_SHAPE;
  if (!aligned16(k) || !aligned16(v) || (reinterpret_cast<uintptr_t>(k_param) & 3u) || (reinterpret_cast<uintptr_t>(v_param) & 3u) ||
      (reinterpret_cast<uintptr_t>(append_indptr) & 3u))
    return ATOM_ERR_ALIGN;
  AppendD64Params p{kv_params(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx, num_heads, page_size),
                    (const uint8_t *)k, (const uint8_t *)v, (const half_t *)k_param, (const half_t *)v_param, append_indptr};
  hipLaunchKernelGGL(kv_append_d64_kernel, dim3((unsigned)total_tokens), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), p);
  return check_launch();
}

size_t atom_batch_prefill_gqa_i4_d64_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                     int max_q_len, int max_pages_per_seq) {
  return d64_workspace_bytes(false, total_q, max_q_len, batch, d64_group(num_qo_heads, num_kv_heads), num_kv_heads, page_size,
                             max_pages_per_seq);
}

int atom_batch_prefill_gqa_i4_d64_splits(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_q_len,
                                         int max_pages_per_seq) {
  const int G = d64_group(num_qo_heads, num_kv_heads);
  if (G == 0 || total_q < 1 || batch < 1 || page_size < 16 || max_q_len < 1) return 0;
  return d64_plan(false, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages_per_seq).splits;
}

size_t atom_batch_decode_gqa_i4_d64_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq) {
  return d64_workspace_bytes(true, batch, 1, batch, d64_group(num_qo_heads, num_kv_heads), num_kv_heads, page_size, max_pages_per_seq);
}

int atom_batch_decode_gqa_i4_d64_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq) {
  const int G = d64_group(num_qo_heads, num_kv_heads);
  if (G == 0 || batch < 1 || page_size < 16) return 0;
  return d64_plan(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq).splits;
}

int atom_batch_prefill_gqa_i4_d64(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                  const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                  const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                  int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  return launch_d64(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                    num_layers, layer_idx, num_qo_heads, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale,
                    max_pages_per_seq, workspace, workspace_bytes, stream);
}

int atom_batch_decode_gqa_i4_d64(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                 const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                 int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                 const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  return launch_d64(true, o, q, nullptr, batch, 1, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers,
                    layer_idx, num_qo_heads, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale,
                    max_pages_per_seq, workspace, workspace_bytes, stream);
}

}  // extern "C"
