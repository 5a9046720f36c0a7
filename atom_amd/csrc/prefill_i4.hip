// Prefill / chunked-prefill attention over the INT4 paged KV cache on gfx950: causal multi-query attention with RoPE fused.
//
//   atom_batch_prefill_i4   o[row, h] = softmax_{j <= p}( <RoPE(q[row, h], p), RoPE(deq K[b, h, j], j)> / sqrt(128) ) . deq V[b, h, j]
//
// Sequence b holds len_b tokens in the cache (layout of kv_i4.hip); its queries are rows qo_indptr[b] .. qo_indptr[b+1] and sit at its
// LAST q_b positions: query i at p = len_b - q_b + i.  So a prompt from an empty cache, a chunk on a cached prefix and a multi-token
// verification step are one operation; with q_b = 1 it is what atom_batch_decode_i4 computes.  (The reference never bound an INT4
// prefill: its prefill attends to random K/V, punica/models/llama.py:164-167.)
//
// Geometry: one workgroup of 4 waves per (query block of 64 rows, sequence, head, KV split); wave w owns rows 16 w .. 16 w + 15 of the
// block.  The query blocks farthest from the diagonal (most key tiles) are dispatched first.  Per 64-key tile the 256 threads read the
// tile's INT4 K / V (thread = (key, quarter): K as the two 8-byte halves of its 16 RoPE pairs, V as 16 bytes -- the decode kernel's
// load), de-quantise to FP32 (nibble * scale - zero), rotate K at each key's own position, round to f16 and stage both in LDS; keys
// past the sequence end (uninitialised memory, possibly NaN / Inf) are staged as zeros and never loaded.  K is de-quantised again in
// every query block of its (sequence, head): VALU work in place of a second pass through HBM for an f16 copy of the whole cache.
//
// Products, per wave, on v_mfma_f32_16x16x32_f16 with FP32 accumulation:
//   S^T[key][q] = K . Q^T   A = K rows from LDS (ds_read_b128, 16-byte chunks XOR-swizzled by key), B = the rotated q in registers.
//                           The accumulator puts a query row on the lane (lane & 15) and 4 keys in the registers: the softmax state
//                           (running maximum, denominator) of a row lives in the 4 lanes that share lane & 15.
//   O^T[d][q]  = V^T . P^T  B = P straight from the S accumulator (keys 16kt + 4g + r in the order the registers hold them, k-step s
//                           takes tiles 2s, 2s+1), A = the V rows of the SAME key order, read column-wise from the row-major V image
//                           with ds_read_b64_tr_b16 (T10; chunks XOR-swizzled by (key & 7) << 1 so a half-wave's two 4-row blocks
//                           hit distinct banks).  O^T has the row on the lane too: rescaling by the row's factor is lane-local.
// Softmax: online, FP32, base 2 (scores scaled by log2(e) / sqrt(128)); the maximum is reduced over the 4 lanes of a row per tile, the
// denominator once at the end.  Causal mask: tiles past a wave's last row are skipped, the select (-inf score) runs only on tiles that
// cross a wave's first row; masking is a select before the exponent, and masked / zeroed entries enter the MFMAs as exact zeros.
//
// Numerics: q, rotated K, P and V are rounded to f16 as MFMA operands -- the only departure from the FP32 decode op (no bf16: its
// 8x larger rounding would need another bound).  RoPE angles in revolutions through v_sin / v_cos, as the decode kernel.
//
// Short chunks on long prefixes (few query blocks, many key tiles): the KV range of a block is split over `splits` workgroups that
// write the decode op's partial states float [rows][heads][splits][130] to the workspace, merged by decode_merge_kernel (kv_attn.h)
// with the query rows as its "batch".
//
// Host side: the three entry points (prefill, grouped-query prefill, grouped-query decode) are one kernel and one host path:
// prefill_plan() decides rows, query blocks and splits for the workspace queries and for launch_prefill(), which checks the arguments,
// fills PrefillParams by name, launches and merges (launch_merge, kv_attn.h).
#include <math.h>

#include <algorithm>
#include <type_traits>
#include "common.h"
#include "kv_attn.h"
#include "rope_math.h"

namespace atom {

constexpr int kPfRows = 64;    // query rows per workgroup (4 waves x 16)
constexpr int kPfKeys = 64;    // keys per tile
constexpr int kPfThreads = 256;

typedef _Float16 pf_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 pf_h4 __attribute__((ext_vector_type(4)));
typedef short pf_s4 __attribute__((ext_vector_type(4)));
typedef float pf_f2 __attribute__((ext_vector_type(2)));

struct PrefillParams {
  const uint8_t *data;
  const half_t *param;
  const int32_t *kv_indptr, *kv_indices, *last_page_offset, *qo_indptr;
  const half_t *q;   // [T, Nq, 128]
  half_t *o;         // [T, Nq, 128] (splits == 1)
  float *ws;         // splits > 1: [T, Nq, splits, 130]
  int batch, L, layer, N, P;   // N: heads of the cache (K/V heads)
  int nqb;           // query blocks per (sequence, K/V head): ceil(max_q_len * G / 64)
  int splits;
  float qk_scale, log2_theta, rope_inv_scale;
  int G, Nq;         // GQA kernel only: query heads per K/V head, query heads (N * G); qo_indptr NULL = one query per sequence
  const float *rope_table;   // kTable kernels only: float[64], revolutions per position of pair i (the _rope entry points)
  int window;        // kWindow kernels only: W >= 1, the query at position p sees keys p - W < j <= p (the _win entry points)
  const int32_t *kv_start;   // kStart kernels only: int32 [batch], the position of each page list's first token (the _ring entry points)
};

// sin / cos of 2*pi*rev (v_sin_f32 / v_cos_f32 take revolutions)
__device__ __forceinline__ void pf_sincos_rev(float rev, float &s, float &c) {
  const float fr = rev - floorf(rev);
  s = __builtin_amdgcn_sinf(fr);
  c = __builtin_amdgcn_cosf(fr);
}

struct PfTileRegs {   // one thread's share of a 64-key tile, as loaded: K dims [16u, 16u+16) and [64+16u, 64+16u+16), V dims [32u, 32u+32)
  v2u k1, k2;
  v4u v;
  unsigned kq, vq;    // (scale, zero) half2 of the key
};

// LDS images [64 keys][128 dims] f16, 256-byte rows; chunk = 8 dims (16 bytes)
__device__ __forceinline__ int k_off(int key, int ch) { return key * 256 + 16 * (ch ^ (key & 15)); }
__device__ __forceinline__ int v_off(int key, int ch) { return key * 256 + 16 * (ch ^ ((key & 7) << 1)); }

// GQA: a block's rows are (query, head of the group) pairs, query-major -- row r of (sequence b, K/V head h) is query r / G of query head
// h G + r % G -- so every staged tile serves the whole group.  The MHA instantiation is the kernel with G = 1 (the same code).
// kTable (the _rope entry points): the frequency of pair i is p.rope_table[i] as loaded; log2_theta / rope_inv_scale are not read.  The
// query's angle is formed exactly (rope_math.h), and so is a key's from position kRopeExactFrom on: the staging is VALU-bound, so the
// choice is made per key tile (workgroup-uniform) and is a template argument of the staging code.
// kWindow (the _win entry points): sliding window W = p.window, the row at position p sees keys p - W < j <= p, the bound taken from
// each row's own position.  The block's tiles start at the tile of its first row's lowest key and the KV splits divide that range (a
// split that comes out empty writes the empty state m = -inf, l = 0, zeros, which decode_merge_kernel takes); a wave skips the tiles
// wholly below its lowest row's bound, and the lower select runs only on tiles that cross some row's bound -- the causal mask's
// scheme, mirrored.  A row whose keys so far are all masked stays NaN-free through m_use.
// kStart (the _ring entry points; only with kGqa and kWindow): the page list of sequence b starts at position start = p.kv_start[b], a
// multiple of P (kv_step.hip, the ring step), not at 0: len = start + the list's tokens, and load() finds key j in page (j - start) / P
// of the list.  Everything else stays in ABSOLUTE positions -- prefix, pos, kend, the tile grid tile * 64, both masks, a key's RoPE
// angle -- so with equal contents and splits the call does what the _win call does on a cache that still lists pages 0 .. : the same
// operations in the same order.  Keys below `start` are not loaded and staged as zeros (as those past the end); the ring step keeps
// start <= p - W + 1 for every live row, so the lower select masks them.  tlo is clamped to start / 64: a caller that breaks the
// guarantee gets a finite, unspecified result and never a read outside the listed pages.
template <bool kGqa, bool kTable = false, bool kWindow = false, bool kStart = false>
__global__ __launch_bounds__(kPfThreads) void batch_prefill_kernel(PrefillParams p) {
  static_assert(!kStart || (kGqa && kWindow), "a list that starts behind position 0 is read only under a window");
  __shared__ __attribute__((aligned(16))) half_t Ks[kPfKeys * kHeadDim];
  __shared__ __attribute__((aligned(16))) half_t Vs[kPfKeys * kHeadDim];
  __shared__ float rope_fr[64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, P = p.P;
  const int G = kGqa ? p.G : 1, Nq = kGqa ? p.Nq : N;
  // heavy-first order: the last query blocks (the most key tiles) get the lowest workgroup ids
  const int per_qb = p.batch * N * p.splits;
  const int idx = blockIdx.x;
  const int qb = p.nqb - 1 - idx / per_qb;
  const int rem = idx - (idx / per_qb) * per_qb;
  const int bh = rem / p.splits, sp = rem - bh * p.splits;
  const int b = bh / N, h = bh - b * N;

  const bool one_q = kGqa && !p.qo_indptr;               // (the GQA decode entry point)
  const int qbeg = one_q ? b : p.qo_indptr[b], q_b = one_q ? 1 : p.qo_indptr[b + 1] - qbeg;
  const int nrows = q_b * G;
  const int q0 = qb * kPfRows;
  if (q0 >= nrows) return;                                // (uniform over the workgroup: before any barrier)
  const int pg0 = p.kv_indptr[b];
  [[maybe_unused]] int start = 0;                         // position of the page list's first token
  if constexpr (kStart) start = p.kv_start[b];
  const int len = start + (p.kv_indptr[b + 1] - pg0 - 1) * P + p.last_page_offset[b];
  const int prefix = len - q_b;                           // position of query 0
  const int kend = prefix + (min(q0 + kPfRows, nrows) + G - 1) / G;   // keys this block sees: 0 .. kend-1
  const int ntiles = kend > 0 ? (kend + kPfKeys - 1) / kPfKeys : 0;
  int t0, t1;
  if constexpr (kWindow) {                                // the splits divide [tlo, ntiles): tlo holds the lowest key of the block's first row
    int tlo = max(prefix + q0 / G - p.window + 1, 0) / kPfKeys;
    if constexpr (kStart) tlo = max(tlo, start / kPfKeys);   // (a no-op under the ring step's guarantee: no tile wholly below the list)
    const int chunk = (max(ntiles - tlo, 0) + p.splits - 1) / p.splits;
    t0 = tlo + sp * chunk, t1 = min(ntiles, t0 + chunk);
  } else {
    const int chunk = (ntiles + p.splits - 1) / p.splits;
    t0 = sp * chunk, t1 = min(ntiles, t0 + chunk);
  }

  if (tid < 64) {  // decode.cuh:535-539 / batch_decode_kernel: freq = rope_inv_scale * theta^(-2 i / 128), here in revolutions
    if constexpr (kTable)
      rope_fr[tid] = p.rope_table[tid];
    else
      rope_fr[tid] = p.rope_inv_scale * 0.15915494309189535f * __builtin_amdgcn_exp2f(-p.log2_theta * (float)(2 * tid) * (1.0f / kHeadDim));
  }
  __syncthreads();

  // ---- my query row: lane (li, g) = (row 16 w + li of the block, k-group); B operand of S^T: q[row][32 ks + 8 g .. + 7], ks = 0..3.
  // ks = 0 / 2 and 1 / 3 hold the two halves of the RoPE pairs (i, i + 64) with i = 8 g + j and 32 + 8 g + j.
  const int li = lane & 15, g = lane >> 4;
  const int ri = q0 + 16 * w + li;                        // row of the block's (sequence, K/V head)
  const bool row_ok = ri < nrows;
  const int qi = ri / G, hq = h * G + (ri - qi * G);      // query index within the sequence, query head
  const int pos = prefix + qi;
  const bool wave_live = q0 + 16 * w < nrows;             // (wave-uniform) any row of this wave exists
  const int pmin_w = prefix + (q0 + 16 * w) / G, pmax_w = prefix + (q0 + 16 * w + 15) / G;
  pf_h8 qf[4];
  {
    v4u raw[4];
    const half_t *qp = p.q + ((int64_t)(qbeg + (row_ok ? qi : 0)) * Nq + hq) * kHeadDim + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) raw[ks] = row_ok ? *reinterpret_cast<const v4u *>(qp + 32 * ks) : v4u{0u, 0u, 0u, 0u};
    const pf_h8 *x = reinterpret_cast<const pf_h8 *>(raw);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float s, c;
        if constexpr (kTable)
          rope_sincos_exact((float)pos, rope_fr[32 * hf + 8 * g + j], s, c);
        else
          pf_sincos_rev((float)pos * rope_fr[32 * hf + 8 * g + j], s, c);
        const float x1 = (float)x[hf][j], x2 = (float)x[hf + 2][j];
        qf[hf][j] = (half_t)(x1 * c - x2 * s);
        qf[hf + 2][j] = (half_t)(x2 * c + x1 * s);
      }
  }

  // ---- staging: thread (key kk, quarter u)
  const int kk = tid >> 2, u = tid & 3;
  const int64_t blk = (int64_t)N * P;                     // tokens x heads of one (page, layer, K|V) block
  const uint8_t *kbase = p.data + ((int64_t)p.layer * 2 * N + h) * P * 64;
  const half_t *qpbase = p.param + ((int64_t)p.layer * 2 * N + h) * P * 2;
  const int64_t page_bytes = (int64_t)p.L * 2 * blk * 64, page_halves = (int64_t)p.L * 2 * blk * 2;
  auto load = [&](int tile) -> PfTileRegs {
    PfTileRegs r;
    const int j = tile * kPfKeys + kk;
    bool in_list = j < len;
    if constexpr (kStart) in_list = in_list && j >= start;   // 0 <= (j - start) / P < the list's pages, whatever kv_start holds
    if (in_list) {
      const int jl = kStart ? j - start : j;
      const int pg = jl / P, e = jl - pg * P;
      const int64_t page = p.kv_indices[pg0 + pg];
      const uint8_t *kp = kbase + page * page_bytes + e * 64;
      const half_t *pp = qpbase + page * page_halves + e * 2;
      r.k1 = *reinterpret_cast<const v2u *>(kp + 8 * u);
      r.k2 = *reinterpret_cast<const v2u *>(kp + 32 + 8 * u);
      r.v = *reinterpret_cast<const v4u *>(kp + blk * 64 + 16 * u);
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
  auto stage = [&](int tile, const PfTileRegs &r, auto exact) {   // exact: std::bool_constant -- the product of a key's angle (rope_math.h)
    const int j = tile * kPfKeys + kk;
    bool ok = j < len;                                    // past the end: zeros (the loaded registers are zeros too, see load)
    if constexpr (kStart) ok = ok && j >= start;          // ... and so is a key in front of the list
    const float ks = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.kq & 0xFFFF)) : 0.f;
    const float kz = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.kq >> 16)) : 0.f;
    const float vs = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.vq & 0xFFFF)) : 0.f;
    const float vz = ok ? (float)__builtin_bit_cast(half_t, (unsigned short)(r.vq >> 16)) : 0.f;
    // K: pair m = dims (16u + m, 64 + 16u + m); word hw of k1 / k2 holds m = 8 hw .. 8 hw + 7, nibble e at bits 4e
    pf_h8 klo[2], khi[2];
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
          pf_sincos_rev((float)j * rope_fr[16 * u + m], s, c);
        klo[hw][e] = (half_t)(x1 * c - x2 * s);
        khi[hw][e] = (half_t)(x2 * c + x1 * s);
      }
    char *kl = reinterpret_cast<char *>(Ks);
    *reinterpret_cast<pf_h8 *>(kl + k_off(kk, 2 * u)) = klo[0];
    *reinterpret_cast<pf_h8 *>(kl + k_off(kk, 2 * u + 1)) = klo[1];
    *reinterpret_cast<pf_h8 *>(kl + k_off(kk, 8 + 2 * u)) = khi[0];
    *reinterpret_cast<pf_h8 *>(kl + k_off(kk, 8 + 2 * u + 1)) = khi[1];
    // V: word vw holds dims 32u + 8 vw .. + 7
    char *vl = reinterpret_cast<char *>(Vs);
#pragma unroll
    for (int vw = 0; vw < 4; ++vw) {
      pf_h8 vv;
#pragma unroll
      for (int e = 0; e < 8; ++e) vv[e] = (half_t)__builtin_fmaf((float)((r.v[vw] >> (4 * e)) & 0xF), vs, -vz);
      *reinterpret_cast<pf_h8 *>(vl + v_off(kk, 4 * u + vw)) = vv;
    }
  };

  v4f O[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) O[dt] = v4f{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;                   // row state (m reduced over the row's 4 lanes; l: this lane's keys only)

  PfTileRegs regs;
  if (t0 < t1) regs = load(t0);
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();                                      // the previous tile's LDS reads are done
    if constexpr (kTable) {
      if (tile * kPfKeys >= kRopeExactFrom)               // (workgroup-uniform) short contexts never take the exact form
        stage(tile, regs, std::true_type{});
      else
        stage(tile, regs, std::false_type{});
    } else {
      stage(tile, regs, std::false_type{});
    }
    __syncthreads();
    if (tile + 1 < t1) regs = load(tile + 1);             // in flight during this tile's products
    const int kt0 = tile * kPfKeys;
    if (!wave_live || kt0 > pmax_w) continue;             // (wave-uniform) no row of this wave sees a key of this tile
    if constexpr (kWindow) {
      if (kt0 + kPfKeys - 1 < pmin_w - p.window + 1) continue;   // (wave-uniform) ... the tile lies below every row's window
    }
    // ---- S^T = K . Q^T
    v4f S[4];
    const char *kl = reinterpret_cast<const char *>(Ks);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      S[kt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const pf_h8 a = *reinterpret_cast<const pf_h8 *>(kl + k_off(16 * kt + li, 4 * ks + g));
        S[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], S[kt], 0, 0, 0);
      }
    }
    // ---- online softmax; lane holds row li's scores of keys kt0 + 16 kt + 4 g + r
    const bool masked = kt0 + kPfKeys - 1 > pmin_w;       // (wave-uniform) some key of the tile is past some row's position
    [[maybe_unused]] bool lower = false;
    if constexpr (kWindow) lower = kt0 <= pmax_w - p.window;
    float mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = S[kt][r] * p.qk_scale;
        if (masked && kt0 + 16 * kt + 4 * g + r > pos) s = -INFINITY;
        if constexpr (kWindow) {                          // (lower: wave-uniform) some key of the tile is below some row's window
          if (lower && kt0 + 16 * kt + 4 * g + r <= pos - p.window) s = -INFINITY;
        }
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
    pf_h8 pf[2];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __builtin_amdgcn_exp2f(S[kt][r] - m_use);
        ls += pr;
        pf[kt >> 1][4 * (kt & 1) + r] = (half_t)pr;
      }
    l_run = __builtin_fmaf(l_run, alpha, ls);
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) O[dt] *= alpha;
    // ---- O^T += V^T . P^T; k-step s: element j of lane group g is key 32 s + 16 (j >> 2) + 4 g + (j & 3)
    const char *vl = reinterpret_cast<const char *>(Vs);
    const int tq = li >> 2, tp = li & 3;                  // transposed read: lane 4 tq + tp addresses row tq, dims 4 tp .. 4 tp + 3
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        pf_h4 half2x[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const int row = 32 * s + 16 * hh + 4 * g + tq;
          const int off = v_off(row, 2 * dt + (tp >> 1)) + 8 * (tp & 1);
          const pf_s4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pf_s4 *)(const_cast<char *>(vl) + off));
          half2x[hh] = __builtin_bit_cast(pf_h4, t);
        }
        const pf_h8 a = {half2x[0][0], half2x[0][1], half2x[0][2], half2x[0][3], half2x[1][0], half2x[1][1], half2x[1][2], half2x[1][3]};
        O[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[s], O[dt], 0, 0, 0);
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
    for (int dt = 0; dt < 8; ++dt) {
      const pf_h4 hv = {(half_t)(O[dt][0] * rl), (half_t)(O[dt][1] * rl), (half_t)(O[dt][2] * rl), (half_t)(O[dt][3] * rl)};
      *reinterpret_cast<pf_h4 *>(p.o + orow * kHeadDim + 16 * dt + 4 * g) = hv;
    }
  } else {
    float *wp = p.ws + (orow * p.splits + sp) * (kHeadDim + 2);
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      *reinterpret_cast<pf_f2 *>(wp + 16 * dt + 4 * g) = pf_f2{O[dt][0], O[dt][1]};
      *reinterpret_cast<pf_f2 *>(wp + 16 * dt + 4 * g + 2) = pf_f2{O[dt][2], O[dt][3]};
    }
    if (g == 0) {
      wp[kHeadDim] = m_run;
      wp[kHeadDim + 1] = l_all;
    }
  }
}

// KV splits: only where the query blocks leave the chip short of work (short chunks on long prefixes).  Aim at ~2 workgroups per CU
// (256 CUs) with at least 4 key tiles per split.
// win_tiles (the _win entry points; 0: no window): the most key tiles a query block touches under the window, see prefill_plan.
// ring (the _ring entry points): a list of max_pages pages that starts at a multiple of P, not of 64 -- its n = max_pages * P tokens
// touch up to (n + 62) / 64 + 1 tiles of the absolute grid (the bound of n contiguous keys at the worst alignment, as prefill_plan's).
static int64_t cache_tiles(int P, int max_pages, bool ring) {
  const int64_t n = (int64_t)max_pages * P;
  return ring ? (n + kPfKeys - 2) / kPfKeys + 1 : (n + kPfKeys - 1) / kPfKeys;
}

static int prefill_splits(int batch, int N, int max_q_len, int P, int max_pages, int64_t win_tiles = 0, bool ring = false) {
  if (max_pages <= 0) return 1;
  const int64_t blocks = (int64_t)batch * N * ((max_q_len + kPfRows - 1) / kPfRows);
  int64_t tiles = cache_tiles(P, max_pages, ring);
  if (win_tiles > 0) tiles = std::min(tiles, win_tiles);
  if (blocks >= 512 || tiles < 8) return 1;
  int64_t s = (512 + blocks - 1) / blocks;
  s = std::min<int64_t>(s, tiles / 4);
  s = std::min<int64_t>(s, 32);
  return (int)std::max<int64_t>(s, 1);
}

// ---- grouped-query attention (GQA): query head hq reads K/V head hq / G; the batch_prefill_kernel<true> geometry (see there)

static int gqa_group(int num_qo_heads, int num_kv_heads) {   // G, or 0 for a rejected pair of head counts
  if (num_kv_heads < 1 || num_qo_heads < 1 || num_qo_heads % num_kv_heads != 0) return 0;
  return num_qo_heads / num_kv_heads;
}

// Decode: a unit is (sequence, K/V head) -- one workgroup streams the unit's KV range (or one split of it) once for the whole group.
// Splits: the decode op's cost model (kv_i4.hip decode_splits_total) with units in place of (sequence, head) pairs, 64-key tiles, at
// least 2 tiles per split and 512 resident workgroups (2 per CU: 140 VGPRs + 32 AGPRs, 2 waves per SIMD).
static int gqa_decode_splits(int batch, int num_kv_heads, int P, int max_pages, int64_t win_tiles = 0, bool ring = false) {
  if (max_pages <= 0) return 1;
  int64_t tiles = cache_tiles(P, max_pages, ring);
  if (win_tiles > 0) tiles = std::min(tiles, win_tiles);
  const int64_t units = (int64_t)batch * num_kv_heads;
  const int64_t smax = std::max<int64_t>(std::min<int64_t>(tiles / 2, 32), 1);
  int best = 1;
  double best_cost = 1e30;
  for (int64_t s = 1; s <= smax; ++s) {
    const int64_t rounds = (units * s + 511) / 512;
    const double cost = (double)rounds * ((double)tiles / (double)s + 2.0) + 0.15 * (double)s;
    if (cost < best_cost - 1e-9) { best_cost = cost; best = (int)s; }
  }
  return best;
}

// The plan of a call: query rows of a (sequence, K/V head) at most -- max_q_len * G, or G for the decode entry (one query per
// sequence) --, the query blocks they make, and the KV splits by the entry's policy.  window (the _win entry points; 0: none): the
// policies see the most key tiles a query block can touch under the window in place of the cache's -- a block's rows span
// (min(rows, 64) - 1) / G positions, so its keys are n = window + that span contiguous ones, which touch (n + 62) / 64 + 1 tiles at
// the worst alignment; never more than the cache's tiles, so a window that covers the cache gives the un-windowed plan.
// ring (the _ring entry points): max_pages is the ring's size and the list starts off the 64-key grid, see cache_tiles; a ring of
// ceil((W - 1 + max_add) / P) + 1 pages holds more than any block's keys, so the window bound governs and the plan is the _win
// call's on a cache that never released a page (max_pages large).
struct PrefillPlan {
  int rows, nqb, splits;
};
static PrefillPlan prefill_plan(bool decode, int64_t total_q, int max_q_len, int batch, int G, int num_kv_heads, int P, int max_pages,
                                int window = 0, bool ring = false) {
  PrefillPlan pl;
  pl.rows = decode ? G : (int)std::min<int64_t>(std::min<int64_t>(max_q_len, total_q) * G, 0x7fffffff);
  pl.nqb = (int)(((int64_t)pl.rows + kPfRows - 1) / kPfRows);
  const int64_t win_tiles = window > 0 ? ((int64_t)window + (std::min(pl.rows, kPfRows) - 1) / G + kPfKeys - 2) / kPfKeys + 1 : 0;
  pl.splits = decode ? gqa_decode_splits(batch, num_kv_heads, P, max_pages, win_tiles, ring)
                     : prefill_splits(batch, num_kv_heads, pl.rows, P, max_pages, win_tiles, ring);
  return pl;
}

static size_t prefill_workspace_bytes(bool decode, int64_t total_q, int max_q_len, int batch, int G, int num_kv_heads, int P, int max_pages,
                                      int window = 0, bool ring = false) {
  if (total_q < 1 || batch < 1 || num_kv_heads < 1 || P < 16 || max_q_len < 1) return 0;
  const int s = prefill_plan(decode, total_q, max_q_len, batch, G, num_kv_heads, P, max_pages, window, ring).splits;
  return s > 1 ? partial_state_bytes(total_q * num_kv_heads * G, s) : 0;
}

// The one host path of batch_prefill_kernel.  decode: the grouped-query decode entry -- one query per sequence (no qo_indptr, total_q =
// batch), and `o` may be NULL: the partial states stay in the workspace un-merged, as atom_batch_decode_i4 leaves them.  The prefill
// entries refuse total_q / max_q_len (shape) before they look at alignment; the decode entry has no such arguments.  window: NULL, or
// the _win entries' argument (checked behind every other fault); those run the kWindow instantiations, the GQA form at every G.
// ring: the _ring entries -- window is theirs too, kv_start is checked behind it, and the kStart instantiations run.
static int launch_prefill(bool decode, void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                          const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                          int batch, int num_layers, int layer_idx, int G, int num_kv_heads, int page_size, int head_dim, float rope_theta,
                          float rope_scale, const float *rope_table, float attn_scale, int max_pages, void *workspace,
                          size_t workspace_bytes, void *stream, const int *window = nullptr, bool ring = false,
                          const int32_t *kv_start = nullptr) {
  const int st = check_kv(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx, num_kv_heads,
                          page_size, head_dim);
  if (st != ATOM_OK) return st;
  if (!q || !(rope_theta > 0.f) || !(rope_scale > 0.f) || (!decode && (!o || !qo_indptr))) return ATOM_ERR_INVALID_ARG;
  if (!decode && (total_q < 1 || total_q > 0x7fffffff || max_q_len < 1)) return ATOM_ERR_SHAPE;
  if ((o && !aligned16(o)) || !aligned16(q) || (reinterpret_cast<uintptr_t>(qo_indptr) & 3u)) return ATOM_ERR_ALIGN;
  PrefillPlan pl = prefill_plan(decode, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages, window ? std::max(*window, 0) : 0,
                                ring);
  const int num_qo_heads = num_kv_heads * G;
  const int64_t rows_heads = total_q * num_qo_heads;
  if (pl.splits > 1 && !workspace_holds(workspace, workspace_bytes, rows_heads, pl.splits)) pl.splits = 1;
  if (!o && pl.splits < 2) return ATOM_ERR_INVALID_ARG;
  const int64_t grid = (int64_t)pl.nqb * batch * num_kv_heads * pl.splits;
  if (grid > 0x7fffffff || rows_heads > 0x7fffffff) return ATOM_ERR_SHAPE;
  if (const int rs = check_rope_table(rope_table, attn_scale)) return rs;   // (the _rope entries' own faults: behind every older one)
  if (window && *window < 1) return ATOM_ERR_INVALID_ARG;                    // (the _win entries' own fault: behind those)
  if (ring && !kv_start) return ATOM_ERR_INVALID_ARG;                        // (the _ring entries' own faults: behind that)
  if (ring && (reinterpret_cast<uintptr_t>(kv_start) & 3u)) return ATOM_ERR_ALIGN;
  PrefillParams p;                                        // by name: the fields' order is the kernel's business
  p.data = (const uint8_t *)kv_data, p.param = (const half_t *)kv_param;
  p.kv_indptr = kv_indptr, p.kv_indices = kv_indices, p.last_page_offset = last_page_offset, p.qo_indptr = qo_indptr;
  p.q = (const half_t *)q, p.o = (half_t *)o, p.ws = (float *)workspace;
  p.batch = batch, p.L = num_layers, p.layer = layer_idx, p.N = num_kv_heads, p.P = page_size;
  p.nqb = pl.nqb, p.splits = pl.splits;
  p.qk_scale = kLog2e / sqrtf((float)kHeadDim) * attn_scale, p.log2_theta = log2f(rope_theta), p.rope_inv_scale = 1.0f / rope_scale;
  p.G = G, p.Nq = num_qo_heads;                           // (batch_prefill_kernel<false> reads neither)
  p.rope_table = rope_table;
  p.window = window ? *window : 0;                        // (only the kWindow instantiations read it)
  p.kv_start = kv_start;                                  // (only the kStart instantiations read it)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (ring) {                                             // (always with a window)
    if (rope_table)
      hipLaunchKernelGGL((batch_prefill_kernel<true, true, true, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
    else
      hipLaunchKernelGGL((batch_prefill_kernel<true, false, true, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
  } else if (window) {                                           // the GQA form for every head ratio, with or without a table
    if (rope_table)
      hipLaunchKernelGGL((batch_prefill_kernel<true, true, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
    else
      hipLaunchKernelGGL((batch_prefill_kernel<true, false, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
  } else if (rope_table) {                                       // the same plan, the kTable instantiation of the same kernel
    if (G == 1 && !decode)
      hipLaunchKernelGGL((batch_prefill_kernel<false, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
    else
      hipLaunchKernelGGL((batch_prefill_kernel<true, true>), dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
  } else if (G == 1 && !decode)                                  // the MHA entry: the GQA entries forward G = 1 to the MHA ops
    hipLaunchKernelGGL(batch_prefill_kernel<false>, dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
  else
    hipLaunchKernelGGL(batch_prefill_kernel<true>, dim3((unsigned)grid), dim3(kPfThreads), 0, s, p);
  if (pl.splits > 1 && o) launch_merge(workspace, o, rows_heads, pl.splits, s);
  return check_launch();
}

}  // namespace atom

using namespace atom;

extern "C" {

size_t atom_batch_prefill_i4_workspace_bytes(int64_t total_q, int batch, int num_heads, int page_size, int max_q_len,
                                             int max_pages_per_seq) {
  return prefill_workspace_bytes(false, total_q, max_q_len, batch, 1, num_heads, page_size, max_pages_per_seq);
}

int atom_batch_prefill_i4(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                          const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                          int batch, int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, float rope_theta,
                          float rope_scale, int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream) {
  return launch_prefill(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                        num_layers, layer_idx, 1, num_heads, page_size, head_dim, rope_theta, rope_scale, nullptr, 1.0f, max_pages_per_seq,
                        workspace, workspace_bytes, stream);
}

size_t atom_batch_prefill_gqa_i4_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                 int max_q_len, int max_pages_per_seq) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);   // (G = 1 is the MHA plan: the same function)
  return G ? prefill_workspace_bytes(false, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages_per_seq) : 0;
}

int atom_batch_prefill_gqa_i4(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                              const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                              int batch, int num_layers, int layer_idx, int num_qo_heads, int num_kv_heads, int page_size, int head_dim,
                              float rope_theta, float rope_scale, int max_pages_per_seq, void *workspace, size_t workspace_bytes,
                              void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                        num_layers, layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, nullptr, 1.0f, max_pages_per_seq,
                        workspace, workspace_bytes, stream);
}

int atom_batch_prefill_gqa_i4_rope(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                   const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                   const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                   int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                   const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                   size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                        num_layers, layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale,
                        max_pages_per_seq, workspace, workspace_bytes, stream);
}

size_t atom_batch_decode_gqa_i4_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 1) return atom_batch_decode_i4_workspace_bytes(batch, num_qo_heads, page_size, max_pages_per_seq);
  return G ? prefill_workspace_bytes(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq) : 0;
}

int atom_batch_decode_gqa_i4_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 1) return atom_batch_decode_i4_splits(batch, num_qo_heads, page_size, max_pages_per_seq);
  if (G == 0 || batch < 1 || page_size < 16) return 0;
  return prefill_plan(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq).splits;
}

int atom_batch_decode_gqa_i4(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                             const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                             int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                             int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  if (G == 1)
    return atom_batch_decode_i4(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx,
                                num_qo_heads, page_size, head_dim, rope_theta, rope_scale, max_pages_per_seq, workspace, workspace_bytes,
                                stream);
  return launch_prefill(true, o, q, nullptr, batch, 1, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers,
                        layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, nullptr, 1.0f, max_pages_per_seq, workspace,
                        workspace_bytes, stream);
}

int atom_batch_decode_gqa_i4_rope(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                  const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                  int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  if (G == 1)
    return batch_decode_rope(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers, layer_idx, num_qo_heads,
                             page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale, max_pages_per_seq, workspace,
                             workspace_bytes, stream);
  return launch_prefill(true, o, q, nullptr, batch, 1, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers,
                        layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale, max_pages_per_seq,
                        workspace, workspace_bytes, stream);
}

// ---- sliding window: the _rope entries with `window` behind attn_scale (include/atom_hip.h); always the matrix-core kernel

size_t atom_batch_decode_gqa_i4_win_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq,
                                                    int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  return G && window >= 1 ? prefill_workspace_bytes(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq, window) : 0;
}

int atom_batch_decode_gqa_i4_win_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq, int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0 || batch < 1 || page_size < 16 || window < 1) return 0;
  return prefill_plan(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq, window).splits;
}

size_t atom_batch_prefill_gqa_i4_win_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                     int max_q_len, int max_pages_per_seq, int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  return G && window >= 1 ? prefill_workspace_bytes(false, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages_per_seq, window)
                          : 0;
}

int atom_batch_decode_gqa_i4_win(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                 const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                 int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                 const float *rope_table, float attn_scale, int window, int max_pages_per_seq, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(true, o, q, nullptr, batch, 1, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers,
                        layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale, max_pages_per_seq,
                        workspace, workspace_bytes, stream, &window);
}

int atom_batch_prefill_gqa_i4_win(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                  const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                  const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                  int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int window, int max_pages_per_seq, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                        num_layers, layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale,
                        max_pages_per_seq, workspace, workspace_bytes, stream, &window);
}

// ---- rolling cache: the _win entries with `kv_start` behind window (include/atom_hip.h); the page list starts at position kv_start[b]

size_t atom_batch_decode_gqa_i4_ring_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq,
                                                     int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  return G && window >= 1 ? prefill_workspace_bytes(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq, window, true) : 0;
}

int atom_batch_decode_gqa_i4_ring_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq, int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0 || batch < 1 || page_size < 16 || window < 1) return 0;
  return prefill_plan(true, batch, 1, batch, G, num_kv_heads, page_size, max_pages_per_seq, window, true).splits;
}

size_t atom_batch_prefill_gqa_i4_ring_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                      int max_q_len, int max_pages_per_seq, int window) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  return G && window >= 1
             ? prefill_workspace_bytes(false, total_q, max_q_len, batch, G, num_kv_heads, page_size, max_pages_per_seq, window, true)
             : 0;
}

int atom_batch_decode_gqa_i4_ring(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                  const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                  int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int window, const int32_t *kv_start, int max_pages_per_seq,
                                  void *workspace, size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(true, o, q, nullptr, batch, 1, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch, num_layers,
                        layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale, max_pages_per_seq,
                        workspace, workspace_bytes, stream, &window, true, kv_start);
}

int atom_batch_prefill_gqa_i4_ring(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                   const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                   const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                   int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                   const float *rope_table, float attn_scale, int window, const int32_t *kv_start, int max_pages_per_seq,
                                   void *workspace, size_t workspace_bytes, void *stream) {
  const int G = gqa_group(num_qo_heads, num_kv_heads);
  if (G == 0) return ATOM_ERR_SHAPE;
  return launch_prefill(false, o, q, qo_indptr, total_q, max_q_len, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, batch,
                        num_layers, layer_idx, G, num_kv_heads, page_size, head_dim, rope_theta, rope_scale, rope_table, attn_scale,
                        max_pages_per_seq, workspace, workspace_bytes, stream, &window, true, kv_start);
}

}  // extern "C"
