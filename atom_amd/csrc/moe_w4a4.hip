// Mixtral-style sparse mixture of experts on the W4A4 path (include/atom_hip.h, "Sparse mixture of experts"): the router's tables, the
// routed ("grouped") GEMM and the weighted combine -- three kernels with no host work between them, so that a decode step captures.
// The reference runs the block as a Python loop over the experts with a host read per expert (model/qMixtralLayer.py:302-350).
//   * moe_route_kernel: ONE workgroup.  Pass A: a thread per token picks the top_k experts (largest first, the lower index on equal
//     logits), writes their renormalised weights and counts rows per expert (integer LDS atomics: a sum, no order in it).  Then the
//     prefix sums and the tile table.  Pass B walks the tokens again in chunks of 256: per expert a wave ballot gives every selected
//     slot its rank among the chunk's tokens (lower lanes, lower waves, earlier chunks), i.e. rows grouped by expert in ascending
//     token order by construction.
//   * moe_gemm_w4a4_kernel: the 64 x 64 whole-K tile of gemm_w4a4_mid.hip (8 waves, 8-stage LDS ring, LDS-DMA pieces in MFMA order,
//     the de-quantisation of step s behind the loads of step s + 1) with the tile looked up in the router's table: the expert picks
//     the weight bases (SGPRs), the token rows are gathered per lane (row_index), the 64 features go to their segment's output.
//     Every output element is one ordered sum over the K steps: the bits do not depend on the tile a row lands in.
//   * moe_combine_kernel: out = residual + sum over a token's slots in ascending expert id of half(y * w), fp16 adds.
#include "common.h"

namespace atom {
namespace moe {

constexpr int BN = 64, NW = 8, NS = 8, NT = NW * 64;
constexpr int W_OFF = 0;          // 4 fragments x 1 KiB: fragment f = 2 h + k, row i = feature 32 h + 2 i + k of the tile
constexpr int A_OFF = 4096;       // 4 token blocks x 1 KiB: row i = routed row 16 b + i of the tile
constexpr int SB_OFF = 8192;      // 64 weight scales fp16 (a dword piece moves 128: the upper half is not read)
constexpr int SA_OFF = 8448;      // 64 token scales, fp16 zero-extended to a dword each (ushort pieces)
constexpr int STAGE = 8704;
constexpr int LDS_BYTES = NS * STAGE;
constexpr int PPW = 2;            // LDS-DMA instructions per stage on waves 0 / 1 (a data piece + a scale piece); the others: 1
static_assert(PPW * (NS - 2) < 64 && LDS_BYTES <= 160 * 1024, "ring depth");

struct GemmArgs {
  const uint8_t *A4, *B4, *A8, *B8;
  const half_t *sA, *sB, *sA8, *sB8;
  const int32_t *row_index, *expert_indptr, *tile_expert, *tile_row0, *n_tiles;
  half_t *out[2];
  int64_t ldA;                    // halves between the groups of sA
  int R, E, N, N_seg, K4h, G, A_rows, max_tiles, ref_layout;
};

__device__ __forceinline__ v4i even_codes(v4u x) {       // low nibbles  -> int8 16 * code
  return v4i{(int)((x.x << 4) & 0xF0F0F0F0u), (int)((x.y << 4) & 0xF0F0F0F0u), (int)((x.z << 4) & 0xF0F0F0F0u),
             (int)((x.w << 4) & 0xF0F0F0F0u)};
}
__device__ __forceinline__ v4i odd_codes(v4u x) {        // high nibbles -> int8 16 * code
  return v4i{(int)(x.x & 0xF0F0F0F0u), (int)(x.y & 0xF0F0F0F0u), (int)(x.z & 0xF0F0F0F0u), (int)(x.w & 0xF0F0F0F0u)};
}

// what a step leaves for the next one to de-quantise
struct Pending {
  v4i acc[2];
  float sa;                // token scale (x 1 / 256 for the widened int4 operands)
  float sb[8];             // weight scales of the lane's 8 features, [2 r + k]
};

// c[k][r] = fma(idot, sa * sb, c): lane = routed row 16 tb + l15, feature 32 h + 8 kb + 2 r + k (the contract: one product per channel)
__device__ __forceinline__ void dequant(const Pending &q, float (&c)[2][4]) {
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q.sa * q.sb[j];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      c[k][r] = __builtin_fmaf((float)q.acc[k][r], s[2 * r + k], c[k][r]);
      asm volatile("" : "+v"(c[k][r]));
    }
}

__global__ __launch_bounds__(NT) void moe_gemm_w4a4_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __builtin_assume(wave >= 0 && wave < NW);
  const int h = wave & 1, tb = wave >> 1;
  const int nt = min(max(*p.n_tiles, 0), p.max_tiles), nbn = p.N / BN;
  int id = blockIdx.x;
  {                                                        // workgroup b runs on XCD b % 8: every XCD takes a contiguous run of the nt x nbn
    const int nwg = nt * nbn;                              // live tiles, row tiles fastest -- the tiles of an expert are neighbours in the table,
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7, k = id >> 3;   // so the workgroups that share a weight tile share an L2.  The grid is
    if (k >= (xcd < r ? q + 1 : q)) return;                // sized for the worst routing: the rest leave before touching memory
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int tile = id % nt, n0 = (id / nt) * BN;
  const int e = __builtin_amdgcn_readfirstlane(p.tile_expert[tile]);
  const int row0 = __builtin_amdgcn_readfirstlane(p.tile_row0[tile]);
  if ((unsigned)e >= (unsigned)p.E) return;                // (a table the router did not write: never an address from it)
  const int rend = min(__builtin_amdgcn_readfirstlane(p.expert_indptr[e + 1]), p.R);
  if (row0 < 0 || row0 >= rend) return;

  // ---- LDS-DMA, loop invariant: per lane the offsets, per wave (SGPRs) the operand it stages.  Waves 0..3 the weight fragments of
  // expert e, waves 4..7 the token blocks: routed row -> source row through row_index, clamped like the dense kernel's M tail
  unsigned voff, kvoff, svoff;
  const uint8_t *d4, *d8;
  const half_t *s4, *s8;
  int64_t sstride;
  {
    const int i = lane >> 2, j = lane & 3;
    const unsigned chunk = (unsigned)((j ^ ((i >> 1) & 3)) << 4);    // LDS slot j of row i receives source chunk j ^ ((i >> 1) & 3)
    unsigned row;
    if (wave < 4) {
      row = (unsigned)(n0 + 32 * (wave >> 1) + 2 * i + (wave & 1));
      d4 = p.B4 + (int64_t)e * p.N * p.K4h;
      d8 = p.B8 + (int64_t)e * p.N * kKeeper;
    } else {
      const int r = min(row0 + 16 * (wave - 4) + i, rend - 1);
      row = min((unsigned)(p.row_index ? p.row_index[r] : r), (unsigned)(p.A_rows - 1));
      d4 = p.A4;
      d8 = p.A8;
    }
    voff = row * (unsigned)p.K4h + chunk;
    kvoff = row * (unsigned)kKeeper + chunk;
    if (wave & 1) {                                        // token scales: indexed by the SOURCE row
      const int r = min(row0 + lane, rend - 1);
      const int m = (int)min((unsigned)(p.row_index ? p.row_index[r] : r), (unsigned)(p.A_rows - 1));
      svoff = (unsigned)(p.ref_layout ? ref_scale_index(m) : m) * 2u;
      s4 = p.sA; s8 = p.sA8; sstride = p.ldA;
    } else {
      svoff = (unsigned)min(n0 + 2 * lane, p.N - 2) * 2u;
      s4 = p.sB + (int64_t)e * p.G * p.N; s8 = p.sB8 + (int64_t)e * p.N; sstride = p.N;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(voff), "+v"(kvoff), "+v"(svoff)::"memory");   // the table reads are done: from here on vmcnt counts LDS-DMA only
  const unsigned lds0 = lds_addr(lds);
  const unsigned ldsw = lds0 + (unsigned)wave * 1024u;
  const int G = p.G, T = G + 2;                            // stages: G int4 groups + the keeper's two halves
  // stage `st`: 0 .. G - 1 the int4 groups, G / G + 1 the two 64-column halves of the keeper (same row layout, INT8 bytes)
  auto issue_stage = [&](int st, unsigned slot) {
    const bool k8 = st >= G;
    const uint8_t *base = k8 ? d8 + (st - G) * 64 : d4 + (int64_t)st * 64;
    const half_t *sc = k8 ? s8 : s4 + (int64_t)st * sstride;
    lds_dma_sv<16>(base, k8 ? kvoff : voff, ldsw + slot);
    if (wave == 1) lds_dma_sv<2>(sc, svoff, lds0 + slot + SA_OFF);
    else if (wave == 0) lds_dma_sv<4>(sc, svoff, lds0 + slot + SB_OFF);
  };
#pragma unroll 1
  for (int s = 0; s < NS - 1; ++s) issue_stage(min(s, T - 1), (unsigned)(s * STAGE));

  const int l15 = lane & 15, kb = lane >> 4;
  const int coff = l15 * 64 + ((kb ^ ((l15 >> 1) & 3)) << 4);      // the lane's 16-byte chunk of a fragment row (swizzled)
  const int aw = W_OFF + 2 * h * 1024 + coff, aa = A_OFF + tb * 1024 + coff;
  const int asa = SA_OFF + (tb * 16 + l15) * 4, asb = SB_OFF + (32 * h + 8 * kb) * 2;

  float c[2][4];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[k][r] = 0.f;
  Pending q;
  q.sa = 0.f;
  q.acc[0] = q.acc[1] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) q.sb[j] = 0.f;

  int slot = 0, dslot = NS - 1;                            // ring positions of the stage computed / requested in this step
  for (int step = 0; step < G; ++step) {
    if (wave < 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");   // this wave's pieces of stage `step` have landed
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NS - 2) : "memory");
    __builtin_amdgcn_s_barrier();                          // ... everybody's; and everybody is done reading the slot of step - 1
    issue_stage(min(step + NS - 1, T - 1), (unsigned)(dslot * STAGE));   // (past the end: repeats into a dead slot keep the count)
    __builtin_amdgcn_sched_barrier(0);
    const char *sl = lds + slot * STAGE;
    v4u wf[2];
    wf[0] = *reinterpret_cast<const v4u *>(sl + aw);
    wf[1] = *reinterpret_cast<const v4u *>(sl + aw + 1024);
    const v4u bf = *reinterpret_cast<const v4u *>(sl + aa);
    const unsigned sah = *reinterpret_cast<const unsigned *>(sl + asa);
    const v4u sbv = *reinterpret_cast<const v4u *>(sl + asb);
    __builtin_amdgcn_sched_barrier(0);
    dequant(q, c);                                         // the previous step's products, while this step's fragments arrive
    __builtin_amdgcn_sched_barrier(0);
    const v4i be = even_codes(bf), bo = odd_codes(bf);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      v4i a = __builtin_amdgcn_mfma_i32_16x16x64_i8(even_codes(wf[k]), be, v4i{0, 0, 0, 0}, 0, 0, 0);
      q.acc[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(odd_codes(wf[k]), bo, a, 0, 0, 0);
    }
    q.sa = (float)__builtin_bit_cast(half_t, (unsigned short)sah) * (1.0f / 256.0f);
    {
      const half_t *hv = reinterpret_cast<const half_t *>(&sbv);
#pragma unroll
      for (int j = 0; j < 8; ++j) q.sb[j] = (float)hv[j];
    }
    slot = slot + 1 == NS ? 0 : slot + 1;
    dslot = dslot + 1 == NS ? 0 : dslot + 1;
  }
  dequant(q, c);                                           // the last int4 step
  // the keeper: stages G and G + 1 are its two 64-column halves: ONE dot product per output, two chained MFMAs, one de-quantisation
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  {
    const char *s0 = lds + slot * STAGE, *s1 = lds + (slot + 1 == NS ? 0 : slot + 1) * STAGE;
    const v4u sbv = *reinterpret_cast<const v4u *>(s0 + asb);
    const half_t *hv = reinterpret_cast<const half_t *>(&sbv);
#pragma unroll
    for (int j = 0; j < 8; ++j) q.sb[j] = (float)hv[j];
    const v4i b0 = __builtin_bit_cast(v4i, *reinterpret_cast<const v4u *>(s0 + aa));
    const v4i b1 = __builtin_bit_cast(v4i, *reinterpret_cast<const v4u *>(s1 + aa));
    const unsigned sah = *reinterpret_cast<const unsigned *>(s0 + asa);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const v4i w0 = __builtin_bit_cast(v4i, *reinterpret_cast<const v4u *>(s0 + aw + k * 1024));
      const v4i w1 = __builtin_bit_cast(v4i, *reinterpret_cast<const v4u *>(s1 + aw + k * 1024));
      v4i a = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, b0, v4i{0, 0, 0, 0}, 0, 0, 0);
      q.acc[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, b1, a, 0, 0, 0);
    }
    q.sa = (float)__builtin_bit_cast(half_t, (unsigned short)sah);
    dequant(q, c);
  }
  // a lane holds 8 consecutive features of one routed row: one 16-byte store into the segment the tile's 64 features belong to
  const int m = row0 + 16 * tb + l15;
  if (m < rend) {
    v4u o;
    half_t *ov = reinterpret_cast<half_t *>(&o);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ov[2 * r] = f2h(c[0][r]);
      ov[2 * r + 1] = f2h(c[1][r]);
    }
    const int seg = n0 >= p.N_seg ? 1 : 0;
    *reinterpret_cast<v4u *>(p.out[seg] + (int64_t)m * p.N_seg + (n0 - seg * p.N_seg) + 32 * h + 8 * kb) = o;
  }
}

// ------------------------------------------------------------------------------------------------------------ router
constexpr int RT = 256, RW = RT / 64, MAXE = 64, MAXK = 8;

__global__ __launch_bounds__(RT) void moe_route_kernel(const half_t *logits, int T, int E, int K, int32_t *topk_ids, half_t *topk_w,
                                                       int32_t *expert_indptr, int32_t *row_token, int32_t *slot_row,
                                                       int32_t *tile_expert, int32_t *tile_row0, int32_t *n_tiles) {
  __shared__ int cnt[MAXE], base[MAXE], ptr[MAXE + 1], tbase[MAXE + 1], wcnt[MAXE * RW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < MAXE) { cnt[tid] = 0; base[tid] = 0; }
  __syncthreads();
  // pass A: the experts and weights of every token, rows per expert
  for (int64_t t = tid; t < T; t += RT) {
    const half_t *l = logits + t * E;
    unsigned long long taken = 0;
    float ex[MAXK], lmax = 0.f, sum = 0.f;
    int sel[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      sel[j] = 0; ex[j] = 0.f;
      if (j < K) {
        int bi = __builtin_ctzll(~taken);                  // the lowest expert not yet taken: < E while fewer than E are taken
        float best = (float)l[bi];
        for (int x = bi + 1; x < E; ++x) {
          const float v = (float)l[x];
          if (!((taken >> x) & 1) && v > best) { best = v; bi = x; }   // strictly larger: the lower index wins a tie
        }
        taken |= 1ull << bi;
        if (j == 0) lmax = best;
        sel[j] = bi;
        ex[j] = expf(best - lmax);
        sum += ex[j];
        atomicAdd(&cnt[bi], 1);
      }
    }
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < K) {
        topk_ids[(int64_t)t * K + j] = sel[j];
        topk_w[(int64_t)t * K + j] = f2h(ex[j] / sum);
      }
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0, tb = 0;
    for (int x = 0; x < E; ++x) {
      ptr[x] = a; tbase[x] = tb;
      a += cnt[x];
      tb += (cnt[x] + 63) >> 6;
    }
    ptr[E] = a; tbase[E] = tb;
    n_tiles[0] = tb;
  }
  __syncthreads();
  if (tid <= E) expert_indptr[tid] = ptr[tid];
  for (int x = 0; x < E; ++x) {                            // the tile table: for each expert in order, one tile per started 64 rows
    const int n = tbase[x + 1] - tbase[x];
    for (int i = tid; i < n; i += RT) {
      tile_expert[tbase[x] + i] = x;
      tile_row0[tbase[x] + i] = ptr[x] + 64 * i;
    }
  }
  // pass B: chunks of RT tokens in order; a slot's row = its expert's first row + the expert's slots in earlier chunks, lower waves,
  // lower lanes
  const int64_t R = (int64_t)T * K;
  for (int64_t c0 = 0; c0 < T; c0 += RT) {
    const int64_t t = c0 + tid;
    const bool valid = t < T;
    int sel[MAXK], lr[MAXK];
    unsigned long long mask = 0;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      sel[j] = -1; lr[j] = 0;
      if (valid && j < K) {
        sel[j] = topk_ids[(int64_t)t * K + j] & (MAXE - 1);   // (written by this thread in pass A)
        mask |= 1ull << sel[j];
      }
    }
    for (int x = 0; x < E; ++x) {
      const unsigned long long b = __ballot((mask >> x) & 1);
      const int below = __popcll(b & ((1ull << lane) - 1));
#pragma unroll
      for (int j = 0; j < MAXK; ++j)
        if (sel[j] == x) lr[j] = below;
      if (lane == 0) wcnt[x * RW + wave] = __popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (sel[j] >= 0) {
        const int x = sel[j];
        int off = base[x] + lr[j];
        for (int w = 0; w < wave; ++w) off += wcnt[x * RW + w];
        const int64_t row = (int64_t)ptr[x] + off;
        if (row < R) row_token[row] = (int)t;
        slot_row[(int64_t)t * K + j] = (int)row;
      }
    __syncthreads();
    if (tid < E) {
      int s = 0;
      for (int w = 0; w < RW; ++w) s += wcnt[tid * RW + w];
      base[tid] += s;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ combine
__global__ __launch_bounds__(256) void moe_combine_kernel(const half_t *y, const int32_t *slot_row, const int32_t *topk_ids, const half_t *topk_w,
                                                          const half_t *residual, half_t *out, int K, int H8, int cblocks, int R) {
  const int t = blockIdx.x / cblocks;
  const int ch = (blockIdx.x % cblocks) * 256 + threadIdx.x;
  if (ch >= H8) return;
  const int64_t H = (int64_t)H8 * 8;
  int ids[MAXK], rows[MAXK];
  float ws[MAXK];
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    ids[j] = 0x7fffffff; rows[j] = 0; ws[j] = 0.f;
    if (j < K) {
      ids[j] = topk_ids[(int64_t)t * K + j];
      rows[j] = (int)min((unsigned)slot_row[(int64_t)t * K + j], (unsigned)(R - 1));
      ws[j] = (float)topk_w[(int64_t)t * K + j];
    }
  }
  half_t acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (half_t)0.f;
  unsigned done = 0;
#pragma unroll
  for (int pos = 0; pos < MAXK; ++pos) {
    if (pos < K) {
      int bj = 0, bid = 0x7fffffff, brow = 0;              // the slot with the smallest expert id among those left
      float bw = 0.f;
#pragma unroll
      for (int j = 0; j < MAXK; ++j)
        if (j < K && !((done >> j) & 1) && (ids[j] < bid || bid == 0x7fffffff)) { bid = ids[j]; bj = j; brow = rows[j]; bw = ws[j]; }
      done |= 1u << bj;
      const v4u v = *reinterpret_cast<const v4u *>(y + (int64_t)brow * H + (int64_t)ch * 8);
      const half_t *hv = reinterpret_cast<const half_t *>(&v);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const half_t pr = f2h((float)hv[i] * bw);
        acc[i] = f2h((float)acc[i] + (float)pr);
      }
    }
  }
  if (residual) {
    const v4u v = *reinterpret_cast<const v4u *>(residual + (int64_t)t * H + (int64_t)ch * 8);
    const half_t *hv = reinterpret_cast<const half_t *>(&v);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f2h((float)hv[i] + (float)acc[i]);
  }
  v4u o;
  half_t *ov = reinterpret_cast<half_t *>(&o);
#pragma unroll
  for (int i = 0; i < 8; ++i) ov[i] = acc[i];
  *reinterpret_cast<v4u *>(out + (int64_t)t * H + (int64_t)ch * 8) = o;
}

}  // namespace moe
}  // namespace atom

using namespace atom;

static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

extern "C" int64_t atom_moe_max_tiles(int64_t R, int E) {
  if (R < 0 || E < 0) return 0;
  return R / 64 + (E < R ? E : R);
}

extern "C" int atom_moe_route_topk(const void *logits, int64_t T, int E, int top_k, int32_t *topk_ids, void *topk_w, int32_t *expert_indptr,
                                   int32_t *row_token, int32_t *slot_row, int32_t *tile_expert, int32_t *tile_row0, int32_t *n_tiles,
                                   void *stream) {
  if (!logits || !topk_ids || !topk_w || !expert_indptr || !row_token || !slot_row || !tile_expert || !tile_row0 || !n_tiles)
    return ATOM_ERR_INVALID_ARG;
  if (E < 2 || E > moe::MAXE || top_k < 1 || top_k > moe::MAXK || top_k > E || T < 1) return ATOM_ERR_SHAPE;
  if (T * top_k >= (int64_t(1) << 31)) return ATOM_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(logits) & 1u) || (reinterpret_cast<uintptr_t>(topk_w) & 1u) || !aligned4(topk_ids) || !aligned4(expert_indptr) ||
      !aligned4(row_token) || !aligned4(slot_row) || !aligned4(tile_expert) || !aligned4(tile_row0) || !aligned4(n_tiles))
    return ATOM_ERR_ALIGN;
  hipLaunchKernelGGL(moe::moe_route_kernel, dim3(1), dim3(moe::RT), 0, (hipStream_t)stream, (const half_t *)logits, (int)T, E, top_k, topk_ids,
                     (half_t *)topk_w, expert_indptr, row_token, slot_row, tile_expert, tile_row0, n_tiles);
  return check_launch();
}

extern "C" int atom_moe_gemm_w4a4_f16(const void *A4, const void *B4, const void *sA, const void *sB, const void *A8, const void *B8,
                                      const void *sA8, const void *sB8, const int32_t *row_index, const int32_t *expert_indptr,
                                      const int32_t *tile_expert, const int32_t *tile_row0, const int32_t *n_tiles, void *out0, void *out1,
                                      int64_t A_rows, int64_t R, int E, int64_t N_seg, int nseg, int64_t K_total, int group, int keeper,
                                      int scale_layout, void *stream) {
  if (!A4 || !B4 || !sA || !sB || !A8 || !B8 || !sA8 || !sB8 || !expert_indptr || !tile_expert || !tile_row0 || !n_tiles || !out0)
    return ATOM_ERR_INVALID_ARG;
  if (nseg < 1 || nseg > 2 || (nseg == 2 && !out1)) return ATOM_ERR_INVALID_ARG;
  if (scale_layout != ATOM_SCALE_LAYOUT_REF && scale_layout != ATOM_SCALE_LAYOUT_PLAIN) return ATOM_ERR_INVALID_ARG;
  if (group != kGroup || keeper != kKeeper) return ATOM_ERR_SHAPE;
  if (E < 1 || E > moe::MAXE || R < 1 || R >= (int64_t(1) << 31) || A_rows < 1 || A_rows > (1 << 24)) return ATOM_ERR_SHAPE;
  if (N_seg < 64 || (N_seg % 64) != 0 || N_seg > (1 << 24)) return ATOM_ERR_SHAPE;
  if (K_total < 256 || ((K_total - kKeeper) % kGroup) != 0 || K_total > (1 << 20)) return ATOM_ERR_SHAPE;
  const int64_t N = N_seg * nseg, K4h = (K_total - kKeeper) / 2;
  if (A_rows * K4h >= (int64_t(1) << 32) || N * K4h >= (int64_t(1) << 32)) return ATOM_ERR_SHAPE;   // 32-bit lane offsets
  const int64_t max_tiles = atom_moe_max_tiles(R, E);
  if (max_tiles * (N / 64) >= (int64_t(1) << 31)) return ATOM_ERR_SHAPE;
  if (!aligned16(A4) || !aligned16(B4) || !aligned16(A8) || !aligned16(B8) || !aligned16(out0) || (out1 && !aligned16(out1))) return ATOM_ERR_ALIGN;
  if (!aligned4(sB) || !aligned4(sB8) || (reinterpret_cast<uintptr_t>(sA) & 1u) || (reinterpret_cast<uintptr_t>(sA8) & 1u)) return ATOM_ERR_ALIGN;
  if ((row_index && !aligned4(row_index)) || !aligned4(expert_indptr) || !aligned4(tile_expert) || !aligned4(tile_row0) || !aligned4(n_tiles))
    return ATOM_ERR_ALIGN;
  moe::GemmArgs p;
  p.A4 = (const uint8_t *)A4; p.B4 = (const uint8_t *)B4; p.A8 = (const uint8_t *)A8; p.B8 = (const uint8_t *)B8;
  p.sA = (const half_t *)sA; p.sB = (const half_t *)sB; p.sA8 = (const half_t *)sA8; p.sB8 = (const half_t *)sB8;
  p.row_index = row_index; p.expert_indptr = expert_indptr; p.tile_expert = tile_expert; p.tile_row0 = tile_row0; p.n_tiles = n_tiles;
  p.out[0] = (half_t *)out0; p.out[1] = (half_t *)(nseg == 2 ? out1 : out0);
  p.ldA = (int64_t)atom_scale_size(A_rows, scale_layout);
  p.R = (int)R; p.E = E; p.N = (int)N; p.N_seg = (int)N_seg; p.K4h = (int)K4h; p.G = (int)((K_total - kKeeper) / kGroup);
  p.A_rows = (int)A_rows; p.max_tiles = (int)max_tiles; p.ref_layout = scale_layout == ATOM_SCALE_LAYOUT_REF;
  static std::atomic<uint64_t> attr_done{0};
  if (ensure_max_lds(reinterpret_cast<const void *>(&moe::moe_gemm_w4a4_kernel), moe::LDS_BYTES, attr_done) != ATOM_OK) return ATOM_ERR_LAUNCH;
  hipLaunchKernelGGL(moe::moe_gemm_w4a4_kernel, dim3((unsigned)(max_tiles * (N / 64))), dim3(moe::NT), moe::LDS_BYTES, (hipStream_t)stream, p);
  return check_launch();
}

extern "C" int atom_moe_combine_f16(const void *y, const int32_t *slot_row, const int32_t *topk_ids, const void *topk_w, const void *residual,
                                    void *out, int64_t T, int top_k, int64_t H, void *stream) {
  if (!y || !slot_row || !topk_ids || !topk_w || !out) return ATOM_ERR_INVALID_ARG;
  if (T < 1 || top_k < 1 || top_k > moe::MAXK || H < 8 || (H % 8) != 0 || H > (1 << 24)) return ATOM_ERR_SHAPE;
  if (T * top_k >= (int64_t(1) << 31)) return ATOM_ERR_SHAPE;
  const int H8 = (int)(H / 8), cblocks = (H8 + 255) / 256;
  if (T * cblocks >= (int64_t(1) << 31)) return ATOM_ERR_SHAPE;
  if (!aligned16(y) || !aligned16(out) || (residual && !aligned16(residual))) return ATOM_ERR_ALIGN;
  if (!aligned4(slot_row) || !aligned4(topk_ids) || (reinterpret_cast<uintptr_t>(topk_w) & 1u)) return ATOM_ERR_ALIGN;
  hipLaunchKernelGGL(moe::moe_combine_kernel, dim3((unsigned)(T * cblocks)), dim3(256), 0, (hipStream_t)stream, (const half_t *)y, slot_row, topk_ids,
                     (const half_t *)topk_w, (const half_t *)residual, (half_t *)out, top_k, H8, cblocks, (int)(T * top_k));
  return check_launch();
}
