// The routed ("grouped") GEMM of the sparse mixture-of-experts block on MX operands (contract: include/atom_hip.h, "Sparse mixture of
// experts on MXFP4"; design: DESIGN.md 4.27).  The router, its tables and the combine are those of moe_w4a4.hip; this file is the
// kernel between them on v_mfma_scale_f32_16x16x128_f8f6f4, which applies the E8M0 scales itself: no de-quantisation behind the MFMA.
//
//   moe_gemm_mxfp4_kernel  workgroup = one router tile (up to 64 routed rows of one expert) x 64 features, 4 waves.
//     * wave w owns weight fragment w of the 64 features (16 features, 1 KiB per K step).  Nobody else reads it, so it goes from global
//       memory straight into VGPRs: a register ring of DW steps, 16 bytes + one scale byte per lane and step, never through LDS.
//     * the tile's (up to) four activation fragments are shared by the four waves: an LDS ring of NS stages filled by LDS-DMA, wave w
//       staging fragment w.  Every lane gives its OWN global address -- the source row of routed row row0 + 16 w + l % 16, block l / 16 --
//       so the gather through row_index is part of the address and costs nothing in the loop.  The lane's scale byte comes with a 2-byte
//       piece from the even address at or below it (zero-extended to the lane's dword of the stage); the LDS read picks the byte.
//     * a tile with fewer than 64 live rows has ceil(live / 16) live fragments (uniform over the workgroup): the waves of the dead ones
//       stage nothing and nobody multiplies them -- at decode a K step is one MFMA per wave.
//     * the keeper (MXFP8, one more K step with format code 0) is requested first, outside the rings: both halves of the weight
//       fragment into 8 registers, the activation halves into their own 8 KiB of LDS.
//   Every output element is one MFMA accumulation chain: K steps 0 .. S - 1 in order, then the keeper -- gemm_mxfp4_tile_kernel's chain,
//   so the bits of a row do not depend on its tile, its expert's row count or the gather.
#include "common.h"

namespace atom {
namespace moemx {

typedef int v8i_t __attribute__((ext_vector_type(8)));

constexpr int FMT_E2M1 = 4, FMT_E4M3 = 0;
constexpr int BN = 64, NW = 4, NT = NW * 64;
constexpr int DA = 4, NS = DA + 1;   // activation stages in flight; ring slots (the slot refilled in step s is the one read in step s - 1)
constexpr int DW = 8;                // weight steps in the register ring
constexpr int FRAG = 1024;
constexpr int SC_OFF = 4 * FRAG;     // 4 fragments x 64 lanes x a dword that holds the lane's scale byte and its even/odd neighbour
constexpr int STAGE = SC_OFF + 4 * 256;
constexpr int K8_OFF = NS * STAGE;   // keeper: [half][fragment] 1 KiB each, then its scale dwords
constexpr int K8_SC = K8_OFF + 8 * FRAG;
constexpr int LDS_BYTES = K8_SC + 4 * 256;
// requests a wave with a live fragment issues behind the two pieces of a stage before it waits for them: the weight refill of that step
// (fragment + scale byte), then DA - 1 whole steps of two pieces + two loads.  The prologue puts at least as many behind its stages.
constexpr int WAIT = 2 + 4 * (DA - 1);
static_assert(DW >= DA && WAIT < 64 && LDS_BYTES <= 64 * 1024, "ring depths");

struct Args {
  const uint8_t *a4, *asc, *a8, *w4, *wsc, *w8;
  const int32_t *row_index, *expert_indptr, *tile_expert, *tile_row0, *n_tiles;
  half_t *out[2];
  int R, E, N, N_seg, S, A_rows, max_tiles;
};

__device__ __forceinline__ v8i_t frag4(v4i f) { return v8i_t{f.x, f.y, f.z, f.w, 0, 0, 0, 0}; }
__device__ __forceinline__ v8i_t frag8(v4i f, v4i g) { return v8i_t{f.x, f.y, f.z, f.w, g.x, g.y, g.z, g.w}; }

__global__ __launch_bounds__(NT) void moe_gemm_mxfp4_kernel(Args p) {
  __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __builtin_assume(w >= 0 && w < NW);
  const int nt = min(max(*p.n_tiles, 0), p.max_tiles), nbn = p.N / BN;
  int id = blockIdx.x;
  {                                                        // workgroup b runs on XCD b % 8: every XCD takes a contiguous run of the nt x nbn
    const int nwg = nt * nbn;                              // live tiles, row tiles fastest (moe_gemm_w4a4_kernel's remap): the tiles of an
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7, k = id >> 3;   // expert that share a weight fragment share an L2.  The grid is sized
    if (k >= (xcd < r ? q + 1 : q)) return;                // for the worst routing: the rest leave before touching memory
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int tile = id % nt, n0 = (id / nt) * BN;
  const int e = __builtin_amdgcn_readfirstlane(p.tile_expert[tile]);
  const int row0 = __builtin_amdgcn_readfirstlane(p.tile_row0[tile]);
  if ((unsigned)e >= (unsigned)p.E) return;                // (a table the router did not write: never an address from it)
  const int rend = min(__builtin_amdgcn_readfirstlane(p.expert_indptr[e + 1]), p.R);
  if (row0 < 0 || row0 >= rend) return;
  const int S = p.S, T = S + 1;
  const int nf = (min(rend - row0, 64) + 15) >> 4;         // live activation fragments, 1 .. 4
  const bool live = w < nf;                                // this wave stages one

  // ---- loop invariant, per lane: the source row of each fragment's routed row l % 16 (clamped like the INT4 kernel's), the parity of
  // its scale byte's address, and for fragment w the offsets of the lane's 16 code bytes / its scale byte in the operand
  unsigned par[4], mine = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = min(row0 + 16 * i + (l & 15), rend - 1);
    const unsigned src = min((unsigned)(p.row_index ? p.row_index[r] : r), (unsigned)(p.A_rows - 1));
    par[i] = src & 1u;                                     // (a row tile's scale bytes start at a multiple of 64, a block's at 16 b)
    if (i == w) mine = src;
  }
  const unsigned lane_in = (mine & 15u) + (unsigned)(l >> 4) * 16u;
  unsigned voff = (mine >> 4) * (unsigned)S * 1024u + lane_in * 16u;
  unsigned kvoff = (mine >> 4) * 2048u + lane_in * 16u;
  unsigned svoff = ((mine >> 4) * (unsigned)T * 64u + lane_in) & ~1u;
  // the table reads are done: from here on vmcnt counts the rings' requests only
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(voff), "+v"(kvoff), "+v"(svoff), "+v"(par[0]), "+v"(par[1]), "+v"(par[2]), "+v"(par[3])::"memory");

  const int64_t wf = (int64_t)e * (p.N >> 4) + (n0 >> 4) + w;      // the wave's weight fragment row of the stacked operand
  const uint8_t *wq = p.w4 + wf * S * FRAG + l * 16, *wsc = p.wsc + wf * T * 64 + l, *wk = p.w8 + wf * 2 * FRAG + l * 16;
  const unsigned lds0 = lds_addr(lds);
  auto stage = [&](int st, int slot) {                     // (past the end: the last step again into a dead slot, which keeps the count)
    if (live) {
      const int s = min(st, S - 1);
      lds_dma_sv<16>(p.a4 + (int64_t)s * FRAG, voff, lds0 + (unsigned)(slot * STAGE + w * FRAG));
      lds_dma_sv<2>(p.asc + (int64_t)s * 64, svoff, lds0 + (unsigned)(slot * STAGE + SC_OFF + w * 256));
    }
  };
  // the keeper first: whatever is waited for later has it behind it
  if (live) {
    lds_dma_sv<16>(p.a8, kvoff, lds0 + (unsigned)(K8_OFF + w * FRAG));
    lds_dma_sv<16>(p.a8 + FRAG, kvoff, lds0 + (unsigned)(K8_OFF + (4 + w) * FRAG));
    lds_dma_sv<2>(p.asc + (int64_t)S * 64, svoff, lds0 + (unsigned)(K8_SC + w * 256));
  }
  const v4i kw0 = *reinterpret_cast<const v4i *>(wk), kw1 = *reinterpret_cast<const v4i *>(wk + FRAG);
  const int ksw = wsc[S * 64];
#pragma unroll
  for (int s = 0; s < DA; ++s) stage(s, s);
  v4i wr[DW];
  int ws[DW];
#pragma unroll
  for (int u = 0; u < DW; ++u) {
    const int s = min(u, S - 1);
    wr[u] = *reinterpret_cast<const v4i *>(wq + (int64_t)s * FRAG);
    ws[u] = wsc[s * 64];
  }
  __builtin_amdgcn_sched_barrier(0);

  v4f acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
  const int afrag = l * 16, asc0 = SC_OFF + l * 4;

  int slot = 0, dslot = DA;                                // ring positions of the stage computed / requested in this step
  for (int st0 = 0; st0 < S; st0 += DW) {
#pragma unroll
    for (int u = 0; u < DW; ++u) {                         // (unrolled over the register ring: static slots)
      const int st = st0 + u;
      if (st >= S) break;
      // this wave's pieces of stage st have landed, its reads of the slot about to be refilled are done; the barrier: everybody's
      if (live) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WAIT) : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stage(st + DA, dslot);
      __builtin_amdgcn_sched_barrier(0);
      const char *sl = lds + slot * STAGE;
      const v8i_t fw = frag4(wr[u]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nf) {
          const v8i_t fa = frag4(*reinterpret_cast<const v4i *>(sl + i * FRAG + afrag));
          const int sa = *reinterpret_cast<const uint8_t *>(sl + asc0 + i * 256 + par[i]);
          acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa, acc[i], FMT_E2M1, FMT_E2M1, 0, ws[u], 0, sa);
        }
      __builtin_amdgcn_sched_barrier(0);
      {                                                    // the slot's next tenant, DW steps ahead
        const int s = min(st + DW, S - 1);
        wr[u] = *reinterpret_cast<const v4i *>(wq + (int64_t)s * FRAG);
        ws[u] = wsc[s * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      slot = slot + 1 == NS ? 0 : slot + 1;
      dslot = dslot + 1 == NS ? 0 : dslot + 1;
    }
  }
  // the keeper: one more step of the same chain.  Nothing may still be on its way into LDS when the workgroup ends, either
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  {
    const v8i_t fw = frag8(kw0, kw1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nf) {
        const char *k0 = lds + K8_OFF + i * FRAG + afrag;
        const v8i_t fa = frag8(*reinterpret_cast<const v4i *>(k0), *reinterpret_cast<const v4i *>(k0 + 4 * FRAG));
        const int sa = *reinterpret_cast<const uint8_t *>(lds + K8_SC + i * 256 + l * 4 + par[i]);
        acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa, acc[i], FMT_E4M3, FMT_E4M3, 0, ksw, 0, sa);
      }
  }
  // lane l: routed row l % 16 of fragment i, features 4 (l / 16) .. + 3 of the wave's 16: one 8-byte store into the tile's segment
  const int seg = n0 >= p.N_seg ? 1 : 0;
  half_t *ob = p.out[seg] + (n0 - seg * p.N_seg) + 16 * w + 4 * (l >> 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = row0 + 16 * i + (l & 15);
    if (i < nf && m < rend) {
      const half_t h[4] = {(half_t)acc[i][0], (half_t)acc[i][1], (half_t)acc[i][2], (half_t)acc[i][3]};
      *reinterpret_cast<v2u *>(ob + (int64_t)m * p.N_seg) = __builtin_bit_cast(v2u, h);
    }
  }
}

}  // namespace moemx
}  // namespace atom

using namespace atom;

extern "C" int64_t atom_moe_max_tiles(int64_t R, int E);

extern "C" int atom_moe_gemm_mxfp4_f16(const void *a_q4, const void *a_sc, const void *a_q8, const void *w_q4, const void *w_sc, const void *w_q8,
                                       const int32_t *row_index, const int32_t *expert_indptr, const int32_t *tile_expert,
                                       const int32_t *tile_row0, const int32_t *n_tiles, void *out0, void *out1, int64_t A_rows, int64_t R,
                                       int E, int64_t N_seg, int nseg, int64_t K, void *stream) {
  auto aligned4 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; };
  if (!a_q4 || !a_sc || !a_q8 || !w_q4 || !w_sc || !w_q8 || !expert_indptr || !tile_expert || !tile_row0 || !n_tiles || !out0)
    return ATOM_ERR_INVALID_ARG;
  if (nseg < 1 || nseg > 2 || (nseg == 2 && !out1)) return ATOM_ERR_INVALID_ARG;
  if (E < 1 || E > 64 || R < 1 || R >= (int64_t(1) << 31) || A_rows < 1 || A_rows > (1 << 24)) return ATOM_ERR_SHAPE;
  if (N_seg < 64 || (N_seg % 64) != 0 || N_seg > (1 << 24)) return ATOM_ERR_SHAPE;
  if (K < 256 || (K % 128) != 0 || K > (1 << 20)) return ATOM_ERR_SHAPE;
  const int64_t N = N_seg * nseg, S = K / 128 - 1, Ra = (A_rows + 15) / 16;
  if (Ra * S * 1024 >= (int64_t(1) << 32)) return ATOM_ERR_SHAPE;   // 32-bit lane offsets into the activation operand
  const int64_t max_tiles = atom_moe_max_tiles(R, E);
  if (max_tiles * (N / 64) >= (int64_t(1) << 31)) return ATOM_ERR_SHAPE;
  if (!aligned16(a_q4) || !aligned16(a_sc) || !aligned16(a_q8) || !aligned16(w_q4) || !aligned16(w_sc) || !aligned16(w_q8) || !aligned16(out0) ||
      (out1 && !aligned16(out1)))
    return ATOM_ERR_ALIGN;
  if ((row_index && !aligned4(row_index)) || !aligned4(expert_indptr) || !aligned4(tile_expert) || !aligned4(tile_row0) || !aligned4(n_tiles))
    return ATOM_ERR_ALIGN;
  moemx::Args p;
  p.a4 = (const uint8_t *)a_q4; p.asc = (const uint8_t *)a_sc; p.a8 = (const uint8_t *)a_q8;
  p.w4 = (const uint8_t *)w_q4; p.wsc = (const uint8_t *)w_sc; p.w8 = (const uint8_t *)w_q8;
  p.row_index = row_index; p.expert_indptr = expert_indptr; p.tile_expert = tile_expert; p.tile_row0 = tile_row0; p.n_tiles = n_tiles;
  p.out[0] = (half_t *)out0; p.out[1] = (half_t *)(nseg == 2 ? out1 : out0);
  p.R = (int)R; p.E = E; p.N = (int)N; p.N_seg = (int)N_seg; p.S = (int)S; p.A_rows = (int)A_rows; p.max_tiles = (int)max_tiles;
  hipLaunchKernelGGL(moemx::moe_gemm_mxfp4_kernel, dim3((unsigned)(max_tiles * (N / 64))), dim3(moemx::NT), 0, (hipStream_t)stream, p);
  return check_launch();
}
