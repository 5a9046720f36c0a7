// Beam search on the device: atom_beam_select picks the next beams of every prompt group from the per-row top-n of
// atom_logprob_f16, atom_kv_beam_fork_i4 makes row r of a static INT4 paged cache continue row parent[r]'s history.  Both are one
// launch, read nothing back and are capturable; neither touches an attention or GEMM kernel.
//
// ---- atom_beam_select: one workgroup of 256 threads per group, no workgroup reads what another writes.
// A group has at most 16 x 32 = 512 candidates: thread t holds the order words (beam_math.h) of candidates t and t + 256 in two
// registers.  A round is a workgroup maximum (wave64 shuffles, then 4 words in LDS); the owner of the winner zeroes its register;
// thread i keeps round i's winner and writes output i at the end.  Every global input is read before the first barrier into LDS or
// registers and every output is written after the last round, so an output may be the input of the same name (w_in == w_out).
//
// ---- atom_kv_beam_fork_i4: grid (row, slice of the page copy).  With L the row's length, full = L / P, off = L % P and
// p = the row's parent (same group):
//   j < full               out[r][j] = in[p][j]      full pages are immutable, shared by reference
//   j == full, off > 0     p == r: in[r][j];  else the page in[p][j] is copied into page spare[r], out[r][j] = spare[r] and
//                          spare[r] becomes in[r][j]
//   later j                out[r][j] = in[r][j]      the row's own untouched reserve
// Ownership.  Before a launch every partial page and every reserve page is in exactly one row, and no table holds a spare.  A row that
// copies takes its spare into the table and retires its own old partial page -- which no other row held -- as its new spare; a row that
// is its own parent changes nothing.  So afterwards no partial page is referenced by two rows again: the 2-cycle r <-> p swaps two
// histories through the two spares, and "everyone takes parent 0" leaves row 0 alone and gives every other row a copy.
// Races.  The only page a workgroup writes is spare[r]; a page another workgroup READS is in a table, and spares are in no table.
// Table rows are read by other rows' workgroups, and spare[r] is read by every slice of row r: so the launch gathers from table_in /
// spare_in and writes table_out / spare_out, which must not overlap them; the caller copies back on the same stream.  It writes no
// length (the double-buffered `lens` of atom_kv_step_i4 are read at the current parity).
// Safety.  A parent is compared with 0 and w before it becomes an index: a bad one keeps the row and sets ATOM_KV_BEAM_BAD_PARENT.  A
// length outside the row's reserve is clamped and flagged as atom_kv_step_i4 does.  A page id outside the pool (a corrupted table)
// is never used as an address: the copy is skipped and ATOM_KV_BEAM_BAD_PAGE set.  Every id written comes from table_in or spare_in.
// The stale tail of a copied page is harmless: attention reads up to last_page_offset.
#include "common.h"
#include "beam_math.h"
#include "vocab_row.h"
#include "kv_attn.h"

namespace atom {

constexpr int kBeamThreads = 256;

struct BeamSelectParams {
  const int64_t *top_ids;
  const float *top_lp, *cum;
  const int32_t *finished, *length;
  int32_t *parent;
  int64_t *token;
  float *cum_out;
  int32_t *finished_out, *length_out;
  int w_in, w_out, C;
  int64_t eos;
};

__global__ __launch_bounds__(kBeamThreads) void beam_select_kernel(BeamSelectParams p) {
  __shared__ float s_cum[beam::kMaxBeams];
  __shared__ int s_fin[beam::kMaxBeams], s_len[beam::kMaxBeams];
  __shared__ unsigned long long s_best[kBeamThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * p.w_in;
  if (tid < p.w_in) {
    s_cum[tid] = p.cum[row0 + tid];
    s_fin[tid] = p.finished[row0 + tid] != 0;
    s_len[tid] = p.length[row0 + tid];
  }
  __syncthreads();

  // candidate idx = b * C + c: a live row has C of them, a finished row the one at c == 0
  const int total = p.w_in * p.C;
  unsigned long long word[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int idx = tid + k * kBeamThreads;
    word[k] = 0;
    if (idx < total) {
      const int b = idx / p.C, c = idx - b * p.C;
      if (!s_fin[b]) word[k] = beam::order_word(beam::score_key(beam::score(s_cum[b], p.top_lp[(row0 + b) * p.C + c])), idx);
      else if (c == 0) word[k] = beam::order_word(beam::score_key(s_cum[b]), idx);
    }
  }

  unsigned long long mine = 0;
  for (int round = 0; round < p.w_out; ++round) {
    unsigned long long m = word[0] > word[1] ? word[0] : word[1];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned hi = __shfl_xor((unsigned)(m >> 32), d, 64), lo = __shfl_xor((unsigned)m, d, 64);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      m = o > m ? o : m;
    }
    if (lane == 0) s_best[wave] = m;
    __syncthreads();
    unsigned long long best = s_best[0];
#pragma unroll
    for (int k = 1; k < kBeamThreads / 64; ++k) best = s_best[k] > best ? s_best[k] : best;
    if (best != 0) {                                         // words are distinct: exactly one register holds the winner
      if (word[0] == best) word[0] = 0;
      if (word[1] == best) word[1] = 0;
    }
    if (tid == round) mine = best;
    __syncthreads();
  }

  if (tid < p.w_out) {
    const int64_t o = (int64_t)blockIdx.x * p.w_out + tid;
    const int64_t frozen = p.eos < 0 ? 0 : p.eos;            // the token a finished row repeats (never a negative id)
    if (mine == 0) {                                         // fewer candidates than w_out (w_in == 1 with a finished row): padding
      p.parent[o] = 0, p.token[o] = frozen, p.cum_out[o] = -INFINITY, p.finished_out[o] = 1, p.length_out[o] = s_len[0];
    } else {
      const int idx = (int)beam::word_index(mine);
      const int b = idx / p.C, c = idx - b * p.C;
      p.parent[o] = b;
      if (s_fin[b]) {
        p.token[o] = frozen, p.cum_out[o] = s_cum[b], p.finished_out[o] = 1, p.length_out[o] = s_len[b];
      } else {
        const int64_t t = p.top_ids[(row0 + b) * p.C + c];
        p.token[o] = t;
        p.cum_out[o] = beam::score(s_cum[b], p.top_lp[(row0 + b) * p.C + c]);
        p.finished_out[o] = (p.eos >= 0 && t == p.eos) ? 1 : 0;
        p.length_out[o] = s_len[b] + 1;
      }
    }
  }
}

struct BeamForkParams {
  uint8_t *data, *param;
  const int32_t *table_in, *spare_in, *rows, *lens, *parent;
  int32_t *table_out, *spare_out, *state;
  int batch, w, cap, P;
  int64_t capacity, data_vecs, param_vecs;                   // pages of the pool; 16-byte vectors per page of each pool buffer
};

__global__ __launch_bounds__(kBeamThreads) void kv_beam_fork_kernel(BeamForkParams q) {
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int32_t *in_r = q.table_in + (int64_t)r * q.cap;
  int flag = 0;
  // the row's length, clamped into its reserve as atom_kv_step_i4 clamps it
  const int maxlen = min(max(q.rows[r], 0), q.cap) * q.P;
  int len = q.lens[(int64_t)(q.state[1] & 1) * q.batch + r];
  if (len < 0) { len = 0; flag = ATOM_KV_STEP_BAD_LENGTH; }
  if (len > maxlen) { len = maxlen; flag = ATOM_KV_STEP_BAD_LENGTH; }
  const int full = len / q.P, off = len - full * q.P;        // off > 0 implies full < cap
  // the parent: compared before it becomes an index
  const int par = q.parent[r];
  int p = r;
  if (par < 0 || par >= q.w) flag |= ATOM_KV_BEAM_BAD_PARENT;
  else p = r - r % q.w + par;                                // batch is a multiple of w: p < batch
  const int32_t *in_p = q.table_in + (int64_t)p * q.cap;

  bool copy = off > 0 && p != r;
  int src = 0, dst = 0;
  if (copy) {
    src = in_p[full], dst = q.spare_in[r];
    if (src < 0 || src >= q.capacity || dst < 0 || dst >= q.capacity || src == dst) {
      copy = false, p = r, flag |= ATOM_KV_BEAM_BAD_PAGE;    // keep the row as it is
      in_p = in_r;
    }
  }

  if (blockIdx.y == 0) {
    int32_t *out_r = q.table_out + (int64_t)r * q.cap;
    for (int j = tid; j < q.cap; j += kBeamThreads) out_r[j] = j < full ? in_p[j] : (copy && j == full ? dst : in_r[j]);
    if (tid == 0) {
      q.spare_out[r] = copy ? in_r[full] : q.spare_in[r];
      if (flag) atomicOr(&q.state[0], flag);
    }
  }
  if (!copy) return;

  // the partial page: both pool buffers hold a page as one contiguous run (all layers, K and V, all heads)
  const v4u *sd = reinterpret_cast<const v4u *>(q.data) + (int64_t)src * q.data_vecs;
  v4u *dd = reinterpret_cast<v4u *>(q.data) + (int64_t)dst * q.data_vecs;
  const v4u *sp = reinterpret_cast<const v4u *>(q.param) + (int64_t)src * q.param_vecs;
  v4u *dp = reinterpret_cast<v4u *>(q.param) + (int64_t)dst * q.param_vecs;
  const int64_t stride = (int64_t)gridDim.y * kBeamThreads;
  for (int64_t i = (int64_t)blockIdx.y * kBeamThreads + tid; i < q.data_vecs; i += stride) dd[i] = sd[i];
  for (int64_t i = (int64_t)blockIdx.y * kBeamThreads + tid; i < q.param_vecs; i += stride) dp[i] = sp[i];
}

// slices of the page copy (gridDim.y): about 16 vectors of 16 bytes per thread, at most 128 slices
static int fork_slices(int64_t vecs) {
  const int64_t s = (vecs + kBeamThreads * 16 - 1) / (kBeamThreads * 16);
  return (int)(s < 1 ? 1 : (s > 128 ? 128 : s));
}

static bool overlap(const void *a, const void *b, int64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_beam_select(const int64_t *top_ids, const float *top_lp, const float *cum, const int32_t *finished, const int32_t *length,
                     int64_t groups, int w_in, int w_out, int C, int64_t eos, int32_t *parent, int64_t *token, float *cum_out,
                     int32_t *finished_out, int32_t *length_out, void *stream) {
  if (!top_ids || !top_lp || !cum || !finished || !length || !parent || !token || !cum_out || !finished_out || !length_out)
    return ATOM_ERR_INVALID_ARG;
  if (groups < 1 || groups > 0x7fffffff / (beam::kMaxBeams * beam::kMaxCand)) return ATOM_ERR_SHAPE;
  if (w_out < 1 || w_out > beam::kMaxBeams || (w_in != 1 && w_in != w_out) || C < w_out || C > beam::kMaxCand) return ATOM_ERR_SHAPE;
  for (const void *q : {(const void *)top_ids, (const void *)token})
    if (off_by(q, 7u)) return ATOM_ERR_ALIGN;
  for (const void *q : {(const void *)top_lp, (const void *)cum, (const void *)finished, (const void *)length, (const void *)parent,
                        (const void *)cum_out, (const void *)finished_out, (const void *)length_out})
    if (off_by(q, 3u)) return ATOM_ERR_ALIGN;
  BeamSelectParams p{top_ids, top_lp, cum, finished, length, parent, token, cum_out, finished_out, length_out, w_in, w_out, C, eos};
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)groups), dim3(kBeamThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  return check_launch();
}

int atom_kv_beam_fork_i4(void *kv_data, void *kv_param, const int32_t *table_in, int32_t *table_out, const int32_t *spare_in,
                         int32_t *spare_out, const int32_t *row_pages, const int32_t *lens, int32_t *state, const int32_t *parent,
                         int batch, int w, int cap, int64_t capacity, int num_layers, int num_heads, int page_size, int head_dim,
                         void *stream) {
  if (!row_pages || !lens || !state || !parent || !spare_in || !spare_out) return ATOM_ERR_INVALID_ARG;
  if (const int st = check_kv(kv_data, kv_param, table_in, table_out, spare_in, batch, num_layers, 0, num_heads, page_size, head_dim))
    return st;
  if (w < 1 || w > beam::kMaxBeams || batch % w != 0 || cap < 1 || capacity < 1 || capacity > 0x7fffffff) return ATOM_ERR_SHAPE;
  if ((int64_t)cap * page_size > 0x7fffffff || (int64_t)batch * cap > 0x7fffffff) return ATOM_ERR_SHAPE;
  if (!aligned16(kv_param)) return ATOM_ERR_ALIGN;
  for (const void *q : {(const void *)table_in, (const void *)table_out, (const void *)spare_in, (const void *)spare_out,
                        (const void *)row_pages, (const void *)lens, (const void *)state, (const void *)parent})
    if (off_by(q, 3u)) return ATOM_ERR_ALIGN;
  // the launch gathers from rows that other workgroups own: it must not write what it reads
  if (overlap(table_in, table_out, (int64_t)batch * cap * 4) || overlap(spare_in, spare_out, (int64_t)batch * 4)) return ATOM_ERR_INVALID_ARG;
  const int64_t slots = (int64_t)num_layers * 2 * num_heads * page_size;          // (layer, K/V, head, token) per page
  BeamForkParams q{(uint8_t *)kv_data, (uint8_t *)kv_param, table_in, spare_in, row_pages, lens, parent, table_out, spare_out, state,
                   batch, w, cap, page_size, capacity, slots * (head_dim / 2) / 16, slots * 4 / 16};
  const dim3 grid((unsigned)batch, (unsigned)fork_slices(q.data_vecs + q.param_vecs));
  hipLaunchKernelGGL(kv_beam_fork_kernel, grid, dim3(kBeamThreads), 0, reinterpret_cast<hipStream_t>(stream), q);
  return check_launch();
}

}  // extern "C"
