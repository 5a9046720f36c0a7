// Device-side step of the INT4 paged KV cache's page tables (atom_kv_step_i4): what BatchedKvCacheInt4 builds on the host for
// every new token -- kv_indptr / kv_indices / last_page_offset of kv_i4.hip -- rebuilt in ONE launch from data that stays at fixed
// device addresses, so a captured decode step can be replayed for the next token.
//
//   page_table  i32 [batch, cap]   the pages RESERVED for each sequence, in order (read only)
//   row_pages   i32 [batch]        how many entries of each row are reserved pages (read only; clamped into 0 .. cap)
//   lens        i32 [2, batch]     the lengths, double-buffered: row state[1] & 1 is current, the launch writes the other row
//   state       i32 [4]            [0] status bits (ATOM_KV_STEP_OVERFLOW / _BAD_LENGTH, only ever set here), [1] parity of `lens`,
//                                  [2] arrival counter of the launch's workgroups (0 between launches), [3] unused
//
// Every sequence's new length is len + add unless that needs more than its row_pages pages: then it keeps its length and the overflow
// bit is set.  A length outside 0 .. row_pages * page_size (a corrupted buffer) is clamped into it and flagged, so no page count above
// a row's reserve and no index from outside a row ever reaches the tables.  The tables are rebuilt whole: kv_indptr is an exclusive prefix sum of the page
// counts, and a sequence that gains a page moves every later sequence's entries, so there is nothing to patch in place.
//
// Grid (groups of 64 sequences) x (slices of the copy).  A workgroup does not wait for any other: it sums the page counts of all
// sequences in front of its group itself (256 threads, wave64 shuffle reduction + LDS), wave 0 scans the group's own 64 counts
// (__shfl_up, 6 steps), then the four waves copy the group's rows, lane j of slice s taking entries s * 64 + j, + slices * 64, ...
// Why the lengths are double-buffered: every workgroup reads ALL current lengths while slice 0 of each group writes the new ones.  The
// last workgroup to arrive (one agent-scope atomic per workgroup, after its reads) flips the parity for the next launch; nothing in
// a launch ever reads what the same launch wrote.
//
// atom_kv_step_rows_i4 (speculative decoding) is the same kernel body with the count read per sequence from a device
// array `adds` and a look-ahead: `lens` receives the COMMITTED length len + adds[b], the tables are built for that length + lookahead.
// The slots behind the committed length are tentative -- a verify step writes K + 1 tokens there, the next launch commits the accepted
// ones and the rest is overwritten; there is no rollback and no negative count.
//
// atom_kv_step_ring_i4 (rolling cache of a sliding-window model) is the same kernel body again, with a row of the page
// table read as a RING: logical page g of sequence b (tokens g P .. g P + P - 1) lives in slot g % R, R = min(row_pages[b], cap).
// `lens` stays the absolute length.  For the new length n = len + add the live logical pages are f .. l,
//   f = max(0, n - max(add, 1) - W + 1) / P     the lowest key the oldest of the step's new rows still sees, floored to a page
//   l = (n - 1) / P                             the page of token n - 1
// and kv_indices lists them in LOGICAL order, dst[j] = row[(f + j) % R]; kv_start[b] = f P is the position of the list's first token
// (what the _ring attention entries take: prefill_i4.hip, kStart).  More than R live pages: the sequence is not advanced, overflow bit.
// Why a slot may be reused: the page that receives token n - 1 sits in slot l % R, and that slot's previous tenant was logical page
// l - R < f (l - f + 1 <= R), which is no longer listed -- no listed page is ever written over.  The bytes of that slot beyond n are
// the old tenant's, stale: they must never be read, and the attention kernels stop at the length (keys >= len are staged as zeros and
// not loaded); the append kernels write a token's slot before any launch reads it.
#include <type_traits>

#include "common.h"
#include "kv_attn.h"
#include "vocab_row.h"

namespace atom {

constexpr int kStepRows = 64;       // sequences per workgroup group: one lane each in the scan
constexpr int kStepThreads = 256;

struct KvStepParams {
  const int32_t *table, *rows;
  int32_t *lens, *indptr, *indices, *lpo, *state;
  int batch, cap, P, add;
  const int32_t *adds;   // atom_kv_step_rows_i4: the count per sequence instead of `add`
  int look;              // ... and the tentative slots behind the committed length that the tables cover too
};
// atom_kv_step_ring_i4: a block of its own, so that the other two kernels keep theirs byte for byte (the launch's implicit arguments,
// gridDim among them, sit behind the block)
struct KvRingParams : KvStepParams {
  int window;            // W >= 1
  int32_t *start;        // kv_start [batch]
};

// A sequence's new COMMITTED length (the return value, what goes into `lens`), the length its tables are built for (`tab`: the
// committed length + look) and its status bits; its reserve holds min(row_pages, cap) * P tokens.  If add + look does not fit the
// reserve, the whole request is refused: the sequence keeps its length and its tables are those of that length.
__device__ __forceinline__ int step_len(int len, int add, int look, int row_pages, int cap, int P, int &flag, int &tab) {
  const int maxlen = min(max(row_pages, 0), cap) * P;
  flag = 0;
  if (len < 0) { len = 0; flag = ATOM_KV_STEP_BAD_LENGTH; }
  if (len > maxlen) { len = maxlen; flag = ATOM_KV_STEP_BAD_LENGTH; }
  if (add < 0) { add = 0; flag |= ATOM_KV_STEP_BAD_LENGTH; }           // (a per-sequence count only: the scalar entry refuses it on the host)
  if (add > maxlen - len || look > maxlen - len - add) { flag |= ATOM_KV_STEP_OVERFLOW; return tab = len; }
  tab = len + add + look;
  return len + add;
}

// The ring step of one sequence (atom_kv_step_ring_i4): its new length (the return value), the first live logical page `f` and the
// count of live pages `cnt` its tables list, and its status bits; R = min(row_pages, cap) slots.  add >= 0 (the host refuses the rest).
// A request that needs more than R pages is refused: the sequence keeps its length and its tables are those of that length (the
// pages a step of 0 or 1 tokens to that length lists).  A stored length that R slots cannot describe at all (a corrupted buffer) is
// flagged and the list cut to its last R pages -- 0 with no slot: the sequence is then empty -- so cnt <= R whatever the buffers hold.
struct RingRow {
  int f, cnt;
};
__device__ __forceinline__ RingRow ring_pages(int n, int add, int W, int P) {
  if (n <= 0) return RingRow{0, 0};
  const int f = max(n - max(add, 1) - W + 1, 0) / P, l = (n - 1) / P;
  return RingRow{f, l - f + 1};
}
__device__ __forceinline__ int ring_len(int len, int add, int W, int row_pages, int cap, int P, int &flag, RingRow &pg) {
  const int R = min(max(row_pages, 0), cap);
  flag = 0;
  if (len < 0) { len = 0; flag = ATOM_KV_STEP_BAD_LENGTH; }
  if (len > 0x7fffffff - add) { len = 0x7fffffff - add; flag = ATOM_KV_STEP_BAD_LENGTH; }
  pg = ring_pages(len + add, add, W, P);
  if (pg.cnt <= R) return len + add;
  flag |= ATOM_KV_STEP_OVERFLOW;
  pg = ring_pages(len, 0, W, P);
  if (pg.cnt > R) {                                        // (the stored length itself is outside what the ring can hold)
    flag |= ATOM_KV_STEP_BAD_LENGTH;
    if (R == 0) { pg = RingRow{0, 0}; return 0; }
    pg.f += pg.cnt - R, pg.cnt = R;
  }
  return len;
}

template <bool RING>
struct RingLds {};
template <>
struct RingLds<true> {
  int rot[kStepRows], slots[kStepRows];                   // per sequence of the group: f % R and R
};

// ROWS: atom_kv_step_rows_i4 (p.adds, p.look); else the scalar step (p.add for every sequence, no look-ahead: tab == the new length)
// RING: atom_kv_step_ring_i4 (KvRingParams: p.window, p.start; never with ROWS) -- all of its code sits under `if constexpr (RING)`
template <bool ROWS, bool RING = false>
__global__ __launch_bounds__(kStepThreads) void kv_step_kernel(std::conditional_t<RING, KvRingParams, KvStepParams> p) {
  static_assert(!(ROWS && RING), "the ring step has no per-sequence counts");
  __shared__ int s_part[kStepThreads / 64];
  __shared__ int s_off[kStepRows], s_cnt[kStepRows];
  [[maybe_unused]] __shared__ RingLds<RING> s_ring;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int parity = p.state[1] & 1;
  const int32_t *cur = p.lens + (int64_t)parity * p.batch;
  int32_t *nxt = p.lens + (int64_t)(parity ^ 1) * p.batch;
  const int row0 = blockIdx.x * kStepRows;
  const int look = ROWS ? p.look : 0;
  const auto add_of = [&](int r) { return ROWS ? p.adds[r] : p.add; };

  // pages of every sequence in front of this group
  int acc = 0, flag, tab;
  [[maybe_unused]] RingRow pg{0, 0};
  for (int r = tid; r < row0; r += kStepThreads) {
    if constexpr (RING) {
      ring_len(cur[r], p.add, p.window, p.rows[r], p.cap, p.P, flag, pg);
      acc += pg.cnt;
    } else {
      step_len(cur[r], add_of(r), look, p.rows[r], p.cap, p.P, flag, tab);
      acc += (tab + p.P - 1) / p.P;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) s_part[wave] = acc;

  // the group's own sequences: one lane each, inclusive scan of the page counts over the wave
  const int row = row0 + lane;
  int len = 0, cnt = 0, inc = 0;
  flag = 0, tab = 0;
  if (wave == 0) {
    if constexpr (RING) {
      pg = RingRow{0, 0};
      int R = 0;
      if (row < p.batch) {
        len = ring_len(cur[row], p.add, p.window, p.rows[row], p.cap, p.P, flag, pg);
        cnt = pg.cnt, tab = len;                            // (no look-ahead: the tables are those of the new length)
        R = min(max(p.rows[row], 0), p.cap);
      }
      s_ring.rot[lane] = R > 0 ? pg.f % R : 0;
      s_ring.slots[lane] = R;
    } else if (row < p.batch) {
      len = step_len(cur[row], add_of(row), look, p.rows[row], p.cap, p.P, flag, tab);
      cnt = (tab + p.P - 1) / p.P;
    }
    inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    s_off[lane] = inc - cnt;
    s_cnt[lane] = cnt;
  }
  __syncthreads();
  const int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];

  if (wave == 0 && blockIdx.y == 0 && row < p.batch) {
    nxt[row] = len;
    p.lpo[row] = tab > 0 ? (tab - 1) % p.P + 1 : 0;       // an empty sequence: no page, offset 0 (what the attention ops skip)
    p.indptr[row + 1] = base + inc;
    if (row == 0) p.indptr[0] = 0;
    if constexpr (RING) p.start[row] = pg.f * p.P;        // (f P <= len: no overflow)
    if (flag) atomicOr(&p.state[0], flag);
  }

  // compaction: the first cnt entries of each row (cnt <= cap: the reads stay inside the row, the writes below batch * cap)
  const int rows_here = min(kStepRows, p.batch - row0);
  const int stride = gridDim.y * 64;
  for (int r = wave; r < rows_here; r += kStepThreads / 64) {
    const int n = s_cnt[r];
    const int32_t *src = p.table + (int64_t)(row0 + r) * p.cap;
    int32_t *dst = p.indices + base + s_off[r];
    if constexpr (RING) {                                   // logical order: entry j is slot (f + j) % R; j < n <= R <= cap
      const int rot = s_ring.rot[r], R = s_ring.slots[r];
      for (int j = blockIdx.y * 64 + lane; j < n; j += stride) dst[j] = src[rot + j - (rot + j >= R ? R : 0)];
    } else {
      for (int j = blockIdx.y * 64 + lane; j < n; j += stride) dst[j] = src[j];
    }
  }

  // arrival: this workgroup has read everything it needs of the current lengths (their values went into LDS in front of the barrier
  // above).  No data passes between workgroups inside a launch, so the counter needs no fence (an agent-scope fence costs microseconds
  // here): it only tells the last workgroup that nobody reads the parity any more; its two stores are for the NEXT launch.
  if (tid == 0) {
    const int total = gridDim.x * gridDim.y;
    if (__hip_atomic_fetch_add(&p.state[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1) {
      __hip_atomic_store(&p.state[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      p.state[1] = parity ^ 1;
    }
  }
}

// slices of the copy (gridDim.y)
static int step_slices(int batch, int cap) {
  // a slice is 64 entries of every row per pass; enough slices that a workgroup makes at most 4 passes over a row, at most 16,
  // and no more than 1024 workgroups in all
  const int groups = (batch + kStepRows - 1) / kStepRows;
  int s = (cap + 255) / 256;
  s = s > 16 ? 16 : s;
  while (s > 1 && (int64_t)s * groups > 1024) --s;
  return s;
}

// the checks all entries share (`adds`: null for the scalar entries; ring: window and kv_start too), then the launch
static int kv_step(KvRingParams p, bool rows, hipStream_t stream, bool ring = false) {
  if (!p.table || !p.rows || !p.lens || !p.indptr || !p.indices || !p.lpo || !p.state || (rows && !p.adds)) return ATOM_ERR_INVALID_ARG;
  if (p.add < 0 || p.look < 0) return ATOM_ERR_INVALID_ARG;
  if (ring && (p.window < 1 || !p.start)) return ATOM_ERR_INVALID_ARG;
  if (p.batch < 1 || p.cap < 1 || p.P < 16 || (p.P % 16) != 0) return ATOM_ERR_SHAPE;
  if ((int64_t)p.cap * p.P > 0x7fffffff || (int64_t)p.batch * p.cap > 0x7fffffff) return ATOM_ERR_SHAPE;
  for (const void *q : {(const void *)p.table, (const void *)p.rows, (const void *)p.lens, (const void *)p.indptr, (const void *)p.indices,
                        (const void *)p.lpo, (const void *)p.state, (const void *)p.adds, (const void *)p.start})
    if (off_by(q, 3u)) return ATOM_ERR_ALIGN;
  const dim3 grid((unsigned)((p.batch + kStepRows - 1) / kStepRows), (unsigned)step_slices(p.batch, p.cap));
  if (ring) hipLaunchKernelGGL((kv_step_kernel<false, true>), grid, dim3(kStepThreads), 0, stream, p);
  else if (rows) hipLaunchKernelGGL(kv_step_kernel<true>, grid, dim3(kStepThreads), 0, stream, static_cast<const KvStepParams &>(p));
  else hipLaunchKernelGGL(kv_step_kernel<false>, grid, dim3(kStepThreads), 0, stream, static_cast<const KvStepParams &>(p));
  return check_launch();
}

}  // namespace atom

using namespace atom;

extern "C" {

int atom_kv_step_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                    int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, int add, void *stream) {
  return kv_step(KvRingParams{{page_table, row_pages, lens, kv_indptr, kv_indices, last_page_offset, state, batch, cap, page_size, add, nullptr, 0}, 0, nullptr},
                 false, reinterpret_cast<hipStream_t>(stream));
}

int atom_kv_step_rows_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                         int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, const int32_t *adds, int lookahead,
                         void *stream) {
  return kv_step(KvRingParams{{page_table, row_pages, lens, kv_indptr, kv_indices, last_page_offset, state, batch, cap, page_size, 0, adds, lookahead}, 0, nullptr},
                 true, reinterpret_cast<hipStream_t>(stream));
}

int atom_kv_step_ring_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                         int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, int add, int window,
                         int32_t *kv_start, void *stream) {
  return kv_step(KvRingParams{{page_table, row_pages, lens, kv_indptr, kv_indices, last_page_offset, state, batch, cap, page_size, add, nullptr, 0},
                              window, kv_start},
                 false, reinterpret_cast<hipStream_t>(stream), true);
}

}  // extern "C"
