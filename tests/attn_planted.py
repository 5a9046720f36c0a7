"""Planted inputs and FP64 references for the paged INT4 attention ops (atom_batch_decode_i4, atom_batch_decode_gqa_i4,
atom_batch_prefill_i4, atom_batch_prefill_gqa_i4), shared by tests/test_attn_planted_cpu.py and tests/test_gpu_attn_planted.py.
numpy only: importable without torch and without a GPU.

Why: with uniform random cache bytes and positive (scale, zero) the softmax is spread over hundreds of keys and every output row is
close to the mean value vector -- one lost key, one position off by one or one wrong head moves the output less than the ops' bound.
Two input families make single errors large:

  membership  every key de-quantises to exactly 0 (nibble 8, scale 1, zero 8): the softmax is exactly uniform, whatever RoPE does.
              Values are 0 (codes 0, scale 1, zero 0) except in a window of 128 positions [w, w + 128): token w + d has code 15 in
              dimension d alone, with an fp16 scale s drawn per (token, K/V head) from [32, 64).  Output = 15 s / S in one dimension
              per window token the row can see: a dropped key zeroes a dimension, a doubled key doubles it, another K/V head gives
              another magnitude.  The slots behind a sequence's end and every page nobody owns carry the hot pattern at scale 64;
              the other layer holds random bytes.
  needle      random codes, centred (zero = 8 scale, fp16 scale in [0.125, 0.25]): zero-mean keys and values; queries N(0, 1) * a
              (NEEDLE_A): logits with a standard deviation of ~2.5, a softmax that a few keys dominate -- sensitive to every
              position, frequency and page.

The references take ``mutate={name: argument}``: exactly ONE deliberate error (MUTANTS).  The CPU test shows that each mutant leaves
the correct reference by at least 10 x the bound that the GPU test applies to the kernels; the GPU test compares the kernels with the
unmutated reference.

The bound is the ops' existing formula (decode 2e-3 max|ref| + 1e-3, prefill and GQA 4e-3 max|ref| + 1e-3) taken per (query row,
head) instead of once per call: a call holds sequences of 1 and of 2100 tokens, and the membership outputs scale with 1 / S -- a
per-call maximum would come from the one-token sequence and leave the long one unchecked.  Per row and head is never wider."""
import numpy as np

from oracle import atom_oracle as O

D = 128
LAYERS, LAYER = 2, 1                     # the caches have two layers; the ops run on layer 1
WINDOW = 128

MUTANTS = ("drop_key", "double_key", "causal_plus_one", "q_pos_minus_one", "key_pos_plus_one", "theta", "ignore_rope_scale",
           "interleaved_pairs", "swap_pages", "head_mod", "other_layer", "read_past_end")

# ------------------------------------------------------------------------------------------------ the cases both test files run
LENS16 = [1, 15, 16, 17, 300, 2100]
LENS48 = [1, 47, 48, 49, 210]
# (sequence lengths, page size, K/V heads, G).  5 heads on pages of 48: the decode kernel's reciprocal division by neither a power of two
DECODE_CASES = [
    (LENS16, 16, 2, 1),
    (LENS16, 16, 4, 1),
    (LENS16, 16, 2, 4),
    (LENS16, 16, 4, 7),
    (LENS48, 48, 4, 1),
    (LENS48, 48, 5, 1),
    (LENS48, 48, 2, 4),
]
PREFILL_ALL = [(0, 64), (15, 16), (16, 65), (300, 7), (2000, 8)]         # (prefix, q_len) per sequence
# ((prefix, q_len) list, page size, K/V heads, G)
PREFILL_CASES = [
    (PREFILL_ALL, 16, 2, 1),
    (PREFILL_ALL, 16, 4, 4),
    (PREFILL_ALL, 48, 2, 7),
    (PREFILL_ALL, 48, 2, 1),
    ([(2000, 8)], 16, 2, 1),
    ([(2000, 8)], 16, 2, 4),
]
ROPE_PARAMS = [(1e4, 1.0), (5e5, 1.0), (1e4, 2.0), (1e6, 4.0)]          # (rope_theta, rope_scale)
OTHER_THETA = {1e4: 5e5, 5e5: 1e4, 1e6: 1e4}                             # the `theta` mutant of each pair
NEEDLE_A = 3.0


def case_id(case):
    shape, P, nkv, G = case
    return f"{len(shape)}seq-p{P}-kv{nkv}-g{G}"


def rel_bound(G, prefill):
    """the relative part of the ops' bound: the FP32 decode op 2e-3, the fp16 matrix-core ops (prefill, GQA) 4e-3"""
    return 4e-3 if (prefill or G > 1) else 2e-3


def bound(ref, rel):
    """[rows, heads]: rel * max|ref| + 1e-3 per (row, head)"""
    return rel * np.abs(ref).max(axis=-1) + 1e-3


def error_ratio(got, ref, rel):
    """[rows, heads]: max|got - ref| / bound, per (row, head).  <= 1: within the bound"""
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=-1) / bound(ref, rel)


def key_tile(G, prefill):
    """keys per tile of the op: its KV-split boundaries are multiples of this"""
    return 64 if (prefill or G > 1) else 16


def window_starts(max_len):
    """Window positions of a case: steps of 64 (half a window), so that every position lies in a window AND both sides of every
    multiple of 16 -- every KV-split boundary of every op is one -- lie in ONE window; plus the last 128 positions.  Sequence b's
    window is [min(w, max(S_b - 128, 0)), .. + 128): shorter sequences keep their last (or only) window."""
    return sorted(set(range(0, max(max_len - WINDOW, 0) + 1, 64)) | {max(max_len - WINDOW, 0)})


def checked_keys(S, P, tile):
    """the keys whose loss / doubling the CPU test checks: the edges of tiles, pages and of the sequence, and both sides of every
    multiple of the op's key tile (a superset of its KV-split boundaries)"""
    js = {0, 1, 15, 16, 17, P - 1, P, S - 17, S - 16, S - 2, S - 1}
    for b in range(tile, S, tile):
        js |= {b - 1, b}
    return sorted(j for j in js if 0 <= j < S)


# ------------------------------------------------------------------------------------------------ builders
def page_tables(seqlens, P, seed, extra=3):
    """indptr, indices, last_page_offset (int32) and the pool's page count: page numbers from a scrambled list"""
    npages = [-(-s // P) for s in seqlens]
    cap = sum(npages) + extra
    perm = np.random.default_rng(seed).permutation(cap).astype(np.int32)
    indptr = np.cumsum([0] + npages).astype(np.int32)
    lpo = np.array([s - (n - 1) * P for s, n in zip(seqlens, npages)], dtype=np.int32)
    return indptr, perm[:indptr[-1]].copy(), lpo, cap


def _hot_codes(dims):
    """u8 [n, 64]: code 15 in dimension dims[i] of row i, 0 elsewhere (element 2j in the low nibble)"""
    dims = np.asarray(dims)
    c = np.zeros((len(dims), D // 2), dtype=np.uint8)
    c[np.arange(len(dims)), dims // 2] = np.where(dims % 2 == 0, 0x0F, 0xF0)
    return c


def build_membership(seqlens, nkv, P, w, seed):
    """The membership cache with the window at w (see window_starts).  Returns a dict: data u8 [pages, L, 2, N, P, 64], param f16
    [pages, L, 2, N, P, 2], indptr, indices, lpo, and for the closed form: win [B] (each sequence's window start) and scale
    [B][N, <= 128] (float64: the value scales of its window tokens)."""
    indptr, indices, lpo, cap = page_tables(seqlens, P, seed)
    rng = np.random.default_rng(seed + 1)
    data = np.zeros((cap, LAYERS, 2, nkv, P, D // 2), dtype=np.uint8)
    param = np.zeros((cap, LAYERS, 2, nkv, P, 2), dtype=np.float16)
    other = 1 - LAYER
    data[:, other] = rng.integers(0, 256, data[:, other].shape, dtype=np.uint8)
    param[:, other] = rng.uniform(0.01, 0.21, param[:, other].shape)
    data[:, LAYER, 0] = 0x88                                  # keys: (8 * 1 - 8) = 0 exactly, everywhere
    param[:, LAYER, 0, ..., 0] = 1.0
    param[:, LAYER, 0, ..., 1] = 8.0
    data[:, LAYER, 1] = _hot_codes(np.arange(P) % D)          # values: hot at scale 64 wherever no sequence's token lives
    param[:, LAYER, 1, ..., 0] = 64.0
    win, scales = [], []
    for b, S in enumerate(seqlens):
        pages = indices[indptr[b]:indptr[b + 1]]
        slots = len(pages) * P
        wb = min(w, max(S - WINDOW, 0))
        nw = min(WINDOW, S)
        j = np.arange(slots)
        codes = _hot_codes((j - wb) % D)                      # behind the end: the hot pattern continues
        codes[:wb] = 0
        codes[wb + nw:S] = 0
        s = rng.uniform(32.0, 64.0, (nkv, nw)).astype(np.float16)
        for h in range(nkv):
            prm = np.zeros((slots, 2), dtype=np.float16)
            prm[:S, 0] = 1.0
            prm[wb:wb + nw, 0] = s[h]
            prm[S:, 0] = 64.0
            data[pages, LAYER, 1, h] = codes.reshape(len(pages), P, D // 2)
            param[pages, LAYER, 1, h] = prm.reshape(len(pages), P, 2)
        win.append(wb)
        scales.append(s.astype(np.float64))
    return dict(data=data, param=param, indptr=indptr, indices=indices, lpo=lpo, win=win, scale=scales, seqlens=list(seqlens))


def membership_expected(c, qo, G):
    """The closed form: row at position p of sequence b, query head h: 15 s[h // G, d] / (p + 1) in every dimension d with
    w_b + d <= p, 0 elsewhere.  float64 [T, nkv * G, 128]."""
    nkv = c["data"].shape[3]
    out = np.zeros((int(qo[-1]), nkv * G, D))
    for b, S in enumerate(c["seqlens"]):
        r0, r1 = int(qo[b]), int(qo[b + 1])
        s = c["scale"][b]
        for r in range(r0, r1):
            p = S - (r1 - r0) + (r - r0)
            nd = min(max(p - c["win"][b] + 1, 0), s.shape[1])
            out[r, :, :nd] = np.repeat(15.0 * s[:, :nd] / (p + 1), G, axis=0)
    return out


def build_needle(seqlens, nkv, P, seed):
    """The needle cache: random codes everywhere (both layers, behind the ends, pages nobody owns), fp16 scale in [0.125, 0.25],
    zero = 8 * scale (exact in fp16)."""
    indptr, indices, lpo, cap = page_tables(seqlens, P, seed)
    rng = np.random.default_rng(seed + 1)
    data = rng.integers(0, 256, (cap, LAYERS, 2, nkv, P, D // 2), dtype=np.uint8)
    param = np.empty((cap, LAYERS, 2, nkv, P, 2), dtype=np.float16)
    param[..., 0] = rng.uniform(0.125, 0.25, param.shape[:-1])
    param[..., 1] = param[..., 0] * np.float16(8.0)
    return dict(data=data, param=param, indptr=indptr, indices=indices, lpo=lpo, seqlens=list(seqlens))


def needle_queries(rows, heads, seed, a=NEEDLE_A):
    return (np.random.default_rng(seed + 2).standard_normal((rows, heads, D)) * a).astype(np.float16)


def membership_queries(rows, heads, seed):
    """N(0, 1) queries, the ops' usual scale, for the membership family.  The FP64 output does not depend on them (zero keys), and
    the matrix-core ops' do not either.  The FP32 decode kernel forms a score as ks * sum((1024 + u) A) - (kz + 1024 ks) * sum(A)
    (kv_i4.hip: the nibble bias is removed once per token): with u = 8, ks = 1, kz = 8 two terms of size ~1e3 |q| cancel to FP32
    rounding, so its softmax weights are uniform to ~2e-4 |q| only -- a property of that op's arithmetic on a cache with scale 1 (real
    scales are ~0.1), proportional to |q|.  At needle_queries' a = 3 it alone fills the 2e-3 bound (measured on the MI355X: 1.004 x
    the bound at 300 tokens, unsplit); at the unit scale it leaves the bound to what the test is about."""
    return needle_queries(rows, heads, seed, a=1.0)


def prefill_shape(shape):
    """(prefix, q_len) list -> sequence lengths, qo_indptr int32"""
    return [p + n for p, n in shape], np.cumsum([0] + [n for _, n in shape]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ references
_PERM = np.concatenate([np.arange(0, D, 2), np.arange(1, D, 2)])


def _rope(x, pos, theta, rope_scale, interleaved=False):
    """RoPE at pos / rope_scale (freq_i = (1 / rope_scale) theta^(-2 i / 128)), pairs (i, i + 64); interleaved: pairs (2i, 2i + 1)"""
    pos = np.asarray(pos, dtype=np.float64) / rope_scale
    if not interleaved:
        return O._rope_llama(x, pos, theta)
    y = O._rope_llama(x[..., _PERM], pos, theta)
    out = np.empty_like(y)
    out[..., _PERM] = y
    return out


def _mutation(mutate):
    if not mutate:
        return None, None
    (kind, arg), = mutate.items()
    assert kind in MUTANTS, kind
    return kind, arg


def ref_prefill(q, c, qo, *, G=1, theta=1e4, rope_scale=1.0, layer=LAYER, mutate=None, seqs=None, memo=None):
    """FP64 causal attention of the cache c (a builder's dict): sequence b's queries are rows qo[b] .. qo[b + 1] at its last
    positions, query head h reads K/V head h // G.  q f16 [T, nkv * G, 128] -> float64 [T, nkv * G, 128].  ``seqs``: compute these
    sequences only (the other rows stay 0).  ``memo``: a dict that keeps the de-quantised rows of c between calls (one per cache; entries ("k", ..) the
    keys, ("v", ..) the values).
    ``mutate``: one deliberate error:
      drop_key=j / double_key=j   key j of every sequence that has one is left out / counted twice
      causal_plus_one             the row at position p also sees key p + 1
      q_pos_minus_one             queries rotated at their position - 1
      key_pos_plus_one            keys rotated at their position + 1
      theta=x                     another RoPE base
      ignore_rope_scale           rope_scale taken as 1
      interleaved_pairs           RoPE pairs (2i, 2i + 1) instead of (i, i + 64)
      swap_pages=(a, b)           pages a and b of every sequence that has both change places
      head_mod                    query head h reads K/V head h % nkv
      other_layer                 the other layer's cache
      read_past_end               the slots of the last page behind last_page_offset count as keys that every row sees"""
    kind, arg = _mutation(mutate)
    data, param, indptr, indices, lpo = c["data"], c["param"], c["indptr"], c["indices"], c["lpo"]
    qn = np.asarray(q).astype(np.float64)
    T, Nq, _ = qn.shape
    nkv, P = data.shape[3], data.shape[4]
    assert Nq == nkv * G
    if kind == "theta":
        theta = float(arg)
    if kind == "ignore_rope_scale":
        rope_scale = 1.0
    if kind == "other_layer":
        layer = (layer + 1) % data.shape[1]
    inter = kind == "interleaved_pairs"
    memo = {} if memo is None else memo
    out = np.zeros((T, Nq, D))
    for b in (range(len(lpo)) if seqs is None else seqs):
        S = O.kv_seq_len(indptr, lpo, P, b)
        r0, r1 = int(qo[b]), int(qo[b + 1])
        pos = np.arange(S - (r1 - r0), S)
        pages = [int(x) for x in indices[int(indptr[b]):int(indptr[b + 1])]]
        if kind == "swap_pages" and max(arg) < len(pages):
            pages[arg[0]], pages[arg[1]] = pages[arg[1]], pages[arg[0]]
        slots = np.arange(len(pages) * P)
        count = (slots < S).astype(np.float64)               # how often each slot of the sequence's pages counts as a key
        if kind == "read_past_end":
            count[:] = 1.0
        if kind in ("drop_key", "double_key") and arg < S:
            count[arg] = 0.0 if kind == "drop_key" else 2.0
        shift = 1 if kind == "key_pos_plus_one" else 0
        qpos = pos - (1 if kind == "q_pos_minus_one" else 0)
        reach = pos + (1 if kind == "causal_plus_one" else 0)
        hidden = (slots[None, :] > reach[:, None]) & (slots[None, :] < S)
        weight = np.where(hidden, 0.0, count[None, :])       # [rows, slots]
        qf = _rope(qn[r0:r1].transpose(1, 0, 2), qpos, theta, rope_scale, inter)            # [heads, rows, D]
        for hk in range(nkv):
            hs = [h for h in range(Nq) if (h % nkv if kind == "head_mod" else h // G) == hk]  # the query heads that read K/V head hk
            if not hs:
                continue
            gather = lambda a, which: a[pages, layer, which, hk].reshape(len(slots), -1)
            kkey, vkey = ("k", hk, layer, tuple(pages), theta, rope_scale, inter, shift), ("v", hk, layer, tuple(pages))
            if kkey not in memo:                             # every slot, de-quantised (and the keys rotated) once
                memo[kkey] = _rope(O._dequant_u4_rows(gather(data, 0), gather(param, 0)), slots + shift, theta, rope_scale, inter)
            if vkey not in memo:
                memo[vkey] = O._dequant_u4_rows(gather(data, 1), gather(param, 1))
            kf, vf = memo[kkey], memo[vkey]
            wgt = np.tile(weight, (len(hs), 1))              # rows of (head, query row)
            s = np.where(wgt > 0, qf[hs].reshape(-1, D) @ kf.T / np.sqrt(D), -np.inf)
            m = s.max(axis=1, keepdims=True)
            pr = np.exp(s - np.where(np.isfinite(m), m, 0.0)) * wgt
            den = pr.sum(axis=1, keepdims=True)
            o = (pr / np.where(den > 0, den, 1.0)) @ vf      # a row that sees no key: zeros, as the ops give
            out[r0:r1, hs] = o.reshape(len(hs), r1 - r0, D).transpose(1, 0, 2)
    return out


def top_key(q, c, qo, b, h, *, G=1, theta=1e4, rope_scale=1.0, layer=LAYER):
    """the key that holds the largest softmax weight of sequence b's LAST query row, query head h (unmutated)"""
    data, param, P = c["data"], c["param"], c["data"].shape[4]
    S = O.kv_seq_len(c["indptr"], c["lpo"], P, b)
    pages = [int(x) for x in c["indices"][int(c["indptr"][b]):int(c["indptr"][b + 1])]]
    gather = lambda a: a[pages, layer, 0, h // G].reshape(len(pages) * P, -1)[:S]
    kf = _rope(O._dequant_u4_rows(gather(data), gather(param)), np.arange(S), theta, rope_scale)
    qf = _rope(np.asarray(q[int(qo[b + 1]) - 1, h]).astype(np.float64)[None, :], [S - 1], theta, rope_scale)[0]
    return int(np.argmax(kf @ qf))


def ref_decode(q, c, **kw):
    """FP64 decode attention: one query per sequence at its last position.  q f16 [B, nkv * G, 128]; arguments of ref_prefill."""
    return ref_prefill(q, c, np.arange(len(c["lpo"]) + 1), **kw)
