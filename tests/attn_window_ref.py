"""FP64 references and the closed form of SLIDING-WINDOW attention over the paged INT4 cache (atom_batch_decode_gqa_i4_win,
atom_batch_prefill_gqa_i4_win) on the planted inputs of tests/attn_planted.py, shared by tests/test_attn_window_cpu.py and
tests/test_gpu_attn_window.py.  numpy only.

A window W >= 1: the query at position p sees the keys j with p - W < j <= p (HF's kv_idx > q_idx - sliding_window), the bound taken
from each row's OWN position.  Everything else -- RoPE, head mapping, paging -- is attn_planted.ref_prefill's.

``mutate=`` names ONE deliberate error of the lower bound (MUTANTS); the CPU test shows that each moves the closed form by >= 10 x the
bound the GPU test applies, on the cases the GPU test runs."""
import numpy as np

from oracle import atom_oracle as O
from tests import attn_planted as A

D = A.D
WINDOWS = (1, 2, 16, 63, 64, 65, 100, 128, 300, 600)
MUTANTS = ("window_plus_one", "window_minus_one", "window_from_end", "window_from_first_row", "no_window")

# (sequence lengths, page size, K/V heads, G) and ((prefix, q_len) list, page size, K/V heads, G): the issue's shapes.  (0, 200) and
# (40, 150) put rows beyond the window inside a fresh chunk and across query blocks; 2100 and (2000, 8) put split boundaries inside
# the window's tiles and leave the batch's short sequences with empty splits.
DECODE_CASES = [
    (A.LENS16, 16, 2, 1),
    (A.LENS16, 16, 2, 4),
    (A.LENS16, 16, 4, 7),
    (A.LENS48, 48, 2, 4),
    (A.LENS48, 48, 5, 1),
]
PREFILL_SHAPE = [(0, 64), (15, 16), (16, 65), (300, 7), (2000, 8), (0, 200), (40, 150)]
PREFILL_CASES = [(PREFILL_SHAPE, P, 2, G) for P in (16, 48) for G in (1, 4, 7)]
REL = 4e-3                                                   # the windowed op is always the matrix-core kernel: 4e-3 max|ref| + 1e-3


def lower_bounds(pos, S, window, mutate=None):
    """float [rows]: row r sees the keys j with lo[r] < j <= pos[r].  pos: the positions of one sequence's query rows (ascending),
    S its length.
      window_plus_one        also sees key p - W
      window_minus_one       misses key p - W + 1 (from W >= 2: at W = 1 the row would see nothing)
      window_from_end        every row's bound from the sequence's last position
      window_from_first_row  ... from the chunk's first row
      no_window"""
    pos = np.asarray(pos, dtype=np.float64)
    assert mutate is None or mutate in MUTANTS, mutate
    if mutate == "no_window":
        return np.full(pos.shape, -np.inf)
    if mutate == "window_plus_one":
        return pos - window - 1
    if mutate == "window_minus_one":
        assert window >= 2
        return pos - window + 1
    if mutate == "window_from_end":
        return np.full(pos.shape, float(S - 1 - window))
    if mutate == "window_from_first_row":
        return np.full(pos.shape, float(pos[0] - window))
    return pos - window


def _rows(c, qo):
    """(b, S, r0, r1, pos) per sequence"""
    for b, S in enumerate(c["seqlens"]):
        r0, r1 = int(qo[b]), int(qo[b + 1])
        yield b, S, r0, r1, np.arange(S - (r1 - r0), S)


def applies(seqlens, qo, window, mutate):
    """the mutant changes the key set of some row of the case (a mutant that changes none cannot be noticed and is not asked for)"""
    if mutate == "window_minus_one" and window < 2:
        return False
    for _, S, _, _, pos in _rows(dict(seqlens=seqlens), qo):
        if len(pos) and np.any(np.maximum(lower_bounds(pos, S, window), -1) != np.maximum(lower_bounds(pos, S, window, mutate), -1)):
            return True
    return False


def membership_expected(c, qo, G, window, mutate=None):
    """The closed form of the membership family under a window: the row at position p of sequence b, query head h, holds
    15 s[h // G, d] / n in every dimension d whose planted token w_b + d lies among its n visible keys (unmutated: the keys of
    (p - W, p], n = min(p + 1, W)) and 0 elsewhere.  float64 [T, nkv * G, 128]."""
    nkv = c["data"].shape[3]
    out = np.zeros((int(qo[-1]), nkv * G, D))
    for b, S, r0, r1, pos in _rows(c, qo):
        s, wb = c["scale"][b], c["win"][b]
        if r1 == r0:
            continue
        lo = np.maximum(lower_bounds(pos, S, window, mutate), -1)
        n = np.maximum(pos - lo, 0)                           # keys lo + 1 .. p
        t = wb + np.arange(s.shape[1])                        # the planted tokens' positions, dimension d at w_b + d
        seen = (t[None, :] > lo[:, None]) & (t[None, :] <= pos[:, None])                  # [rows, dims]
        val = 15.0 * s[None, :, :] * (seen / np.maximum(n, 1)[:, None])[:, None, :]       # [rows, nkv, dims]
        out[r0:r1, :, :s.shape[1]] = np.repeat(val, G, axis=1)
    return out


def ref_prefill(q, c, qo, window, *, G=1, theta=1e4, rope_scale=1.0, layer=A.LAYER, mutate=None, memo=None):
    """attn_planted.ref_prefill with the lower bound: FP64 attention of the cache c, sequence b's queries at its last positions, query
    head h reads K/V head h // G, the row at p sees keys p - window < j <= p.  q f16 [T, nkv * G, 128] -> float64 [T, nkv * G, 128].
    ``memo``: a dict that keeps the de-quantised, rotated rows of c between calls."""
    data, param, indptr, indices, lpo = c["data"], c["param"], c["indptr"], c["indices"], c["lpo"]
    qn = np.asarray(q).astype(np.float64)
    T, Nq, _ = qn.shape
    nkv, P = data.shape[3], data.shape[4]
    assert Nq == nkv * G
    memo = {} if memo is None else memo
    out = np.zeros((T, Nq, D))
    for b in range(len(lpo)):
        S = O.kv_seq_len(indptr, lpo, P, b)
        r0, r1 = int(qo[b]), int(qo[b + 1])
        pos = np.arange(S - (r1 - r0), S)
        lo = lower_bounds(pos, S, window, mutate)
        pages = [int(x) for x in indices[int(indptr[b]):int(indptr[b + 1])]]
        j = np.arange(S)
        seen = (j[None, :] <= pos[:, None]) & (j[None, :] > lo[:, None])                  # [rows, S]
        qf = A._rope(qn[r0:r1].transpose(1, 0, 2), pos, theta, rope_scale)                # [heads, rows, D]
        for hk in range(nkv):
            gather = lambda a, which: a[pages, layer, which, hk].reshape(len(pages) * P, -1)[:S]
            kkey, vkey = ("k", b, hk, layer, theta, rope_scale), ("v", b, hk, layer)
            if kkey not in memo:
                memo[kkey] = A._rope(O._dequant_u4_rows(gather(data, 0), gather(param, 0)), j, theta, rope_scale)
            if vkey not in memo:
                memo[vkey] = O._dequant_u4_rows(gather(data, 1), gather(param, 1))
            kf, vf = memo[kkey], memo[vkey]
            hs = list(range(hk * G, hk * G + G))
            vis = np.tile(seen, (G, 1))                      # rows of (head, query row)
            s = np.where(vis, qf[hs].reshape(-1, D) @ kf.T / np.sqrt(D), -np.inf)
            m = s.max(axis=1, keepdims=True)
            pr = np.where(vis, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
            den = pr.sum(axis=1, keepdims=True)
            o = (pr / np.where(den > 0, den, 1.0)) @ vf      # a row that sees no key: zeros, as the ops give
            out[r0:r1, hs] = o.reshape(G, r1 - r0, D).transpose(1, 0, 2)
    return out


def ref_decode(q, c, window, **kw):
    """one query per sequence at its last position.  q f16 [B, nkv * G, 128]; arguments of ref_prefill."""
    return ref_prefill(q, c, np.arange(len(c["lpo"]) + 1), window, **kw)


def case_shape(case, prefill):
    """(sequence lengths, qo_indptr as the references take it, qo_indptr for the op or None, max_q_len)"""
    shape = case[0]
    if prefill:
        lens, qo = A.prefill_shape(shape)
        return lens, qo, qo, max(n for _, n in shape)
    return list(shape), np.arange(len(shape) + 1), None, 1
