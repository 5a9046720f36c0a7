"""References of the ROLLING INT4 paged KV cache (atom_kv_step_ring_i4, atom_batch_decode_gqa_i4_ring,
atom_batch_prefill_gqa_i4_ring), shared by tests/test_kv_ring_cpu.py and tests/test_gpu_kv_ring.py.  numpy only.

A sequence's row of the page table is a ring of R slots: logical page g (tokens g P .. g P + P - 1) lives in slot g % R.  A step to the
length n that adds ``add`` tokens lists the logical pages f .. l in logical order,
    f = max(0, n - max(add, 1) - W + 1) // P        l = (n - 1) // P
and kv_start = f P is the position of the list's first token.  The attention ops keep every position absolute and only FETCH key j
from page (j - kv_start) // P of the list.

``ring_step`` restates the step kernel; ``ring_cache`` turns a planted cache of tests/attn_planted.py into the rolling cache that holds
the same sequences -- every byte that no correct kernel may read set to 0xFF (an fp16 NaN as scale or zero point); ``ring_prefill`` is
the FP64 attention that reads such a cache, with ``mutate=`` for ONE deliberate error (MUTANTS).  The unmutated ``ring_prefill`` is
``attn_window_ref.ref_prefill`` on the un-released cache."""
import numpy as np

from oracle import atom_oracle as O
from tests import attn_planted as A
from tests import attn_window_ref as W

D = A.D
OVERFLOW, BAD_LENGTH = 1, 2
INT_MAX = 0x7FFFFFFF
MUTANTS = ("positions_from_list", "slot_order", "start_plus_page", "start_minus_page", "window_from_list_len")
REL = W.REL                                                  # the windowed op's bound: 4e-3 max|ref| + 1e-3 per (row, head)


def ring_size(window, P, max_add=1):
    """R = ceil((W - 1 + max_add) / P) + 1: the most pages that the keys of ``max_add`` consecutive rows can touch"""
    return -(-(window - 1 + max_add) // P) + 1


def live_pages(n, add, window, P):
    """(f, cnt): first live logical page and the count of live pages of a step of ``add`` tokens to the length n"""
    if n <= 0:
        return 0, 0
    f = max(0, n - max(add, 1) - window + 1) // P
    return f, (n - 1) // P - f + 1


def ring_step(table, row_pages, lens, add, window, P):
    """atom_kv_step_ring_i4 on the host: table int [B, cap], row_pages [B], lens [B] (the CURRENT lengths).  Returns
    (lens', indptr, indices, lpo, kv_start, status), int32 arrays (indices holds indptr[-1] entries) and the status bits."""
    table = np.asarray(table)
    B, cap = table.shape
    new, cnts, idx, lpo, start, status = [], [], [], [], [], 0
    for b in range(B):
        R = min(max(int(row_pages[b]), 0), cap)
        n = int(lens[b])
        if n < 0:
            n, status = 0, status | BAD_LENGTH
        if n > INT_MAX - add:
            n, status = INT_MAX - add, status | BAD_LENGTH
        f, cnt = live_pages(n + add, add, window, P)
        if cnt <= R:
            n += add
        else:                                                # refused: the tables of the old length
            status |= OVERFLOW
            f, cnt = live_pages(n, 0, window, P)
            if cnt > R:                                      # a length that the ring cannot describe at all
                status |= BAD_LENGTH
                if R == 0:
                    n, f, cnt = 0, 0, 0
                else:
                    f, cnt = f + cnt - R, R
        new.append(n)
        cnts.append(cnt)
        idx += [int(table[b, (f + j) % R]) for j in range(cnt)]
        lpo.append((n - 1) % P + 1 if n > 0 else 0)
        start.append(f * P)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return i32(new), i32(np.cumsum([0] + cnts)), i32(idx), i32(lpo), i32(start), status


def ring_cache(c, window, R, adds=None, seed=0):
    """The planted cache ``c`` (a builder's dict of tests/attn_planted.py) as a rolling cache after a step of ``adds[b]`` tokens
    (default 1: a decode step) to each sequence's length: the same sequences, every one on a ring of R pages from a scrambled pool.
    The live pages f .. l sit in slots g % R; ``indices`` lists them in logical order, ``kv_start`` = f P, ``table`` int32 [B, R] is
    the ring.  Every slot that holds no live page, every page that nobody owns and every byte of a last page behind the sequence's
    end is 0xFF, in both layers -- a NaN scale: one stale byte read shows."""
    data, param, P = c["data"], c["param"], c["data"].shape[4]
    B = len(c["seqlens"])
    adds = [1] * B if adds is None else list(adds)
    cap = B * R + 3
    perm = np.random.default_rng(seed + 17).permutation(cap).astype(np.int32)
    table = perm[:B * R].reshape(B, R).copy()
    nd = np.full((cap,) + data.shape[1:], 0xFF, dtype=np.uint8)
    npar = np.full((cap,) + param.shape[1:], 0xFFFF, dtype=np.uint16).view(np.float16)
    cnts, idx, start = [], [], []
    for b, S in enumerate(c["seqlens"]):
        old = c["indices"][int(c["indptr"][b]):int(c["indptr"][b + 1])]
        f, cnt = live_pages(S, adds[b], window, P)
        assert cnt <= R, (S, adds[b], window, P, R)
        for g in range(f, f + cnt):
            dst = table[b, g % R]
            nd[dst], npar[dst] = data[old[g]], param[old[g]]
            if g == f + cnt - 1 and S % P:                   # behind the end: stale bytes that must never be read
                nd[dst][:, :, :, S % P:] = 0xFF
                npar[dst].view(np.uint16)[:, :, :, S % P:] = 0xFFFF
            idx.append(dst)
        cnts.append(cnt)
        start.append(f * P)
    out = dict(c)
    out.update(data=nd, param=npar, indptr=np.cumsum([0] + cnts).astype(np.int32), indices=np.asarray(idx, dtype=np.int32),
               kv_start=np.asarray(start, dtype=np.int32), table=table, R=R, window=window)
    return out


def ring_prefill(q, rc, qo, window, *, G=1, theta=1e4, layer=A.LAYER, mutate=None, reads=None):
    """FP64 windowed attention that reads the rolling cache ``rc`` (ring_cache's dict) the way the _ring kernels must: sequence b is
    start_b + (pages - 1) P + lpo tokens long, its queries sit at its last positions, the row at p sees keys p - window < j <= p, and
    key j is fetched from page (j - start_b) // P of the list; a key that a row sees but the list does not hold reads as zeros (what
    the kernel stages).  Only keys that some row sees are fetched.  q f16 [T, nkv * G, 128] -> float64 [T, nkv * G, 128].
    ``reads``: a dict; ["bad"] counts the fetched (scale, zero) values that are not finite -- stale 0xFF bytes.
    ``mutate``: one deliberate error:
      positions_from_list    a key's position (its RoPE angle and its side of both masks) is its index in the LIST, kv_start taken as 0
      slot_order             the list is the ring's slots 0 .. cnt - 1 as they lie, not rotated into logical order
      start_plus_page        key j is fetched with kv_start + P: from the list's page (j - start) // P - 1
      start_minus_page       ... with kv_start - P: from page (j - start) // P + 1
      window_from_list_len   the lower bound is the list's first key for every row: a row sees all listed keys up to its own"""
    assert mutate is None or mutate in MUTANTS, mutate
    data, param, indptr, indices, lpo = rc["data"], rc["param"], rc["indptr"], rc["indices"], rc["lpo"]
    qn = np.asarray(q).astype(np.float64)
    T, Nq, _ = qn.shape
    nkv, P = data.shape[3], data.shape[4]
    assert Nq == nkv * G
    out = np.zeros((T, Nq, D))
    for b in range(len(lpo)):
        start = int(rc["kv_start"][b])
        npg = int(indptr[b + 1]) - int(indptr[b])
        pages = np.asarray(indices[int(indptr[b]):int(indptr[b + 1])], dtype=np.int64)
        if mutate == "slot_order":
            pages = np.asarray(rc["table"][b][:npg], dtype=np.int64)
        n_list = (npg - 1) * P + int(lpo[b])
        S = start + n_list
        r0, r1 = int(qo[b]), int(qo[b + 1])
        if r1 == r0 or S <= 0:
            continue
        pos = np.arange(S - (r1 - r0), S)
        lo = np.maximum(pos - window, -1)
        if mutate == "window_from_list_len":
            lo = np.full(pos.shape, start - 1)
        fetch_start = start + (P if mutate == "start_plus_page" else -P if mutate == "start_minus_page" else 0)
        j = np.arange(min(int(lo.min()) + 1, start), S)       # candidates: every key a row may see, and the whole list
        kp = j - start if mutate == "positions_from_list" else j
        seen = (kp[None, :] <= pos[:, None]) & (kp[None, :] > lo[:, None])                 # [rows, keys]
        src = j - fetch_start
        held = (src >= 0) & (src < n_list) & seen.any(axis=0)
        pg, e = pages[np.where(held, src // P, 0)], np.where(held, src % P, 0)
        qf = A._rope(qn[r0:r1].transpose(1, 0, 2), pos, theta, 1.0)                        # [heads, rows, D]
        for hk in range(nkv):
            kf, vf = np.zeros((len(j), D)), np.zeros((len(j), D))
            for which, dst in ((0, kf), (1, vf)):
                prm = param[pg[held], layer, which, hk, e[held]]
                if reads is not None:
                    reads["bad"] = reads.get("bad", 0) + int((~np.isfinite(prm.astype(np.float64))).sum())
                dst[held] = O._dequant_u4_rows(data[pg[held], layer, which, hk, e[held]], prm)
            kf = A._rope(kf, kp, theta, 1.0)
            hs = list(range(hk * G, hk * G + G))
            vis = np.tile(seen, (G, 1))
            s = np.where(vis, qf[hs].reshape(-1, D) @ kf.T / np.sqrt(D), -np.inf)
            m = s.max(axis=1, keepdims=True)
            pr = np.where(vis, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
            den = pr.sum(axis=1, keepdims=True)
            o = (pr / np.where(den > 0, den, 1.0)) @ vf
            out[r0:r1, hs] = o.reshape(G, r1 - r0, D).transpose(1, 0, 2)
    return out


def applies(rc, qo, window, mutate):
    """the mutant changes what some row of the case reads (a mutant that changes nothing cannot be noticed and is not asked for)"""
    P = rc["data"].shape[4]
    for b in range(len(rc["lpo"])):
        start, npg = int(rc["kv_start"][b]), int(rc["indptr"][b + 1]) - int(rc["indptr"][b])
        nq = int(qo[b + 1]) - int(qo[b])
        if npg == 0 or nq == 0:
            continue
        S = start + (npg - 1) * P + int(rc["lpo"][b])
        if mutate == "positions_from_list" and start > 0:
            return True
        if mutate == "slot_order" and (start // P) % rc["R"] != 0:
            return True
        if mutate in ("start_plus_page", "start_minus_page"):
            return True
        if mutate == "window_from_list_len" and start < max(S - 1 - window + 1, 0):
            return True                                      # (the last row's lowest key lies behind the list's first)
    return False


# ------------------------------------------------------------------------------------------------ the cases both test files run
# (sequence lengths, page size, K/V heads, G, windows): decode steps.  Lengths of 1 .. W keep kv_start at 0; 300 and up put it on a
# multiple of P that is no multiple of 64 for some window of the case (P = 16, W = 16, S = 300: 272; P = 48, W = 63, S = 210: 144)
# and wrap the ring several times (S = 1000, W = 16, P = 16: R = 2, 31 wraps).
DECODE_CASES = [
    ([1, 15, 17, 300, 1000], 16, 2, 1, (1, 16, 64, 300)),
    ([1, 16, 300, 1000, 2100], 16, 2, 4, (16, 63, 65, 100)),
    ([17, 300, 2100], 16, 4, 7, (1, 63, 100, 300)),
    ([1, 47, 49, 210, 1000], 48, 2, 4, (16, 64, 65, 300)),
    ([48, 210, 1000], 48, 5, 1, (1, 63, 100)),
    ([49, 1000], 48, 2, 7, (16, 65, 300)),
    # split boundaries inside the window; 1239: the page floor leaves 15 keys in front of the window (639 = 39 * 16 + 15), the most
    # that `window_from_list_len` can add -- at 2100 it adds 12 of 600
    ([2100, 1239, 40], 16, 2, 4, (600,)),
]
# ((prefix, q_len) list, page size, K/V heads, G, windows): chunks, after a step of q_len tokens on rings sized for max_add = MAX_ADD
MAX_ADD = 8
PREFILL_SHAPE = [(0, 5), (20, 8), (300, 7), (2000, 8)]
PREFILL_CASES = [
    (PREFILL_SHAPE, 16, 2, 1, (1, 16, 65, 300)),
    (PREFILL_SHAPE, 16, 2, 4, (16, 63, 64, 100)),
    (PREFILL_SHAPE, 16, 2, 7, (1, 64, 300)),
    (PREFILL_SHAPE, 48, 2, 1, (16, 63, 100)),
    (PREFILL_SHAPE, 48, 2, 4, (1, 65, 300)),
    (PREFILL_SHAPE, 48, 2, 7, (63, 64, 65, 100)),
]
WINDOWS = (1, 16, 63, 64, 65, 100, 300)
for _cases in (DECODE_CASES, PREFILL_CASES):
    assert all(sum(w in c[4] for c in _cases) >= 2 for w in WINDOWS)


def case_id(case):
    return A.case_id(case[:4]) + "-w" + "_".join(map(str, case[4]))


def case_shape(case, prefill):
    """(sequence lengths, qo_indptr for the references, qo_indptr for the op or None, max_q_len, adds per sequence, max_add)"""
    shape = case[0]
    if prefill:
        lens, qo = A.prefill_shape(shape)
        return lens, qo, qo, max(n for _, n in shape), [n for _, n in shape], MAX_ADD
    return list(shape), np.arange(len(shape) + 1), None, 1, [1] * len(shape), 1
