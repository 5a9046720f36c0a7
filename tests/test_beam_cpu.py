"""CPU checks of the host restatement of beam search (tests/beam_ref.py), which the GPU tests hold the kernels against: the selection
against a float64 brute force and hand-written orders, the backtracking and ranking on a hand-made table, the page-ownership
invariant of the fork over 200 random steps."""
import random

import numpy as np
import pytest

from tests import beam_ref

NEG = float("-inf")


def _brute(top_ids, top_lp, cum, finished, length, eos, w_in, w_out):
    """float64 full sort over all candidates (inputs without score ties): [(parent, token, finished, length)] per group"""
    out = []
    for g in range(len(cum) // w_in):
        cands = []
        for b in range(w_in):
            r = g * w_in + b
            if finished[r]:
                cands.append((float(cum[r]), b, eos, 1, int(length[r])))
            else:
                for c in range(top_ids.shape[1]):
                    t = int(top_ids[r, c])
                    cands.append((float(cum[r]) + float(top_lp[r, c]), b, t, int(t == eos), int(length[r]) + 1))
        cands.sort(key=lambda x: -x[0])
        out.append(cands[:w_out])
    return out


@pytest.mark.parametrize("w_in_is_one", [False, True])
@pytest.mark.parametrize("W,C,G", [(1, 1, 2), (2, 2, 3), (4, 32, 2), (5, 7, 3), (16, 16, 1), (16, 32, 2)])
def test_ref_select_equals_the_float64_full_sort(W, C, G, w_in_is_one):
    rng = np.random.default_rng(W * 100 + C + G)
    w_in = 1 if w_in_is_one else W
    rows = G * w_in
    # multiples of 2^-10 below 2^13 in magnitude: every sum is exact in FP32 and in float64, so equal sums are real ties -- redrawn
    while True:
        top_lp = -np.sort(rng.integers(1, 2 ** 22, (rows, C)), axis=1).astype(np.float32) / 1024
        cum = -rng.integers(0, 2 ** 22, rows).astype(np.float32) / 1024
        finished = (rng.random(rows) < 0.3).astype(np.int32) if w_in > 1 else np.zeros(rows, np.int32)
        scores = [float(cum[r]) + float(x) for r in range(rows) if not finished[r] for x in top_lp[r]] + [float(cum[r]) for r in range(rows) if finished[r]]
        if len(set(scores)) == len(scores):
            break
    top_ids = rng.integers(0, 50, (rows, C)).astype(np.int64)
    length = rng.integers(1, 9, rows).astype(np.int32)
    eos = 7
    parent, token, ncum, nfin, nlen = beam_ref.select(top_ids, top_lp, cum, finished, length, eos, w_in, W)
    want = _brute(top_ids, top_lp, cum, finished, length, eos, w_in, W)
    for g in range(G):
        for i, (s, b, t, f, n) in enumerate(want[g]):
            o = g * W + i
            assert (int(parent[o]), int(token[o]), int(nfin[o]), int(nlen[o])) == (b, t, f, n), (g, i)
            assert float(ncum[o]) == s


def test_ref_select_orders_planted_ties_by_parent_then_candidate():
    ids = np.arange(12, dtype=np.int64).reshape(3, 4) + 10
    # equal scores across rows: row 0's second (-1 + -2) = row 1's first (-2 + -1) = row 2's first (-3 + 0)
    lp = np.array([[-1, -2, -5, -6], [-1, -4, -5, -6], [0, -7, -8, -9]], dtype=np.float32)
    cum = np.array([-1, -2, -3], dtype=np.float32)
    z = np.zeros(3, np.int32)
    parent, token, ncum, nfin, nlen = beam_ref.select(ids, lp, cum, z, z + 2, None, 3, 3)
    assert parent.tolist() == [0, 0, 1] and token.tolist() == [10, 11, 14] and ncum.tolist() == [-2, -3, -3]
    assert nfin.tolist() == [0, 0, 0] and nlen.tolist() == [3, 3, 3]
    # equal log-probabilities within a row: candidate order decides (ops.logprob has ordered them by token id)
    lp = np.array([[-1, -1, -1, -1], [-1, -1, -3, -3], [-9, -9, -9, -9]], dtype=np.float32)
    cum = np.zeros(3, np.float32)
    parent, token, *_ = beam_ref.select(ids, lp, cum, z, z, None, 3, 3)
    assert parent.tolist() == [0, 0, 0] and token.tolist() == [10, 11, 12]
    # all -inf: every key is the smallest, the order is (parent, candidate); -inf + -inf is -inf, not NaN
    lp = np.full((3, 4), NEG, dtype=np.float32)
    parent, token, ncum, *_ = beam_ref.select(ids, lp, np.array([NEG, -1, 0], np.float32), z, z, None, 3, 3)
    assert parent.tolist() == [0, 0, 0] and token.tolist() == [10, 11, 12] and np.isneginf(ncum).all()
    # -0 and +0 are one score; a NaN ranks as -inf
    assert beam_ref.score_key(np.float32(-0.0))[0] == beam_ref.score_key(np.float32(0.0))[0]
    assert beam_ref.score_key(np.float32("nan"))[0] == beam_ref.score_key(np.float32(NEG))[0] == 0x007FFFFF
    k = beam_ref.score_key(np.array([NEG, -3e38, -1, -1e-45, 0, 1e-45, 2, np.inf], np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_ref_select_freezes_finished_rows_and_pads():
    ids = np.array([[5, 6], [7, 5]], dtype=np.int64)
    lp = np.array([[-1, -2], [-0.5, -3]], dtype=np.float32)
    # row 0 finished at -1.25 with 4 tokens: one candidate, unchanged; row 1 live: -1 - 0.5 loses to it, and its eos candidate finishes
    parent, token, ncum, nfin, nlen = beam_ref.select(ids, lp, np.array([-1.25, -1], np.float32), [1, 0], [4, 9], 5, 2, 2)
    assert parent.tolist() == [0, 1] and token.tolist() == [5, 7] and ncum.tolist() == [-1.25, -1.5]
    assert nfin.tolist() == [1, 0] and nlen.tolist() == [4, 10]
    parent, token, ncum, nfin, nlen = beam_ref.select(ids, lp, np.array([-9, -1], np.float32), [1, 0], [4, 9], 5, 2, 2)
    assert parent.tolist() == [1, 1] and token.tolist() == [7, 5] and nfin.tolist() == [0, 1] and nlen.tolist() == [10, 10]
    # one finished row into two outputs: the second is padding
    parent, token, ncum, nfin, nlen = beam_ref.select(ids[:1], lp[:1], np.array([-2], np.float32), [1], [3], 5, 1, 2)
    assert parent.tolist() == [0, 0] and token.tolist() == [5, 5] and ncum.tolist() == [-2, NEG] and nfin.tolist() == [1, 1]


# a hand-made search: 1 group, 3 beams, 4 steps, eos 9.  Final rows: 0 <- 0 <- 1 <- 0, 1 <- 2 <- 2 <- 1 (eos at step 1), 2 <- 0 <- 1 <- 0
PARENTS = [[0, 0, 0], [0, 0, 1], [1, 1, 2], [0, 2, 0]]
TOKENS = [[1, 2, 3], [4, 5, 9], [6, 7, 9], [8, 9, 3]]
CUM = [-4.0, -1.5, -4.0]


def test_backtracking_cuts_after_eos_and_ranks_by_length_penalty():
    # row 1 is (2, 9): steps 3 -> row 2 at step 2 (token 9) -> row 2 at step 1 (token 9) -> row 1 at step 0 (token 2): cut after the first 9
    for fn in (beam_ref.backtrack, _product_backtrack):
        got = fn(PARENTS, TOKENS, CUM, 3, 9, 1.0)[0]
        assert [h[0] for h in got] == [[2, 9], [1, 5, 6, 8], [1, 5, 6, 3]]
        assert [h[1] for h in got] == [-1.5, -4.0, -4.0] and [h[2] for h in got] == [-0.75, -1.0, -1.0]      # the tie goes to the lower beam
        got = fn(PARENTS, TOKENS, CUM, 3, 9, 0.0)[0]
        assert [h[2] for h in got] == [-1.5, -4.0, -4.0]
        got = fn(PARENTS, TOKENS, [-4.0, -1.5, -3.0], 3, 9, 2.0)[0]                  # -4/16, -1.5/4, -3/16
        assert [h[0] for h in got] == [[1, 5, 6, 3], [1, 5, 6, 8], [2, 9]] and [h[2] for h in got] == [-0.1875, -0.25, -0.375]
        got = fn(PARENTS, TOKENS, CUM, 3, None, 1.0)[0]                              # no eos: nothing is cut
        assert [h[0] for h in got] == [[2, 9, 9, 9], [1, 5, 6, 8], [1, 5, 6, 3]] and [h[2] for h in got] == [-0.375, -1.0, -1.0]


def _product_backtrack(parents, tokens, cum, num_beams, eos, length_penalty):
    """the package's own host side, in the reference's shape"""
    from atom_amd.e2e import backtrack_beams
    return [[(h.tokens, h.sum_logprob, h.score) for h in hyps] for hyps in backtrack_beams(parents, tokens, cum, num_beams, eos, length_penalty)]


def test_backtracking_of_two_groups_stays_inside_each_group():
    parents = [[0, 0, 0, 0], [1, 0, 1, 1]]
    tokens = [[1, 2, 3, 4], [5, 6, 7, 8]]
    got = beam_ref.backtrack(parents, tokens, [-1, -2, -2, -1], 2)
    assert [h[0] for h in got[0]] == [[2, 5], [1, 6]] and [h[0] for h in got[1]] == [[4, 8], [4, 7]]
    assert _product_backtrack(parents, tokens, [-1, -2, -2, -1], 2, None, 1.0) == got


@pytest.mark.parametrize("P,W,G,starts", [(16, 4, 2, [5, 16]), (32, 2, 3, [31, 32, 1]), (16, 16, 1, [15])])
def test_ref_fork_keeps_the_ownership_invariant(P, W, G, starts):
    """200 rounds of step + fork with random parents on a cache laid out as StaticBeamKvCacheInt4 lays it out: after every fork no
    partial or reserve page is in two rows, the spares are in no table, every row's writable set is the one it had, and every row
    reads its lineage's tokens"""
    rnd = random.Random(P + W)
    steps = 200
    fresh = iter(range(10 ** 6))
    tables, spare, row_pages, lens, lineage = [], [], [], [], []
    cap = max(-(-(n + steps) // P) for n in starts)
    for g, n in enumerate(starts):
        prompt = [next(fresh) for _ in range(-(-n // P))]
        rp = -(-(n + steps) // P)
        for b in range(W):
            start = len(prompt) if b == 0 else n // P
            row = prompt[:start] + [next(fresh) for _ in range(rp - start)]
            tables.append(row + [row[-1]] * (cap - rp))
            spare.append(next(fresh))
            row_pages.append(rp)
            lens.append(n)
            lineage.append([(g, "prompt", i) for i in range(n)])
    all_pages = set(range(next(fresh)))
    content = np.zeros((len(all_pages), P), dtype=object)             # one tag per slot
    for g, n in enumerate(starts):
        for i in range(n):
            content[tables[g * W][i // P], i % P] = (g, "prompt", i)
    ref = beam_ref.RefBeamCache(tables, spare, row_pages, lens, P, W, [content])
    ref.fork([0] * (G * W))
    ref.check_ownership(all_pages)
    for step in range(steps):
        ref.step()
        for r in range(G * W):                                          # the forward: every row writes its new slot
            page, off = ref.slot(r, ref.lens[r] - 1)
            content[page, off] = (r, step)
            lineage[r] = lineage[r] + [(r, step)]
        parent = [rnd.randrange(W) for _ in range(G * W)]
        before = ref.writable()
        ref.fork(parent)
        assert ref.writable() == before
        ref.check_ownership(all_pages)
        lineage = [lineage[r - r % W + parent[r]] for r in range(G * W)]
        for r in range(G * W):
            assert [content[ref.slot(r, i)] for i in range(ref.lens[r])] == lineage[r], (step, r)
    assert ref.status == 0 and ref.lens == [n + steps for n in starts for _ in range(W)]
    ref.fork([W, -1] + [0] * (G * W - 2))                               # parents outside the group: the rows stay, the bit is set
    assert ref.status == beam_ref.BAD_PARENT and ref.writable() == before
    ref.check_ownership(all_pages)
