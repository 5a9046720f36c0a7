"""CPU tests of the rolling-cache references (tests/kv_ring_ref.py): the ring step walked token by token agrees with a brute-force
"which pages hold the keys a step's rows see", never lists the slot that is about to be reused, and stays inside its ring whatever the
buffers hold; on the cases tests/test_gpu_kv_ring.py runs, the FP64 reader of a rolling cache is the windowed reference of the
un-released cache, reads none of the 0xFF bytes, and each of its mutants leaves it by >= 10 x the bound the GPU test applies."""
import numpy as np
import pytest

from tests import attn_planted as A
from tests import attn_window_ref as W
from tests import kv_ring_ref as K

MARGIN = 10.0


def _brute_pages(n, add, window, P):
    """the logical pages that hold a key some row of the step sees: rows at n - max(add, 1) .. n - 1, keys (p - W, p]; and the pages
    of the step's own tokens.  (add = 0: the tables of the length n as a step of one token left them)"""
    rows = range(max(n - max(add, 1), 0), n)
    keys = {j for p in rows for j in range(max(p - window + 1, 0), p + 1)}
    return sorted({j // P for j in keys})


@pytest.mark.parametrize("P,window,add", [(16, 1, 1), (16, 16, 1), (16, 17, 1), (16, 63, 1), (48, 100, 1), (16, 40, 5), (48, 17, 5),
                                          (16, 100, 3)])
def test_walk_from_empty_agrees_with_brute_force(P, window, add):
    R = K.ring_size(window, P, add)
    table = np.arange(100, 100 + R)[None, :]
    lens, n, written = np.array([0]), 0, {}                  # written: slot -> the logical page whose tokens it holds
    steps = (3 * R * P) // add + 2
    assert steps * add >= 3 * R * P                          # at least three wraps of the ring
    for _ in range(steps):
        lens2, indptr, indices, lpo, start, status = K.ring_step(table, [R], lens, add, window, P)
        n += add
        assert status == 0 and lens2[0] == n
        want = _brute_pages(n, add, window, P)
        f, cnt = start[0] // P, indptr[1]
        assert start[0] % P == 0 and list(range(f, f + cnt)) == want, (n, f, cnt, want)
        assert cnt <= K.ring_size(window, P, add) and lpo[0] == (n - 1) % P + 1
        assert [int(x) for x in indices] == [100 + g % R for g in want]                  # logical order, slot g % R
        # the step's tokens go to the pages of positions n - add .. n - 1: a slot that gets a NEW tenant held no listed page
        for g in sorted({p // P for p in range(n - add, n)}):
            slot = g % R
            if written.get(slot, g) != g:
                assert written[slot] < f, (n, g, written[slot], f)
            written[slot] = g
        assert all(written[g % R] == g for g in want)        # every listed page still holds its own tokens
        lens = lens2
    # add = 0 rebuilds the tables of the current length
    lens3, indptr, indices, lpo, start, status = K.ring_step(table, [R], lens, 0, window, P)
    assert status == 0 and lens3[0] == n and list(range(start[0] // P, start[0] // P + indptr[1])) == _brute_pages(n, 0, window, P)


@pytest.mark.parametrize("P,window", [(16, 16), (48, 100), (16, 63)])
def test_overflow_and_bad_lengths_set_the_bits_and_leave_the_row_legal(P, window):
    R = K.ring_size(window, P, 1)
    table = np.arange(7 * (R + 2)).reshape(7, R + 2)
    rows = [R, R - 1, R + 2, 0, R, R, R]
    # row 1: a ring one page short; row 3: no slot; rows 4-6: corrupted lengths
    lens = np.array([5, 0, 9, 0, -3, K.INT_MAX, K.INT_MAX - 1])
    seen_overflow = False
    for step in range(3 * R * P):
        lens2, indptr, indices, lpo, start, status = K.ring_step(table, rows, lens, 1, window, P)
        for b in range(7):
            cnt, Rb = indptr[b + 1] - indptr[b], min(rows[b], R + 2)
            assert 0 <= cnt <= Rb
            assert set(indices[indptr[b]:indptr[b + 1]]) <= set(table[b, :Rb])             # nothing from outside the row
            assert 0 <= lens2[b] and (lpo[b] == 0) == (lens2[b] == 0) and start[b] % P == 0 and 0 <= start[b] <= max(lens2[b], 0)
        assert lens2[0] == lens[0] + 1 and lens2[2] == lens[2] + 1                        # the healthy rows advance exactly
        assert lens2[3] == 0
        if step == 0:
            assert status & K.BAD_LENGTH and lens2[4] == 1
        if lens2[1] == lens[1]:
            seen_overflow = True
            assert status & K.OVERFLOW
        else:
            assert not seen_overflow                         # once refused, always refused: the row keeps its length
        lens = lens2
    assert seen_overflow and status & K.OVERFLOW


def _cases():
    return [(c, False) for c in K.DECODE_CASES] + [(c, True) for c in K.PREFILL_CASES]


def _id(cp):
    return ("prefill-" if cp[1] else "decode-") + K.case_id(cp[0])


def _ring_case(case, prefill, win, seed=5):
    _, P, nkv, G, _ = case
    lens, qo_ref, _, _, adds, max_add = K.case_shape(case, prefill)
    c = A.build_needle(lens, nkv, P, seed=seed)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, seed)
    return c, K.ring_cache(c, win, K.ring_size(win, P, max_add), adds), qn, qo_ref


@pytest.mark.parametrize("cp", _cases(), ids=_id)
def test_ring_reader_is_the_window_reference_and_reads_no_stale_byte(cp):
    case, prefill = cp
    G, memo = case[3], {}
    for win in case[4]:
        c, rc, qn, qo = _ring_case(case, prefill, win)
        reads = {}
        got = K.ring_prefill(qn, rc, qo, win, G=G, reads=reads)
        want = W.ref_prefill(qn, c, qo, win, G=G, memo=memo)
        assert reads["bad"] == 0 and np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-9, win
        # the cache does hold the sentinel: every slot without a live page, and the bytes behind every end
        assert np.isnan(rc["param"].astype(np.float32)).any()
    # ring_cache's tables against ring_step's, sequence by sequence with its own add
    win = case[4][-1]
    c, rc, _, _ = _ring_case(case, prefill, win)
    adds = K.case_shape(case, prefill)[4]
    for b, (S, a) in enumerate(zip(c["seqlens"], adds)):
        lens2, indptr, indices, lpo, start, status = K.ring_step(rc["table"][b:b + 1], [rc["R"]], [S - a], a, win, case[1])
        assert status == 0 and lens2[0] == S and start[0] == rc["kv_start"][b] and lpo[0] == rc["lpo"][b]
        assert list(indices) == list(rc["indices"][rc["indptr"][b]:rc["indptr"][b + 1]])


@pytest.mark.parametrize("cp", _cases(), ids=_id)
def test_every_mutant_moves_the_reference(cp):
    case, prefill = cp
    G = case[3]
    moved_by, skipped = {}, 0
    for win in case[4]:
        c, rc, qn, qo = _ring_case(case, prefill, win)
        want = K.ring_prefill(qn, rc, qo, win, G=G)
        bnd = A.bound(want, K.REL)
        for m in K.MUTANTS:
            if not K.applies(rc, qo, win, m):
                skipped += 1
                continue
            got = K.ring_prefill(qn, rc, qo, win, G=G, mutate=m)
            diff = np.where(np.isfinite(got), np.abs(got - want), np.inf).max(axis=-1) / bnd    # a NaN read: moved beyond any bound
            moved_by[win, m] = float(diff.max())
    assert {m for _, m in moved_by} == set(K.MUTANTS)        # every mutant bites at some window of every case
    worst = min(moved_by, key=moved_by.get)
    print(f"{_id(cp)}: {len(moved_by)} (window, mutant) pairs ({skipped} change nothing); the least: {worst} moves the reference by "
          f"{moved_by[worst]:.0f} x the bound")
    assert moved_by[worst] >= MARGIN, (worst, moved_by[worst])
