"""Without a GPU: (1) every error of the sliding window's lower bound that tests/attn_window_ref.py can make (its MUTANTS) moves the
membership closed form by >= 10 x the bound tests/test_gpu_attn_window.py applies, at some planted-range position of
attn_planted.window_starts, for every case, window and mutant that applies (the margin of tests/test_attn_planted_cpu.py); (2) the
FP64 reference agrees with the closed form and, with the window off, with attn_planted.ref_prefill; (3) the host side of the _win entry
points: the symbols, the refusal of window < 1 behind every older fault, and the plan queries against the un-windowed ones."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import attn_host_tables as H
from tests import attn_planted as A
from tests import attn_window_ref as W

MARGIN = 10.0
CASES = [(c, False) for c in W.DECODE_CASES] + [(c, True) for c in W.PREFILL_CASES]


def _id(cp):
    return ("prefill-" if cp[1] else "decode-") + A.case_id(cp[0])


@pytest.mark.parametrize("cp", CASES, ids=_id)
def test_every_mutant_moves_the_closed_form(cp):
    case, prefill = cp
    _, P, nkv, G = case
    lens, qo, _, _ = W.case_shape(case, prefill)
    todo = [(win, m) for win in W.WINDOWS for m in W.MUTANTS if W.applies(lens, qo, win, m)]
    if prefill:                                              # the chunk-relative mutants bite in every prefill case at every window
        assert {m for _, m in todo} == set(W.MUTANTS) and all((win, "window_from_first_row") in todo for win in W.WINDOWS)
    else:
        assert not any(m in ("window_from_end", "window_from_first_row") for _, m in todo)
    best = dict.fromkeys(todo, 0.0)
    for w in A.window_starts(max(lens)):
        c = A.build_membership(lens, nkv, P, w, seed=3)
        for win in W.WINDOWS:                                # (G = 1: the group's query heads repeat their K/V head's row)
            want = W.membership_expected(c, qo, 1, win)
            bnd = A.bound(want, W.REL)
            for m in W.MUTANTS:
                if (win, m) in best:
                    moved = np.abs(W.membership_expected(c, qo, 1, win, mutate=m) - want).max(axis=-1) / bnd
                    best[win, m] = max(best[win, m], float(moved.max()))
    worst = min(best, key=best.get)
    print(f"{_id(cp)}: {len(best)} (window, mutant) pairs; the least: {worst} moves the closed form by {best[worst]:.0f} x the bound")
    assert best[worst] >= MARGIN, (worst, best[worst])


def test_closed_form_is_the_unmutated_one():
    """n = min(p + 1, W) keys per row, and a window that covers every sequence gives attn_planted's closed form"""
    case = W.PREFILL_CASES[1]
    lens, qo, _, _ = W.case_shape(case, True)
    c = A.build_membership(lens, case[2], case[1], 64, seed=3)
    want = A.membership_expected(c, qo, case[3])
    assert want.max() > 1.0
    assert np.abs(W.membership_expected(c, qo, case[3], 5000) - want).max() < 1e-12
    assert np.abs(W.membership_expected(c, qo, case[3], 100, mutate="no_window") - want).max() < 1e-12


@pytest.mark.parametrize("win", [1, 64, 100])
def test_reference_agrees_with_the_closed_form(win):
    """the FP64 reference on the membership cache IS the closed form (uniform softmax over the visible keys), mutants included; and
    without a bound it is attn_planted.ref_prefill"""
    shape = [(0, 64), (15, 16), (300, 7), (40, 150)]
    lens, qo = A.prefill_shape(shape)
    c = A.build_membership(lens, 2, 16, 192, seed=3)
    q = A.membership_queries(int(qo[-1]), 4, 3)
    for m in (None,) + tuple(m for m in W.MUTANTS if W.applies(lens, qo, win, m)):
        got = W.ref_prefill(q, c, qo, win, G=2, mutate=m)
        assert np.abs(got - W.membership_expected(c, qo, 2, win, mutate=m)).max() < 1e-9, m
    n = A.build_needle(lens, 2, 16, seed=5)
    qn = A.needle_queries(int(qo[-1]), 4, 5)
    assert np.abs(W.ref_prefill(qn, n, qo, win, G=2, mutate="no_window") - A.ref_prefill(qn, n, qo, G=2)).max() < 1e-12
    assert np.abs(W.ref_prefill(qn, n, qo, win, G=2) - A.ref_prefill(qn, n, qo, G=2)).max() > 1e-2


# ------------------------------------------------------------------------------------------------ the host side
_ROPE_WIN = [("rope_theta", 1e4), ("rope_scale", 1.0), ("rope_table", "null"), ("attn_scale", 1.0), ("window", 4), ("max_pages_per_seq", 0),
             ("workspace", "null"), ("workspace_bytes", 0), ("stream", "null")]
VALID = {
    "atom_batch_decode_gqa_i4_win": [("o", "mem"), ("q", "mem")] + H._KV + H._GQA + _ROPE_WIN,
    "atom_batch_prefill_gqa_i4_win": [("o", "mem"), ("q", "mem"), ("qo_indptr", "mem"), ("total_q", 3), ("max_q_len", 2)] + H._KV + H._GQA + _ROPE_WIN,
}


def _call(L, fn, **changes):
    names = [n for n, _ in VALID[fn]]
    assert set(changes) <= set(names), changes
    return getattr(L, fn)(*(H._value(changes.get(n, v)) for n, v in VALID[fn]))


@pytest.fixture(scope="module")
def L():
    from atom_amd._lib import lib
    return lib()


def test_symbols_resolve(L):
    from atom_amd import _lib
    for name in ("atom_batch_decode_gqa_i4_win", "atom_batch_prefill_gqa_i4_win", "atom_batch_decode_gqa_i4_win_workspace_bytes",
                 "atom_batch_decode_gqa_i4_win_splits", "atom_batch_prefill_gqa_i4_win_workspace_bytes"):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value


@pytest.mark.parametrize("fn", sorted(VALID))
def test_window_below_one_is_refused_behind_the_older_faults(L, fn):
    """host pointers: every call here must come back before a launch"""
    from atom_amd import _lib
    prefill = "prefill" in fn
    for win in (0, -1, -(1 << 31)):
        assert _call(L, fn, window=win) == _lib.ERR_INVALID_ARG                  # the only fault
        # one older fault with another code in front of it: the older code comes back
        assert _call(L, fn, window=win, head_dim=64) == _lib.ERR_SHAPE
        assert _call(L, fn, window=win, num_qo_heads=6) == _lib.ERR_SHAPE
        assert _call(L, fn, window=win, q="+8") == _lib.ERR_ALIGN
        assert _call(L, fn, window=win, kv_data="+8") == _lib.ERR_ALIGN
        assert _call(L, fn, window=win, rope_table="+2") == _lib.ERR_ALIGN      # the _rope entries' own fault: still in front
        assert _call(L, fn, window=win, batch=0) == _lib.ERR_SHAPE
        if prefill:
            assert _call(L, fn, window=win, total_q=0) == _lib.ERR_SHAPE
            assert _call(L, fn, window=win, total_q=(1 << 31) - 1) == _lib.ERR_SHAPE
        else:
            assert _call(L, fn, window=win, batch=1 << 30) == _lib.ERR_SHAPE
    # a valid window changes no older code (the calls the _rope entries refuse)
    for kw in (dict(q="null"), dict(rope_theta=0.0), dict(attn_scale=0.0), dict(attn_scale=float("nan"))):
        assert _call(L, fn, **kw) == _lib.ERR_INVALID_ARG
    assert _call(L, fn, head_dim=64) == _lib.ERR_SHAPE and _call(L, fn, o="+8") == _lib.ERR_ALIGN
    if not prefill:                                          # un-merged needs a split, as its parent
        assert _call(L, fn, o="null") == _lib.ERR_INVALID_ARG
        assert _call(L, fn, o="null", max_pages_per_seq=64) == _lib.ERR_INVALID_ARG


def test_plan_queries_follow_the_unwindowed_plan(L):
    """Never more splits (or workspace) than the un-windowed grouped-query plan of the shape, and its values once the window covers
    max_pages * page_size keys.  The windowed op is the grouped-query kernel at EVERY head ratio, so at G = 1 its decode plan is the
    grouped-query policy's, which the un-windowed G = 1 queries (they forward to the FP32 decode op's plan) do not expose: there the
    comparison is with the windowed plan whose window covers the cache."""
    n = 0
    for b, nkv, g, p, mp in itertools.product(H.BATCH, H.KV_HEADS, H.GROUP, H.PAGE, H.MAX_PAGES):
        cover = max(mp * p, 1)
        ds_full = L.atom_batch_decode_gqa_i4_win_splits(b, nkv * g, nkv, p, mp, cover)
        dw_full = L.atom_batch_decode_gqa_i4_win_workspace_bytes(b, nkv * g, nkv, p, mp, cover)
        if g > 1:
            assert ds_full == L.atom_batch_decode_gqa_i4_splits(b, nkv * g, nkv, p, mp)
            assert dw_full == L.atom_batch_decode_gqa_i4_workspace_bytes(b, nkv * g, nkv, p, mp)
        assert dw_full == (b * nkv * g * ds_full * 130 * 4 if ds_full > 1 else 0)
        pw_full = [L.atom_batch_prefill_gqa_i4_workspace_bytes(T, b, nkv * g, nkv, p, mq, mp) for T, mq in H.PREFILL]
        assert pw_full == [L.atom_batch_prefill_gqa_i4_win_workspace_bytes(T, b, nkv * g, nkv, p, mq, mp, cover) for T, mq in H.PREFILL]
        for win in W.WINDOWS + (4096, (1 << 31) - 1):
            ds = L.atom_batch_decode_gqa_i4_win_splits(b, nkv * g, nkv, p, mp, win)
            assert 1 <= ds <= ds_full, (b, nkv, g, p, mp, win, ds, ds_full)
            assert L.atom_batch_decode_gqa_i4_win_workspace_bytes(b, nkv * g, nkv, p, mp, win) == (b * nkv * g * ds * 130 * 4 if ds > 1 else 0)
            for (T, mq), full in zip(H.PREFILL, pw_full):
                assert L.atom_batch_prefill_gqa_i4_win_workspace_bytes(T, b, nkv * g, nkv, p, mq, mp, win) <= full
            if win >= cover:
                assert ds == ds_full
            n += 1
    assert n > 30000


def test_plan_queries_reject(L):
    """window < 1, and what the parents' queries reject: 0"""
    for win in (0, -5):
        assert L.atom_batch_decode_gqa_i4_win_splits(8, 8, 4, 16, 64, win) == 0
        assert L.atom_batch_decode_gqa_i4_win_workspace_bytes(1, 8, 4, 16, 256, win) == 0
        assert L.atom_batch_prefill_gqa_i4_win_workspace_bytes(8, 1, 8, 4, 16, 8, 256, win) == 0
    assert L.atom_batch_decode_gqa_i4_win_workspace_bytes(1, 8, 4, 16, 256, 4096) > 0
    assert L.atom_batch_prefill_gqa_i4_win_workspace_bytes(8, 1, 8, 4, 16, 8, 256, 4096) > 0
    for a in ((0, 8, 4, 16, 64), (1, 0, 4, 16, 64), (1, 8, 0, 16, 64), (1, 8, 4, 8, 64), (1, 6, 4, 16, 64), (1, -8, 4, 16, 64)):
        assert L.atom_batch_decode_gqa_i4_win_splits(*a, 64) == 0 and L.atom_batch_decode_gqa_i4_win_workspace_bytes(*a, 64) == 0
    for a in ((8, 0, 8, 4, 16, 8, 256), (8, 1, 6, 4, 16, 8, 256), (0, 1, 8, 4, 16, 8, 256), (8, 1, 8, 4, 16, 0, 256), (8, 1, 8, 4, 8, 8, 256)):
        assert L.atom_batch_prefill_gqa_i4_win_workspace_bytes(*a, 64) == 0
