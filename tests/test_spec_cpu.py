"""CPU tests of speculative decoding's rules (tests/spec_ref.py): the n-gram drafter against a brute-force search and hand-written
cases, the host speculative loop against the plain one-token loop, and the argument checks of the new entry points -- the calls that
return before any launch."""
import random

import numpy as np
import pytest

from tests import spec_ref


# ------------------------------------------------------------------------------------------------ the draft rule
def _brute(h, K, nmax, nmin):
    """every (n, s) pair tested on its own, then ranked: n descending, s descending"""
    L = len(h)
    found = [(n, s) for n in range(nmin, nmax + 1) for s in range(L) if n < L and s + n <= L - 1
             and all(h[s + i] == h[L - n + i] for i in range(n))]
    if not found:
        return [h[-1]] * K, False
    n, s = max(found)
    return [h[s + n + j] if s + n + j < L else h[-1] for j in range(K)], True


def test_draft_rule_equals_brute_force_on_random_histories():
    rng = random.Random(7)
    hits = 0
    for _ in range(200):
        alphabet, L = rng.randint(2, 5), rng.randint(1, 60)
        h = [rng.randrange(alphabet) + 10 for _ in range(L)]
        nmin = rng.randint(1, 4)
        nmax, K = rng.randint(nmin, 8), rng.randint(1, 8)
        want, matched = _brute(h, K, nmax, nmin)
        cap = L + rng.randint(0, 3)
        row = h + [99] * (cap - L)
        assert spec_ref.draft_rule(row, L, K, nmax, nmin) == want
        assert spec_ref.draft_words(row, L, K, nmax, nmin) == want       # the kernel's one-maximum form
        hits += matched
    assert hits > 100                                        # small alphabets: most histories repeat an n-gram


def test_draft_rule_hand_written_cases():
    d = spec_ref.draft_rule
    for f in (spec_ref.draft_rule, spec_ref.draft_words):
        # a longer n beats a more recent shorter match: "1 2 3" occurs at 0, "3" alone again at 5
        assert f([1, 2, 3, 7, 8, 3, 9, 1, 2, 3], 10, 2, 3, 1) == [7, 8]
        assert f([1, 2, 3, 7, 8, 3, 9, 1, 2, 3], 10, 2, 1, 1) == [9, 1]
        # the most recent match of equal n wins
        assert f([5, 6, 1, 5, 6, 2, 5, 6], 8, 3, 2, 2) == [2, 5, 6]
        # a continuation shorter than K is padded with the last token
        assert f([4, 9, 4], 3, 4, 3, 1) == [9, 4, 4, 4]
        # no match
        assert f([1, 2, 3, 4], 4, 3, 3, 1) == [4, 4, 4]
        # len of 1, n, n + 1 (n = 2 .. 2): nothing can match below n + 1 tokens, and at n + 1 only a run does
        assert f([8], 1, 2, 2, 2) == [8, 8]
        assert f([8, 8], 2, 2, 2, 2) == [8, 8]
        assert f([8, 8, 8], 3, 2, 2, 2) == [8, 8]           # s = 0: hist[0:2] == hist[1:3], the continuation is hist[2]
        assert f([7, 8, 8], 3, 2, 2, 2) == [8, 8] and f([7, 8, 7], 3, 2, 1, 1) == [8, 7]
        # ngram_min keeps a shorter match out
        assert f([1, 2, 9, 3, 2], 5, 2, 3, 2) == [2, 2] and f([1, 2, 9, 3, 2], 5, 2, 3, 1) == [9, 3]
        # lengths outside the buffer: token 0
        assert f([1, 2, 3], 0, 2, 3, 1) == [0, 0] and f([1, 2, 3], 4, 2, 3, 1) == [0, 0] and f([1, 2, 3], -1, 2, 3, 1) == [0, 0]
    assert d([3, 3, 3, 3], 4, 1, 8, 1) == [3]


# ------------------------------------------------------------------------------------------------ the loop
def _toy(h):
    a, b = (h[-2] if len(h) > 1 else 3), h[-1]
    return (a * 31 + b * 17 + 5) % 7


@pytest.mark.parametrize("K", range(1, 9))
def test_speculative_loop_equals_the_plain_loop(K):
    prompt = [2, 5, 1]
    truth = spec_ref.plain_loop(_toy, prompt, 20 + K + 1)
    proposers = {
        "wrong": lambda h, n: [(truth[n + j] + 1) % 7 for j in range(K)],
        "right": lambda h, n: [truth[n + j] for j in range(K)],
        "mixed": lambda h, n: [truth[n + j] if (n + j) % 3 else (truth[n + j] + 1) % 7 for j in range(K)],
        "ngram": lambda h, n: spec_ref.draft_rule(h, len(h), K, 3, 1),
    }
    for budget in range(1, 21):
        want = spec_ref.plain_loop(_toy, prompt, budget)
        for name, propose in proposers.items():
            got, accepted, steps, counts = spec_ref.spec_loop(_toy, prompt, budget, K, propose)
            assert got == want, (name, budget)
            assert len(got) == 1 + accepted + steps        # the bookkeeping: every step emits its accepted drafts and one more token
            if name == "wrong":
                assert accepted == 0 and steps == budget - 1
            if name == "right":
                assert steps == -(-(budget - 1) // (K + 1)) and all(a == K for a in counts)


# ------------------------------------------------------------------------------------------------ the accept rule and step_rows on the host
def test_ref_accept_commits_the_agreed_prefix_and_clamps_at_the_budget():
    K = 3
    targets = np.array([[5, 6, 7, 8], [5, 6, 7, 8], [5, 6, 7, 8]])
    ids = np.array([[1, 5, 6, 9], [1, 5, 6, 9], [1, 4, 6, 7]])
    z = np.zeros(3, np.int32)
    o = spec_ref.accept(targets, ids, [1, 4, 2], [9, 5, 2], np.full((3, 9), -1), np.full((3, 12), -1), [3, 6, 4], z, z.astype(np.int64), z, z)
    assert o["adds"].tolist() == [3, 1, 0] and o["n_out"].tolist() == [4, 5, 2] and o["done"].tolist() == [0]
    assert o["tokens"][0].tolist() == [-1, 5, 6, 7, -1, -1, -1, -1, -1] and o["tokens"][1, 4] == 5 and (o["tokens"][2] == -1).all()
    assert o["input_ids"][:, 0].tolist() == [7, 5, 1] and o["hist_len"].tolist() == [6, 7, 4] and o["draw"].tolist() == [4, 5, 0]
    assert o["accepted"].tolist() == [2, 0, 0] and o["steps"].tolist() == [1, 1, 0] and K == targets.shape[1] - 1


def test_ref_step_rows_commits_and_looks_ahead():
    r = spec_ref.StepRows([15, 16, 1], [3, 3, 1], 16)
    r.step([0, 0, 0], 5)
    assert r.lens == [15, 16, 1] and r.tab == [20, 21, 6] and r.indptr == [0, 2, 4, 5] and r.last_page_offset == [4, 5, 6] and r.status == 0
    r.step([3, -1, 11], 5)                                   # a negative count is 0 and flagged; 1 + 11 + 5 > 16 overflows
    assert r.lens == [18, 16, 1] and r.tab == [23, 21, 1] and r.status == 3


# ------------------------------------------------------------------------------------------------ argument checks (no launch)
P = 0x10000


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def test_draft_entry_rejects_bad_arguments():
    L, lib = _lib()
    call = lambda hist=P, hl=P, batch=2, cap=64, nmin=1, nmax=3, K=4, out=P, ld=5: lib.atom_spec_draft_ngram(hist, hl, batch, cap, nmin, nmax, K, out, ld, None)
    for name in ("hist", "hl", "out"):
        assert call(**{name: None}) == L.ERR_INVALID_ARG
    for kw in (dict(batch=0), dict(batch=2 ** 31), dict(cap=0), dict(cap=2 ** 31), dict(K=0), dict(K=9), dict(nmin=0), dict(nmin=4), dict(nmax=9),
               dict(ld=3)):
        assert call(**kw) == L.ERR_SHAPE, kw
    assert call(hist=P + 2) == L.ERR_ALIGN and call(hl=P + 2) == L.ERR_ALIGN and call(out=P + 4) == L.ERR_ALIGN


def test_accept_entry_rejects_bad_arguments():
    L, lib = _lib()

    def call(ptrs=None, batch=2, K=4, max_new=16, cap=64):
        return lib.atom_spec_accept(*([P] * 12 if ptrs is None else ptrs), batch, K, max_new, cap, None)
    for i in range(12):
        assert call([P] * i + [None] + [P] * (11 - i)) == L.ERR_INVALID_ARG
    for kw in (dict(batch=0), dict(batch=2 ** 31), dict(K=0), dict(K=9), dict(max_new=0), dict(cap=0), dict(max_new=2 ** 31), dict(cap=2 ** 31)):
        assert call(**kw) == L.ERR_SHAPE, kw
    wide = (0, 1, 4, 8)                                      # targets, input_ids, tokens, draw: int64
    for i in range(12):
        by = 4 if i in wide else 2
        assert call([P] * i + [P + by] + [P] * (11 - i)) == L.ERR_ALIGN, i


def test_step_rows_entry_rejects_bad_arguments():
    L, lib = _lib()
    t = [P] * 7
    call = lambda ptrs=t, batch=2, cap=4, page=16, adds=P, look=5: lib.atom_kv_step_rows_i4(*ptrs, batch, cap, page, adds, look, None)
    assert call(batch=0) == L.ERR_SHAPE and call(cap=0) == L.ERR_SHAPE and call(page=24) == L.ERR_SHAPE and call(page=0) == L.ERR_SHAPE
    assert call(cap=2 ** 30, page=16) == L.ERR_SHAPE
    assert call(look=-1) == L.ERR_INVALID_ARG and call(adds=None) == L.ERR_INVALID_ARG and call(adds=P + 2) == L.ERR_ALIGN
    for i in range(7):
        assert call(t[:i] + [None] + t[i + 1:]) == L.ERR_INVALID_ARG
        assert call(t[:i] + [P + 2] + t[i + 1:]) == L.ERR_ALIGN


def test_sample_rows_entry_rejects_bad_arguments():
    L, lib = _lib()
    call = lambda logits=P, batch=6, vocab=100, step=P, rps=3, tokens=P, ld=100: lib.atom_sample_rows_f16(logits, ld, batch, vocab, None, None, None, None,
                                                                                                           step, rps, 0, tokens, None)
    assert call(step=None) == L.ERR_INVALID_ARG and call(logits=None) == L.ERR_INVALID_ARG and call(tokens=None) == L.ERR_INVALID_ARG
    for kw in (dict(rps=0), dict(rps=4), dict(batch=0), dict(vocab=0), dict(ld=99)):
        assert call(**kw) == L.ERR_SHAPE, kw
    assert call(step=P + 4) == L.ERR_ALIGN and call(logits=P + 1) == L.ERR_ALIGN


def test_speculative_params_are_validated():
    from atom_amd.e2e import SpeculativeParams
    assert SpeculativeParams() == SpeculativeParams(4, 3, 1, 8)
    for kw in (dict(num_draft_tokens=0), dict(num_draft_tokens=9), dict(ngram_min=0), dict(ngram_max=9), dict(ngram_max=2, ngram_min=3),
               dict(poll_every=0)):
        with pytest.raises(ValueError):
            SpeculativeParams(**kw)
    with pytest.raises(Exception):
        SpeculativeParams().num_draft_tokens = 2             # frozen
