"""CPU-only checks of the log-probability op: the entry point's argument validation (it precedes the launch, so no GPU is needed),
the reference (tests/logprob_ref.py) against the contract's known answers and against a float64 log-softmax, and the planted
families of tests/logprob_cases.py: each must tell its rule from the obvious wrong one."""
import numpy as np
import pytest

from tests import logprob_cases, logprob_ref
from tests.sample_cases import half_bits

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _call(lib, logits=P, ld=1000, rows=4, vocab=1000, targets=P, logprob=P, rank=P, top_n=5, top_ids=P, top_lp=P):
    return lib.atom_logprob_f16(logits, ld, rows, vocab, targets, logprob, rank, top_n, top_ids, top_lp, None)


def test_new_symbols_resolve():
    L, lib = _lib()
    assert "atom_logprob_f16" in L.SIGNATURES and hasattr(lib, "atom_logprob_f16")
    from atom_amd import ops
    from atom_amd.e2e import DecodeGraph, TokenLogprobs, generate, perplexity, score  # noqa: F401
    assert callable(ops.logprob) and callable(score) and callable(perplexity)
    assert [f.name for f in __import__("dataclasses").fields(TokenLogprobs)] == ["token_logprobs", "token_ranks", "top_ids", "top_logprobs"]


def test_logprob_rejects_bad_arguments():
    L, lib = _lib()
    assert _call(lib, logits=None) == L.ERR_INVALID_ARG
    assert _call(lib, top_ids=None) == L.ERR_INVALID_ARG and _call(lib, top_lp=None) == L.ERR_INVALID_ARG
    assert _call(lib, top_n=1, top_ids=None) == L.ERR_INVALID_ARG
    # nothing to do: no top-n and no targets, or targets with neither output
    assert _call(lib, top_n=0, logprob=None, rank=None) == L.ERR_INVALID_ARG
    assert _call(lib, top_n=0, targets=None) == L.ERR_INVALID_ARG
    assert _call(lib, rows=0) == L.ERR_SHAPE and _call(lib, rows=-1) == L.ERR_SHAPE
    assert _call(lib, vocab=0, ld=0) == L.ERR_SHAPE and _call(lib, vocab=0) == L.ERR_SHAPE
    assert _call(lib, vocab=262145, ld=262145) == L.ERR_SHAPE
    assert _call(lib, ld=999) == L.ERR_SHAPE and _call(lib, ld=-1000) == L.ERR_SHAPE
    assert _call(lib, top_n=33) == L.ERR_SHAPE and _call(lib, top_n=-1) == L.ERR_SHAPE
    assert _call(lib, top_n=-1, top_ids=None, top_lp=None) == L.ERR_SHAPE
    assert _call(lib, logits=P + 1) == L.ERR_ALIGN
    for name, by in (("targets", 4), ("logprob", 2), ("rank", 2), ("top_ids", 4), ("top_lp", 2), ("rank", 1), ("targets", 2)):
        assert _call(lib, **{name: P + by}) == L.ERR_ALIGN, name
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _call(lib, logits=None, rows=0) == L.ERR_INVALID_ARG and _call(lib, rows=0, rank=P + 2) == L.ERR_SHAPE


def test_ops_logprob_refuses_cpu_tensors_and_wrong_types():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    with pytest.raises(AtomHipError):
        ops.logprob(torch.zeros((2, 8), dtype=torch.float16), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AtomHipError):
        ops.logprob(torch.zeros((2, 8), dtype=torch.float16), None, 3)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises((TypeError, AtomHipError)):
            ops.logprob(torch.zeros((2, 8), dtype=dtype), None, 3)
    from atom_amd.e2e import DecodeGraph  # noqa: F401
    from atom_amd.e2e.generate import _check_logprobs
    assert _check_logprobs(None) is None and _check_logprobs(0) == 0 and _check_logprobs(32) == 32
    for bad in (-1, 33):
        with pytest.raises(ValueError):
            _check_logprobs(bad)


def test_equal_logits_known_answer():
    """2^18 equal logits: Z = 2^58, every lp = float32(-18 ln 2), rank = t"""
    row = np.full(1 << 18, 0x3C00, dtype=np.uint16)
    want = np.float32(-18.0 * np.log(2.0))
    assert abs(float(want) + 12.476649) < 1e-6
    for t in (0, 1, 12345, (1 << 18) - 1):
        r = logprob_ref.logprob_row(row, t, 3)
        assert r.z == 1 << 58 and r.logprob == want and r.rank == t
        assert r.top_ids.tolist() == [0, 1, 2] and (r.top_logprobs == want).all()


def test_one_hot_known_answer():
    """one token at 65504 among tokens at -65504: Z = 2^40, lz = 0, lp = 0 and -131008"""
    row = half_bits([-65504.0] * 100)
    row[37] = half_bits([65504.0])[0]
    a, b = logprob_ref.logprob_row(row, 37, 2), logprob_ref.logprob_row(row, 5, 2)
    assert a.z == 1 << 40 and a.lz == 0 and a.logprob == 0 and a.rank == 0
    assert b.logprob == np.float32(-131008.0) and b.rank == 6
    assert a.top_ids.tolist() == [37, 0] and a.top_logprobs.tolist() == [0.0, -131008.0]


def test_vocab_one():
    for value in (2.5, -np.inf, np.nan):
        r = logprob_ref.logprob_row(half_bits([value]), 0, 2)
        lp = 0.0 if value == 2.5 else -np.inf
        assert r.logprob == lp and r.rank == 0 and r.top_ids.tolist() == [0, -1] and r.top_logprobs.tolist() == [lp, -np.inf]
        r = logprob_ref.logprob_row(half_bits([value]), 1, 0)
        assert r.logprob == 0 and r.rank == -1


@pytest.mark.parametrize("vocab", [7, 1000, 8193, 32000, 128256, 1 << 18])
def test_reference_matches_a_float64_log_softmax(vocab):
    """|lp - exact| <= 5e-6 + 2^-22 + 2^-23 |exact|: the weight function's relative bound (tests/test_sample_cpu.py), the most that
    the dropped tail weights of vocab <= 2^18 tokens can move Z, and the two float32 roundings."""
    worst = 0.0
    for sigma in (1.0, 3.0, 8.0):
        rng = np.random.default_rng(vocab + int(sigma))
        bits = half_bits(rng.normal(0.0, sigma, vocab))
        l = bits.view(np.float16).astype(np.float64)
        exact = (l - l.max()) - np.log(np.exp(l - l.max()).sum())
        targets = rng.integers(0, vocab, 8).tolist() + [int(l.argmax()), int(l.argmin())]
        r = logprob_ref.logprob_row(bits, None, min(32, vocab))
        got = {int(i): float(x) for i, x in zip(r.top_ids, r.top_logprobs)}
        for t in targets:
            got[t] = float(logprob_ref.logprob_row(bits, t).logprob)
        for t, lp in got.items():
            bound = 5e-6 + 2.0 ** -22 + 2.0 ** -23 * abs(exact[t])
            worst = max(worst, abs(lp - exact[t]) / bound)
            assert abs(lp - exact[t]) <= bound, (sigma, t, lp, exact[t])
    print(f"vocab {vocab}: worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("wrong", logprob_ref.WRONG)
def test_planted_families_tell_the_rule_from_the_wrong_one(wrong):
    cases = [c for c in logprob_cases.planted() if wrong in c.tells]
    assert cases
    for c in cases:
        right = logprob_ref.logprob(c.bits, c.targets, c.top_n)
        other = logprob_ref.logprob(c.bits, c.targets, c.top_n, wrong=wrong)
        changed = sum(a.rank != b.rank or a.logprob != b.logprob or a.top_ids.tolist() != b.top_ids.tolist()
                      or a.top_logprobs.tolist() != b.top_logprobs.tolist() for a, b in zip(right, other))
        print(f"{wrong}: {c.name} changes {changed} of {len(right)} rows")
        assert changed > 0, c.name


def test_planted_families_hold_what_they_name():
    by = {c.name: c for c in logprob_cases.planted()}
    assert len(by) == 9
    r = logprob_ref.logprob(by["ties_across_top_n"].bits, by["ties_across_top_n"].targets, 3)
    assert r[0].top_ids.tolist() == [2, 1, 3] and [x.rank for x in r] == [0, 1, 6, 7]
    r = logprob_ref.logprob(by["target_in_a_run"].bits, by["target_in_a_run"].targets, 0)
    assert [x.rank for x in r] == [2 + 4, 2, 2 + 9, 1]
    c = by["special_values"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert r[0].top_ids.tolist() == [1, 2, 7, 8, 6, 3, 4, 0, 5]
    assert [x.rank for x in r] == [7, 0, 1, 5, 6, 8, 4, 2] and r[0].logprob == -np.inf == r[5].logprob
    assert r[1].logprob == r[2].logprob == r[7].logprob
    c = by["neg_inf_target"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert [x.rank for x in r] == [3, 4, 5] and all(x.logprob == -np.inf for x in r)
    c = by["all_neg_inf"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert [x.rank for x in r] == c.targets and all(x.logprob == -np.inf for x in r)
    assert r[0].top_ids.tolist() == [0, 1, 2, 3] and (r[0].top_logprobs == -np.inf).all()
    c = by["ignored_targets"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert [(x.logprob, x.rank) for x in r[:4]] == [(0.0, -1)] * 4 and r[4].rank >= 0 and r[4].logprob < 0
    c = by["top_n_over_vocab"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert r[0].top_ids.tolist() == [1, 2, 4, 0, 3, -1, -1, -1] and r[0].top_logprobs[4:].tolist() == [-np.inf] * 4
    c = by["top_32"]
    r = logprob_ref.logprob(c.bits, c.targets, c.top_n)
    assert [x.rank for x in r[:3]] == [0, 31, 32] and r[0].top_ids[31] == c.targets[1] and c.targets[2] not in r[0].top_ids
    l = c.bits[0].view(np.float16)
    assert l[c.targets[1]] == l[c.targets[2]], "the top-32 boundary must cut a run of equal logits"
