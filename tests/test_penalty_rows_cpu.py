"""CPU-only checks of the penalties under speculative decoding: the reference tests/penalty_rows_ref.py against the
token-by-token path it must equal, its mutants against the planted sequences of tests/penalty_rows_cases.py, the argument validation
of atom_penalize_rows_f16 (it precedes the launch, so no GPU is needed) and the Python surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests import penalty_cases, penalty_ref, penalty_rows_cases, penalty_rows_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = penalty_rows_cases.planted()


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _call(lib, logits=P, ld=1000, batch=4, rows=5, vocab=1000, state=3 * P, state_ld=1000, ids=P, ids_ld=5, ctok=P, commit_ld=5, ccnt=P,
          rep=P, pres=P, freq=P, bids=P, bvals=P, max_bias=16, out=2 * P, out_ld=1000):
    return lib.atom_penalize_rows_f16(logits, ld, batch, rows, vocab, state, state_ld, ids, ids_ld, ctok, commit_ld, ccnt, rep, pres, freq,
                                      bids, bvals, max_bias, out, out_ld, None)


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_equals_the_token_by_token_path(case):
    """row j is what ``penalty_ref.penalize_row(fed=)`` writes after the pending tokens and drafts 1 .. j went through a scratch copy
    of the state one at a time, and the state is the one after the pending tokens alone"""
    out, words = penalty_rows_cases.expected(case)
    want, after = penalty_rows_ref.sequential(case.bits, case.words, case.ids, case.pending, case.count, case.rep, case.pres, case.freq,
                                              case.bias_ids, case.bias_vals)
    assert out.dtype == np.uint16 and out.shape == case.bits.shape
    assert np.array_equal(out, want) and np.array_equal(words, after)


def test_reference_on_random_sequences_equals_the_token_by_token_path():
    rng = np.random.default_rng(4)
    for rows in (1, 2, 9):
        vocab = 300
        bits = np.stack([penalty_cases.background(rng, vocab) for _ in range(rows)])
        words = np.where(rng.random(vocab) < 0.2, rng.integers(0, 5, vocab), 0).astype(np.uint16)
        words |= np.where(rng.random(vocab) < 0.1, 0x8000, 0).astype(np.uint16)
        ids = rng.integers(-2, 12, rows).tolist()                      # few values: drafts repeat, some are out of range
        pending = rng.integers(-2, 12, 9).tolist()
        for count in (0, 1, 9, 12):
            args = (bits, words, ids, pending, count, 1.3, 0.4, 0.7, [3, 250, 5], [1.0, -2.0, float("-inf")])
            out, after = penalty_rows_ref.penalize_rows_seq(*args)
            want, want_after = penalty_rows_ref.sequential(*args)
            assert np.array_equal(out, want) and np.array_equal(after, want_after), (rows, count)


def test_batched_reference_and_commit_only_form():
    three = CASES[:3]
    bits = np.concatenate([c.bits for c in three])
    state = np.stack([c.words for c in three])
    pend = [(c.pending + [0] * 9)[:9] for c in three]
    out, after = penalty_rows_ref.penalize_rows(bits, state, [c.ids for c in three], pend, [c.count for c in three],
                                                [c.rep for c in three], [c.pres for c in three], [c.freq for c in three])
    for b, c in enumerate(three):
        o, w = penalty_rows_cases.expected(c)
        assert np.array_equal(out[b * penalty_rows_cases.ROWS:(b + 1) * penalty_rows_cases.ROWS], o) and np.array_equal(after[b], w)
    none, only = penalty_rows_ref.penalize_rows(None, state, None, pend, [c.count for c in three])
    assert none is None and np.array_equal(only, after)


@pytest.mark.parametrize("wrong", penalty_rows_ref.WRONG)
def test_every_mutant_is_caught_by_a_planted_case(wrong):
    cases = [c for c in CASES if wrong in c.tells]
    assert cases
    for c in cases:
        out, words = penalty_rows_cases.expected(c)
        bad, bad_words = penalty_rows_cases.expected(c, wrong=wrong)
        changed = int((out != bad).sum()) + int((words != bad_words).sum())
        print(f"{wrong}: {c.name} changes {changed} words")
        assert changed > 0, c.name


def test_planted_cases_cover_the_contract():
    by_name = {c.name: c for c in CASES}
    assert len(by_name) == len(CASES)
    V = penalty_rows_cases.VOCAB
    assert penalty_rows_cases.expected(by_name["count_32766"])[0] is not None
    out, words = penalty_rows_cases.expected(by_name["count_32767"])
    assert words[penalty_rows_cases.TILE] == 32767 and words[penalty_rows_cases.TILE - 1] == 0xFFFF
    c = by_name["neutral"]
    out, words = penalty_rows_cases.expected(c)
    assert np.array_equal(out, c.bits) and words[1] == 4 and words[penalty_rows_cases.TILE] == 0x8001 and words[V - 1] == 1
    c = by_name["out_of_range"]
    out, words = penalty_rows_cases.expected(c)
    assert words[3] == 1 and int((words != c.words).sum()) == 1
    assert np.array_equal(penalty_rows_cases.expected(by_name["count_negative"])[1], by_name["count_negative"].words)
    assert penalty_rows_cases.expected(by_name["count_large"])[1][8] == 2
    assert penalty_rows_ref.clamp_count(40, 12) == 9 and penalty_rows_ref.clamp_count(40, 3) == 3 and penalty_rows_ref.clamp_count(-3, 3) == 0
    for c in CASES:                                        # drafts never reach the state: it is the one after the pending tokens
        want = c.words.copy()
        for t in c.pending[:penalty_rows_ref.clamp_count(c.count, len(c.pending))]:
            if 0 <= t < V:
                want[t] = penalty_ref.count_up(want[t])
        assert np.array_equal(penalty_rows_cases.expected(c)[1], want), c.name


# ------------------------------------------------------------------------------------------------ 2. argument validation
def test_symbol_and_signature():
    L, lib = _lib()
    assert "atom_penalize_rows_f16" in L.SIGNATURES and hasattr(lib, "atom_penalize_rows_f16")
    res, args = L.SIGNATURES["atom_penalize_rows_f16"]
    assert res is ctypes.c_int and len(args) == 21
    with open(os.path.join(ROOT, "include", "atom_hip.h")) as f:
        assert "int atom_penalize_rows_f16(" in f.read()


def test_penalize_rows_rejects_null_pointers():
    L, lib = _lib()
    assert _call(lib, state=None) == L.ERR_INVALID_ARG and _call(lib, ids=None) == L.ERR_INVALID_ARG
    assert _call(lib, logits=None) == L.ERR_INVALID_ARG and _call(lib, out=None) == L.ERR_INVALID_ARG        # exactly one of the two
    assert _call(lib, ctok=None) == L.ERR_INVALID_ARG and _call(lib, ccnt=None) == L.ERR_INVALID_ARG         # exactly one of the two
    assert _call(lib, logits=None, out=None, ctok=None, ccnt=None) == L.ERR_INVALID_ARG                      # nothing to do
    assert _call(lib, logits=None, out=None, state=None) == L.ERR_INVALID_ARG
    assert _call(lib, bids=None) == L.ERR_INVALID_ARG and _call(lib, bvals=None) == L.ERR_INVALID_ARG
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _call(lib, ids=None, batch=0) == L.ERR_INVALID_ARG and _call(lib, batch=0, out=2 * P + 1) == L.ERR_SHAPE


def test_penalize_rows_rejects_bad_shapes():
    L, lib = _lib()
    for kw in (dict(batch=0), dict(batch=-1), dict(batch=65536), dict(rows=0), dict(rows=10, ids_ld=10), dict(rows=-1),
               dict(batch=1 << 40), dict(rows=1 << 40, ids_ld=1 << 40), dict(vocab=0), dict(vocab=0, ld=0, out_ld=0, state_ld=0),
               dict(vocab=262145, ld=262145, out_ld=262145, state_ld=262145), dict(ld=999), dict(ld=-1000), dict(out_ld=999),
               dict(state_ld=999), dict(ids_ld=4), dict(commit_ld=0), dict(commit_ld=-1), dict(max_bias=513), dict(max_bias=-1),
               dict(max_bias=1 << 40), dict(out=P, out_ld=1008)):
        assert _call(lib, **kw) == L.ERR_SHAPE, kw
    assert _call(lib, max_bias=513, ids=P + 4) == L.ERR_SHAPE             # ... before the alignment
    assert _call(lib, logits=None, out=None, ids=None, state_ld=999) == L.ERR_SHAPE
    assert _call(lib, logits=None, out=None, ids=None, rows=0) == L.ERR_SHAPE


def test_penalize_rows_rejects_misaligned_pointers():
    L, lib = _lib()
    for name, by in (("logits", 1), ("out", 1), ("state", 1), ("ids", 4), ("ids", 2), ("ctok", 4), ("ctok", 1), ("ccnt", 2), ("rep", 2),
                     ("pres", 2), ("freq", 1), ("bids", 2), ("bvals", 2)):
        base = {"out": 2 * P, "state": 3 * P}.get(name, P)
        assert _call(lib, **{name: base + by}) == L.ERR_ALIGN, name
    assert _call(lib, logits=None, out=None, ids=None, ctok=P + 4) == L.ERR_ALIGN      # the commit alone is checked as well
    assert _call(lib, ctok=None, ccnt=None, max_bias=0, bids=None, bvals=None, rep=P + 2) == L.ERR_ALIGN


# ------------------------------------------------------------------------------------------------ 3. the Python surface
def test_ops_penalize_rows_checks_its_arguments_on_the_host():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    assert ops.PENALTY_MAX_ROWS == ops.GUIDE_MAX_ROWS == 9
    names = list(inspect.signature(ops.penalize_rows).parameters)
    assert names == ["logits", "state", "input_ids", "commit_tokens", "commit_counts", "repetition", "presence", "frequency", "bias_ids",
                     "bias_vals", "out"]
    with pytest.raises(TypeError):
        ops.penalize_rows(torch.zeros((2, 8), dtype=torch.float16), torch.zeros((2, 8), dtype=torch.int16), torch.zeros((2, 1), dtype=torch.int64))
    with pytest.raises((TypeError, AtomHipError)):
        ops.penalize_rows(torch.zeros((2, 8), dtype=torch.float16), None, None)


def test_speculative_params_gain_a_last_argument_that_defaults_to_off():
    """``penalised`` comes last in the constructor, after ``force_drafts``, and takes part in ==, hash and repr; the six fields that were
    there, and what ``dataclasses.astuple`` gives, stay as they were"""
    import dataclasses
    from atom_amd.e2e import SpeculativeParams
    assert list(inspect.signature(SpeculativeParams).parameters)[-2:] == ["force_drafts", "penalised"]
    assert inspect.signature(SpeculativeParams).parameters["penalised"].default is False
    assert SpeculativeParams() == SpeculativeParams(penalised=False) and SpeculativeParams().penalised is False
    assert SpeculativeParams() != SpeculativeParams(penalised=True) and hash(SpeculativeParams()) == hash(SpeculativeParams(penalised=False))
    assert SpeculativeParams(4, 3, 1, 8, False, True) == SpeculativeParams()
    assert SpeculativeParams(4, 3, 1, 8, False, True, True) == SpeculativeParams(penalised=True) != SpeculativeParams(guided=True, penalised=True)
    assert len({SpeculativeParams(), SpeculativeParams(penalised=False), SpeculativeParams(penalised=True)}) == 2
    assert "penalised=True" in repr(SpeculativeParams(penalised=True)) and "penalised=False" in repr(SpeculativeParams())
    assert dataclasses.astuple(SpeculativeParams(penalised=True)) == (4, 3, 1, 8, False, True)
    with pytest.raises(dataclasses.FrozenInstanceError):
        SpeculativeParams().penalised = True
    with pytest.raises(ValueError):
        SpeculativeParams(num_draft_tokens=0, penalised=True)


PENALTY_FIELDS = (dict(repetition_penalty=1.3), dict(presence_penalty=0.5), dict(frequency_penalty=0.25), dict(logit_bias={3: 1.0}))


def _check(**kw):
    from atom_amd.e2e.generate import _check_combination
    args = dict(caches=None, return_logits=False, sampling=None, logprobs=None, num_beams=None, speculative=None, drafter=None,
                return_spec_stats=False, guide=None)
    args.update(kw)
    return _check_combination(**args)


@pytest.mark.parametrize("field", PENALTY_FIELDS, ids=[next(iter(f)) for f in PENALTY_FIELDS])
def test_penalised_speculation_takes_every_penalty_field(field):
    from atom_amd.e2e import SamplingParams, SpeculativeParams
    for spec in (SpeculativeParams(penalised=True), SpeculativeParams(penalised=True, guided=True)):
        assert _check(speculative=spec, sampling=SamplingParams(**field)) is None
        assert _check(speculative=spec, sampling=[SamplingParams(), SamplingParams(**field)], return_spec_stats=True) is None
    with pytest.raises(ValueError) as e:
        _check(speculative=SpeculativeParams(), sampling=SamplingParams(**field))
    assert str(e.value) == f"generate: speculative does not combine with {next(iter(field))}"


def test_penalised_speculation_refuses_what_speculation_refuses():
    from atom_amd.e2e import SamplingParams, SpeculativeParams
    spec, s = SpeculativeParams(penalised=True), SamplingParams(frequency_penalty=0.5, logit_bias={3: 1.0})
    for kw, name in ((dict(logprobs=0), "logprobs"), (dict(return_logits=True), "return_logits"), (dict(caches=[]), "caches"),
                     (dict(num_beams=2), "num_beams")):
        with pytest.raises(ValueError) as e:
            _check(speculative=spec, sampling=s, **kw)
        assert str(e.value) == f"generate: speculative does not combine with {name}"
    with pytest.raises(ValueError) as e:
        _check(speculative=spec, sampling=s, num_beams=2, logprobs=0, return_logits=True, caches=[])
    assert str(e.value) == "generate: speculative does not combine with num_beams, logprobs, return_logits, caches"


def test_graph_and_penalties_take_the_new_arguments():
    from atom_amd.e2e import LogitPenalties
    from atom_amd.e2e.generate import SpecDecodeGraph
    assert "penalties" in inspect.signature(SpecDecodeGraph.__init__).parameters
    assert list(inspect.signature(LogitPenalties.apply_rows).parameters) == ["self", "logits", "input_ids", "commit_tokens", "commit_counts", "out"]
    assert list(inspect.signature(LogitPenalties.commit).parameters) == ["self", "tokens", "counts"]
