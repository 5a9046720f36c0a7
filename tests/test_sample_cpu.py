"""CPU-only checks of the sampler: the entry point's argument validation (it precedes the launch, so no GPU is needed), the
reference (tests/sample_ref.py) against the contract's known answers, against a float64 softmax and against its own frequencies, and
the planted families of tests/sample_cases.py: each must tell its rule from the obvious wrong one."""
import numpy as np
import pytest

from tests import sample_cases, sample_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _call(lib, logits=P, ld=1000, batch=4, vocab=1000, T=P, k=P, p=P, seeds=P, step=P, off=0, tokens=P):
    return lib.atom_sample_f16(logits, ld, batch, vocab, T, k, p, seeds, step, off, tokens, None)


def test_new_symbols_resolve():
    L, lib = _lib()
    assert "atom_sample_f16" in L.SIGNATURES and hasattr(lib, "atom_sample_f16")
    from atom_amd import ops
    from atom_amd.e2e import DecodeGraph, Sampler, SamplingParams, generate  # noqa: F401
    assert callable(ops.sample)
    assert SamplingParams() == SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=0)


def test_sample_rejects_bad_arguments():
    L, lib = _lib()
    assert _call(lib, logits=None) == L.ERR_INVALID_ARG and _call(lib, tokens=None) == L.ERR_INVALID_ARG
    assert _call(lib, batch=0) == L.ERR_SHAPE and _call(lib, batch=-1) == L.ERR_SHAPE
    assert _call(lib, vocab=0, ld=0) == L.ERR_SHAPE and _call(lib, vocab=0) == L.ERR_SHAPE
    assert _call(lib, vocab=262145, ld=262145) == L.ERR_SHAPE
    assert _call(lib, ld=999) == L.ERR_SHAPE and _call(lib, ld=-1000) == L.ERR_SHAPE
    assert _call(lib, logits=P + 1) == L.ERR_ALIGN
    for name, by in (("T", 2), ("k", 2), ("p", 1), ("seeds", 4), ("step", 4), ("tokens", 4), ("tokens", 2)):
        assert _call(lib, **{name: P + by}) == L.ERR_ALIGN, name
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _call(lib, logits=None, batch=0) == L.ERR_INVALID_ARG and _call(lib, batch=0, tokens=P + 2) == L.ERR_SHAPE


def test_ops_sample_refuses_cpu_tensors_and_wrong_types():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    with pytest.raises(AtomHipError):
        ops.sample(torch.zeros((2, 8), dtype=torch.float16))
    from atom_amd.e2e import Sampler, SamplingParams
    with pytest.raises(ValueError):
        Sampler(3, "cpu", [SamplingParams()] * 2)
    s = Sampler(2, "cpu", [SamplingParams(0.5, 3, 0.25, 2 ** 64 - 1), SamplingParams(seed=2 ** 63)])
    assert s.seeds.tolist() == [-1, -2 ** 63] and s.top_k.tolist() == [3, 0] and s.temperature.tolist() == [0.5, 1.0]


def test_philox_known_answers():
    assert sample_ref.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert sample_ref.philox4x32_10([ones] * 4, [ones] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert sample_ref.draw_word(0, 0) == 0x6627E8D5 and sample_ref.draw_word(-1, -1) != sample_ref.draw_word(0, 0)


def test_equal_logits_cross_check():
    """2^18 equal logits, T = 1, k and p off, seed 5: the token is R >> 14"""
    row = np.full(1 << 18, 0x3C00, dtype=np.uint16)
    got = [sample_ref.sample_row(row, 1.0, 0, 1.0, 5, s) for s in range(3)]
    assert got == [200797, 91021, 252626] == [sample_ref.draw_word(5, s) >> 14 for s in range(3)]


def test_weight_function_properties():
    """the maximum's weight is exactly 2^40, every weight is at most 2^41, -inf and x < -40 weigh nothing"""
    l = sample_ref.canonical(sample_cases.half_bits([3.0, 3.0, 2.999, -60.0, 1.0]))
    l[4] = -np.inf
    for T in (2.0 ** -10, 0.7, 1.0, 1024.0):
        w = sample_ref.weights(l, np.float32(T))
        assert int(w[0]) == int(w[1]) == 1 << 40 and int(w.max()) <= 1 << 41 and int(w[4]) == 0
    assert int(sample_ref.weights(l, np.float32(1.0))[3]) == 0 and int(sample_ref.weights(l, np.float32(1024.0))[3]) > 0


@pytest.mark.parametrize("T", [0.7, 1.0, 1.5])
def test_probabilities_match_a_float64_softmax(T):
    """bound 5e-6 relative on tokens of probability > 1e-6: the polynomial's 3.7e-7 plus three float32 roundings of |x| <= 20"""
    rng = np.random.default_rng(11)
    bits = sample_cases.half_bits(rng.normal(0.0, 3.0, 1000))
    got = sample_ref.probabilities(bits, T)
    l = bits.view(np.float16).astype(np.float64)
    e = np.exp((l - l.max()) / float(np.float32(T)))
    want = e / e.sum()
    live = want > 1e-6
    err = float(np.abs(got[live] / want[live] - 1).max())
    print(f"T = {T}: {int(live.sum())} tokens above 1e-6, worst relative error {err:.3g}")
    assert live.sum() > 100 and err <= 5e-6


def test_frequencies_follow_the_reference_probabilities():
    """20,000 seeds at one step: chi-square against the reference's own probabilities, 6 degrees of freedom, 0.999 quantile 22.46"""
    bits = sample_cases.half_bits([2, 1, 1, 0, -1, -3, -np.inf, 0.5])
    n = 20000
    counts = np.zeros(8)
    for seed in range(n):
        counts[sample_ref.sample_row(bits, 1.0, 0, 1.0, seed, 3)] += 1
    prob = sample_ref.probabilities(bits, 1.0)
    live = [0, 1, 2, 3, 4, 5, 7]
    chi2 = float((((counts - n * prob) ** 2)[live] / (n * prob[live])).sum())
    print("chi-square", chi2, "counts", counts.tolist())
    assert counts[6] == 0 and prob[6] == 0 and chi2 < 22.46


def test_boundary_steps_land_on_a_cumulative_weight():
    for steps, n, shift in ((sample_cases.BOUNDARY_STEPS_2_18, 1 << 18, 14), (sample_cases.BOUNDARY_STEPS_2_16, 1 << 16, 16)):
        for s in steps:
            r = sample_ref.draw_word(sample_cases.BOUNDARY_SEED, s)
            assert r % (1 << shift) == 0
            target = ((n << 40) * r) >> 32
            assert target % (1 << 40) == 0 and 0 < target < (n << 40)


@pytest.mark.parametrize("wrong", sample_ref.WRONG)
def test_planted_families_tell_the_rule_from_the_wrong_one(wrong):
    cases = [c for c in sample_cases.planted() if c.tells == wrong]
    assert cases
    total = 0
    for c in cases:
        changed = sum(a != b for s in c.steps for a, b in zip(sample_cases.expected(c, s), sample_cases.expected(c, s, wrong=wrong)))
        print(f"{wrong}: {c.name} changes {changed} of {len(c.steps) * len(c.seeds)} draws")
        assert changed > 0, c.name
        total += changed
    assert total > 0


def test_planted_cases_stay_inside_the_row_and_the_masked_tokens_are_never_drawn():
    for c in sample_cases.planted():
        l = sample_ref.canonical(c.bits)
        for s in c.steps[:1]:
            for t in sample_cases.expected(c, s):
                assert 0 <= t < c.bits.size
                assert l.max() == -np.inf or l[t] > -np.inf, c.name
