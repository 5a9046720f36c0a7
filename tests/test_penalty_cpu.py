"""CPU-only checks of the logit penalties: the entry point's argument validation (it precedes the launch, so no GPU is needed), the
Python surface (ops.penalize, SamplingParams, LogitPenalties on "cpu"), the reference (tests/penalty_ref.py) against an independent
float64 formulation and against a host build of csrc/penalty_math.h on every fp16 pattern, and the planted families of
tests/penalty_cases.py: each must tell its rule from the obvious wrong one."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import penalty_cases, penalty_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _call(lib, logits=P, ld=1000, batch=4, vocab=1000, state=P, state_ld=1000, fed=P, rep=P, pres=P, freq=P, ids=P, vals=P, max_bias=16,
          out=2 * P, out_ld=1000):
    return lib.atom_penalize_f16(logits, ld, batch, vocab, state, state_ld, fed, rep, pres, freq, ids, vals, max_bias, out, out_ld, None)


# ------------------------------------------------------------------------------------------------ 1. symbols and API
def test_new_symbols_resolve():
    L, lib = _lib()
    assert "atom_penalize_f16" in L.SIGNATURES and hasattr(lib, "atom_penalize_f16")
    res, args = L.SIGNATURES["atom_penalize_f16"]
    assert res is ctypes.c_int and len(args) == 16
    from atom_amd import ops
    from atom_amd.e2e import DecodeGraph, LogitPenalties, SamplingParams, generate  # noqa: F401
    assert callable(ops.penalize) and ops.PENALTY_MAX_BIAS == 512 and ops.PENALTY_TILE >= 8 and ops.PENALTY_TILE % 8 == 0
    with open(os.path.join(ROOT, "include", "atom_hip.h")) as f:
        assert "int atom_penalize_f16(" in f.read()


def test_sampling_params_keep_their_positions_and_gain_neutral_defaults():
    from atom_amd.e2e import SamplingParams
    d = SamplingParams()
    assert d == SamplingParams(1.0, 0, 1.0, 0)
    assert (d.repetition_penalty, d.presence_penalty, d.frequency_penalty, d.logit_bias) == (1.0, 0.0, 0.0, None)
    q = SamplingParams(0.5, 3, 0.25, 9, 1.3, 0.5, 0.25, {7: -1.0})
    assert (q.temperature, q.top_k, q.top_p, q.seed, q.repetition_penalty, q.presence_penalty, q.frequency_penalty) == (0.5, 3, 0.25, 9, 1.3, 0.5, 0.25)
    assert not d.penalises and q.penalises
    assert not SamplingParams(repetition_penalty=0.0).penalises and not SamplingParams(repetition_penalty=-1.0, logit_bias={}).penalises
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=-0.5), dict(frequency_penalty=0.1), dict(logit_bias={3: 0.0})):
        assert SamplingParams(**kw).penalises, kw


def test_ops_penalize_refuses_cpu_tensors():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    with pytest.raises(AtomHipError):
        ops.penalize(torch.zeros((2, 8), dtype=torch.float16))


def test_logit_penalties_fill_their_buffers():
    import torch
    from atom_amd.e2e import LogitPenalties, SamplingParams
    inf = float("inf")
    params = [SamplingParams(repetition_penalty=1.3, logit_bias={9: -inf, 2: 1.5, 4: 0.0}), SamplingParams(),
              SamplingParams(presence_penalty=0.5, frequency_penalty=-0.25, logit_bias={0: 2.0})]
    lp = LogitPenalties(3, 10, "cpu", params)
    assert lp.max_bias == 3 and lp.state.dtype == torch.int16 and lp.state.shape == (3, 16) and not lp.state.any()
    assert lp.bias_ids.dtype == torch.int32 and lp.bias_ids.tolist() == [[2, 4, 9], [-1, -1, -1], [0, -1, -1]]
    assert lp.bias_vals.dtype == torch.float32 and lp.bias_vals.tolist() == [[1.5, 0.0, -inf], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    assert lp.repetition.tolist() == [np.float32(1.3), 1.0, 1.0] and lp.presence.tolist() == [0.0, 0.0, 0.5]
    assert lp.frequency.tolist() == [0.0, 0.0, -0.25]
    addresses = [t.data_ptr() for t in (lp.state, lp.repetition, lp.presence, lp.frequency, lp.bias_ids, lp.bias_vals)]
    lp.reset([[1, 2, 2, 9], [0], [3, 10, -1, 12345]])                      # ids outside the vocabulary are skipped
    want = np.zeros((3, 16), dtype=np.int16)
    want[0, [1, 2, 9]] = want[1, 0] = want[2, 3] = -32768
    assert np.array_equal(lp.state.numpy(), want)
    lp.state[1, 5] = 7
    lp.set(SamplingParams(frequency_penalty=2.0))                         # in place: the same buffers, the state untouched
    assert addresses == [t.data_ptr() for t in (lp.state, lp.repetition, lp.presence, lp.frequency, lp.bias_ids, lp.bias_vals)]
    assert lp.frequency.tolist() == [2.0] * 3 and lp.bias_ids.tolist() == [[-1] * 3] * 3 and int(lp.state[1, 5]) == 7
    lp.reset([[1], [1], [1]])
    assert int(lp.state[1, 5]) == 0 and lp.state[:, 1].tolist() == [-32768] * 3
    with pytest.raises(ValueError):
        lp.set([SamplingParams()] * 2)
    with pytest.raises(ValueError):
        lp.set(SamplingParams(logit_bias={i: 1.0 for i in range(4)}))      # more entries than the table holds
    with pytest.raises(ValueError):
        lp.set(SamplingParams(logit_bias={-1: 1.0}))
    full = LogitPenalties(1, 1000, "cpu", SamplingParams(logit_bias={i: float(i) for i in range(512)}))
    assert full.max_bias == 512 and full.bias_ids[0].tolist() == list(range(512))
    with pytest.raises(ValueError):
        LogitPenalties(1, 1000, "cpu", SamplingParams(logit_bias={i: 1.0 for i in range(513)}))
    with pytest.raises(ValueError):
        LogitPenalties(1, 1000, "cpu", max_bias=513)
    assert LogitPenalties(2, 8, "cpu", max_bias=5).bias_ids.tolist() == [[-1] * 5] * 2


# ------------------------------------------------------------------------------------------------ 2. argument validation
def test_penalize_rejects_null_pointers():
    L, lib = _lib()
    assert _call(lib, logits=None) == L.ERR_INVALID_ARG and _call(lib, out=None) == L.ERR_INVALID_ARG
    assert _call(lib, state=None) == L.ERR_INVALID_ARG                   # fed without state
    assert _call(lib, ids=None) == L.ERR_INVALID_ARG and _call(lib, vals=None) == L.ERR_INVALID_ARG
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _call(lib, logits=None, batch=0) == L.ERR_INVALID_ARG and _call(lib, state=None, vocab=0) == L.ERR_INVALID_ARG
    assert _call(lib, batch=0, out=2 * P + 1) == L.ERR_SHAPE


def test_penalize_rejects_bad_shapes():
    L, lib = _lib()
    for kw in (dict(batch=0), dict(batch=-1), dict(batch=65536), dict(vocab=0), dict(vocab=0, ld=0, out_ld=0, state_ld=0),
               dict(vocab=262145, ld=262145, out_ld=262145, state_ld=262145), dict(ld=999), dict(ld=-1000), dict(out_ld=999),
               dict(state_ld=999), dict(max_bias=513), dict(max_bias=-1), dict(max_bias=1 << 40),
               dict(out=P, out_ld=1008)):
        assert _call(lib, **kw) == L.ERR_SHAPE, kw
    assert _call(lib, max_bias=513, fed=P + 4) == L.ERR_SHAPE             # ... before the alignment
    assert _call(lib, state=None, fed=None, state_ld=0, batch=0) == L.ERR_SHAPE   # state_ld is not looked at without state


def test_penalize_rejects_misaligned_pointers():
    L, lib = _lib()
    for name, by in (("logits", 1), ("out", 1), ("state", 1), ("fed", 4), ("fed", 2), ("rep", 2), ("pres", 2), ("freq", 1), ("ids", 2), ("vals", 2)):
        base = 2 * P if name == "out" else P
        assert _call(lib, **{name: base + by}) == L.ERR_ALIGN, name
    assert _call(lib, state=None, fed=None, state_ld=0, rep=P + 2) == L.ERR_ALIGN


# ------------------------------------------------------------------------------------------------ 3. planted families
@pytest.mark.parametrize("wrong", penalty_ref.WRONG)
def test_planted_families_tell_the_rule_from_the_wrong_one(wrong):
    cases = [c for c in penalty_cases.planted() if c.tells == wrong]
    assert cases
    for c in cases:
        out, _ = penalty_cases.expected(c)
        bad, _ = penalty_cases.expected(c, wrong=wrong)
        changed = int((out != bad).sum())
        print(f"{wrong}: {c.name} changes {changed} output words")
        assert changed > 0, c.name


def test_planted_cases_copy_what_is_neither_seen_nor_biased():
    names = set()
    for c in penalty_cases.planted():
        assert c.name not in names
        names.add(c.name)
        out, words = penalty_cases.expected(c)
        after = words != 0
        plain = ~after
        plain[[i for i in c.bias_ids if 0 <= i < c.bits.size]] = False
        assert plain.sum() > c.bits.size // 2 and np.array_equal(out[plain], c.bits[plain]), c.name
        assert out.dtype == np.uint16 and words.dtype == np.uint16, c.name


def test_count_saturates_and_keeps_the_flag():
    assert [penalty_ref.count_up(w) for w in (0, 1, 32766, 32767, 0x8000, 0xFFFE, 0xFFFF)] == [1, 2, 32767, 32767, 0x8001, 0xFFFF, 0xFFFF]
    by_name = {c.name: c for c in penalty_cases.planted()}
    assert penalty_cases.expected(by_name["count_32766"])[1][0] == 32767
    assert penalty_cases.expected(by_name["count_32767"])[1][0] == 32767
    c = by_name["count_32767_prompt"]
    assert penalty_cases.expected(c)[1][c.fed] == 0xFFFF


# ------------------------------------------------------------------------------------------------ 4. an independent formulation
def _float64_formulation(logits, words, rep, pres, freq, bias):
    """the HF / vLLM way, in float64: scores of seen tokens divided or multiplied, minus frequency * counts, minus presence * (counts
    > 0), plus the bias"""
    x = logits.astype(np.float64)
    count = (words & 0x7FFF).astype(np.float64)
    seen = words != 0
    x = np.where(seen, np.where(x > 0, x / rep, x * rep), x)
    x = x - freq * count - pres * (count > 0)
    for i, v in bias.items():
        x[i] += v
    return x


@pytest.mark.parametrize("rep,pres,freq", [(1.3, 0.0, 0.0), (1.0, 0.5, 0.25), (0.8, -0.5, 0.1), (2.0, 1.5, 0.7)])
def test_reference_matches_a_float64_formulation(rep, pres, freq):
    """|logit| of a few units, counts up to 20, |bias| up to 5: every intermediate stays below 64, where an fp16 ulp is at most 2^-5
    and the FP32 roundings (2^-18 each at most) cannot move the result by more than one fp16 ulp of the exact value"""
    rng = np.random.default_rng(int(rep * 100 + pres * 10))
    vocab = 5000
    logits = rng.normal(0.0, 3.0, vocab).astype(np.float16)
    words = np.where(rng.random(vocab) < 0.3, rng.integers(0, 21, vocab), 0).astype(np.uint16)
    words |= np.where(rng.random(vocab) < 0.1, 0x8000, 0).astype(np.uint16)
    bias = {int(i): float(v) for i, v in zip(rng.choice(vocab, 40, replace=False), rng.normal(0.0, 2.5, 40).astype(np.float32))}
    got, _ = penalty_ref.penalize_row(logits.view(np.uint16), words, None, rep, pres, freq, list(bias), list(bias.values()))
    want = _float64_formulation(logits, words, float(np.float32(rep)), float(np.float32(pres)), float(np.float32(freq)), bias)
    touched = words != 0
    touched[list(bias)] = True
    assert np.array_equal(got[~touched], logits.view(np.uint16)[~touched]) and touched.sum() > 1000
    g = got.view(np.float16).astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    err = np.abs(g - want)[touched] / ulp[touched]
    print(f"rep {rep} pres {pres} freq {freq}: {int(touched.sum())} touched, worst error {err.max():.3f} fp16 ulp")
    assert np.abs(want).max() < 64 and err.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 5. the kernel's arithmetic, built for the host
WRAPPER = r"""
#include "penalty_math.h"
namespace pm = atom::penalty;
extern "C" void penalise_all(uint32_t word, float rep, float pres, float freq, int biased, float bias, uint16_t *out) {
  float r;
  const bool on = pm::repetition(rep, r), neutral = pm::neutral(on, r, pres, freq) && !biased;
  for (uint32_t bits = 0; bits < 65536u; ++bits) {
    float l = pm::penalise(bits, word, on, r, pres, freq);
    if (biased) l = l + bias;
    out[bits] = (uint16_t)((neutral || (word == 0 && !biased)) ? bits : pm::half_bits(l));
  }
}
extern "C" uint32_t count_up(uint32_t word) { return pm::count_up(word); }
"""


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("penalty_math")
    with open(os.path.join(ROOT, "atom_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    flags = [x for x in re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split() if not x.startswith("--offload-arch")]
    assert "-ffp-contract=off" in flags
    src, so = tmp / "penalty_host.cpp", tmp / "penalty_host.so"
    src.write_text(WRAPPER)
    cmd = [hipcc, "-x", "c++"] + flags + ["-shared", "-I", os.path.join(ROOT, "atom_amd", "csrc"), str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    lib.penalise_all.argtypes = [ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    lib.penalise_all.restype = None
    lib.count_up.argtypes, lib.count_up.restype = [ctypes.c_uint32], ctypes.c_uint32
    return lib


HOST_SETS = [  # (rep, pres, freq, count, flag, bias or None)
    (1.3, 0.0, 0.0, 1, 0, None), (1.3, 0.0, 0.0, 0, 1, None), (0.7, 0.5, 0.25, 3, 1, None), (1.0, 0.37, 0.1, 32767, 0, None),
    (1.0, 0.0, 0.0, 0, 0, 1.5), (1.0, 0.0, 0.0, 0, 0, float("-inf")), (2.0, -0.5, 0.013, 7, 0, -3.25), (1e9, 0.0, 0.0, 2, 0, None),
    (1e-9, 0.0, 0.0, 2, 0, None), (-1.0, 1.0, 1.0, 5, 1, 0.1), (float("nan"), 0.0, 0.5, 1, 0, None), (1.1, 0.0, float("inf"), 0, 1, 2.0),
    (1.0, 0.0, 0.0, 4, 1, None), (1.0, 0.0, 0.0, 0, 0, None), (3.0, 100.0, 3.0, 20000, 1, 60000.0), (1.0, 0.0, 0.0, 1, 0, 0.0),
]


@pytest.mark.parametrize("rep,pres,freq,count,flag,bias", HOST_SETS)
def test_host_build_of_the_arithmetic_equals_the_reference_on_every_pattern(host_math, rep, pres, freq, count, flag, bias):
    word = count | (flag << 15)
    got = np.zeros(65536, dtype=np.uint16)
    host_math.penalise_all(word, rep, pres, freq, int(bias is not None), 0.0 if bias is None else bias, got.ctypes.data)
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want, _ = penalty_ref.penalize_row(bits, np.full(65536, word, dtype=np.uint16), None, rep, pres, freq,
                                       [] if bias is None else list(range(65536)), [] if bias is None else [bias] * 65536)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(b)), hex(int(got[b])), hex(int(want[b]))) for b in bad[:8]]


def test_host_count_up_equals_the_reference(host_math):
    for w in list(range(0, 70000, 997)) + [32766, 32767, 32768, 65534, 65535]:
        w &= 0xFFFF
        assert host_math.count_up(w) == penalty_ref.count_up(w), w
