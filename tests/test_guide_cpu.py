"""CPU-only checks of guided decoding: the two entry points' argument validation (it precedes the launch, so no GPU is needed), the
Python surface (ops.guide_*, TokenAutomaton, LogitGuide on "cpu"), a host build of csrc/guide_math.h against tests/guide_ref.py on the
planted cases of tests/guide_cases.py, and TokenAutomaton.from_regex against Python's ``re`` on every token sequence of length 0 .. 4
over a 12-token vocabulary."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import guide_cases, guide_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _mask(lib, logits=P, ld=1000, batch=4, vocab=1000, state=3 * P, mask=4 * P, mask_ld=32, num_states=10, out=2 * P, out_ld=1000,
          status=5 * P):
    return lib.atom_guide_mask_f16(logits, ld, batch, vocab, state, mask, mask_ld, num_states, out, out_ld, status, None)


def _advance(lib, state=P, tokens=2 * P, batch=4, indptr=3 * P, edge_tok=4 * P, edge_next=5 * P, num_states=10, num_edges=50,
             status=6 * P):
    return lib.atom_guide_advance(state, tokens, batch, indptr, edge_tok, edge_next, num_states, num_edges, status, None)


# ------------------------------------------------------------------------------------------------ 1. symbols and API
def test_new_symbols_resolve():
    L, lib = _lib()
    for name, nargs in (("atom_guide_mask_f16", 12), ("atom_guide_advance", 10)):
        assert name in L.SIGNATURES and hasattr(lib, name)
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    from atom_amd import ops
    from atom_amd.e2e import DecodeGraph, LogitGuide, TokenAutomaton, generate  # noqa: F401
    assert callable(ops.guide_mask) and callable(ops.guide_advance) and ops.GUIDE_TILE == 2048
    assert (ops.GUIDE_FREE, ops.GUIDE_DEAD, ops.GUIDE_REJECTED, ops.GUIDE_BAD_STATE) == (-1, -2, 1, 2)
    assert (guide_ref.FREE, guide_ref.DEAD, guide_ref.REJECTED, guide_ref.BAD_STATE) == (-1, -2, 1, 2)
    with open(os.path.join(ROOT, "include", "atom_hip.h")) as f:
        header = f.read()
    assert "int atom_guide_mask_f16(" in header and "int atom_guide_advance(" in header
    for name, value in (("FREE", "(-1)"), ("DEAD", "(-2)"), ("REJECTED", "1"), ("BAD_STATE", "2")):
        assert re.search(rf"^#define ATOM_GUIDE_{name} {re.escape(value)}$", header, re.M), name


def test_ops_guide_refuse_cpu_tensors():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    i32 = lambda *a: torch.zeros(a, dtype=torch.int32)
    with pytest.raises(AtomHipError):
        ops.guide_mask(torch.zeros((2, 8), dtype=torch.float16), i32(2), i32(3, 1))
    with pytest.raises(AtomHipError):
        ops.guide_advance(i32(2), torch.zeros(2, dtype=torch.int64), i32(4), i32(5), i32(5))


# ------------------------------------------------------------------------------------------------ 2. argument validation
def test_mask_rejects_null_pointers():
    L, lib = _lib()
    for name in ("logits", "state", "mask", "out", "status"):
        assert _mask(lib, **{name: None}) == L.ERR_INVALID_ARG, name
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _mask(lib, logits=None, batch=0) == L.ERR_INVALID_ARG and _mask(lib, batch=0, out=2 * P + 1) == L.ERR_SHAPE


def test_mask_rejects_bad_shapes():
    L, lib = _lib()
    for kw in (dict(batch=0), dict(batch=-1), dict(batch=65536), dict(vocab=0), dict(vocab=0, ld=0, out_ld=0, mask_ld=0),
               dict(vocab=262145, ld=262145, out_ld=262145, mask_ld=8193), dict(ld=999), dict(ld=-1000), dict(out_ld=999),
               dict(mask_ld=31), dict(mask_ld=0), dict(mask_ld=-32), dict(num_states=0), dict(num_states=-1),
               dict(num_states=1 << 26, mask_ld=32), dict(num_states=1 << 40), dict(mask_ld=1 << 40), dict(out=P, out_ld=1008)):
        assert _mask(lib, **kw) == L.ERR_SHAPE, kw
    assert _mask(lib, num_states=0, state=3 * P + 2) == L.ERR_SHAPE        # ... before the alignment


def test_mask_rejects_misaligned_pointers():
    L, lib = _lib()
    for name, base, by in (("logits", P, 1), ("out", 2 * P, 1), ("state", 3 * P, 2), ("state", 3 * P, 1), ("mask", 4 * P, 2), ("mask", 4 * P, 1),
                           ("status", 5 * P, 2)):
        assert _mask(lib, **{name: base + by}) == L.ERR_ALIGN, name


def test_advance_rejects_bad_arguments():
    L, lib = _lib()
    for name in ("state", "tokens", "indptr", "edge_tok", "edge_next", "status"):
        assert _advance(lib, **{name: None}) == L.ERR_INVALID_ARG, name
    assert _advance(lib, state=None, batch=0) == L.ERR_INVALID_ARG
    for kw in (dict(batch=0), dict(batch=-1), dict(batch=65536), dict(num_states=0), dict(num_states=-5), dict(num_states=1 << 31),
               dict(num_edges=-1), dict(num_edges=1 << 31)):
        assert _advance(lib, **kw) == L.ERR_SHAPE, kw
    assert _advance(lib, batch=0, tokens=2 * P + 4) == L.ERR_SHAPE
    for name, base, by in (("state", P, 2), ("tokens", 2 * P, 4), ("tokens", 2 * P, 2), ("indptr", 3 * P, 2), ("edge_tok", 4 * P, 1),
                           ("edge_next", 5 * P, 2), ("status", 6 * P, 2)):
        assert _advance(lib, **{name: base + by}) == L.ERR_ALIGN, name


# ------------------------------------------------------------------------------------------------ 3. the rules, built for the host
WRAPPER = r"""
#include "guide_math.h"
namespace gm = atom::guide;
extern "C" void advance_all(const int32_t *states, const int64_t *tokens, int64_t n, const int32_t *indptr, const int32_t *edge_tok,
                            const int32_t *edge_next, int64_t num_states, int64_t num_edges, int32_t *out, int32_t *status) {
  for (int64_t i = 0; i < n; ++i) {
    int32_t bits = 0;
    out[i] = gm::advance(states[i], tokens[i], indptr, edge_tok, edge_next, num_states, num_edges, bits);
    status[i] = bits;
  }
}
// one element in state s: its mask word is looked up exactly as the contract says
extern "C" uint32_t mask_one(uint32_t bits, int32_t s, int64_t num_states, const uint32_t *mask, int64_t mask_ld, uint32_t v) {
  if (gm::row_kind(s, num_states) != gm::kMasked) return bits;
  return gm::select(bits, gm::allowed(mask[(int64_t)s * mask_ld + (v >> 5)], v));
}
extern "C" int row_kind(int32_t s, int64_t num_states) { return gm::row_kind(s, num_states); }
"""


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("guide_math")
    with open(os.path.join(ROOT, "atom_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "guide.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1) and "guide_math.h" in re.search(r"^HDRS := (.*)$", mk, re.M).group(1)
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    flags = [x for x in re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split() if not x.startswith("--offload-arch")]
    src, so = tmp / "guide_host.cpp", tmp / "guide_host.so"
    src.write_text(WRAPPER)
    cmd = [hipcc, "-x", "c++"] + flags + ["-shared", "-I", os.path.join(ROOT, "atom_amd", "csrc"), str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    lib.advance_all.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 2 + [ctypes.c_void_p] * 2
    lib.advance_all.restype = None
    lib.mask_one.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]
    lib.mask_one.restype = ctypes.c_uint32
    lib.row_kind.argtypes, lib.row_kind.restype = [ctypes.c_int32, ctypes.c_int64], ctypes.c_int
    return lib


def test_host_advance_equals_the_reference_on_every_planted_case(host_math):
    indptr, tok, nxt = guide_cases.advance_table()
    states, tokens = guide_cases.advance_pairs()
    S, E = indptr.size - 1, tok.size
    s_np, t_np = np.array(states, dtype=np.int32), np.array(tokens, dtype=np.int64)
    out, status = np.zeros(len(states), dtype=np.int32), np.zeros(len(states), dtype=np.int32)
    host_math.advance_all(s_np.ctypes.data, t_np.ctypes.data, len(states), indptr.ctypes.data, tok.ctypes.data, nxt.ctypes.data, S, E,
                          out.ctypes.data, status.ctypes.data)
    want = [guide_ref.advance_one(s, t, indptr, tok, nxt, S, E) for s, t in zip(states, tokens)]
    assert [(int(a), int(b)) for a, b in zip(out, status)] == want
    seen = {w for w in want if w[0] < 0} | {("moved", 0) for w in want if w[0] >= 0}
    assert seen == {(-1, 0), (-2, 0), (-2, guide_ref.REJECTED), (-2, guide_ref.BAD_STATE), ("moved", 0)}   # the cases reach every branch


def test_planted_advance_cases_say_what_the_contract_says():
    indptr, tok, nxt = guide_cases.advance_table()
    S, E = indptr.size - 1, tok.size
    one = lambda s, t: guide_ref.advance_one(s, t, indptr, tok, nxt, S, E)
    assert one(8, 3) == ((7 * 8) % S, 0) and one(8, 3 + 2 * 1024) == ((7 * 8 + 1024) % S, 0)
    assert one(8, 4) == (-2, 1) and one(8, 2 ** 32 + 5) == (-2, 1) and one(0, 3) == (-2, 1)
    assert one(guide_cases.BAD_NEXT_STATE, 10) == (-2, 2) and one(guide_cases.BAD_NEXT_STATE, 20) == (4, 0)
    assert one(guide_cases.DECREASING_STATE, 20) == (-2, 1)                 # its range is empty after the clamp
    assert one(guide_cases.BEYOND_STATE, 20) == (4, 0) and one(guide_cases.BEYOND_STATE, 10) == (-2, 1)
    assert one(-1, 3) == (-1, 0) and one(-2, 3) == (-2, 0) and one(-3, 3) == (-2, 2) and one(S, 3) == (-2, 2)


@pytest.mark.parametrize("vocab", [1, 31, 32, 33, 64, 2049])
def test_host_mask_equals_the_reference_at_the_word_boundaries(host_math, vocab):
    mask, S = guide_cases.mask_table(vocab)
    positions = sorted({v for v in (0, 31, 32, vocab - 1) if v < vocab})
    for s in list(range(S)) + [guide_ref.FREE, guide_ref.DEAD, -3, S]:
        for bits in (0x3C00, 0x8000, 0x7E01, 0xFC00):
            row = np.full(vocab, bits, dtype=np.uint16)
            want, _ = guide_ref.mask_row(row, s, mask, S)
            for v in positions:
                got = host_math.mask_one(bits, s, S, mask.ctypes.data, mask.shape[1], v)
                assert got == int(want[v]), (s, hex(bits), v)
        assert host_math.row_kind(s, S) == (0 if 0 <= s < S else (1 if s in (-1, -2) else 2))
    allow = np.stack([guide_ref.allowed_row(mask[s], vocab) for s in range(S)])
    assert not allow[0].any() and allow[1].all() and allow[2].sum() == 1 and allow[2, 0] and allow[3].sum() == 1 and allow[3, vocab - 1]
    assert (mask[:, -3:] == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ 4. TokenAutomaton
def test_token_automaton_validates_its_edges():
    from atom_amd.e2e import TokenAutomaton
    ok = TokenAutomaton(2, [(0, 5, 1), (1, 2, 0), (0, 3, 0)], vocab_size=8)
    assert ok.indptr.tolist() == [0, 2, 3] and ok.edge_tok.tolist() == [3, 5, 2] and ok.edge_next.tolist() == [0, 1, 0]
    assert ok.step(0, 5) == 1 and ok.step(0, 4) is None and ok.step(1, 2) == 0 and ok.allowed(0) == [3, 5]
    assert ok.accepts([5, 2, 3, 3]) and not ok.accepts([5, 5]) and ok.accepts([])
    for kw in (dict(num_states=2, edges=[(0, 5, 1)]),                              # state 1 has no edge
               dict(num_states=1, edges=[]),
               dict(num_states=2, edges=[(0, 5, 1), (1, 2, 0), (0, 5, 0)]),        # duplicate (state, token)
               dict(num_states=2, edges=[(0, 5, 2), (1, 2, 0)]),                   # next out of range
               dict(num_states=2, edges=[(0, 5, -1), (1, 2, 0)]),
               dict(num_states=2, edges=[(0, 5, 1), (1, 2, 0)], start=2),
               dict(num_states=2, edges=[(0, 5, 1), (1, 2, 0)], start=-1),
               dict(num_states=2, edges=[(0, -1, 1), (1, 2, 0)]),
               dict(num_states=2, edges=[(0, 8, 1), (1, 2, 0)], vocab_size=8),
               dict(num_states=2, edges=[(0, 5, 1), (2, 2, 0), (1, 1, 1)])):
        with pytest.raises(ValueError):
            TokenAutomaton(**kw)


def test_from_sequences_accepts_exactly_the_sequences_followed_by_eos():
    from atom_amd.e2e import TokenAutomaton
    seqs, eos = [[1], [2, 3], [2, 4, 5], [6, 7, 8, 9], [2, 3, 1]], 0
    a = TokenAutomaton.from_sequences(seqs, eos, 10)
    got = {seq for n in range(6) for seq in itertools.product(range(10), repeat=n) if a.accepts(seq)}
    strip = lambda seq: seq[:min(i for i in range(len(seq) + 1) if all(t == eos for t in seq[i:]))]
    assert all(seq and seq[-1] == eos for seq in got)                            # nothing is accepted before its EOS ...
    assert {strip(seq) for seq in got} == {tuple(s) for s in seqs}                # ... and what is, is a given sequence, then EOS only
    assert all(a.accepts(s + [eos]) and a.accepts(s + [eos, eos]) and not a.accepts(s) and not a.accepts(s + [eos, 1]) for s in seqs)
    end = a.num_states - 1
    assert a.allowed(end) == [eos] and a.step(end, eos) == end and a.final == frozenset([end])
    assert a.allowed(0) == [1, 2, 6] and not a.accepts([2, 3]) and not a.accepts([2])
    with pytest.raises(ValueError):
        TokenAutomaton.from_sequences([[1, 0]], 0, 10)
    with pytest.raises(ValueError):
        TokenAutomaton.from_sequences([[1, 10]], 0, 10)
    assert TokenAutomaton.from_sequences([[]], 0, 10).accepts([0])


REGEX_VOCAB = ["0", "1", "7", "12", "-", ".", "a", "ab", "true", "false", "t", "e", None]
REGEX_EOS = 12
REGEX_PATTERNS = [r"-?(0|[1-9][0-9]*)", r"(true|false)", r"a{2,3}b?", r"[^0-9]+", r"(ab|a)*1", r".\.[01]{2}",
                  r"\d+\.\w*", r"(a|ab)(t|e){0,2}", r"[a\-.]*", r"(-|\.){2,}a?", r"\w\s*|1+"]


@pytest.fixture(scope="module")
def all_sequences():
    seqs = [seq for n in range(5) for seq in itertools.product(range(12), repeat=n)]
    assert len(seqs) == 22621
    return seqs, ["".join(REGEX_VOCAB[i] for i in seq) for seq in seqs]


@pytest.mark.parametrize("pattern", REGEX_PATTERNS)
def test_from_regex_accepts_what_re_fullmatch_accepts(all_sequences, pattern):
    from atom_amd.e2e import TokenAutomaton
    seqs, texts = all_sequences
    a = TokenAutomaton.from_regex(pattern, REGEX_VOCAB, REGEX_EOS)
    rx = re.compile(pattern)
    wrong = [seq for seq, text in zip(seqs, texts) if a.accepts(seq + (REGEX_EOS,)) != (rx.fullmatch(text) is not None)]
    matched = sum(rx.fullmatch(text) is not None for text in texts)
    print(f"{pattern}: {a.num_states} states, {a.num_edges} edges, {matched} of {len(seqs)} sequences match")
    assert not wrong, wrong[:5]
    assert matched > 0
    end = a.num_states - 1
    assert a.allowed(end) == [REGEX_EOS] and a.step(end, REGEX_EOS) == end and a.start == 0
    assert all(len(a.allowed(s)) > 0 for s in range(a.num_states))


@pytest.mark.parametrize("pattern", [r"^a", r"a$", r"a*?", r"a+?", r"a??", r"a{2}?", r"a++", r"(?:a)", r"(?=a)b", r"(?!a)", r"(?<=a)b", r"(?P<x>a)",
                                     r"(a)\1", r"\b", r"\B", r"\A", r"\Z", r"\D", r"\W", r"\S", r"(?i)a", r"a**", r"a{2}{3}", r"(a", r"a)", r"[a",
                                     r"a{2,1}", r"*a", r"a{,3}", r"a{x}", r"[z-a]", r"[[:alpha:]]", "a\\", r"a{2000}"])
def test_from_regex_refuses_what_it_does_not_support(pattern):
    from atom_amd.e2e import TokenAutomaton
    with pytest.raises(ValueError, match="from_regex"):
        TokenAutomaton.from_regex(pattern, REGEX_VOCAB, REGEX_EOS)


def test_from_regex_enforces_max_states_and_empty_languages():
    from atom_amd.e2e import TokenAutomaton
    pattern = r"(a|t)*a(a|t){6}"                               # the textbook blow-up: 2^7 DFA states
    with pytest.raises(ValueError, match="max_states"):
        TokenAutomaton.from_regex(pattern, REGEX_VOCAB, REGEX_EOS, max_states=100)
    assert TokenAutomaton.from_regex(pattern, REGEX_VOCAB, REGEX_EOS, max_states=200).accepts([10, 6, 10, 6, 6, 10, 10, 6, REGEX_EOS])   # "tataatta"
    with pytest.raises(ValueError):
        TokenAutomaton.from_regex(r"xyz", REGEX_VOCAB, REGEX_EOS)          # no token spells it
    with pytest.raises(ValueError):
        TokenAutomaton.from_regex(r"a", REGEX_VOCAB, 99)


# ------------------------------------------------------------------------------------------------ 5. LogitGuide on "cpu"
def test_logit_guide_stacks_its_automata():
    import torch
    from atom_amd.e2e import LogitGuide, TokenAutomaton
    a = TokenAutomaton.from_sequences([[1], [2, 3]], 0, 40)
    b = TokenAutomaton.from_regex(r"(true|false)", REGEX_VOCAB, REGEX_EOS)
    c = TokenAutomaton(2, [(0, 39, 1), (1, 32, 1), (1, 31, 0)], start=1, vocab_size=40)
    g = LogitGuide(6, 40, "cpu", [b, None, a, b, c, a])
    assert g.automata == [b, a, c] and g.offsets.tolist() == [0, b.num_states, b.num_states + a.num_states, b.num_states + a.num_states + 2]
    assert g.num_states == g.offsets[-1] and g.num_edges == a.num_edges + b.num_edges + 3
    assert g.start.dtype == torch.int32 and g.start.tolist() == [0, -1, b.num_states, 0, g.offsets[2] + 1, b.num_states]
    assert g.state.tolist() == g.start.tolist() and g.status.tolist() == [0] and g.status.dtype == torch.int32
    indptr, tok, nxt = g.indptr.numpy(), g.edge_tok.numpy(), g.edge_next.numpy()
    assert indptr.dtype == tok.dtype == nxt.dtype == np.int32 and indptr.size == g.num_states + 1 and indptr[-1] == g.num_edges
    for k, auto in enumerate(g.automata):                       # every automaton's walk, through the stacked tables
        for s in range(auto.num_states):
            lo, hi = indptr[g.offsets[k] + s], indptr[g.offsets[k] + s + 1]
            assert tok[lo:hi].tolist() == auto.allowed(s)
            assert (nxt[lo:hi] - g.offsets[k]).tolist() == [auto.step(s, t) for t in auto.allowed(s)]
    assert g.mask_ld == 4 and g.mask_bits.shape == (g.num_states, 4) and g.mask_bits.dtype == torch.int32
    assert np.array_equal(g.mask_bits.numpy().view(np.uint32), guide_ref.mask_from_csr(indptr, tok, 4))
    words = g.mask_bits.numpy().view(np.uint32)[g.offsets[2]:]
    assert words.tolist() == [[0, 1 << 7, 0, 0], [1 << 31, 1, 0, 0]]          # tokens 39; 31 and 32: both sides of a word boundary
    addresses = [t.data_ptr() for t in (g.state, g.status, g.indptr, g.mask_bits)]
    g.state[0], g.status[0] = 3, 1
    g.reset()
    assert g.state.tolist() == g.start.tolist() and g.status.tolist() == [0]
    assert addresses == [t.data_ptr() for t in (g.state, g.status, g.indptr, g.mask_bits)]
    one = LogitGuide(3, 64, "cpu", a)
    assert one.automata == [a] and one.start.tolist() == [0, 0, 0] and one.mask_ld == 4
    assert LogitGuide(1, 4097, "cpu", a).mask_ld == 132
    for bad in ([a, b], [None] * 6, [a] * 5 + ["x"]):
        with pytest.raises(ValueError):
            LogitGuide(6, 40, "cpu", bad)
    with pytest.raises(ValueError):
        LogitGuide(1, 39, "cpu", a)                             # an automaton over more tokens than the logits have
