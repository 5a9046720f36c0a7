"""CPU-only checks of the guided speculative step's device op: atom_guide_walk_rows' argument validation (it precedes
the launch, so no GPU is needed), a host build of csrc/guide_math.h's ``walk`` against tests/guide_walk_ref.py on the planted and random
cases of tests/guide_walk_cases.py, the walk's properties stated over tests/guide_ref.py alone, and the Python surface."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from tests import guide_ref, guide_walk_cases as C, guide_walk_ref as W

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _walk(lib, state=P, adds=2 * P, row_state=3 * P, input_ids=4 * P, ids_ld=5, batch=4, rows=5, indptr=5 * P, edge_tok=6 * P,
          edge_next=7 * P, num_states=10, num_edges=50, force=1, status=8 * P):
    return lib.atom_guide_walk_rows(state, adds, row_state, input_ids, ids_ld, batch, rows, indptr, edge_tok, edge_next, num_states,
                                    num_edges, force, status, None)


# ------------------------------------------------------------------------------------------------ 1. symbol and API
def test_the_symbol_resolves():
    L, lib = _lib()
    assert "atom_guide_walk_rows" in L.SIGNATURES and hasattr(lib, "atom_guide_walk_rows")
    res, args = L.SIGNATURES["atom_guide_walk_rows"]
    assert res is ctypes.c_int and len(args) == 15
    with open(os.path.join(ROOT, "include", "atom_hip.h")) as f:
        assert "int atom_guide_walk_rows(" in f.read()
    from atom_amd import ops
    from atom_amd.e2e import LogitGuide
    assert callable(ops.guide_walk_rows) and ops.GUIDE_MAX_ROWS == W.MAX_ROWS == 9
    assert all(callable(getattr(LogitGuide, name)) for name in ("rows", "walk_rows", "mask_rows"))


def test_op_refuses_cpu_tensors():
    import torch
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    i32 = lambda *a: torch.zeros(a, dtype=torch.int32)
    with pytest.raises(AtomHipError):
        ops.guide_walk_rows(i32(2), i32(2), i32(2, 3), torch.zeros((2, 3), dtype=torch.int64), i32(4), i32(5), i32(5))


def test_logit_guide_rows_are_allocated_once():
    import torch
    from atom_amd.e2e import LogitGuide, TokenAutomaton
    g = LogitGuide(3, 40, "cpu", TokenAutomaton.from_sequences([[1], [2, 3]], 0, 40))
    assert g.row_state is None
    with pytest.raises(RuntimeError):
        g.walk_rows(torch.zeros(3, dtype=torch.int32), None)
    rows = g.rows(5)
    assert rows.shape == (3, 5) and rows.dtype == torch.int32 and g.rows(5).data_ptr() == rows.data_ptr() and g.row_state is rows
    for bad in (4, 0, 10):
        with pytest.raises(ValueError):
            g.rows(bad)


# ------------------------------------------------------------------------------------------------ 2. argument validation
def test_walk_rows_rejects_null_pointers():
    L, lib = _lib()
    for name in ("state", "adds", "row_state", "indptr", "edge_tok", "edge_next", "status"):
        assert _walk(lib, **{name: None}) == L.ERR_INVALID_ARG, name
    # a null pointer is checked before a shape, a shape before an alignment (the order of every entry point)
    assert _walk(lib, state=None, batch=0) == L.ERR_INVALID_ARG and _walk(lib, batch=0, state=P + 2) == L.ERR_SHAPE
    # the commit-only form passes validation as far as it goes: the next check it meets is the shape's, then the alignment's
    assert _walk(lib, input_ids=None, rows=0) == L.ERR_SHAPE and _walk(lib, input_ids=None, status=8 * P + 2) == L.ERR_ALIGN
    assert _walk(lib, edge_tok=None, edge_next=None, num_edges=0, batch=0) == L.ERR_SHAPE     # no edges: the edge arrays may be null


def test_walk_rows_rejects_bad_shapes():
    L, lib = _lib()
    for kw in (dict(batch=0), dict(batch=-1), dict(batch=65536), dict(rows=0), dict(rows=-1), dict(rows=10, ids_ld=10), dict(ids_ld=4),
               dict(ids_ld=0), dict(rows=9, ids_ld=8), dict(num_states=0), dict(num_states=-5), dict(num_states=1 << 31),
               dict(num_edges=-1), dict(num_edges=1 << 31)):
        assert _walk(lib, **kw) == L.ERR_SHAPE, kw
    assert _walk(lib, rows=10, ids_ld=10, input_ids=4 * P + 4) == L.ERR_SHAPE      # ... before the alignment


def test_walk_rows_rejects_misaligned_pointers():
    L, lib = _lib()
    for name, base, by in (("state", P, 2), ("state", P, 1), ("adds", 2 * P, 2), ("row_state", 3 * P, 2), ("input_ids", 4 * P, 4),
                           ("input_ids", 4 * P, 2), ("indptr", 5 * P, 2), ("edge_tok", 6 * P, 1), ("edge_next", 7 * P, 2),
                           ("status", 8 * P, 2)):
        assert _walk(lib, **{name: base + by}) == L.ERR_ALIGN, name


# ------------------------------------------------------------------------------------------------ 3. the rules, built for the host
WRAPPER = r"""
#include "guide_math.h"
namespace gm = atom::guide;
// as the kernel calls it: one sequence after the other, the last row states and the new ones in the same array
extern "C" void walk_all(int32_t *state, const int32_t *adds, int32_t *row_state, int64_t *ids, int64_t n, int Q, const int32_t *indptr,
                         const int32_t *edge_tok, const int32_t *edge_next, int64_t num_states, int64_t num_edges, int force,
                         int32_t *status) {
  for (int64_t i = 0; i < n; ++i) {
    int32_t bits = 0;
    int32_t *row = row_state + i * Q;
    state[i] = gm::walk(state[i], adds[i], row, ids ? ids + i * Q : nullptr, row, Q, indptr, edge_tok, edge_next, num_states, num_edges,
                        force != 0, bits);
    status[i] = bits;
  }
}
"""


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("guide_walk")
    with open(os.path.join(ROOT, "atom_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    flags = [x for x in re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split() if not x.startswith("--offload-arch")]
    src, so = tmp / "guide_walk_host.cpp", tmp / "guide_walk_host.so"
    src.write_text(WRAPPER)
    cmd = [hipcc, "-x", "c++"] + flags + ["-shared", "-I", os.path.join(ROOT, "atom_amd", "csrc"), str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    lib.walk_all.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 2 + [
        ctypes.c_int, ctypes.c_void_p]
    lib.walk_all.restype = None
    return lib


def _host(lib, table, states, adds, prev, ids, force, commit_only=False):
    """the host build over copies: (states, row states, ids, status per sequence)"""
    indptr, tok, nxt = table
    s, rows, i = states.copy(), np.ascontiguousarray(prev).copy(), np.ascontiguousarray(ids).copy()
    status = np.zeros(len(s), dtype=np.int32)
    lib.walk_all(s.ctypes.data, adds.ctypes.data, rows.ctypes.data, None if commit_only else i.ctypes.data, len(s), prev.shape[1],
                 indptr.ctypes.data, tok.ctypes.data, nxt.ctypes.data, indptr.size - 1, tok.size, int(force), status.ctypes.data)
    return s.tolist(), rows.tolist(), i.tolist(), status.tolist()


def _want(table, states, adds, prev, ids, force, commit_only=False):
    indptr, tok, nxt = table
    S, E = indptr.size - 1, tok.size
    out = [W.walk(states[b], adds[b], prev[b].tolist(), ids[b].tolist(), indptr, tok, nxt, S, E, force, commit_only) for b in range(len(states))]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], [o[3] for o in out]


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("Q", C.QS)
def test_host_walk_equals_the_restatement(host_walk, Q, force):
    seen_bits, forced_writes, dead_rows = set(), 0, 0
    for name, table in C.tables():
        states, adds, prev, ids = C.cases(table, Q)
        got, want = _host(host_walk, table, states, adds, prev, ids, force), _want(table, states, adds, prev, ids, force)
        assert got == want, name
        seen_bits |= set(want[3])
        forced_writes += int((np.array(want[2], dtype=np.int64) != ids).sum())
        dead_rows += sum(guide_ref.DEAD in row for row in want[1])
        assert _host(host_walk, table, states, adds, prev, ids, force, True) == _want(table, states, adds, prev, ids, force, True), name
    assert {0, 1, 2} <= seen_bits and dead_rows > 0                    # the cases reach every status bit, and no bit
    assert (forced_writes > 0) == (force and Q > 1)                  # ... and drafts are overwritten exactly when forcing can


def test_planted_cases_say_what_the_contract_says():
    indptr, tok, nxt = table = C.planted_table()
    S, E = indptr.size - 1, tok.size
    one = lambda state, add, prev, ids, force=True: W.walk(state, add, prev, ids, indptr, tok, nxt, S, E, force)
    D, F = guide_ref.DEAD, guide_ref.FREE
    # the commit: add 0 keeps the state, 1 .. Q take a row state, anything else keeps it and sets BAD_STATE
    assert one(0, 0, [5, 6], [3, 11])[0::3] == (0, 0) and one(0, 2, [5, 6], [16, 17])[0::3] == (6, 0)
    assert one(0, 3, [5, 6], [3, 11])[0::3] == (0, 2) and one(0, -1, [5, 6], [3, 11])[0::3] == (0, 2)
    # REJECTED: only when the committed state BECOMES dead
    assert one(0, 1, [D, 6], [3, 11])[0::3] == (D, 1) and one(D, 1, [D, 6], [3, 11])[0::3] == (D, 0) and one(D, 0, [5, 6], [3, 11])[0::3] == (D, 0)
    assert one(F, 1, [F, 6], [3, 11]) == (F, [F, F], [3, 11], 0)
    # the walk: 0 -3-> 1 -11-> 2 -12-> 3; the chain forces its drafts
    assert one(0, 0, [0] * 4, [3, 11, 12, 13]) == (0, [1, 2, 3, 4], [3, 11, 12, 13], 0)
    assert one(0, 0, [0] * 4, [3, 77, 78, 79]) == (0, [1, 2, 3, 4], [3, 11, 12, 13], 0)
    assert one(0, 0, [0] * 4, [3, 77, 12, 13], False) == (0, [1, D, D, D], [3, 77, 12, 13], 0)      # a wrong draft: DEAD, and no bit
    assert one(0, 0, [0] * 3, [C.NO_EDGE, 11, 12]) == (0, [D, D, D], [C.NO_EDGE, 11, 12], 0)          # ids[0] is never forced
    assert one(1, 0, [0] * 2, [3, 12]) == (1, [D, D], [3, 12], 0)                                     # ... even in a forced state
    assert one(0, 0, [0] * 2, [3 + 2 ** 32, 11]) == (0, [D, D], [3 + 2 ** 32, 11], 0)                 # compared as int64
    # the rule's other half: the NEXT commit sets REJECTED for the token without an edge
    s, rows, _, bits = one(0, 0, [0] * 3, [C.NO_EDGE, 11, 12])
    assert one(s, 1, rows, [5, 5, 5])[0::3] == (D, 1)
    # a forced edge whose target is outside the table, out-of-range states, the clamped ranges
    assert one(13, 0, [0] * 3, [6, 1, 1]) == (13, [C.BAD_SINGLE, D, D], [6, 8, 1], 2)
    assert one(S, 0, [0] * 2, [3, 3]) == (S, [D, D], [3, 3], 2) and one(-3, 0, [0], [3]) == (-3, [D], [3], 2)
    assert one(C.BAD_NEXT, 0, [0] * 2, [20, 14]) == (C.BAD_NEXT, [4, 5], [20, 14], 0)
    assert one(C.BAD_NEXT, 0, [0] * 2, [10, 14]) == (C.BAD_NEXT, [D, D], [10, 14], 2)
    assert one(C.DECREASING, 0, [0] * 2, [20, 14]) == (C.DECREASING, [D, D], [20, 14], 0)              # an empty range forces nothing
    assert one(C.BEYOND, 0, [0] * 2, [20, 1]) == (C.BEYOND, [4, 5], [20, 14], 0)
    assert W.forced_token(C.BEYOND, indptr, tok, S, E) is None and W.forced_token(1, indptr, tok, S, E) == 11


@pytest.mark.parametrize("Q", C.QS)
def test_rows_are_repeated_advances_and_forced_drafts_are_the_single_allowed_token(host_walk, Q):
    """the properties, over guide_ref alone and the sane random tables"""
    checked = 0
    for name, table in C.tables()[1:]:
        indptr, tok, nxt = table
        S = indptr.size - 1
        states, adds, prev, ids = C.cases(table, Q)
        for force in (False, True):
            s_out, rows, ids_out, _ = _host(host_walk, table, states, adds, prev, ids, force)
            for b in range(len(states)):
                if not 0 <= s_out[b] < S:
                    continue
                assert rows[b] == guide_ref.walk(s_out[b], ids_out[b], indptr, tok, nxt), (name, b)
                assert ids_out[b][0] == ids[b, 0]
                for j in range(1, Q):
                    before = rows[b][j - 1]
                    single = 0 <= before < S and indptr[before + 1] - indptr[before] == 1
                    if force and single:
                        assert ids_out[b][j] == tok[indptr[before]] and rows[b][j] == nxt[indptr[before]]
                    else:
                        assert ids_out[b][j] == ids[b, j]
                    checked += 1
    assert checked > 0 or Q == 1


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_speculative_params_keep_their_defaults():
    from atom_amd.e2e import SpeculativeParams
    p = SpeculativeParams()
    assert dataclasses.astuple(p) == (4, 3, 1, 8, False, True)
    assert [f.name for f in dataclasses.fields(p)] == ["num_draft_tokens", "ngram_max", "ngram_min", "poll_every", "guided", "force_drafts"]
    assert SpeculativeParams(2, 3, 1, 4) == SpeculativeParams(num_draft_tokens=2, poll_every=4)
    assert SpeculativeParams(guided=True).guided and not SpeculativeParams(force_drafts=False).force_drafts


def test_generate_refusal_names_the_opt_in():
    """the checks precede everything that touches the model or the pool"""
    from atom_amd.e2e import SpeculativeParams, TokenAutomaton, generate
    auto = TokenAutomaton.from_sequences([[1], [2, 3]], 0, 40)
    with pytest.raises(ValueError, match=r"guide does not combine with speculative.*SpeculativeParams\(guided=True\)"):
        generate(None, [[1]], 4, None, guide=auto, speculative=SpeculativeParams())
    with pytest.raises(ValueError, match="guide does not combine with num_beams"):
        generate(None, [[1]], 4, None, guide=auto, speculative=SpeculativeParams(guided=True), num_beams=2)
    with pytest.raises(ValueError, match="speculative does not combine with logprobs"):
        generate(None, [[1]], 4, None, guide=auto, speculative=SpeculativeParams(guided=True), logprobs=0)
