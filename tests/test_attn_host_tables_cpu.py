"""CPU-only: the host side of the INT4 paged-KV attention ops against the tables recorded before its copies were folded into one plan
and one launcher per kernel family (tests/attn_host_tables.py): every plan query over the grid, and the error code of every rejected
call -- which of two faults is reported is part of the C ABI's behaviour."""
import json
import os

import pytest

from tests import attn_host_tables as T


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "attn_host_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def L():
    from atom_amd._lib import lib
    return lib()


def test_plan_queries_equal_the_recorded_tables(L, recorded):
    got = T.plan_tables(L)
    n = len(T.BATCH) * len(T.KV_HEADS) * len(T.PAGE) * len(T.MAX_PAGES)
    assert [len(got[k]) for k in ("decode", "prefill", "decode_gqa", "prefill_gqa")] == [2 * n, 6 * n, 8 * n, 24 * n]
    for name, values in got.items():
        want = recorded["plan." + name]
        assert len(values) == len(want), name
        bad = [i for i, (a, b) in enumerate(zip(values, want)) if a != b]
        assert not bad, (name, len(bad), bad[:5], [values[i] for i in bad[:5]], [want[i] for i in bad[:5]])
    assert any(v > 1 for v in got["decode"][1::2]) and any(v > 1 for v in got["decode_gqa"][1::2]) and any(got["prefill"]) and any(got["prefill_gqa"])


def test_rejected_query_inputs_equal_the_recorded_values(L, recorded):
    assert [(f, list(a)) for f, a in T.REJECTED] == [(f, a) for f, a, _ in recorded["rejected"]]
    for f, a, want in recorded["rejected"]:
        assert getattr(L, f)(*a) == want == 0, (f, a)


def test_error_codes_equal_the_recorded_matrix(L, recorded):
    """every call of the matrix is refused before a launch (host memory: nothing may start on a device), with the recorded code"""
    from atom_amd import _lib
    assert [[f, c] for f, c in T.matrix()] == [[f, c] for f, c, _ in recorded["errors"]]
    assert {f for f, _, _ in recorded["errors"]} == set(T.VALID)
    assert {st for _, _, st in recorded["errors"]} == {_lib.ERR_INVALID_ARG, _lib.ERR_SHAPE, _lib.ERR_ALIGN}
    wrong = [(f, c, st, T.call(L, f, c)) for f, c, st in recorded["errors"]]
    wrong = [w for w in wrong if w[2] != w[3]]
    assert not wrong, wrong[:10]
