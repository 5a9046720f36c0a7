"""CPU-only: the host side of the W4A4 GEMM entry points against the tables recorded before the route decision was folded into one
function (tests/gemm_host_tables.py): every route, workspace and fits query over the grid, the queries on rejected inputs, and the error
code of every rejected call -- which of two faults is reported is part of the C ABI's behaviour."""
import json
import os

import pytest

from tests import gemm_host_tables as T


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "gemm_host_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def L():
    from atom_amd._lib import lib
    return lib()


def test_plan_queries_equal_the_recorded_tables(L, recorded):
    got = T.plan_tables(L)
    n, ns = len(T.shapes()), len(T.seg_shapes())
    assert n == 5100 and ns == 1575
    for name, values in got.items():
        want = T.decode(name, recorded["plan." + name])
        per = {"multi_fits": ns, "multi_q_fits": ns * len(T.Q_OPS), "multi_merge_q_fits": ns * len(T.MERGE_SPLITS)}.get(name, n)
        assert len(values) == len(want) == per, name
        bad = [i for i, (a, b) in enumerate(zip(values, want)) if a != b]
        shape = lambda i: T.shapes()[i] if per == n else T.seg_shapes()[i // (per // ns)] + (i % (per // ns),)
        assert not bad, (name, len(bad), [(shape(i), values[i], want[i]) for i in bad[:5]])
    orders = set(got["packed_order_0"]) | set(got["packed_order_1"]) | set(got["packed_order_2"])
    assert orders == set(T.ORDERS) and set(got["f6_order"]) == {1, 2}
    assert all(set(got[k]) == {0, 1} for k in ("ws_recodes", "ws_recodes_cached", "multi_fits", "multi_q_fits", "multi_merge_q_fits"))


def test_rejected_query_inputs_equal_the_recorded_values(L, recorded):
    assert [[f, list(a)] for f, a in T.rejected()] == [[f, a] for f, a, _ in recorded["rejected"]]
    wrong = [(f, a, want, getattr(L, f)(*a)) for f, a, want in recorded["rejected"]]
    wrong = [w for w in wrong if w[2] != w[3]]
    assert not wrong, wrong[:10]
    assert any(want != 0 for _, _, want in recorded["rejected"]) and any(want == 0 for _, _, want in recorded["rejected"])


def test_error_codes_equal_the_recorded_matrix(L, recorded):
    """every call of the matrix is refused before a launch (host memory: nothing may start on a device), with the recorded code"""
    from atom_amd import _lib
    calls = T.matrix()
    assert len(calls) == len(recorded["errors"]) and {f for f, _ in calls} == set(T.VALID) and len(T.VALID) == 9
    assert set(recorded["errors"]) == {_lib.ERR_INVALID_ARG, _lib.ERR_SHAPE, _lib.ERR_ALIGN}
    wrong = [(f, c, st, T.call(L, f, c)) for (f, c), st in zip(calls, recorded["errors"])]
    wrong = [w for w in wrong if w[2] != w[3]]
    assert not wrong, wrong[:10]
