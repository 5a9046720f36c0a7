"""What makes tests/test_gpu_layer_ref.py mean something, without a GPU: on the SAME inputs (tests/layer_cases.py) the staged
reference's own trace passes its checker, and every deliberate wiring error of tests/layer_ref.py: WRONG is reported, first at the
stage it touches.  A wiring error that a route's inputs cannot show (rope_theta at its default, no cached prefix, no decode request,
h // G == h % kv_heads, no mixed batch) is run where they can; every error is shown on at least one route."""
import functools

import numpy as np
import pytest

from oracle import atom_oracle as O
from tests import layer_cases as C
from tests import layer_ref as R


def _shows(name, route, kv_heads):
    """can this route's inputs tell the wiring error from the right wiring?"""
    return {"theta_default": route == "E", "chunk_positions_from_zero": route in "BE", "decode_position_plus_one": route in "CDE",
            "gqa_head_modulo": kv_heads == 2, "mixed_rows_from_front": route in "DE"}.get(name, True)


LAYER_WRONG = [n for n in R.WRONG if n not in R.MODEL_WRONG]


@functools.lru_cache(maxsize=None)
def _prepared(route, kv_heads):
    """the case with the pool as the first call (the cached prefixes) left it"""
    case = C.layer_case(route, kv_heads)
    pool = case["pool"]
    if case["first"] is not None:
        tr = R.forward(case["first"], case["lay"], pool, case["x_first"])
        assert R.check(tr, dict(req=case["first"], lay=case["lay"], pool=pool, x=case["x_first"])) == []
        pool = (tr["cache"]["buf"], tr["cache"]["param"])
    return dict(req=case["req"], lay=case["lay"], pool=pool, x=case["x"])


def test_every_wiring_error_has_a_route_that_shows_it():
    for name in LAYER_WRONG:
        assert any(_shows(name, r, kv) for r, kv in C.LAYER_CASES), name
    assert set(R.WRONG.values()) <= set(R.LAYER_STAGES) | {"final_norm", "logits"}


@pytest.mark.parametrize("route,kv_heads", C.LAYER_CASES)
def test_own_trace_passes(route, kv_heads):
    inp = _prepared(route, kv_heads)
    before = inp["pool"][0].copy(), inp["pool"][1].copy()
    tr = R.forward(inp["req"], inp["lay"], inp["pool"], inp["x"])
    assert R.check(tr, inp) == []
    assert np.array_equal(before[0], inp["pool"][0]) and np.array_equal(before[1].view(np.uint16), inp["pool"][1].view(np.uint16))
    # the call wrote this layer's slice of the request's pages and nothing else
    changed = np.argwhere((tr["cache"]["buf"] != before[0]).any(axis=(2, 3, 4, 5)))
    pages = {p for _, _, pg in inp["req"].prefills for p in pg} | {p for _, pg in inp["req"].decodes for p in pg}
    assert len(changed) and set(changed[:, 1]) == {1} and set(changed[:, 0]) <= pages
    for stage in R.LAYER_STAGES:                                # a stage cannot pass by being absent
        short = {k: v for k, v in tr.items() if k != stage}
        assert [s for s, _ in R.check(short, inp)] == [stage]


@pytest.mark.parametrize("route,kv_heads,name", [(r, kv, n) for r, kv in C.LAYER_CASES for n in LAYER_WRONG if _shows(n, r, kv)])
def test_wiring_error_is_reported_at_its_stage(route, kv_heads, name):
    inp = _prepared(route, kv_heads)
    fails = R.check(R.forward(inp["req"], inp["lay"], inp["pool"], inp["x"], wrong=name), inp)
    assert fails and fails[0][0] == R.WRONG[name], (name, fails)


@pytest.mark.parametrize("route,kv_heads", C.MODEL_CASES)
def test_model_trace_and_its_wiring_errors(route, kv_heads):
    case = C.model_case(route, kv_heads)
    inp = dict(req=case["req"], mdl=case["mdl"], pool=case["pool"], ids=case["ids"])
    assert R.check_model(R.model_forward(case["req"], case["mdl"], case["pool"], case["ids"]), inp) == []
    for name, first in (("no_final_norm", "final_norm"), ("head_before_norm", "logits"), ("cache_layer_zero", "layer1.cache")):
        fails = R.check_model(R.model_forward(case["req"], case["mdl"], case["pool"], case["ids"], wrong=name), inp)
        assert fails and fails[0][0] == first, (name, fails)
    tr = R.model_forward(case["req"], case["mdl"], case["pool"], case["ids"])
    tr["embed"] = np.roll(tr["embed"], 1, axis=0)
    assert R.check_model(tr, inp)[0][0] == "embed"


@pytest.mark.parametrize("theta", [1e4, 5e5])
def test_restated_attention_is_the_oracles_decode(theta):
    """one query per sequence, MHA: tests/layer_ref.py's attention against oracle.batch_decode_i4 (pinned to the reference's CPU code)"""
    req, _ = C.requests("C", 4, 5)
    buf, param = C.random_pool(4, 6)
    q = (np.random.default_rng(7).standard_normal((req.rows, C.HIDDEN))).astype(np.float16)
    for layer in (0, 1):
        got = R.attention(req, q, (buf, param), layer, theta)
        want = O.batch_decode_i4(q.reshape(req.rows, 4, 128), buf, param, *req.decode_tables(), layer, theta)
        assert np.abs(got - want.reshape(req.rows, -1)).max() <= 1e-12 * np.abs(want).max()


def test_o4_bound_tells_a_code_one_step_off():
    """the k / v bound is on values: a scale two ulps off, or one code a whole step off where it is not at a rounding boundary, fails"""
    inp = _prepared("A", 2)
    tr = R.forward(inp["req"], inp["lay"], inp["pool"], inp["x"])
    D, A = R.gemm(tr["norm1"], inp["lay"]["w"]["k"]), R.gemm_abs(tr["norm1"], inp["lay"]["w"]["k"])
    assert R._check_o4(tr["k"], D, A, 4)[0]
    sz = tr["k"]["sz"].copy()
    sz[3, 1, 0] = (sz[3, 1, 0].view(np.uint16) + 2).view(np.float16)
    assert not R._check_o4(dict(codes=tr["k"]["codes"], sz=sz), D, A, 4)[0]
    # the element of row 0, head 0 that sits closest to the middle of its step: one code up or down is a whole step away
    s, z = float(tr["k"]["sz"][0, 0, 0]), float(tr["k"]["sz"][0, 0, 1])
    u = (D[0, :128] + z) / s
    j = int(np.argmin(np.abs(u - np.rint(u)) + 10 * ((np.rint(u) < 1) | (np.rint(u) > 14))))
    for step in (1, -1):
        codes = tr["k"]["codes"].copy()
        nib = int(np.rint(u[j])) + step
        codes[0, j // 2] = (codes[0, j // 2] & (0xF0 if j % 2 == 0 else 0x0F)) | (nib << (0 if j % 2 == 0 else 4))
        assert not R._check_o4(dict(codes=codes, sz=tr["k"]["sz"]), D, A, 4)[0]
