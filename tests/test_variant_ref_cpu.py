"""What makes tests/test_gpu_variant_ref.py mean something, without a GPU (the pattern of tests/test_layer_ref_cpu.py): on the SAME
inputs (tests/variant_cases.py) the staged Mixtral and LoRA references' own traces pass their checkers, every deliberate wiring error
of tests/variant_ref.py -- and every attention-half error of tests/layer_ref.py that these routes can show -- is reported, first at
the stage it touches, and the conditions on the inputs hold: no empty expert on route A, an empty one on C, every adapter delta at
least half its base output in rms.

Not shown here: ``chunk_positions_from_zero`` needs a cached prefix, which routes A, C and D do not have (both variants run
LlamaAttention's / the prefill op's own position code, which tests/test_gpu_layer_ref.py holds to routes B and E); ``gqa_head_modulo``
is shown by Mixtral's 2 K/V heads and cannot be by 4 or 1."""
import functools

import numpy as np
import pytest

from tests import layer_ref as R
from tests import variant_cases as V
from tests import variant_ref as X


def _shows(name, route, kv_heads):
    return {"chunk_positions_from_zero": False, "decode_position_plus_one": route in "CD", "gqa_head_modulo": kv_heads == 2,
            "mixed_rows_from_front": route == "D", "prefill_ids_per_row": route in "AD", "decode_ids_from_front": route == "D"}.get(name, True)


def _inputs(case):
    return dict(req=case["req"], lay=case["lay"], pool=case["pool"], x=case["x"])


def _own_trace_passes(forward, check, stages, inp):
    before = inp["pool"][0].copy(), inp["pool"][1].copy()
    tr = forward(inp["req"], inp["lay"], inp["pool"], inp["x"])
    assert check(tr, inp) == []
    assert np.array_equal(before[0], inp["pool"][0]) and np.array_equal(before[1].view(np.uint16), inp["pool"][1].view(np.uint16))
    for stage in stages:                                        # a stage cannot pass by being absent
        assert [s for s, _ in check({k: v for k, v in tr.items() if k != stage}, inp)] == [stage]
    return tr


# ---------------------------------------------------------------------------------------------------- Mixtral
MIXTRAL_NAMES = dict(X.ATTN_WRONG, **X.MIXTRAL_WRONG)


@functools.lru_cache(maxsize=None)
def _mixtral(route):
    return _inputs(V.mixtral_case(route))


def test_every_wiring_error_has_a_route_that_shows_it():
    hidden = {"chunk_positions_from_zero"}
    for name in MIXTRAL_NAMES:
        assert any(_shows(name, r, V.MIXTRAL_KV) for r in V.ROUTES) != (name in hidden), name
    for name in dict(X.ATTN_WRONG, **X.LORA_WRONG):
        assert any(_shows(name, r, kv) for r, kv in V.LORA_CASES) != (name in hidden | {"gqa_head_modulo"}), name
    assert set(X.MIXTRAL_WRONG.values()) <= set(X.MOE_STAGES) and set(X.LORA_WRONG.values()) <= set(X.LORA_STAGES)
    assert set(X.ATTN_WRONG) == {n for n, s in R.WRONG.items() if s in R.ATTN_STAGES} and "kv_swapped" in X.ATTN_WRONG


@pytest.mark.parametrize("route", V.ROUTES)
def test_mixtral_own_trace_passes_and_the_experts_are_filled_as_stated(route):
    inp = _mixtral(route)
    tr = _own_trace_passes(X.mixtral_forward, X.mixtral_check, X.MIXTRAL_STAGES, inp)
    counts = np.diff(tr["route"]["expert_indptr"])
    assert counts.sum() == inp["req"].rows * V.TOP_K and len(counts) == V.EXPERTS
    if route == "A":
        assert counts.min() >= 1, counts                      # every expert receives a row
    if route == "C":
        assert counts.min() == 0, counts                      # an expert without a row, and so without a tile


@pytest.mark.parametrize("route,name", [(r, n) for r in V.ROUTES for n in MIXTRAL_NAMES if _shows(n, r, V.MIXTRAL_KV)])
def test_mixtral_wiring_error_is_reported_at_its_stage(route, name):
    inp = _mixtral(route)
    fails = X.mixtral_check(X.mixtral_forward(inp["req"], inp["lay"], inp["pool"], inp["x"], wrong=name), inp)
    assert fails and fails[0][0] == MIXTRAL_NAMES[name], (name, fails)


def _model_trace_and_its_wiring_errors(case, forward, check, layer_error):
    inp = dict(req=case["req"], mdl=case["mdl"], pool=case["pool"], ids=case["ids"])
    run = lambda wrong=None: R.model_forward(case["req"], case["mdl"], case["pool"], case["ids"], wrong=wrong, layer_forward=forward)
    assert R.check_model(run(), inp, layer_check=check) == []
    for name, first in (("no_final_norm", "final_norm"), ("head_before_norm", "logits"), ("cache_layer_zero", "layer1.cache"), layer_error):
        fails = R.check_model(run(name), inp, layer_check=check)
        assert fails and fails[0][0] == first, (name, fails)
    tr = run()
    tr["embed"] = np.roll(tr["embed"], 1, axis=0)
    assert R.check_model(tr, inp, layer_check=check)[0][0] == "embed"


@pytest.mark.parametrize("route", V.MODEL_ROUTES)
def test_mixtral_model_trace_and_its_wiring_errors(route):
    _model_trace_and_its_wiring_errors(V.mixtral_model_case(route), X.mixtral_forward, X.mixtral_check, ("router_reads_residual", "layer0.gate_in"))


# ---------------------------------------------------------------------------------------------------- LoRA
LORA_NAMES = dict(X.ATTN_WRONG, **X.LORA_WRONG)


@functools.lru_cache(maxsize=None)
def _lora(route, kv_heads):
    return _inputs(V.lora_case(route, kv_heads))


def test_lora_ids_are_as_stated():
    for route, ids in V.LORA_IDS.items():
        assert -1 in ids and len(set(ids) - {-1}) == 2 and max(ids) < V.NADAPT
    req = V.lora_case("D", 4)["req"]
    P = len(req.prefills)
    assert V.LORA_IDS["D"][:P] != V.LORA_IDS["D"][P:] and V.ALPHA != V.RANK
    assert X.row_ids(req, V.LORA_IDS["D"]).tolist() == [0] * 5 + [2] * 17 + [-1, 0]


@pytest.mark.parametrize("route,kv_heads", V.LORA_CASES)
def test_lora_own_trace_passes_and_the_deltas_are_large(route, kv_heads):
    inp = _lora(route, kv_heads)
    tr = _own_trace_passes(X.lora_forward, X.lora_check, X.LORA_STAGES + ("d_x",), inp)
    shares = X.adapter_shares(tr, inp["req"], inp["lay"])
    print({m: round(s, 3) for m, s in shares.items()})
    assert set(shares) == set(V.LORA_MODULES) and min(shares.values()) >= 0.5, shares


@pytest.mark.parametrize("route,kv_heads,name", [(r, kv, n) for r, kv in V.LORA_CASES for n in LORA_NAMES if _shows(n, r, kv)])
def test_lora_wiring_error_is_reported_at_its_stage(route, kv_heads, name):
    inp = _lora(route, kv_heads)
    fails = X.lora_check(X.lora_forward(inp["req"], inp["lay"], inp["pool"], inp["x"], wrong=name), inp)
    assert fails and fails[0][0] == LORA_NAMES[name], (name, fails)


@pytest.mark.parametrize("route,kv_heads", V.LORA_MODEL_CASES)
def test_lora_model_trace_and_its_wiring_errors(route, kv_heads):
    _model_trace_and_its_wiring_errors(V.lora_model_case(route, kv_heads), X.lora_forward, X.lora_check, ("adapter_of_layer_zero", "layer1.q"))
