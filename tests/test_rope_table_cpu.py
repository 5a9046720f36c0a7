"""CPU-only: the table path of the paged INT4 attention ops (``rope_table=``, ``attn_scale=``) -- everything about it that needs no GPU.

  * the FP64 reference of tests/rope_table_ref.py equals tests/attn_planted.ref_prefill where a table restates theta / rope_scale, and
    notices each way of mishandling the new arguments (rope_table_ref.MUTANTS) by >= 10 x the bound the GPU tests apply;
  * the three ``_rope`` entry points return their parents' recorded error codes for every call of tests/attn_host_tables.matrix() with
    (NULL, 1.0f), and report their own faults behind the old ones;
  * atom_amd.e2e.rope.rope_init against tests/golden/rope_tables.json (written by transformers 5.15.0) and against transformers live;
  * ops.rope_table rounds once."""
import json
import math
import os
import types

import numpy as np
import pytest

from tests import attn_host_tables as T
from tests import attn_planted as A
from tests import rope_table_ref as RT
from tests.golden import gen_golden_rope_tables as GEN

# Relative tolerance of rope_init (float64) against transformers (fp32 arithmetic).  Largest relative difference measured per config
# with transformers 5.15.0: llama-3.1-8b 3.21e-7, llama-3.2 4.09e-7, linear-2 6.97e-8, yarn-4 1.29e-7, yarn-4-options 1.44e-7.
# The tolerance is 4 x the largest of them.
ROPE_INIT_RTOL = 4 * 4.09e-7


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("theta,scale", [(1e4, 1.0), (5e5, 1.0), (1e6, 4.0)])
@pytest.mark.parametrize("case", [A.PREFILL_CASES[1], A.PREFILL_CASES[3]], ids=A.case_id)
def test_reference_restates_the_theta_reference(case, theta, scale):
    """a float64 table equal to theta^(-2i/128) / rope_scale / 2 pi: the new reference IS attn_planted.ref_prefill (to 1e-12)"""
    shape, P, nkv, G = case
    lens, qo = A.prefill_shape(shape)
    c = A.build_needle(lens, nkv, P, seed=5)
    q = A.needle_queries(int(qo[-1]), nkv * G, 5)
    want = A.ref_prefill(q, c, qo, G=G, theta=theta, rope_scale=scale)
    got = RT.ref_prefill(q, c, qo, RT.theta_table(theta, scale), G=G)
    err = np.abs(got - want).max()
    print(f"{A.case_id(case)} theta={theta:g} scale={scale:g}: max |new - old| {err:.2e}")
    assert err <= 1e-12


def test_attn_scale_is_a_factor_on_the_logits():
    """attn_scale = s on queries q equals attn_scale = 1 on queries s q (s a power of two: exact in fp16)"""
    shape, P, nkv, G = A.PREFILL_CASES[5]
    lens, qo = A.prefill_shape(shape)
    c = A.build_needle(lens, nkv, P, seed=5)
    q = A.needle_queries(int(qo[-1]), nkv * G, 5, a=1.0)
    table, _ = RT.config_table(RT.LLAMA31)
    a = RT.ref_prefill(q, c, qo, table, G=G, attn_scale=2.0)
    b = RT.ref_prefill((q * np.float16(2.0)).astype(np.float16), c, qo, table, G=G)
    assert np.abs(a - b).max() <= 1e-12


def _mutant_inputs():
    """(name, cache, queries, qo, G, rows to check): the 2100-token sequence of DECODE_CASES[0] (MHA) and [2] (G = 4), and a
    32,768-token aliased cache (G = 4)"""
    out = []
    for case in (A.DECODE_CASES[0], A.DECODE_CASES[2]):
        lens, P, nkv, G = case
        b = lens.index(2100)
        out.append((A.case_id(case), A.build_needle(lens, nkv, P, seed=5), A.needle_queries(len(lens), nkv * G, 5), np.arange(len(lens) + 1), G, b))
    out.append(("aliased-32768-g4", RT.aliased_cache(32768), A.needle_queries(1, 8, 7), np.array([0, 1]), 4, 0))
    return out


@pytest.fixture(scope="module")
def mutant_inputs():
    return _mutant_inputs()


@pytest.mark.parametrize("kind", RT.MUTANTS)
def test_mutants_leave_the_reference(kind, mutant_inputs):
    """Each way of mishandling the new arguments moves the reference by >= 10 x the ops' bound in EVERY head, so the GPU tests' bound
    cannot hide it.  Measured for table_ignored (error / bound, smallest head): 2100 tokens MHA 94, G = 4 39 (the figures that say a
    Llama 3.1 config run with plain theta = 5e5 is wrong at every length)."""
    if kind == "attn_scale_ignored":
        table, scale = RT.config_table(RT.YARN)[0], 1.3
    else:
        table, scale = RT.config_table(RT.LLAMA31)
    mt, ms = RT.mutant(kind, table, scale)
    for name, c, q, qo, G, b in mutant_inputs:
        rel = A.rel_bound(G, False)
        ref = RT.ref_prefill(q, c, qo, table, G=G, attn_scale=scale, seqs=[b])
        bad = RT.ref_prefill(q, c, qo, mt, G=G, attn_scale=ms, seqs=[b])
        r = A.error_ratio(bad[b], ref[b], rel)
        print(f"{kind} {name}: error / bound per head, smallest {r.min():.1f}, largest {r.max():.1f}")
        assert r.min() >= 10.0, (kind, name, r)


def test_aliased_cache_is_small_and_long():
    c = RT.aliased_cache(131072)
    assert c["data"].nbytes + c["param"].nbytes < 640 * 1024 and len(set(c["indices"].tolist())) == 64
    assert int(c["indptr"][1]) == 8192 and int(c["lpo"][0]) == 16


# ------------------------------------------------------------------------------------------------ the C entry points, host side
PARENTS = {"atom_batch_decode_gqa_i4": "atom_batch_decode_gqa_i4_rope", "atom_batch_prefill_gqa_i4": "atom_batch_prefill_gqa_i4_rope",
           "atom_batch_decode_append_i4": "atom_batch_decode_append_i4_rope"}


@pytest.fixture(scope="module")
def L():
    from atom_amd._lib import lib
    return lib()


def _call_rope(L, parent, changes, rope_table="null", attn_scale=1.0):
    """tests/attn_host_tables.call through the _rope entry: (rope_table, attn_scale) behind rope_scale"""
    args = []
    for n, v in T.VALID[parent]:
        args.append(T._value(changes.get(n, v)))
        if n == "rope_scale":
            args += [T._value(rope_table), T._value(attn_scale)]
    assert set(changes) <= {n for n, _ in T.VALID[parent]}
    return getattr(L, PARENTS[parent])(*args)


def test_parents_error_codes_through_the_rope_entries(L, golden_dir):
    """every recorded call of the three parents, sent through the _rope entry with (NULL, 1.0f): the recorded code"""
    with open(os.path.join(golden_dir, "attn_host_tables.json")) as f:
        recorded = [(fn, c, st) for fn, c, st in json.load(f)["errors"] if fn in PARENTS]
    assert [(fn, c) for fn, c, _ in recorded] == [(fn, c) for fn, c in T.matrix() if fn in PARENTS]
    assert {fn for fn, _, _ in recorded} == set(PARENTS) and len(recorded) > 150
    wrong = [(fn, c, st, got) for fn, c, st in recorded for got in [_call_rope(L, fn, c)] if got != st]
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("parent", sorted(PARENTS))
def test_new_faults_and_their_place(L, parent):
    from atom_amd import _lib
    for s in (0.0, -1.0, "nan"):
        assert _call_rope(L, parent, {}, attn_scale=s) == _lib.ERR_INVALID_ARG, s
        assert _call_rope(L, parent, {}, rope_table="mem", attn_scale=s) == _lib.ERR_INVALID_ARG, s
    for off in ("+1", "+2", "+3"):
        assert _call_rope(L, parent, {}, rope_table=off) == _lib.ERR_ALIGN, off
    assert _call_rope(L, parent, {}, rope_table="+2", attn_scale=0.0) == _lib.ERR_INVALID_ARG      # the scale first
    # an old fault and a new one: the old code, whichever kind the new one is
    assert _call_rope(L, parent, {"o": "+8"}, attn_scale=0.0) == _lib.ERR_ALIGN
    assert _call_rope(L, parent, {"page_size": 24}, rope_table="+2") == _lib.ERR_SHAPE
    assert _call_rope(L, parent, {"page_size": 24}, attn_scale="nan") == _lib.ERR_SHAPE
    assert _call_rope(L, parent, {"rope_theta": 0.0}, rope_table="+2") == _lib.ERR_INVALID_ARG      # theta is still checked with a table
    assert _call_rope(L, parent, {"o": "null"}, rope_table="+2") == _lib.ERR_INVALID_ARG            # un-merged needs a split: before the table
    if "total_q" in dict(T.VALID[parent]):
        assert _call_rope(L, parent, {"total_q": (1 << 31) - 1}, rope_table="+2") == _lib.ERR_SHAPE  # the last of the old checks


# ------------------------------------------------------------------------------------------------ rope_init
def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _expected(inv_freq_hf):
    return np.asarray(inv_freq_hf, dtype=np.float64)


def _inv_freq_of(config):
    from atom_amd.e2e.rope import rope_init
    theta, rope_scale, inv_freq, af = rope_init(config)
    if inv_freq is None:
        inv_freq = theta ** (-np.arange(0, 128, 2, dtype=np.float64) / 128) / rope_scale
    return inv_freq, af, (theta, rope_scale)


@pytest.fixture(scope="module")
def golden_tables(golden_dir):
    with open(os.path.join(golden_dir, "rope_tables.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(GEN.CONFIGS))
def test_rope_init_equals_the_recorded_transformers_values(name, golden_tables):
    rec = golden_tables["configs"][name]
    assert rec["rope_parameters"] == GEN.CONFIGS[name] and len(rec["inv_freq"]) == 64
    inv_freq, af, (theta, rope_scale) = _inv_freq_of(_ns(rope_theta=None, rope_parameters=rec["rope_parameters"]))
    rel = np.abs(inv_freq - _expected(rec["inv_freq"])) / _expected(rec["inv_freq"])
    print(f"{name}: largest relative difference {rel.max():.3e} (tolerance {ROPE_INIT_RTOL:.3e})")
    assert rel.max() <= ROPE_INIT_RTOL
    assert af == pytest.approx(rec["attention_factor"], rel=1e-12) and theta == rec["rope_parameters"]["rope_theta"]
    kind = rec["rope_parameters"]["rope_type"]
    from atom_amd.e2e.rope import rope_init
    assert (rope_init(_ns(rope_parameters=rec["rope_parameters"]))[2] is None) == (kind == "linear")
    assert rope_scale == (2.0 if kind == "linear" else 1.0)


@pytest.mark.parametrize("name", sorted(GEN.CONFIGS))
def test_rope_init_equals_transformers_live(name):
    pytest.importorskip("transformers")
    try:
        hf_inv, hf_af = GEN.hf_values(GEN.CONFIGS[name])
        config = GEN.hf_config(GEN.CONFIGS[name])
    except Exception as e:                                    # another transformers: other config classes, nothing to compare with
        pytest.skip(f"this transformers does not take the config: {e!r}")
    inv_freq, af, _ = _inv_freq_of(config)                    # the HF config object itself: rope_theta None / absent, rope_parameters set
    rel = np.abs(inv_freq - _expected(hf_inv)) / _expected(hf_inv)
    assert rel.max() <= ROPE_INIT_RTOL and af == pytest.approx(hf_af, rel=1e-12)


def test_both_config_spellings():
    from atom_amd.e2e.rope import rope_init
    rp = dict(GEN.CONFIGS["llama-3.1-8b"])
    new = rope_init(_ns(rope_theta=None, rope_parameters=rp))
    scaling = {k: v for k, v in rp.items() if k != "rope_theta"}
    old = rope_init(_ns(rope_theta=5e5, rope_scaling=scaling))
    legacy = rope_init(_ns(rope_theta=5e5, rope_scaling={**{k: v for k, v in scaling.items() if k != "rope_type"}, "type": "llama3"}))
    for other in (old, legacy):
        assert other[:2] == new[:2] and np.array_equal(other[2], new[2]) and other[3] == new[3]
    assert new[0] == 5e5 and new[2].dtype == np.float64 and new[2].shape == (64,)
    # pairs 0..28 untouched, 35..63 divided by 8, 29..34 blended
    plain = 5e5 ** (-np.arange(64) / 64.0)
    assert np.allclose(new[2][:29], plain[:29], rtol=1e-14, atol=0) and np.allclose(new[2][35:], plain[35:] / 8, rtol=1e-14, atol=0)
    assert np.all(new[2][29:35] < plain[29:35]) and np.all(new[2][29:35] > plain[29:35] / 8)
    # no scaling, in every spelling: nothing changes
    for cfg in (_ns(rope_theta=5e5), _ns(rope_theta=5e5, rope_scaling=None), _ns(rope_theta=None, rope_parameters=dict(rope_type="default", rope_theta=5e5)),
                _ns(rope_parameters=dict(rope_theta=5e5))):
        assert rope_init(cfg) == (5e5, 1.0, None, 1.0)
    assert rope_init(_ns()) == (1e4, 1.0, None, 1.0)
    assert rope_init(_ns(rope_theta=1e4, rope_scaling=dict(type="linear", factor=4.0))) == (1e4, 4.0, None, 1.0)
    yarn = rope_init(_ns(rope_parameters=GEN.CONFIGS["yarn-4"]))
    assert yarn[3] == pytest.approx(0.1 * math.log(4.0) + 1.0) and yarn[1] == 1.0


@pytest.mark.parametrize("rp", [dict(rope_type="dynamic", factor=2.0), dict(rope_type="longrope", factor=2.0), dict(rope_type="proportional"),
                                dict(type="dynamic", factor=2.0), dict(rope_type="su"),
                                dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=4096, mscale=1.0, mscale_all_dim=0.7)])
def test_unsupported_types_raise(rp):
    from atom_amd.e2e.rope import rope_init
    kind = rp.get("rope_type", rp.get("type"))
    with pytest.raises(NotImplementedError, match=kind):
        rope_init(_ns(rope_theta=1e4, rope_scaling=rp))
    with pytest.raises(NotImplementedError, match=kind):
        rope_init(_ns(rope_theta=None, rope_parameters={**rp, "rope_theta": 1e4}))


def test_rope_table_rounds_once():
    import torch
    from atom_amd import ops
    from atom_amd.e2e.rope import rope_init
    inv = rope_init(_ns(rope_parameters=GEN.CONFIGS["llama-3.1-8b"]))[2]
    want = (inv / (2.0 * np.pi)).astype(np.float32)
    for arg in (inv, torch.from_numpy(inv), list(inv)):
        t = ops.rope_table(arg, "cpu")
        assert t.dtype == torch.float32 and t.shape == (64,) and t.is_contiguous()
        assert np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, RT.table_f32(inv))
    twice = inv.astype(np.float32) / np.float32(2.0 * np.pi)  # rounding inv_freq first and dividing in fp32 is NOT the same table
    assert (twice.view(np.uint32) != want.view(np.uint32)).any()
    with pytest.raises(ValueError):
        ops.rope_table(inv[:32], "cpu")
