"""Without a GPU: the host side of head size 64 (csrc/attn_d64.hip) -- the symbols, the documented codes of the argument checks (host
pointers: every call comes back before a launch), the plan queries' self-consistency -- and the model classes' acceptance / refusals."""
import ctypes
import itertools
import types

import pytest
import torch

from tests import attn_host_tables as H

_KV64 = H._KV + H._DIMS + [("num_qo_heads", 8), ("num_kv_heads", 4), ("page_size", 16), ("head_dim", 64)]
_TAIL = [("rope_theta", 1e4), ("rope_scale", 1.0), ("rope_table", "null"), ("attn_scale", 1.0), ("max_pages_per_seq", 0), ("workspace", "null"),
         ("workspace_bytes", 0), ("stream", "null")]
VALID = {
    "atom_batch_decode_gqa_i4_d64": [("o", "mem"), ("q", "mem")] + _KV64 + _TAIL,
    "atom_batch_prefill_gqa_i4_d64": [("o", "mem"), ("q", "mem"), ("qo_indptr", "mem"), ("total_q", 3), ("max_q_len", 2)] + _KV64 + _TAIL,
    "atom_kv_append_i4_d64": H._KV + [("k", "mem"), ("v", "mem"), ("k_param", "mem"), ("v_param", "mem"), ("append_indptr", "mem"), ("total_tokens", 3)]
                             + H._DIMS + [("num_heads", 4), ("page_size", 16), ("head_dim", 64), ("stream", "null")],
    "atom_kv_quant_u4_f16_d64": [("k", "mem"), ("packed", "mem"), ("param", "mem"), ("T", 3), ("kv_heads", 4), ("head_dim", 64), ("stream", "null")],
}
FIRST_PTR = {"atom_batch_decode_gqa_i4_d64": "q", "atom_batch_prefill_gqa_i4_d64": "q", "atom_kv_append_i4_d64": "k", "atom_kv_quant_u4_f16_d64": "k"}


@pytest.fixture(scope="module")
def L():
    from atom_amd._lib import lib
    return lib()


def _call(L, fn, **changes):
    assert set(changes) <= {n for n, _ in VALID[fn]}, changes
    return getattr(L, fn)(*(H._value(changes.get(n, v)) for n, v in VALID[fn]))


@pytest.mark.parametrize("fn", sorted(VALID))
def test_argument_checks(L, fn):
    from atom_amd import _lib
    assert fn in _lib.SIGNATURES and ctypes.cast(getattr(L, fn), ctypes.c_void_p).value
    for dim in (128, 96, 0):
        assert _call(L, fn, head_dim=dim) == _lib.ERR_SHAPE
    ptr = FIRST_PTR[fn]
    assert _call(L, fn, **{ptr: "null"}) == _lib.ERR_INVALID_ARG and _call(L, fn, **{ptr: "+8"}) == _lib.ERR_ALIGN
    if "kv_data" in dict(VALID[fn]):
        assert _call(L, fn, kv_data="null") == _lib.ERR_INVALID_ARG and _call(L, fn, kv_data="+8") == _lib.ERR_ALIGN
        assert _call(L, fn, page_size=24) == _lib.ERR_SHAPE and _call(L, fn, layer_idx=2) == _lib.ERR_SHAPE
    if "rope_table" in dict(VALID[fn]):
        assert _call(L, fn, num_qo_heads=6) == _lib.ERR_SHAPE and _call(L, fn, o="null") == _lib.ERR_INVALID_ARG
        assert _call(L, fn, rope_table="+2") == _lib.ERR_ALIGN and _call(L, fn, attn_scale=0.0) == _lib.ERR_INVALID_ARG


def test_plan_queries_are_self_consistent(L):
    split = 0
    for b, nkv, g, p, mp in itertools.product(H.BATCH, H.KV_HEADS, H.GROUP, H.PAGE, H.MAX_PAGES):
        s = L.atom_batch_decode_gqa_i4_d64_splits(b, nkv * g, nkv, p, mp)
        assert 1 <= s <= 32 and (mp > 0 or s == 1)
        assert L.atom_batch_decode_gqa_i4_d64_workspace_bytes(b, nkv * g, nkv, p, mp) == (b * nkv * g * s * 66 * 4 if s > 1 else 0)
        for T, mq in H.PREFILL:
            s = L.atom_batch_prefill_gqa_i4_d64_splits(T, b, nkv * g, nkv, p, mq, mp)
            assert 1 <= s <= 32 and (mp > 0 or s == 1)
            assert L.atom_batch_prefill_gqa_i4_d64_workspace_bytes(T, b, nkv * g, nkv, p, mq, mp) == (T * nkv * g * s * 66 * 4 if s > 1 else 0)
            split += s > 1
    assert split > 1000
    assert L.atom_batch_decode_gqa_i4_d64_splits(1, 6, 4, 16, 64) == 0 and L.atom_batch_decode_gqa_i4_d64_workspace_bytes(1, 8, 4, 8, 64) == 0


def _cfg(heads, **kw):
    return types.SimpleNamespace(hidden_size=512, num_attention_heads=heads, num_key_value_heads=2, intermediate_size=1408, rms_norm_eps=1e-5,
                                 rope_theta=1e4, num_hidden_layers=1, vocab_size=64, pad_token_id=None, **kw)


def test_model_classes_accept_64_and_refuse_the_rest():
    from atom_amd import ops
    from atom_amd.e2e.llama import LlamaAttention, LlamaForCausalLM
    from atom_amd.e2e.llama_lora import LlamaForCausalLMWithLora
    from atom_amd.e2e.mixtral import MixtralForCausalLM
    at = LlamaAttention(_cfg(8), 0)
    assert at.head_dim == 64 and at.k_proj.out_dtype == at.v_proj.out_dtype == "fp16" and at.k_proj.out_features == 128
    assert LlamaAttention(_cfg(4), 0).k_proj.out_dtype == "int4"                       # head 128: what it always built
    assert LlamaAttention(_cfg(8, head_dim=64), 0).head_dim == 64 and LlamaForCausalLM(_cfg(8)).model.layers[0].self_attn.head_dim == 64
    for bad in (_cfg(16), _cfg(4, head_dim=96), _cfg(8, head_dim=128)):              # 32; 96; 8 x 128 is not the hidden size
        with pytest.raises(ValueError):
            LlamaAttention(bad, 0)
    for build in (lambda: LlamaAttention(_cfg(8, sliding_window=64), 0), lambda: LlamaForCausalLMWithLora(_cfg(8)),
                  lambda: MixtralForCausalLM(_cfg(8, num_local_experts=4, num_experts_per_tok=2))):
        with pytest.raises(NotImplementedError):
            build()
    assert ops.rope_table([0.5] * 32, "cpu", 64).shape == (32,) and ops.rope_table([0.5] * 64, "cpu").shape == (64,)
    with pytest.raises(ValueError):
        ops.rope_table([0.5] * 64, "cpu", 64)
    kv = types.SimpleNamespace(data=torch.zeros(1, 1, 2, 2, 16, 32, dtype=torch.uint8))
    for call in (lambda: ops.quant_append_kv_i4(kv, None, None, 0), lambda: ops.kv_beam_fork_i4(kv, None), lambda: ops.decode_splits(1, kv, window=8)):
        with pytest.raises(NotImplementedError):
            call()
