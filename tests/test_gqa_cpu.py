"""CPU-only checks of grouped-query attention (GQA): the layer's K/V projection shapes and configuration errors, and the host-side
queries of the GQA decode / prefill entry points (workspace sizes, split counts, shape errors before any pointer is used)."""
import ctypes
import types

import pytest


def _cfg(kv_heads=None, heads=4):
    c = types.SimpleNamespace(hidden_size=512, num_attention_heads=heads, intermediate_size=1408, rms_norm_eps=1e-5, rope_theta=1e4)
    if kv_heads is not None:
        c.num_key_value_heads = kv_heads
    return c


def test_layer_kv_projection_shapes():
    from atom_amd.e2e.llama import LlamaAttention, LlamaDecoderLayer
    at = LlamaAttention(_cfg(2), 0)
    assert at.k_proj.out_features == at.v_proj.out_features == 256 and at.q_proj.out_features == at.o_proj.out_features == 512
    assert at.num_kv_heads == 2 and at.gqa
    layer = LlamaDecoderLayer(types.SimpleNamespace(num_hidden_layers=1, **vars(_cfg(2))), 0)
    assert layer.self_attn.k_proj.weight_int4.shape == (256, (512 - 128) // 2)
    assert layer.self_attn.v_proj.scale_int4.shape[0] == 512 // 128 - 1
    for bad in (3, 0, 8):
        with pytest.raises(ValueError):
            LlamaAttention(_cfg(bad), 0)


def test_mha_config_shapes_unchanged():
    from atom_amd.e2e.llama import LlamaAttention
    shapes = [{k: tuple(v.shape) for k, v in LlamaAttention(c, 0).state_dict().items()} for c in (_cfg(None), _cfg(4))]
    assert shapes[0] == shapes[1]
    assert shapes[0]["k_proj.weight_int4"] == (512, 192) and shapes[0]["v_proj.weight_int8"] == (512, 128)
    assert not LlamaAttention(_cfg(None), 0).gqa


def test_host_queries_equal_mha_at_g1():
    from atom_amd._lib import lib
    L = lib()
    for b, n, p, mp in [(1, 32, 16, 256), (16, 32, 16, 64), (64, 8, 16, 256), (3, 4, 48, 0), (200, 8, 16, 300), (1, 1, 16, 1)]:
        assert L.atom_batch_decode_gqa_i4_workspace_bytes(b, n, n, p, mp) == L.atom_batch_decode_i4_workspace_bytes(b, n, p, mp)
        assert L.atom_batch_decode_gqa_i4_splits(b, n, n, p, mp) == L.atom_batch_decode_i4_splits(b, n, p, mp)
    for T, b, n, p, mq, mp in [(8, 1, 32, 16, 8, 256), (2048, 1, 32, 16, 2048, 128), (100, 3, 4, 48, 60, 50), (5, 5, 8, 16, 1, 0)]:
        assert L.atom_batch_prefill_gqa_i4_workspace_bytes(T, b, n, n, p, mq, mp) == L.atom_batch_prefill_i4_workspace_bytes(T, b, n, p, mq, mp)


def test_host_queries_gqa():
    from atom_amd._lib import lib
    L = lib()
    seen = set()
    for b, nq, nkv, p, mp in [(1, 32, 8, 16, 256), (16, 32, 8, 16, 256), (64, 32, 8, 16, 256), (1, 28, 4, 16, 128), (40, 32, 8, 16, 6),
                              (1, 7, 1, 16, 125), (300, 8, 1, 48, 2)]:
        s = L.atom_batch_decode_gqa_i4_splits(b, nq, nkv, p, mp)
        assert s >= 1
        seen.add(s > 1)
        assert L.atom_batch_decode_gqa_i4_workspace_bytes(b, nq, nkv, p, mp) == (b * nq * s * 130 * 4 if s > 1 else 0)
        assert L.atom_batch_decode_gqa_i4_splits(b, nq, nkv, p, 0) == 1 and L.atom_batch_decode_gqa_i4_workspace_bytes(b, nq, nkv, p, 0) == 0
    assert seen == {True, False}
    # a short chunk on a long prefix splits its KV range; the workspace holds every query head's partial states
    ws = L.atom_batch_prefill_gqa_i4_workspace_bytes(8, 1, 32, 8, 16, 8, 256)
    assert ws > 0 and ws % (8 * 32 * 130 * 4) == 0
    for nq, nkv in ((6, 4), (6, 0), (0, 2), (8, -1)):
        assert L.atom_batch_decode_gqa_i4_splits(1, nq, nkv, 16, 64) == 0
        assert L.atom_batch_decode_gqa_i4_workspace_bytes(1, nq, nkv, 16, 64) == 0
        assert L.atom_batch_prefill_gqa_i4_workspace_bytes(8, 1, nq, nkv, 16, 8, 64) == 0


def test_rejected_head_counts_before_any_pointer():
    """ATOM_ERR_SHAPE for num_qo_heads % num_kv_heads != 0 or num_kv_heads < 1 comes back before the library looks at a pointer (the
    buffers below are host memory: no device work is started)."""
    from atom_amd import _lib as L
    lib = L.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    for nq, nkv in ((6, 4), (6, 0), (4, -2), (0, 1)):
        st = lib.atom_batch_decode_gqa_i4(p, p, p, p, p, p, p, 1, 1, 0, nq, nkv, 16, 128, 1e4, 1.0, 0, None, 0, None)
        assert st == L.ERR_SHAPE, (nq, nkv, st)
        st = lib.atom_batch_prefill_gqa_i4(p, p, p, 1, 1, p, p, p, p, p, 1, 1, 0, nq, nkv, 16, 128, 1e4, 1.0, 0, None, 0, None)
        assert st == L.ERR_SHAPE, (nq, nkv, st)
