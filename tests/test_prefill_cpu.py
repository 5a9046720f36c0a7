"""CPU-only checks of the prefill attention's host side: the op refuses CPU tensors, the decoder layer refuses a prefill request
longer than its cache, and the cache bookkeeping for chunked prefill (KvCacheInt4.acquire, BatchedKvCacheInt4.seqlens)."""
import types

import pytest
import torch


def _cpu_cache(seqlens, heads=4, block=16):
    from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    pool = KvPoolInt4(2, heads, 128, 16, block, torch.device("cpu"))
    cs = [KvCacheInt4(pool, s) for s in seqlens]
    return pool, cs, BatchedKvCacheInt4(cs)


def test_batch_prefill_refuses_cpu_tensors():
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    _, _, kv = _cpu_cache([5, 3])
    q = torch.zeros((8, 4, 128), dtype=torch.float16)
    with pytest.raises(AtomHipError):
        ops.batch_prefill_i4(q, torch.tensor([0, 5, 8], dtype=torch.int32), kv, 0)


def test_layer_rejects_negative_prefix():
    from atom_amd.e2e.llama import LlamaAttention
    from atom_amd.utils import BatchLenInfo
    cfg = types.SimpleNamespace(hidden_size=512, num_attention_heads=4, intermediate_size=1408, rms_norm_eps=1e-5, rope_theta=1e4)
    attn = LlamaAttention(cfg, 0)
    _, _, kv = _cpu_cache([5, 9])
    x = tuple(torch.zeros((17, 8)) for _ in range(4))
    with pytest.raises(ValueError):
        attn(x, BatchLenInfo([8, 9], 0, torch.device("cpu")), kv, None)     # 8 new tokens in a 5-token cache


def test_acquire_and_seqlens():
    pool, cs, kv = _cpu_cache([0, 16, 20])
    assert kv.seqlens == [0, 16, 20]
    free = pool.num_free_blocks
    cs[0].acquire(17)                      # 0 -> 17 tokens: two pages
    cs[1].acquire(1)                       # 16 -> 17: a new page
    cs[2].acquire(0)
    assert [c.seqlen for c in cs] == [17, 17, 20] and [len(c.indicies) for c in cs] == [2, 2, 2]
    assert pool.num_free_blocks == free - 3
    with pytest.raises(ValueError):
        cs[2].acquire(-1)
    from atom_amd.utils.kvcache import BatchedKvCacheInt4
    kv2 = BatchedKvCacheInt4(cs)
    assert kv2.seqlens == [17, 17, 20] and kv2.last_page_offset.tolist() == [1, 1, 4]
