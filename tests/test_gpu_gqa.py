"""GPU tests of grouped-query attention (GQA) over the INT4 paged KV cache (atom_batch_decode_gqa_i4 / atom_batch_prefill_gqa_i4,
csrc/prefill_i4.hip): query head h reads K/V head h // G.  Against FP64 on the cache with its K/V heads repeated G times, against the MHA
ops (G = 1 bit for bit, the replicated cache within the op's bound), robustness, the decoder layer against an MHA layer with replicated
k_proj / v_proj rows, and the grouped-query flow model exported into the serving model."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests.helpers import t2n

pytestmark = pytest.mark.gpu


def _setup(seqlens, heads, layers=2, block=16, seed=0, extra_blocks=3):
    """a random cache of `heads` K/V heads (codes and (scale, zero) everywhere, also past the ends), pages in a scrambled order"""
    from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    g = torch.Generator(device="cuda").manual_seed(seed)
    cap = sum(-(-s // block) for s in seqlens) + extra_blocks
    pool = KvPoolInt4(layers, heads, 128, cap, block, torch.device("cuda"))
    pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device="cuda", generator=g, dtype=torch.uint8))
    pool.param.copy_((torch.rand(pool.param.shape, device="cuda", generator=g) * 0.2 + 0.01).half())
    cs = [KvCacheInt4(pool, s) for s in seqlens]
    kv = BatchedKvCacheInt4(cs)
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(cap)).to(device="cuda", dtype=torch.int32)
    kv.indicies = perm[kv.indicies.long()].contiguous()
    return pool, kv, g


def _replicated(kv, G):
    """the same cache with every K/V head repeated G times (HF's repeat_kv): today's only way to run a GQA model on the MHA ops"""
    return types.SimpleNamespace(data=kv.data.repeat_interleave(G, dim=3).contiguous(), param=kv.param.repeat_interleave(G, dim=3).contiguous(),
                                 indptr=kv.indptr, indicies=kv.indicies, last_page_offset=kv.last_page_offset, max_pages=kv.max_pages)


def _ref_decode(q, kv, layer, G):
    return O.batch_decode_i4(t2n(q), np.repeat(t2n(kv.data), G, axis=3), np.repeat(t2n(kv.param), G, axis=3), t2n(kv.indptr),
                             t2n(kv.indicies), t2n(kv.last_page_offset), layer)


def _ref_prefill(q, kv, qo, layer, G, theta=1e4):
    """tests/test_gpu_prefill_i4.py::_ref with query head h on K/V head h // G (each K/V head de-quantised once per sequence)"""
    qn = t2n(q).astype(np.float64)
    data, param = t2n(kv.data), t2n(kv.param)
    indptr, indices, lpo = t2n(kv.indptr), t2n(kv.indicies), t2n(kv.last_page_offset)
    P = data.shape[4]
    T, Nq, D = qn.shape
    out = np.zeros((T, Nq, D))
    for b in range(len(lpo)):
        S = O.kv_seq_len(indptr, lpo, P, b)
        r0, r1 = int(qo[b]), int(qo[b + 1])
        pos = np.arange(S - (r1 - r0), S)
        pages = [int(x) for x in indices[int(indptr[b]):int(indptr[b + 1])]]
        for hk in range(Nq // G):
            kp = np.concatenate([data[pg, layer, 0, hk] for pg in pages], axis=0)[:S]
            vp = np.concatenate([data[pg, layer, 1, hk] for pg in pages], axis=0)[:S]
            kq = np.concatenate([param[pg, layer, 0, hk] for pg in pages], axis=0)[:S]
            vq = np.concatenate([param[pg, layer, 1, hk] for pg in pages], axis=0)[:S]
            kf = O._rope_llama(O._dequant_u4_rows(kp, kq), np.arange(S), theta)
            vf = O._dequant_u4_rows(vp, vq)
            for h in range(hk * G, hk * G + G):
                qf = O._rope_llama(qn[r0:r1, h], pos, theta)
                s = qf @ kf.T / np.sqrt(D)
                s[np.arange(S)[None, :] > pos[:, None]] = -np.inf
                pr = np.exp(s - s.max(axis=1, keepdims=True))
                out[r0:r1, h] = (pr / pr.sum(axis=1, keepdims=True)) @ vf
    return out


def _bound(o, ref, rel=4e-3):
    err = np.abs(t2n(o).astype(np.float64) - ref).max()
    return err <= rel * np.abs(ref).max() + 1e-3, (err, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ decode
# (G, K/V heads, sequence lengths, page size): lengths 1, page edges and >= 2000; batch x K/V heads from 1 to 320 (every split regime)
DECODE_CASES = [
    (2, 2, [1, 15, 16, 17, 2100], 16),
    (4, 2, [1, 47, 48, 49, 300], 48),
    (7, 1, [2000, 17], 16),
    (8, 4, [5, 16, 33, 130], 48),
    (4, 8, [1 + (37 * i) % 90 for i in range(40)], 16),
]


@pytest.mark.parametrize("G,nkv,seqlens,block", DECODE_CASES)
def test_decode_gqa_matches_fp64(G, nkv, seqlens, block):
    from atom_amd import ops
    pool, kv, g = _setup(seqlens, nkv, block=block, seed=G + nkv)
    q = torch.randn((len(seqlens), G * nkv, 128), device="cuda", generator=g).half()
    max_pages = kv.max_pages
    for layer in (0, 1):
        ref = _ref_decode(q, kv, layer, G)
        for mp in (max_pages, 0):                          # the host knows the longest sequence (KV split) / does not (no split)
            kv.max_pages = mp
            o = ops.batch_decode_i4(q, kv, layer)
            ok, info = _bound(o, ref)
            assert ok, (layer, mp, info)
        kv.max_pages = max_pages
    if max(seqlens) >= 2000:
        assert ops.decode_splits(len(seqlens), kv, G * nkv) >= 2     # the split path ran


@pytest.mark.parametrize("G,nkv,seqlens", [(4, 1, [1030]), (2, 2, [2500])])
def test_decode_gqa_against_mha_on_replicated_cache(G, nkv, seqlens):
    """The GQA op against today's workaround (the MHA op on the cache replicated to the query heads), within the op's bound; and the
    merged output equals merge=False -> dense_layer_gemm_i4_merge_q's merge bit for bit (as the MHA op: tests/test_gpu_e2e.py)."""
    from atom_amd import ops
    from atom_amd.e2e.llama import LinearInt4
    pool, kv, g = _setup(seqlens, nkv, seed=21)
    nq, batch = G * nkv, len(seqlens)
    q = torch.randn((batch, nq, 128), device="cuda", generator=g).half()
    o = ops.batch_decode_i4(q, kv, 1)
    mha = ops.batch_decode_i4(q, _replicated(kv, G), 1).float()
    assert (o.float() - mha).abs().max().item() <= 4e-3 * mha.abs().max().item()
    splits = ops.decode_splits(batch, kv, nq)
    assert splits >= 2
    part = ops.batch_decode_i4(q, kv, 1, merge=False)
    assert part.shape == (batch, nq, splits, 130)
    hs = nq * 128
    assert ops.merge_q_gemm_fits(batch, hs, 1, hs, splits)
    proj = LinearInt4(hs, hs, "fp16").cuda()
    gw = torch.Generator().manual_seed(2)
    proj.load_fp16_weight((torch.randn(hs, hs, generator=gw) * 0.05).half().cuda())
    ridx = torch.randperm(hs, generator=gw).to(torch.int16).cuda()
    (fused,) = ops.dense_layer_gemm_i4_merge_q(part, splits, proj.single(), reorder_index=ridx)
    (sep,), _ = ops.dense_layer_gemm_i4_multi_q("reorder", o.view(batch, hs), proj.single(), reorder_index=ridx)
    assert torch.equal(fused, sep)


# ------------------------------------------------------------------------------------------------ prefill
# (prefixes, q lens, G, K/V heads, page size)
PREFILL_CASES = [
    ([0, 15], [64, 16], 2, 2, 16),
    ([300, 0, 1], [1, 200, 63], 4, 2, 16),
    ([0], [1000], 8, 1, 16),
    ([2000, 16], [7, 65], 7, 1, 48),
    ([16, 0], [33, 9], 8, 2, 48),
]


@pytest.mark.parametrize("prefixes,qlens,G,nkv,block", PREFILL_CASES)
def test_prefill_gqa_matches_fp64(prefixes, qlens, G, nkv, block):
    from atom_amd import ops
    pool, kv, g = _setup([a + n for a, n in zip(prefixes, qlens)], nkv, block=block, seed=len(qlens) + G)
    qo = np.cumsum([0] + list(qlens)).astype(np.int32)
    q = torch.randn((int(qo[-1]), G * nkv, 128), device="cuda", generator=g).half()
    for layer in (0, 1):
        o = ops.batch_prefill_i4(q, torch.from_numpy(qo).cuda(), kv, layer, max_q_len=max(qlens))
        ok, info = _bound(o, _ref_prefill(q, kv, qo, layer, G))
        assert ok, (layer, info)


@pytest.mark.parametrize("prefixes,qlens,G,nkv", [([2000], [8], 4, 8), ([300, 2000, 16], [7, 16, 1], 2, 2)])
def test_prefill_gqa_split_and_no_split(prefixes, qlens, G, nkv):
    from atom_amd import ops
    from atom_amd._lib import lib
    pool, kv, g = _setup([a + n for a, n in zip(prefixes, qlens)], nkv, seed=7)
    qo = np.cumsum([0] + list(qlens)).astype(np.int32)
    qo_d = torch.from_numpy(qo).cuda()
    nq, T = G * nkv, int(qo[-1])
    q = torch.randn((T, nq, 128), device="cuda", generator=g).half()
    assert lib().atom_batch_prefill_gqa_i4_workspace_bytes(T, len(qlens), nq, nkv, 16, max(qlens), kv.max_pages) > 0
    o_split = ops.batch_prefill_i4(q, qo_d, kv, 1, max_q_len=max(qlens))
    kv.max_pages = 0
    o_one = ops.batch_prefill_i4(q, qo_d, kv, 1, max_q_len=max(qlens))
    ref = _ref_prefill(q, kv, qo, 1, G)
    for o in (o_split, o_one):
        ok, info = _bound(o, ref)
        assert ok, info
    assert (o_split.float() - o_one.float()).abs().max().item() <= 4e-3 * np.abs(ref).max() + 1e-3


def test_prefill_gqa_one_query_per_sequence_is_decode():
    from atom_amd import ops
    seqlens = [37, 5, 16, 1, 300, 2000]
    pool, kv, g = _setup(seqlens, 2, seed=5)
    q = torch.randn((len(seqlens), 8, 128), device="cuda", generator=g).half()
    qo = torch.arange(len(seqlens) + 1, dtype=torch.int32, device="cuda")
    for layer in (0, 1):
        d = ops.batch_decode_i4(q, kv, layer).float()
        o = ops.batch_prefill_i4(q, qo, kv, layer, max_q_len=1).float()
        assert (o - d).abs().max().item() <= 4e-3 * d.abs().max().item(), layer


# ------------------------------------------------------------------------------------------------ G = 1 through the new entry points
def _decode_gqa_raw(q, kv, layer, nq, nkv, o, ws, ws_bytes):
    from atom_amd import _lib as L
    from atom_amd import ops
    num_layers, _, P, D = ops._kv_dims(kv)
    return L.lib().atom_batch_decode_gqa_i4(L.ptr(o), q.data_ptr(), kv.data.data_ptr(), kv.param.data_ptr(), kv.indptr.data_ptr(),
                                            kv.indicies.data_ptr(), kv.last_page_offset.data_ptr(), q.size(0), num_layers, layer, nq, nkv,
                                            P, D, 1e4, 1.0, kv.max_pages, L.ptr(ws), ws_bytes, L.current_stream(q.device))


def test_g1_entry_points_equal_mha():
    from atom_amd import _lib as L
    from atom_amd import ops
    lib = L.lib()
    seqlens = [2100, 17, 1]
    N = 4
    pool, kv, g = _setup(seqlens, N, seed=3)
    B = len(seqlens)
    q = torch.randn((B, N, 128), device="cuda", generator=g).half()
    for args in [(B, N, 16, kv.max_pages), (1, N, 16, kv.max_pages), (64, N, 48, 0), (200, 8, 16, 300)]:
        b, n, p, mp = args
        assert lib.atom_batch_decode_gqa_i4_workspace_bytes(b, n, n, p, mp) == lib.atom_batch_decode_i4_workspace_bytes(b, n, p, mp)
        assert lib.atom_batch_decode_gqa_i4_splits(b, n, n, p, mp) == lib.atom_batch_decode_i4_splits(b, n, p, mp)
    ws_bytes = lib.atom_batch_decode_i4_workspace_bytes(B, N, 16, kv.max_pages)
    splits = lib.atom_batch_decode_i4_splits(B, N, 16, kv.max_pages)
    assert splits >= 2
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device="cuda")
    for layer in (0, 1):
        o = torch.empty_like(q)
        L.check(_decode_gqa_raw(q, kv, layer, N, N, o, ws, ws_bytes), "atom_batch_decode_gqa_i4")
        assert torch.equal(o, ops.batch_decode_i4(q, kv, layer))
        L.check(_decode_gqa_raw(q, kv, layer, N, N, None, ws, ws_bytes), "atom_batch_decode_gqa_i4 (un-merged)")
        assert torch.equal(ws.view(B, N, splits, 130), ops.batch_decode_i4(q, kv, layer, merge=False))
    # prefill
    qlens = [9, 17, 1]
    qp = torch.randn((sum(qlens), N, 128), device="cuda", generator=g).half()
    qo = torch.tensor(np.cumsum([0] + qlens), dtype=torch.int32, device="cuda")
    T, mq = qp.size(0), max(qlens)
    wsb = lib.atom_batch_prefill_i4_workspace_bytes(T, B, N, 16, mq, kv.max_pages)
    assert wsb > 0 and lib.atom_batch_prefill_gqa_i4_workspace_bytes(T, B, N, N, 16, mq, kv.max_pages) == wsb
    wsp = torch.empty(wsb // 4, dtype=torch.float32, device="cuda")
    o = torch.empty_like(qp)
    st = lib.atom_batch_prefill_gqa_i4(o.data_ptr(), qp.data_ptr(), qo.data_ptr(), T, mq, kv.data.data_ptr(), kv.param.data_ptr(),
                                       kv.indptr.data_ptr(), kv.indicies.data_ptr(), kv.last_page_offset.data_ptr(), B, 2, 1, N, N, 16, 128,
                                       1e4, 1.0, kv.max_pages, wsp.data_ptr(), wsb, L.current_stream(qp.device))
    L.check(st, "atom_batch_prefill_gqa_i4")
    assert torch.equal(o, ops.batch_prefill_i4(qp, qo, kv, 1, max_q_len=mq))


# ------------------------------------------------------------------------------------------------ robustness
def test_gqa_nan_past_end_read_only_and_graph_capture():
    from atom_amd import ops
    seqlens = [17, 40, 2000]
    G, nkv = 4, 2
    pool, kv, g = _setup(seqlens, nkv, seed=9)
    ref_q = torch.randn((len(seqlens), G * nkv, 128), device="cuda", generator=g).half()
    qo = torch.arange(len(seqlens) + 1, dtype=torch.int32, device="cuda")
    clean = [ops.batch_decode_i4(ref_q, kv, 0), ops.batch_prefill_i4(ref_q, qo, kv, 0, max_q_len=1)]
    # NaN / Inf in every slot past a sequence's end (its last page's tail)
    P = pool.block_len
    pages, lpo = kv.indicies.tolist(), kv.last_page_offset.tolist()
    ends = np.cumsum([0] + [-(-s // P) for s in seqlens])
    for b in range(len(seqlens)):
        last = pages[ends[b + 1] - 1]
        pool.param[last, :, :, :, lpo[b]:, :] = float("nan")
        pool.param[last, :, :, :, lpo[b]:, 0] = float("inf")
    before = (pool.buf.clone(), pool.param.clone())
    got = [ops.batch_decode_i4(ref_q, kv, 0), ops.batch_prefill_i4(ref_q, qo, kv, 0, max_q_len=1)]
    for a, b in zip(clean, got):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    torch.cuda.synchronize()
    assert torch.equal(pool.buf, before[0]) and torch.equal(pool.param.view(torch.int16), before[1].view(torch.int16))
    # graph capture of both ops equals eager
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.batch_decode_i4(ref_q, kv, 1)
            ops.batch_prefill_i4(ref_q, qo, kv, 1, max_q_len=1)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd = ops.batch_decode_i4(ref_q, kv, 1)
        gp = ops.batch_prefill_i4(ref_q, qo, kv, 1, max_q_len=1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gd, ops.batch_decode_i4(ref_q, kv, 1)) and torch.equal(gp, ops.batch_prefill_i4(ref_q, qo, kv, 1, max_q_len=1))


def test_gqa_rejected_arguments():
    from atom_amd import _lib as L
    from atom_amd import ops
    pool, kv, g = _setup([20, 5], 2, seed=1)
    q = torch.randn((2, 6, 128), device="cuda", generator=g).half()
    o = torch.empty_like(q)
    for nq, nkv in ((6, 4), (6, 0), (0, 2), (6, -1)):
        assert _decode_gqa_raw(q, kv, 0, nq, nkv, o, None, 0) == L.ERR_SHAPE, (nq, nkv)
    assert _decode_gqa_raw(q, kv, 0, 6, 2, None, None, 0) == L.ERR_INVALID_ARG     # un-merged without a split
    assert _decode_gqa_raw(q, kv, 2, 6, 2, o, None, 0) == L.ERR_SHAPE              # layer out of range
    q5 = torch.randn((2, 5, 128), device="cuda", generator=g).half()
    with pytest.raises(ValueError):
        ops.batch_decode_i4(q5, kv, 0)
    with pytest.raises(ValueError):
        ops.batch_prefill_i4(q5, torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"), kv, 0, max_q_len=1)
    with pytest.raises(ValueError):
        ops.decode_splits(2, kv, 5)
    k32 = torch.zeros((2, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ops.batch_decode_i4(q, kv, 0, append_kv=(k32, k32))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ decoder layer
def _cfg(kv_heads, layers=1):
    c = types.SimpleNamespace(hidden_size=512, num_attention_heads=4, intermediate_size=1408, rms_norm_eps=1e-5, rope_theta=1e4,
                              num_hidden_layers=layers, vocab_size=1000, pad_token_id=None)
    if kv_heads is not None:
        c.num_key_value_heads = kv_heads
    return c


def _pair(G):
    """a GQA layer (4 query heads on 4 / G K/V heads) and an MHA layer whose k_proj / v_proj weights are the GQA ones with each head's
    128 rows repeated G times; every other weight, norm and reorder index shared"""
    from atom_amd.e2e import LlamaDecoderLayer
    from atom_amd.e2e.llama import DecodeFusion
    torch.manual_seed(5)                                      # (the modules draw their reorder indices from the global generator)
    gl = LlamaDecoderLayer(_cfg(4 // G), layer_idx=1, fusion=DecodeFusion()).cuda()
    ml = LlamaDecoderLayer(_cfg(None), layer_idx=1, fusion=DecodeFusion()).cuda()
    gen = torch.Generator().manual_seed(5)
    for (name, mg), mm in zip(gl.named_modules(), ml.modules()):
        if type(mg).__name__ == "LinearInt4":
            w = (torch.randn(mg.out_features, mg.in_features, generator=gen) * 0.05).half()
            mg.load_fp16_weight(w.cuda())
            if name.endswith(("k_proj", "v_proj")):
                w = w.view(-1, 128, w.size(1)).repeat_interleave(G, dim=0).reshape(-1, w.size(1))
            mm.load_fp16_weight(w.cuda())
        elif type(mg).__name__ == "LlamaRMSNormInt4":
            mg.weight.data = (1 + 0.1 * torch.randn(mg.weight.shape, generator=gen)).half().cuda()
            mm.weight.data = mg.weight.data.clone()
            mm.reorder_index.data = mg.reorder_index.data.clone()
    ml.self_attn.reorder_index.data = gl.self_attn.reorder_index.data.clone()
    return gl, ml


class _Spy:
    """the attention output of a layer: the input of ops.reorder_fp16_i4 with the attention's reorder index"""

    def __init__(self, layers):
        from atom_amd import ops
        self.ops, self.orig, self.idx, self.got = ops, ops.reorder_fp16_i4, [l.self_attn.reorder_index for l in layers], []

    def __enter__(self):
        def spy(a, idx, **kw):
            if any(idx is i for i in self.idx):
                self.got.append(a.clone())
            return self.orig(a, idx, **kw)
        self.ops.reorder_fp16_i4 = spy
        return self

    def __exit__(self, *exc):
        self.ops.reorder_fp16_i4 = self.orig


def _close(a, b, rel=4e-3):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= rel * b.abs().max().item(), ((a - b).abs().max().item(), b.abs().max().item())


@pytest.mark.parametrize("G", [2, 4])
def test_gqa_layer_prefill_equals_replicated_mha(G):
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    dev = torch.device("cuda")
    gl, ml = _pair(G)
    lens, chunks = [37, 16], [[20, 5], [17, 11]]
    x = [(torch.randn(n, 512, generator=torch.Generator().manual_seed(i)) * 0.7).half().cuda() for i, n in enumerate(lens)]
    for route in ("hip", "torch", "chunked"):
        outs, atts = [], []
        for layer, heads in ((gl, 4 // G), (ml, 4)):
            layer.fusion.prefill_attn = route != "torch"
            pool = KvPoolInt4(num_layers=2, num_heads=heads, head_dim=128, capacity=16, block_len=16, device=dev)
            with _Spy([layer]) as spy:
                if route == "chunked":
                    cs = [KvCacheInt4(pool, 0) for _ in lens]
                    beg, ys = [0, 0], []
                    for ch in chunks:
                        for c, n in zip(cs, ch):
                            c.acquire(n)
                        ys.append(layer(torch.cat([xi[b:b + n] for xi, b, n in zip(x, beg, ch)]), BatchLenInfo(ch, 0, dev), BatchedKvCacheInt4(cs), None))
                        beg = [b + n for b, n in zip(beg, ch)]
                    y, a = torch.cat(ys), torch.cat(spy.got)
                else:
                    y = layer(torch.cat(x), BatchLenInfo(lens, 0, dev), BatchedKvCacheInt4([KvCacheInt4(pool, n) for n in lens]), None)
                    a = spy.got[0]
            outs.append(y)
            atts.append(a)
        ok, info = _close(atts[0], atts[1])
        assert ok, (route, info)
        assert torch.isfinite(outs[0]).all()
        ok, info = _close(outs[0], outs[1], 0.05)
        assert ok, (route, info)


class _DecodeSpy:
    """the decode attention's output: what ops.batch_decode_i4 returns, its partial states merged here where o_proj's launch merges them"""

    def __init__(self):
        from atom_amd import ops
        self.ops, self.orig, self.got = ops, ops.batch_decode_i4, []

    def __enter__(self):
        def spy(q, kv, layer_idx, **kw):
            r = self.orig(q, kv, layer_idx, **kw)
            if kw.get("merge", True):
                self.got.append(r.clone())
            else:                                            # float [batch, heads, splits, 130]: out = sum_s o_s 2^(m_s - M) / sum_s d_s 2^(m_s - M)
                m = r[..., 128:129]
                w = torch.exp2(m - m.max(dim=2, keepdim=True).values)
                self.got.append(((r[..., :128] * w).sum(2) / (r[..., 129:130] * w).sum(2)).half())
            return r
        self.ops.batch_decode_i4 = spy
        return self

    def __exit__(self, *exc):
        self.ops.batch_decode_i4 = self.orig


@pytest.mark.parametrize("bsz,mask,ctx", [(1, 15, 20), (1, 15, 1100), (1, 0, 20), (2, 2, 20), (16, 15, 20)])
def test_gqa_layer_decode_equals_replicated_mha(bsz, mask, ctx):
    """Decode steps through the GQA layer and through the MHA layer on the replicated cache: the attention (fp16 matrix-core operands in
    the GQA op, FP32 in the MHA op) within 4e-3 of its scale -- at 1100 tokens KV-split and merged inside o_proj's launch --; the layer
    outputs finite and close: the W4A4 quantisers behind the attention turn its rounding differences into flipped codes, and this layer's
    random MLP amplifies them -- measured at batch 16: 0.7 % (rel. Frobenius) on the residual stream in front of the MLP, 11 % behind it."""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    dev, G = torch.device("cuda"), 2
    gl, ml = _pair(G)
    lens = [ctx + 7 * i for i in range(bsz)]
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn(sum(lens), 512, generator=gen) * 0.7).half().cuda()
    xd = [(torch.randn(bsz, 512, generator=gen) * 0.7).half().cuda() for _ in range(2)]
    res = []
    for layer, heads in ((gl, 4 // G), (ml, 4)):
        layer.fusion.q_mask = layer.fusion.q_mask2 = mask
        pool = KvPoolInt4(num_layers=2, num_heads=heads, head_dim=128, capacity=sum(-(-n // 16) + 1 for n in lens) + 1, block_len=16,
                          device=dev)
        cs = [KvCacheInt4(pool, n) for n in lens]
        layer(x, BatchLenInfo(lens, 0, dev), BatchedKvCacheInt4(cs), None)
        ys = []
        with _DecodeSpy() as spy:
            for xs in xd:
                for c in cs:
                    c.acquire_one()
                ys.append(layer(xs, BatchLenInfo([], bsz, dev), None, BatchedKvCacheInt4(cs)))
        res.append((ys, spy.got))
    (yg, ag), (ym, am) = res
    assert len(ag) == len(am) == 2
    for a, b in zip(ag, am):
        ok, info = _close(a, b)
        assert ok, info
    for a, b in zip(yg, ym):
        assert torch.isfinite(a).all()
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        assert rel <= 0.25, rel


def test_gqa_layer_rejects_cache_of_query_heads():
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    dev = torch.device("cuda")
    gl, _ = _pair(2)
    pool = KvPoolInt4(num_layers=2, num_heads=4, head_dim=128, capacity=8, block_len=16, device=dev)   # built with num_attention_heads
    cs = [KvCacheInt4(pool, 10)]
    with pytest.raises(ValueError):
        gl(torch.zeros((10, 512), dtype=torch.float16, device=dev), BatchLenInfo([10], 0, dev), BatchedKvCacheInt4(cs), None)
    cs[0].acquire_one()
    with pytest.raises(ValueError):
        gl(torch.zeros((1, 512), dtype=torch.float16, device=dev), BatchLenInfo([], 1, dev), None, BatchedKvCacheInt4(cs))


# ------------------------------------------------------------------------------------------------ export of the grouped-query flow
def test_gqa_flow_model_exports_into_the_e2e_model(golden_dir, tmp_path):
    """The rtn_w4a4_gqa flow model (4 query heads on 2 K/V heads) -> export.save_packed -> e2e.LlamaForCausalLM(num_key_value_heads=2):
    strict load, identical packed operands, prefill perplexity within |log ratio| <= 0.06 of the simulated path (as the MHA export test,
    tests/test_gpu_flow.py), then decode steps with finite logits."""
    from atom_amd import e2e
    from atom_amd.model import eval as E, export, modelutils_llama as F
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    from tests.flow_model import TinyLlamaForCausalLM, TokenStream, make_reorder_index, no_scales, paper_args
    z = np.load(os.path.join(golden_dir, "flow_tokens.npz"))
    tok = torch.from_numpy(z["rtn_w4a4_gqa.eval_96"].astype(np.int64))[None, :]
    args = paper_args()
    m = TinyLlamaForCausalLM(seqlen=96, kv_heads=2).eval()
    m = F.quantize_model_llama(F.add_act_quant_wrapper_llama(F.reorder_model_llama(m, "cuda:0", args, make_reorder_index(m)), "cuda:0", args,
                                                             no_scales()), "cuda:0", args)
    ppl_sim = E.llama_eval(m, TokenStream(tok), "cuda:0")
    path = str(tmp_path / "tiny_gqa.safetensors")
    export.save_packed(m, path)
    sd = export.load_packed(path)
    c = m.config
    cfg = types.SimpleNamespace(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_attention_heads=c.num_attention_heads,
                                num_key_value_heads=c.num_key_value_heads, num_hidden_layers=c.num_hidden_layers, vocab_size=c.vocab_size,
                                rms_norm_eps=c.rms_norm_eps, pad_token_id=None)
    assert cfg.num_key_value_heads == 2 and cfg.num_attention_heads == 4
    em = e2e.LlamaForCausalLM(cfg)
    missing, unexpected = em.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    em = em.cuda()
    for i, layer in enumerate(m.model.layers):
        for mod, proj in (("self_attn", "q_proj"), ("self_attn", "k_proj"), ("self_attn", "v_proj"), ("self_attn", "o_proj"),
                          ("mlp", "gate_proj"), ("mlp", "up_proj"), ("mlp", "down_proj")):
            b4, b8, sb, sb8 = getattr(getattr(layer, mod), proj).packed_weight()
            e4, e8, esb, esb8 = getattr(getattr(em.model.layers[i], mod), proj).packed()
            assert torch.equal(b4.view(torch.uint8), e4.view(torch.uint8)) and torch.equal(b8, e8) and torch.equal(sb, esb) and torch.equal(sb8, esb8)
    seqlen, ns = 96, tok.numel() // 96
    dev = torch.device("cuda:0")
    pool = KvPoolInt4(num_layers=c.num_hidden_layers, num_heads=2, head_dim=128, capacity=ns * 8, block_len=16, device=dev)
    cs = [KvCacheInt4(pool, seqlen) for _ in range(ns)]
    ids = tok[0, :ns * seqlen].cuda()
    logits, _ = em(ids, BatchLenInfo([seqlen] * ns, 0, dev), BatchedKvCacheInt4(cs), None)
    lg = logits.view(ns, seqlen, -1)[:, :-1].float()
    nll = torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), ids.view(ns, seqlen)[:, 1:].reshape(-1))
    ppl_e2e = float(torch.exp(nll))
    assert abs(np.log(ppl_e2e / ppl_sim)) <= 0.06, (ppl_e2e, ppl_sim)
    nxt = logits.view(ns, seqlen, -1)[:, -1].argmax(-1)
    for _ in range(3):
        for c_ in cs:
            c_.acquire_one()
        lg, _ = em(nxt, BatchLenInfo([], ns, dev), None, BatchedKvCacheInt4(cs))
        assert torch.isfinite(lg).all()
        nxt = lg.argmax(-1)
