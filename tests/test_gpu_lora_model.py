"""GPU tests of the LoRA model (e2e/llama_lora.py) on a tiny Llama -- hidden 256, 2 heads of 128 (one variant with 2 query heads on 1
K/V head), intermediate 512, 2 layers, vocabulary 64 -- with 3 adapters of rank 8.  Every comparison is EXACT: without adapters the
model is the base model's code, with adapters the layer is re-executed here from the public ops in the order its docstring gives
(the chain of references of tests/test_gpu_moe.py: the ops themselves are checked in tests/test_gpu_lora.py)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
VOCAB, HIDDEN, INTER, LAYERS, RANK, NADAPT = 64, 256, 512, 2, 8, 3
ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _cfg(kv_heads):
    c = types.SimpleNamespace(hidden_size=HIDDEN, num_attention_heads=2, intermediate_size=INTER, rms_norm_eps=1e-5, rope_theta=1e4,
                              num_hidden_layers=LAYERS, vocab_size=VOCAB, pad_token_id=None)
    if kv_heads is not None:
        c.num_key_value_heads = kv_heads
    return c


def _base(kv_heads, seed=0):
    from atom_amd.e2e import LlamaForCausalLM
    torch.manual_seed(seed)
    model = LlamaForCausalLM(_cfg(kv_heads)).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    return model


_MODELS = {}


def _models(kv_heads):
    """(base model, LoRA model with the same state dict), built once per K/V head count"""
    if kv_heads not in _MODELS:
        from atom_amd.e2e import LlamaForCausalLMWithLora
        base = _base(kv_heads)
        torch.manual_seed(99)
        lora = LlamaForCausalLMWithLora(_cfg(kv_heads)).cuda()
        lora.load_state_dict(base.state_dict())
        _MODELS[kv_heads] = (base, lora)
    return _MODELS[kv_heads]


def _manager(kv_heads, targets=ALL, zero_b=()):
    """3 adapters with normal A and B (adapters in ``zero_b``: B = 0), alpha = 2 r"""
    from atom_amd.utils.lora import LlamaLoraManager
    mgr = LlamaLoraManager(_cfg(kv_heads), NADAPT, RANK, target_modules=targets, device=DEV)
    g = torch.Generator().manual_seed(5)
    for a in range(NADAPT):
        w = mgr.alloc()
        assert w.idx == a
        for layer in range(LAYERS):
            for m in ALL:
                pool = mgr.mgr.get(m)
                shapes = {"down_proj": (INTER, HIDDEN), "gate_proj": (HIDDEN, INTER), "up_proj": (HIDDEN, INTER)}.get(m, (HIDDEN, None))
                A = torch.randn(RANK, shapes[0], generator=g) * 0.05            # (drawn for every module: the same adapters whatever the targets)
                nout = shapes[1] if shapes[1] else (HIDDEN if m in ("q_proj", "o_proj") else 128 * (2 if kv_heads is None else kv_heads))
                B = torch.randn(nout, RANK, generator=g) * 0.05
                if pool is not None:
                    mgr.load(w, layer, m, A, B * (0 if a in zero_b else 1), alpha=2 * RANK)
    return mgr


def _pool(kv_heads, capacity=16):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(LAYERS, 2 if kv_heads is None else kv_heads, 128, capacity, 16, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def _batch(kv_heads, prefills, decode_lens, seed=3):
    """(blen, prefill cache, decode cache, pool): fresh prefill sequences; decode sequences of ``decode_lens`` cached tokens (random cache
    bytes, the same for every call with the same arguments) that have just acquired the step's slot"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    pool = _pool(kv_heads)
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device="cuda", generator=g, dtype=torch.uint8))
    pool.param.copy_((torch.rand(pool.param.shape, device="cuda", generator=g) * 0.2 + 0.01).half())
    pre = [KvCacheInt4(pool, n) for n in prefills]
    dec = [KvCacheInt4(pool, n) for n in decode_lens]
    for c in dec:
        c.acquire_one()
    return (BatchLenInfo(prefills, len(decode_lens), DEV), BatchedKvCacheInt4(pre) if pre else None,
            BatchedKvCacheInt4(dec) if dec else None, pool)


def _ids(n, seed=1):
    return torch.randint(0, VOCAB, (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)


BATCHES = {"prefill": ((5, 17), ()), "decode": ((), (20, 3, 16)), "mixed": ((5, 17), (20, 16))}


@pytest.mark.parametrize("kv_heads", [None, 1])
def test_without_adapters_the_model_is_the_base_model(kv_heads):
    base, lora = _models(kv_heads)
    lora.set_adapters(None)
    for prefills, decode_lens in BATCHES.values():
        rows = sum(prefills) + len(decode_lens)
        blen, pkv, dkv, pool_a = _batch(kv_heads, list(prefills), list(decode_lens))
        want, _ = base(_ids(rows), blen, pkv, dkv)
        blen, pkv, dkv, pool_b = _batch(kv_heads, list(prefills), list(decode_lens))
        got, _ = lora(_ids(rows), blen, pkv, dkv)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(pool_a.buf, pool_b.buf)


def _by_hand(layer, mgr, ids, h, blen, pkv, dkv):
    """the op sequence of LlamaDecoderLayerWithLora's docstring from the public ops"""
    from atom_amd import ops
    from atom_amd.e2e.llama_lora import linear_fp16, rmsnorm_fp16
    at, mlp, il, pl = layer.self_attn, layer.mlp, layer.input_layernorm, layer.post_attention_layernorm
    li, P, doff, D = at.layer_idx, len(blen.prefills), blen.doff, blen.decode
    T, nh, nkv = h.size(0), at.num_heads, at.num_kv_heads

    def lora(y, x, m):
        if m not in mgr.mgr:
            return
        if P:
            ops.add_lora(y[:doff], x[:doff], mgr.mgr[m].wa_T, mgr.mgr[m].wb_T, ids[:P], li, 1.0, seg_indptr=blen.indptr)
        if D:
            ops.add_lora(y[doff:], x[doff:], mgr.mgr[m].wa_T, mgr.mgr[m].wb_T, ids[P:P + D], li, 1.0)

    x_q = ops.rmsnorm_fp16_i4(h, il.weight, il.reorder_index, il.variance_epsilon)
    xn = rmsnorm_fp16(h, il.weight, il.variance_epsilon)
    q, k, v = linear_fp16(at.q_proj, x_q), linear_fp16(at.k_proj, x_q), linear_fp16(at.v_proj, x_q)
    lora(q, xn, "q_proj"), lora(k, xn, "k_proj"), lora(v, xn, "v_proj")
    (k4, ks), (v4, vs) = ops.kv_quant_u4(k.view(T, nkv, 128)), ops.kv_quant_u4(v.view(T, nkv, 128))
    outs = []
    if P:
        ops.init_kv_i4(pkv, k4[:doff], v4[:doff], ks[:doff], vs[:doff], blen.indptr, li)
        outs.append(ops.batch_prefill_i4(q[:doff].view(-1, nh, 128), blen.indptr, pkv, li, rope_theta=at.rope_theta,
                                         max_q_len=max(blen.prefills)).view(doff, HIDDEN))
    if D:
        ops.append_kv_i4(dkv, k4[doff:], v4[doff:], ks[doff:], vs[doff:], li)
        outs.append(ops.batch_decode_i4(q[doff:].view(D, nh, 128), dkv, li, rope_theta=at.rope_theta).view(D, HIDDEN))
    attn = torch.cat(outs, dim=0).contiguous()
    o = linear_fp16(at.o_proj, ops.reorder_fp16_i4(attn, at.reorder_index))
    lora(o, attn, "o_proj")
    out = ops.add_rmsnorm_fp16_i4(o, h, pl.weight, pl.reorder_index, pl.variance_epsilon)
    res, n_q = out[0], out[1:]
    n = rmsnorm_fp16(res, pl.weight, pl.variance_epsilon)
    gate, up = linear_fp16(mlp.gate_proj, n_q), linear_fp16(mlp.up_proj, n_q)
    lora(gate, n, "gate_proj"), lora(up, n, "up_proj")
    d = linear_fp16(mlp.down_proj, ops.activate_fp16_i4(gate, up))
    lora(d, torch.nn.functional.silu(gate) * up, "down_proj")
    return res + d


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("kv_heads", [None, 1])
def test_layer_with_adapters_is_the_documented_op_sequence(kv_heads, batch):
    _, lora = _models(kv_heads)
    mgr = _manager(kv_heads)
    prefills, decode_lens = BATCHES[batch]
    nseq = len(prefills) + len(decode_lens)
    ids = [2, -1, 0, 1][:nseq]
    lora.set_adapters(ids, mgr)
    try:
        rows = sum(prefills) + len(decode_lens)
        h = (torch.randn((rows, HIDDEN), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))).half()
        for li in (0, 1):
            layer = lora.model.layers[li]
            blen, pkv, dkv, pool_a = _batch(kv_heads, list(prefills), list(decode_lens))
            got = layer(h, blen, pkv, dkv)
            blen, pkv, dkv, pool_b = _batch(kv_heads, list(prefills), list(decode_lens))
            want = _by_hand(layer, mgr, torch.tensor(ids, dtype=torch.int32, device="cuda"), h, blen, pkv, dkv)
            assert got.shape == (rows, HIDDEN) and torch.equal(got.view(torch.int16), want.view(torch.int16))
            assert torch.equal(pool_a.buf, pool_b.buf) and torch.equal(pool_a.param.view(torch.int16), pool_b.param.view(torch.int16))
            lora.set_adapters(None)
            blen, pkv, dkv, _ = _batch(kv_heads, list(prefills), list(decode_lens))
            assert not torch.equal(layer(h, blen, pkv, dkv), got)                    # the adapters do change the layer
            lora.set_adapters(ids, mgr)
    finally:
        lora.set_adapters(None)


def _logits(lora, kv_heads, mgr, ids, prefills=(5, 17, 8)):
    lora.set_adapters(ids, mgr)
    try:
        blen, pkv, dkv, _ = _batch(kv_heads, list(prefills), [])
        return lora(_ids(sum(prefills)), blen, pkv, dkv)[0]
    finally:
        lora.set_adapters(None)


@pytest.mark.parametrize("kv_heads", [None, 1])
def test_a_sequence_sees_only_its_own_adapter(kv_heads):
    _, lora = _models(kv_heads)
    mgr = _manager(kv_heads)
    a, b, c = (_logits(lora, kv_heads, mgr, ids) for ids in ((0, -1, 2), (0, 2, 1), (1, -1, 2)))
    assert torch.equal(a[:5].view(torch.int16), b[:5].view(torch.int16))
    assert not torch.equal(a[:5], c[:5])
    assert not torch.equal(a[5:22], b[5:22]) and torch.equal(a[5:].view(torch.int16), c[5:].view(torch.int16))


def test_an_adapter_with_zero_b_is_no_adapter():
    _, lora = _models(None)
    mgr = _manager(None, zero_b=(2,))
    a, b = _logits(lora, None, mgr, (2, 0, 2)), _logits(lora, None, mgr, (-1, 0, -1))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.equal(a[5:22], _logits(lora, None, mgr, (-1, -1, -1))[5:22])


def test_untargeted_projections_launch_no_lora_kernel(monkeypatch):
    from atom_amd import ops
    _, lora = _models(None)
    calls = []
    real = ops.add_lora

    def counted(y, x, wa, wb, *args, **kwargs):
        calls.append((wa.size(3), wb.size(2)))
        return real(y, x, wa, wb, *args, **kwargs)

    monkeypatch.setattr(ops, "add_lora", counted)
    _logits(lora, None, _manager(None, targets=("q_proj", "v_proj")), (0, -1, 2))
    assert calls == [(HIDDEN, HIDDEN), (HIDDEN, HIDDEN)] * LAYERS                     # q_proj and v_proj, once per layer (prefill rows only)
    del calls[:]
    _logits(lora, None, _manager(None), (0, -1, 2))
    assert len(calls) == 7 * LAYERS and calls.count((INTER, HIDDEN)) == LAYERS and calls.count((HIDDEN, INTER)) == 2 * LAYERS
    del calls[:]
    q_v = _logits(lora, None, _manager(None, targets=("q_proj", "v_proj")), (-1, -1, -1))
    lora.set_adapters(None)
    blen, pkv, dkv, _ = _batch(None, [5, 17, 8], [])
    assert len(calls) == 2 * LAYERS and q_v.shape == lora(_ids(30), blen, pkv, dkv)[0].shape and len(calls) == 2 * LAYERS


PROMPT_LENS, NEW = [7, 19], 24


def _eager(model, prompts, pool, steps, cap):
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    logits, _ = model(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    first_logits = logits[torch.tensor(lens).cumsum(0) - 1]
    ids = first_logits.argmax(-1)
    toks, logs = [ids], [first_logits]
    for _ in range(steps):
        for c in seqs:
            c.acquire_one()
        kv = BatchedKvCacheInt4(seqs)
        kv.max_pages = cap
        logits, _ = model(ids, BatchLenInfo([], len(seqs), DEV), None, kv)
        ids = logits.argmax(-1)
        toks.append(ids)
        logs.append(logits)
    return seqs, torch.stack(toks), torch.stack(logs)


@pytest.mark.parametrize("kv_heads", [None, 1])
def test_generate_with_adapters_equals_the_eager_loop(kv_heads):
    """adapters (1, -1): prefill eagerly, then DecodeGraph replay against the loop a user writes, token for token and logit for logit;
    ``max_pages`` of the eager caches is the static cache's, as in tests/test_gpu_generate.py (it sizes the KV split)"""
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    _, lora = _models(kv_heads)
    mgr = _manager(kv_heads)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS]
    cap = max(-(-(len(p) + NEW - 1) // 16) for p in prompts)
    lora.set_adapters((1, -1), mgr)
    try:
        _, toks, logs = _eager(lora, prompts, _pool(kv_heads), NEW - 1, cap)
        pg = _pool(kv_heads)
        caches = [KvCacheInt4(pg, 0) for _ in prompts]
        got_tokens, got_logits = generate(lora, prompts, NEW, pg, caches=caches, return_logits=True)
        assert got_tokens == toks.t().tolist()
        assert torch.equal(got_logits.view(torch.int16), logs.view(torch.int16))
        lora.set_adapters((-1, -1), mgr)
        _, toks0, logs0 = _eager(lora, prompts, _pool(kv_heads), 1, cap)
        assert not torch.equal(logs0[0, 0], logs[0, 0]) and torch.equal(logs0[0, 1], logs[0, 1])     # adapter 1 moved sequence 0 only
    finally:
        lora.set_adapters(None)


def test_replayed_steps_with_adapters_do_not_synchronise_and_follow_set_adapters():
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, StaticBatchedKvCacheInt4
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device="cuda").item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _, lora = _models(1)
    mgr = _manager(1)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS]
    steps, lens = 8, list(PROMPT_LENS)
    lora.set_adapters((1, -1), mgr)
    try:
        def prefill(pool):
            seqs = [KvCacheInt4(pool, n) for n in lens]
            ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
            logits, _ = lora(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
            return seqs, logits[torch.tensor(lens).cumsum(0) - 1].argmax(-1)

        seqs, first = prefill(_pool(1))
        skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
        dg = DecodeGraph(lora, skv, steps, keep_logits=True)
        dg.input_ids.copy_(first)
        dg.step()
        dg.step()                                            # eager warm-up and the capture are allowed to synchronise
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                dg.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lora.set_adapters((1, 2), mgr)                       # in place: the captured step reads the new ids
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            while dg.steps_done < steps:
                dg.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        # the eager loop with the same switch after 5 decode steps
        lora.set_adapters((1, -1), mgr)
        se, first_e = prefill(_pool(1))
        assert torch.equal(first, first_e)
        ids, toks, logs = first_e, [], []
        for i in range(steps):
            if i == 5:
                lora.set_adapters((1, 2), mgr)
            for c in se:
                c.acquire_one()
            kv = BatchedKvCacheInt4(se)
            kv.max_pages = skv.max_pages
            logits, _ = lora(ids, BatchLenInfo([], 2, DEV), None, kv)
            ids = logits.argmax(-1)
            toks.append(ids)
            logs.append(logits)
        assert torch.equal(dg.tokens, torch.stack(toks)) and torch.equal(dg.logits.view(torch.int16), torch.stack(logs).view(torch.int16))
        skv.close()
    finally:
        lora.set_adapters(None)
