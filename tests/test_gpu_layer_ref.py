"""The real-kernel LlamaDecoderLayer / LlamaModel / LlamaForCausalLM (atom_amd/e2e/llama.py) against the staged reference of
tests/layer_ref.py, which shares no wiring with them: every launch of one forward is captured at ``atom_amd.ops`` (inputs and outputs
cloned), turned into the reference's trace format and checked teacher-forced, stage by stage, with the bounds stated there.  The
inputs are those of tests/layer_cases.py, on which tests/test_layer_ref_cpu.py shows that the checker reports every wiring error.
The layers run with one launch per stage, in the reference's call order (a ``DecodeFusion`` of their own, the process-wide one is
untouched); the fused decode routes are tied to that form bit for bit by tests/test_gpu_e2e.py."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import layer_cases as C
from tests import layer_ref as R
from tests.helpers import _check_tail, bits16, t2n

pytestmark = pytest.mark.gpu

SPIED = ("rmsnorm_fp16_i4", "add_rmsnorm_fp16_i4", "reorder_fp16_i4", "activate_fp16_i4", "repack_act_f6", "dense_layer_gemm_i4_fp16",
         "dense_layer_gemm_i4_o4", "dense_layer_gemm_i4_f32", "dense_layer_gemm_i4_multi", "dense_layer_gemm_i4_multi_q",
         "dense_layer_gemm_i4_merge_q", "gate_up_silu_quant_f6", "init_kv_i4", "append_kv_i4", "quant_append_kv_i4", "batch_decode_i4",
         "batch_prefill_i4")
# which quantiser stage each projection must read
READS = dict(q="norm1", k="norm1", v="norm1", o="attn_q", gate="norm2", up="norm2", down="act")


def _unfused():
    from atom_amd.e2e.llama import DecodeFusion
    return DecodeFusion(decode=False, kv_append=False, kv_in_decode=False, merge_in_o_proj=False, q_decode=False)


class _Spy:
    """every call of the listed ops, outermost only: (name, cloned positional arguments, their addresses, cloned outputs)"""

    def __init__(self):
        self.calls, self._depth, self._orig = [], 0, {}

    def _wrap(self, name, orig):
        def spy(*args, **kw):
            if self._depth:
                return orig(*args, **kw)
            self._depth += 1
            try:
                before = [a.clone() if torch.is_tensor(a) else a for a in args]
                out = orig(*args, **kw)
            finally:
                self._depth -= 1
            outs = tuple(o.clone() if torch.is_tensor(o) else o for o in (out if isinstance(out, (tuple, list)) else (out,)))
            self.calls.append((name, before, [a.data_ptr() if torch.is_tensor(a) else None for a in args], outs))
            return out
        return spy

    def __enter__(self):
        from atom_amd import ops
        for name in SPIED:
            self._orig[name] = getattr(ops, name)
            setattr(ops, name, self._wrap(name, self._orig[name]))
        return self

    def __exit__(self, *exc):
        from atom_amd import ops
        for name, orig in self._orig.items():
            setattr(ops, name, orig)


def _quant(outs, rows):
    """(outlier, norms, outlier_scales, norm_scales) of a quantiser op -> the oracle's dict"""
    o8, o4, s8, s4 = outs[:4]
    return dict(q4=O.unpack_int4(t2n(o4).view(np.uint8)), q8=t2n(o8), s4=np.ascontiguousarray(O.scales_from_ref_layout(t2n(s4), rows).T),
                s8=O.scales_from_ref_layout(t2n(s8), rows))


def _same(a, b):
    """the same bytes (the replicated scale layout has slots that no kernel writes: compared as integers, whatever they hold)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _projections(layer):
    at, mlp = layer.self_attn, layer.mlp
    return dict(q=at.q_proj, k=at.k_proj, v=at.v_proj, o=at.o_proj, gate=mlp.gate_proj, up=mlp.up_proj, down=mlp.down_proj)


def _load(layer, fp16, lay):
    """the case's fp16 parameters into the layer; its packed weights are then the oracle's, bit for bit"""
    dev = torch.device("cuda")
    for name, mod in _projections(layer).items():
        mod.load_fp16_weight(torch.from_numpy(fp16[name]).to(dev))
        b4, b8, sb, sb8 = mod.packed()
        w = lay["w"][name]
        assert np.array_equal(O.unpack_int4(t2n(b4).view(np.uint8)), w["q4"]) and np.array_equal(t2n(b8), w["q8"]), name
        assert np.array_equal(bits16(t2n(sb)), bits16(w["s4"])) and np.array_equal(bits16(t2n(sb8)), bits16(w["s8"])), name
    for norm, key in ((layer.input_layernorm, "norm1"), (layer.post_attention_layernorm, "norm2")):
        norm.weight.data = torch.from_numpy(fp16[key + "_w"]).to(dev)
        norm.reorder_index.data = torch.from_numpy(fp16[key + "_idx"]).to(dev)
    layer.self_attn.reorder_index.data = torch.from_numpy(fp16["attn_idx"]).to(dev)


def _config(kv_heads, theta):
    return types.SimpleNamespace(hidden_size=C.HIDDEN, num_attention_heads=C.HEADS, num_key_value_heads=kv_heads, intermediate_size=C.INTER,
                                 rms_norm_eps=C.EPS, rope_theta=theta, num_hidden_layers=C.LAYERS, vocab_size=C.VOCAB, pad_token_id=None)


@functools.lru_cache(maxsize=None)
def _layer(kv_heads, theta):
    from atom_amd.e2e import LlamaDecoderLayer
    layer = LlamaDecoderLayer(_config(kv_heads, theta), layer_idx=1, fusion=_unfused()).cuda()
    fp16, lay = C.layer_params(kv_heads, 1)
    _load(layer, fp16, lay)
    return layer


def _device_pool(pool, kv_heads):
    from atom_amd.utils import KvPoolInt4
    dev = torch.device("cuda")
    p = KvPoolInt4(num_layers=C.LAYERS, num_heads=kv_heads, head_dim=128, capacity=C.CAPACITY, block_len=C.PAGE, device=dev)
    p.buf.copy_(torch.from_numpy(pool[0]).to(dev))
    p.param.copy_(torch.from_numpy(pool[1]).to(dev))
    return p


def _grow(pool, seq, pages, seqlen):
    """``acquire_one`` up to ``seqlen`` tokens, the pool handing out the described pages in their order"""
    while seq.seqlen < seqlen:
        n = len(seq.indicies)
        pool._free = {pages[n]} if n < len(pages) else set()
        seq.acquire_one()
    pool._free = set()
    assert list(seq.indicies) == list(pages[:len(seq.indicies)]) and seq.seqlen == seqlen


def _sequences(pool, req, known=None):
    """KvCacheInt4 objects of a call's requests (prefill, decode); ``known``: page list -> the sequence an earlier call left"""
    from atom_amd.utils import KvCacheInt4
    known = known or {}
    pre, dec = [], []
    for prefix, n, pages in req.prefills:
        seq = known.get(tuple(pages[:-(-prefix // req.page)])) if prefix else None
        assert (seq is None) == (prefix == 0)
        seq = seq or KvCacheInt4(pool, 0)
        _grow(pool, seq, pages, prefix + n)
        pre.append(seq)
    for length, pages in req.decodes:
        seq = KvCacheInt4(pool, 0)
        _grow(pool, seq, pages, length)
        dec.append(seq)
    return pre, dec


def _call(module, pool, req, x, seqs):
    """one forward of a layer or a model on the described batch, every launch captured"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    dev = torch.device("cuda")
    pre, dec = seqs
    blen = BatchLenInfo([n for _, n, _ in req.prefills], len(req.decodes), dev)
    with _Spy() as spy:
        out = module(x, blen, BatchedKvCacheInt4(pre) if pre else None, BatchedKvCacheInt4(dec) if dec else None)
        torch.cuda.synchronize()
    return out, spy.calls


def _expected_ops(req, hip_prefill):
    kv = []
    if req.prefills:
        kv.append("init_kv_i4")
        if hip_prefill or max(a for a, _, _ in req.prefills) > 0:
            kv.append("batch_prefill_i4")
    if req.decodes:
        kv += ["append_kv_i4", "batch_decode_i4"]
    return (["rmsnorm_fp16_i4", "q", "k", "v"] + kv + ["reorder_fp16_i4", "o", "add_rmsnorm_fp16_i4", "gate", "up", "activate_fp16_i4", "down"])


def _trace(calls, layer, req, x, out, pool_after, hip_prefill, lay):
    """The captured launches of ONE layer forward as a tests/layer_ref.py trace.  Asserts on the way: each stage exactly once and in the
    reference's call order, no fused launch in its place, and every projection fed with the very tensors its quantiser stage returned."""
    rows = req.rows
    by_weight = {mod.weight_int8.data_ptr(): name for name, mod in _projections(layer).items()}
    tr, seen, produced, recoded = {"x": t2n(x)}, [], {}, None
    for name, args, ptrs, outs in calls:
        if name == "repack_act_f6":                         # LinearInt4 re-codes its activation first: the GEMM's input is the re-coder's
            recoded = args
            continue
        if name in ("dense_layer_gemm_i4_fp16", "dense_layer_gemm_i4_o4"):
            proj = by_weight[ptrs[5]]
            assert (name == "dense_layer_gemm_i4_o4") == (proj in "kv"), (proj, name)
            a, a_scale, a_keeper, a_keeper_scale = args[0], args[2], args[4], args[6]
            if recoded is not None:
                assert a.dim() == 3 and _same(recoded[1], a_scale), proj
                a, recoded = recoded[0], None
            o8, o4, s8, s4 = produced[READS[proj]][:4]
            assert (_same(a, o4) and _same(a_keeper, o8) and _same(a_scale, s4)
                    and _same(a_keeper_scale, s8)), f"{proj}_proj was not given the output of {READS[proj]}"
            if proj in "kv":
                tr[proj] = dict(codes=t2n(outs[0]), sz=t2n(outs[1]).reshape(rows, req.kv_heads, 2))
            elif proj != "down":
                tr[proj] = t2n(outs[0])
            seen.append(proj)
            continue
        assert recoded is None, name
        seen.append(name)
        if name == "rmsnorm_fp16_i4":
            produced["norm1"], tr["norm1"] = outs, _quant(outs, rows)
            _check_tail(outs, O.rmsnorm_reorder_quant(tr["x"], lay["norm1_w"], lay["eps"], lay["norm1_idx"], "kernel", 1.0), rows, "ref", exact=True)
        elif name == "reorder_fp16_i4":
            produced["attn_q"], tr["attn"], tr["attn_q"] = outs, t2n(args[0]), _quant(outs, rows)
        elif name == "add_rmsnorm_fp16_i4":
            produced["norm2"], tr["residual1"], tr["norm2"] = outs[1:], t2n(outs[0]), _quant(outs[1:], rows)
        elif name == "activate_fp16_i4":
            produced["act"], tr["act"] = outs, _quant(outs, rows)
            _check_tail(outs, O.silu_mul_quant(t2n(args[0]), t2n(args[1]), "kernel", 1.0), rows, "ref", exact=False)
    assert seen == _expected_ops(req, hip_prefill), seen
    tr["out"] = t2n(out)
    tr["cache"] = dict(buf=pool_after[0], param=pool_after[1])
    return tr


def _snapshot(pool):
    torch.cuda.synchronize()
    return t2n(pool.buf).copy(), t2n(pool.param).copy()


def _assert_clean(fails, report, what):
    print(f"\n--- {what}")
    print("\n".join(report))
    assert fails == [], (what, fails)


def _layer_route(route, kv_heads, hip_prefill=False):
    case = C.layer_case(route, kv_heads)
    layer = _layer(kv_heads, case["lay"]["rope_theta"])
    pool = _device_pool(case["pool"], kv_heads)
    dev = torch.device("cuda")
    layer.fusion.prefill_attn = hip_prefill
    try:
        known = {}
        if case["first"] is not None:                       # the call that leaves the prefixes in the cache
            seqs = _sequences(pool, case["first"])
            _call(layer, pool, case["first"], torch.from_numpy(case["x_first"]).to(dev), seqs)
            known = {tuple(pages): seq for (_, _, pages), seq in zip(case["first"].prefills, seqs[0])}
        before = _snapshot(pool)
        x = torch.from_numpy(case["x"]).to(dev)
        out, calls = _call(layer, pool, case["req"], x, _sequences(pool, case["req"], known))
    finally:
        layer.fusion.prefill_attn = False
    tr = _trace(calls, layer, case["req"], x, out, _snapshot(pool), hip_prefill, case["lay"])
    report = []
    fails = R.check(tr, dict(req=case["req"], lay=case["lay"], pool=before, x=case["x"]), report)
    _assert_clean(fails, report, f"route {route}, {kv_heads} K/V heads, prefill op {hip_prefill}")


@pytest.mark.parametrize("hip_prefill", [False, True])
@pytest.mark.parametrize("kv_heads", C.KV_HEADS)
def test_prefill_from_empty_caches(kv_heads, hip_prefill):
    """route A, through the torch route and through the HIP prefill op"""
    _layer_route("A", kv_heads, hip_prefill)


@pytest.mark.parametrize("route,kv_heads", [c for c in C.LAYER_CASES if c[0] != "A"])
def test_layer_route(route, kv_heads):
    """B chunked prefill on cached prefixes, C decode only, D prefill and decode requests in one batch, E the same with cached prefixes
    and rope_theta 5e5; all at layer_idx 1 over a pool of random bytes"""
    _layer_route(route, kv_heads)


@functools.lru_cache(maxsize=None)
def _model(kv_heads):
    from atom_amd.e2e import LlamaForCausalLM
    dev = torch.device("cuda")
    model = LlamaForCausalLM(_config(kv_heads, 1e4)).cuda()
    fusion = _unfused()
    for mod in model.modules():                             # one launch per stage, without touching the process-wide DecodeFusion
        if hasattr(mod, "fusion"):
            mod.fusion = fusion
    fp16, mdl = C.model_params(kv_heads)
    model.model.embed_tokens.weight.data = torch.from_numpy(fp16["embed"]).to(dev)
    model.lm_head.weight.data = torch.from_numpy(fp16["head"]).to(dev)
    model.model.norm.weight.data = torch.from_numpy(fp16["norm_w"]).to(dev)
    for layer, f, lay in zip(model.model.layers, fp16["layers"], mdl["layers"]):
        _load(layer, f, lay)
    return model


@pytest.mark.parametrize("route,kv_heads", C.MODEL_CASES)
def test_model(route, kv_heads):
    """LlamaForCausalLM, 2 layers, vocabulary 1000: the embedding gather, every layer teacher-forced on its observed input and on the
    pool the layer before left (each layer on ITS slice of the pool), the final norm and the logits"""
    case = C.model_case(route, kv_heads)
    model, req = _model(kv_heads), case["req"]
    pool = _device_pool(case["pool"], kv_heads)
    marks, hooks, calls_now = [], [], []
    embed = []
    hooks.append(model.model.embed_tokens.register_forward_hook(lambda m, a, o: embed.append(o.clone())))
    for layer in model.model.layers:
        hooks.append(layer.register_forward_pre_hook(lambda m, a: marks.append(dict(start=len(calls_now[0]), x=a[0].clone(), pool=_snapshot(pool)))))
        hooks.append(layer.register_forward_hook(lambda m, a, o: marks[-1].update(stop=len(calls_now[0]), out=o.clone())))
    try:
        from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
        dev = torch.device("cuda")
        pre, dec = _sequences(pool, req)
        blen = BatchLenInfo([n for _, n, _ in req.prefills], len(req.decodes), dev)
        with _Spy() as spy:
            calls_now.append(spy.calls)
            logits, hidden = model(torch.from_numpy(case["ids"]).to(dev), blen, BatchedKvCacheInt4(pre) if pre else None,
                                   BatchedKvCacheInt4(dec) if dec else None)
            torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    after = [m["pool"] for m in marks[1:]] + [_snapshot(pool)]
    assert len(marks) == C.LAYERS and len(embed) == 1 and marks[-1]["stop"] == len(spy.calls) and marks[0]["start"] == 0
    tr = dict(embed=t2n(embed[0]), final_norm=t2n(hidden), logits=t2n(logits), layers=[])
    for m, layer, lay, pool_after in zip(marks, model.model.layers, case["mdl"]["layers"], after):
        tr["layers"].append(_trace(spy.calls[m["start"]:m["stop"]], layer, req, m["x"], m["out"], pool_after, False, lay))
    report = []
    fails = R.check_model(tr, dict(req=req, mdl=case["mdl"], pool=case["pool"], ids=case["ids"]), report)
    _assert_clean(fails, report, f"model, route {route}, {kv_heads} K/V heads")
