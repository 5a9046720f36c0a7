"""The real-kernel MixtralDecoderLayer / MixtralForCausalLM (atom_amd/e2e/mixtral.py) and LlamaDecoderLayerWithLora /
LlamaForCausalLMWithLora with adapters set (atom_amd/e2e/llama_lora.py) against the staged references of tests/variant_ref.py, which
share no wiring with them -- the method of tests/test_gpu_layer_ref.py: every launch of one forward is captured at ``atom_amd.ops``,
turned into the reference's trace format and checked teacher-forced, stage by stage, with the bounds stated there.  The inputs are
those of tests/variant_cases.py, on which tests/test_variant_ref_cpu.py shows that the checkers report every wiring error.  What no
launch shows -- the router's input, the adapters' un-quantised norms -- comes from a forward pre-hook on the MoE block and from the
LoRA module's ``rmsnorm_fp16``; what the adapters READ is judged by the numbers alone."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import layer_cases as C
from tests import layer_ref as R
from tests import test_gpu_layer_ref as L
from tests import variant_cases as V
from tests import variant_ref as X
from tests.helpers import bits16, t2n

pytestmark = pytest.mark.gpu

SPIED = L.SPIED + ("moe_route_topk", "moe_gemm_i4", "moe_combine", "add_lora", "kv_quant_u4")
GEMMS = ("dense_layer_gemm_i4_fp16", "dense_layer_gemm_i4_o4")
IN_PLACE = ("add_lora",)                                     # ops that write into their first argument


class _Spy(L._Spy):
    """tests/test_gpu_layer_ref.py's, on more ops; a call is (name, cloned arguments, their addresses, cloned outputs, the outputs'
    addresses), and for an op that writes in place the "output" is its first argument cloned AFTER the call"""

    def _wrap(self, name, orig):
        inner = super()._wrap(name, orig)

        def spy(*args, **kw):
            n = len(self.calls)
            out = inner(*args, **kw)
            if len(self.calls) > n:                            # an outermost call: the one just recorded
                c = self.calls[-1]
                live = (args[0],) if name in IN_PLACE else out if isinstance(out, (tuple, list)) else (out,)
                outs = (args[0].clone(),) if name in IN_PLACE else c[3]
                self.calls[-1] = c[:3] + (outs, [o.data_ptr() if torch.is_tensor(o) else None for o in live])
            return out
        return spy

    def __enter__(self):
        from atom_amd import ops
        for name in SPIED:
            self._orig[name] = getattr(ops, name)
            setattr(ops, name, self._wrap(name, self._orig[name]))
        return self


def _config(kv_heads, theta, **more):
    return types.SimpleNamespace(hidden_size=C.HIDDEN, num_attention_heads=C.HEADS, num_key_value_heads=kv_heads, intermediate_size=C.INTER,
                                 rms_norm_eps=C.EPS, rope_theta=theta, num_hidden_layers=C.LAYERS, vocab_size=C.VOCAB, pad_token_id=None, **more)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _load_linear(mod, w16, packed, what):
    """the fp16 weight through LinearInt4.load_fp16_weight; the packed parameters are then the oracle's, bit for bit"""
    mod.load_fp16_weight(_dev(w16))
    b4, b8, sb, sb8 = mod.packed()
    assert np.array_equal(O.unpack_int4(t2n(b4).view(np.uint8)), packed["q4"]) and np.array_equal(t2n(b8), packed["q8"]), what
    assert np.array_equal(bits16(t2n(sb)), bits16(packed["s4"])) and np.array_equal(bits16(t2n(sb8)), bits16(packed["s8"])), what


def _load_norms(layer, fp16):
    for norm, key in ((layer.input_layernorm, "norm1"), (layer.post_attention_layernorm, "norm2")):
        norm.weight.data = _dev(fp16[key + "_w"])
        norm.reorder_index.data = _dev(fp16[key + "_idx"])
    layer.self_attn.reorder_index.data = _dev(fp16["attn_idx"])


def _forward(module, pool, req, x):
    """one forward of a layer on the described batch, every launch captured"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    pre, dec = L._sequences(pool, req)
    blen = BatchLenInfo([n for _, n, _ in req.prefills], len(req.decodes), torch.device("cuda"))
    with _Spy() as spy:
        out = module(x, blen, BatchedKvCacheInt4(pre) if pre else None, BatchedKvCacheInt4(dec) if dec else None)
        torch.cuda.synchronize()
    return out, spy.calls


def _model_forward(model, layers, case, pool, mark_more=None, calls_now=None):
    """One forward of a model with every launch captured and a mark per layer (its window of launches, its input and output, the pool
    before it).  Returns (the model-level trace without its layers, the marks, the pools after each layer, the calls).  ``calls_now``:
    a list that receives the growing list of calls as its only element."""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    req, dev = case["req"], torch.device("cuda")
    calls_now = [] if calls_now is None else calls_now
    marks, hooks, embed = [], [], []
    hooks.append(model.model.embed_tokens.register_forward_hook(lambda m, a, o: embed.append(o.clone())))
    for layer in layers:
        hooks.append(layer.register_forward_pre_hook(lambda m, a: marks.append(dict(start=len(calls_now[0]), x=a[0].clone(), pool=L._snapshot(pool)))))
        hooks.append(layer.register_forward_hook(lambda m, a, o: marks[-1].update(stop=len(calls_now[0]), out=o.clone())))
        if mark_more is not None:
            hooks.append(mark_more(layer, marks))
    try:
        pre, dec = L._sequences(pool, req)
        blen = BatchLenInfo([n for _, n, _ in req.prefills], len(req.decodes), dev)
        with _Spy() as spy:
            calls_now.append(spy.calls)
            logits, hidden = model(_dev(case["ids"]), blen, BatchedKvCacheInt4(pre) if pre else None, BatchedKvCacheInt4(dec) if dec else None)
            torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    after = [m["pool"] for m in marks[1:]] + [L._snapshot(pool)]
    assert len(marks) == C.LAYERS and len(embed) == 1 and marks[-1]["stop"] == len(spy.calls) and marks[0]["start"] == 0
    return dict(embed=t2n(embed[0]), final_norm=t2n(hidden), logits=t2n(logits), layers=[]), marks, after, spy.calls


def _gemm_call(call, by_weight, produced, reads, recoded):
    """a projection's launch: (its name, True) after asserting that it was fed with the very tensors its quantiser stage returned"""
    name, args, ptrs, outs, _ = call
    proj = by_weight[ptrs[5]]
    a, a_scale, a_keeper, a_keeper_scale = args[0], args[2], args[4], args[6]
    if recoded is not None:                                     # LinearInt4 re-coded its activation first: the GEMM's input is the re-coder's
        assert a.dim() == 3 and L._same(recoded[1], a_scale), proj
        a = recoded[0]
    o8, o4, s8, s4 = produced[reads[proj]][:4]
    assert (L._same(a, o4) and L._same(a_keeper, o8) and L._same(a_scale, s4)
            and L._same(a_keeper_scale, s8)), f"{proj}_proj was not given the output of {reads[proj]}"
    return proj


# ==================================================================================================== Mixtral
def _moe_in_hook(layer, marks):
    return layer.block_sparse_moe.register_forward_pre_hook(
        lambda m, a: marks[-1].update(moe_in=([t.clone() for t in a[0]], a[1].clone(), a[2].clone()),
                                      moe_ptrs=([t.data_ptr() for t in a[0]], a[1].data_ptr(), a[2].data_ptr())))


def _load_mixtral(layer, fp16, lay):
    at, moe = layer.self_attn, layer.block_sparse_moe
    for name, mod in dict(q=at.q_proj, k=at.k_proj, v=at.v_proj, o=at.o_proj).items():
        _load_linear(mod, fp16[name], lay["w"][name], name)
    _load_norms(layer, fp16)
    moe.gate.weight.data = _dev(fp16["gate_w"])
    for e, (w1, w3, w2) in enumerate(fp16["experts"]):
        moe.load_expert_fp16(e, _dev(w1), _dev(w3), _dev(w2))
    torch.cuda.synchronize()
    for e in range(V.EXPERTS):                                  # load_expert_fp16 against the independent packer: w1 rows then w3 rows, the slot
        for name, want in (("w13", lay["moe"]["w13"][e]), ("w2", lay["moe"]["w2"][e])):
            b4, b8, sb, sb8 = (t2n(getattr(moe, name + suffix)[e]) for suffix in ("_int4", "_int8", "_scale_int4", "_scale_int8"))
            assert np.array_equal(O.unpack_int4(b4.view(np.uint8)), want["q4"]), (e, name, "int4 codes")
            assert np.array_equal(b8, want["q8"]), (e, name, "int8 codes")
            assert np.array_equal(bits16(sb), bits16(want["s4"])), (e, name, "int4 scales")
            assert np.array_equal(bits16(sb8), bits16(want["s8"])), (e, name, "int8 scales")


def _mixtral_config():
    return _config(V.MIXTRAL_KV, V.MIXTRAL_THETA, num_local_experts=V.EXPERTS, num_experts_per_tok=V.TOP_K, sliding_window=None)


@functools.lru_cache(maxsize=None)
def _mixtral_layer():
    from atom_amd.e2e.mixtral import MixtralDecoderLayer
    layer = MixtralDecoderLayer(_mixtral_config(), layer_idx=1, fusion=L._unfused()).cuda()
    _load_mixtral(layer, *V.mixtral_params(1))
    return layer


def _route_tables(route):
    n = int(route.n_tiles.item())
    return dict(ids=t2n(route.topk_ids), w=t2n(route.topk_w), expert_indptr=t2n(route.expert_indptr), row_token=t2n(route.row_token),
                slot_row=t2n(route.slot_row), tile_expert=t2n(route.tile_expert)[:n], tile_row0=t2n(route.tile_row0)[:n], n_tiles=n)


def _mixtral_trace(calls, layer, req, x, out, pool_after, moe_in, moe_ptrs):
    """The captured launches of ONE Mixtral layer forward as a tests/variant_ref.py trace.  Asserts on the way: each stage exactly once
    and in order, every GEMM fed with the very tensors the stage before it returned, the MoE block given add_rmsnorm_fp16_i4's own
    outputs as ``x_q`` and ``residual``."""
    rows, R_ = req.rows, req.rows * V.TOP_K
    at, moe = layer.self_attn, layer.block_sparse_moe
    by_weight = {mod.weight_int8.data_ptr(): name for name, mod in dict(q=at.q_proj, k=at.k_proj, v=at.v_proj, o=at.o_proj).items()}
    tr, seen, produced, recoded, moe_gemms, route, live = {"x": t2n(x)}, [], {}, None, [], None, {}
    for call in calls:
        name, args, ptrs, outs, out_ptrs = call
        if name == "repack_act_f6":
            recoded = args
            continue
        if name in GEMMS:
            proj = _gemm_call(call, by_weight, produced, L.READS, recoded)
            recoded = None
            assert (name == "dense_layer_gemm_i4_o4") == (proj in "kv"), (proj, name)
            tr[proj] = dict(codes=t2n(outs[0]), sz=t2n(outs[1]).reshape(rows, req.kv_heads, 2)) if proj in "kv" else t2n(outs[0])
            seen.append(proj)
            continue
        assert recoded is None, name
        seen.append(name)
        if name == "rmsnorm_fp16_i4":
            produced["norm1"], tr["norm1"] = outs, L._quant(outs, rows)
        elif name == "reorder_fp16_i4":
            produced["attn_q"], tr["attn"], tr["attn_q"] = outs, t2n(args[0]), L._quant(outs, rows)
        elif name == "add_rmsnorm_fp16_i4":
            produced["norm2"], tr["residual1"], tr["norm2"] = outs[1:], t2n(outs[0]), L._quant(outs[1:], rows)
            live["add_rmsnorm"], produced["residual"] = out_ptrs, outs[0]
            assert L._same(args[1], x), "the post-attention add did not take the layer input"
        elif name == "moe_route_topk":
            route, tr["router_logits"], tr["route"] = outs[0], t2n(args[0]), _route_tables(outs[0])
        elif name == "moe_gemm_i4":
            assert args[5] is route
            moe_gemms.append((args, outs))
        elif name == "activate_fp16_i4":
            produced["act"], tr["act"] = outs, L._quant(outs, R_)
            assert L._same(args[0], moe_gemms[0][1][0]) and L._same(args[1], moe_gemms[0][1][1]), "the activation did not read gate / up"
        elif name == "moe_combine":
            assert args[1] is route and L._same(args[0], moe_gemms[1][1][0]), "the combine did not read the down GEMM's output"
            assert L._same(args[2], produced["residual"]) and ptrs[2] == live["add_rmsnorm"][0], "the combine's residual is not residual1"
            assert L._same(outs[0], out)
    assert seen == L._expected_ops(req, False)[:-4] + ["moe_route_topk", "moe_gemm_i4", "activate_fp16_i4", "moe_gemm_i4", "moe_combine"], seen
    # the block's operands: x_q and residual are add_rmsnorm_fp16_i4's very outputs (address and bytes)
    (x_q, gate_in, residual), (xq_ptrs, _, res_ptr) = moe_in, moe_ptrs
    assert list(xq_ptrs) == list(live["add_rmsnorm"][1:5]) and all(L._same(a, b) for a, b in zip(x_q, produced["norm2"])), "x_q"
    assert res_ptr == live["add_rmsnorm"][0] and L._same(residual, produced["residual"]), "residual"
    tr["gate_in"] = t2n(gate_in)
    # the two routed GEMMs: the norm's codes gathered per token against w13, the activation's rows against w2
    (a1, o1), (a2, o2) = moe_gemms
    o8, o4, s8, s4 = produced["norm2"]
    assert L._same(a1[0], o4) and L._same(a1[1], s4) and L._same(a1[2], o8) and L._same(a1[3], s8), "gate / up did not read norm2"
    assert [t.data_ptr() for t in a1[4]] == [getattr(moe, "w13" + s).data_ptr() for s in ("_int4", "_int8", "_scale_int4", "_scale_int8")]
    a8, a4, t8, t4 = produced["act"]
    assert L._same(a2[0], a4) and L._same(a2[1], t4) and L._same(a2[2], a8) and L._same(a2[3], t8), "down did not read the activation"
    assert [t.data_ptr() for t in a2[4]] == [getattr(moe, "w2" + s).data_ptr() for s in ("_int4", "_int8", "_scale_int4", "_scale_int8")]
    assert len(o1) == 2 and len(o2) == 1
    tr["gate"], tr["up"], tr["y"] = t2n(o1[0]), t2n(o1[1]), t2n(o2[0])
    tr["out"] = t2n(out)
    tr["cache"] = dict(buf=pool_after[0], param=pool_after[1])
    return tr


@pytest.mark.parametrize("route", V.ROUTES)
def test_mixtral_layer(route):
    """A prefill from empty caches (every expert fed), C decode only (6 routed rows: experts without a row), D mixed; layer_idx 1 over a
    pool of random bytes"""
    case = V.mixtral_case(route)
    layer, req = _mixtral_layer(), case["req"]
    pool = L._device_pool(case["pool"], V.MIXTRAL_KV)
    marks = [{}]
    hook = _moe_in_hook(layer, marks)
    try:
        before = L._snapshot(pool)
        x = _dev(case["x"])
        out, calls = _forward(layer, pool, req, x)
    finally:
        hook.remove()
    tr = _mixtral_trace(calls, layer, req, x, out, L._snapshot(pool), marks[0]["moe_in"], marks[0]["moe_ptrs"])
    report = []
    fails = X.mixtral_check(tr, dict(req=req, lay=case["lay"], pool=before, x=case["x"]), report)
    L._assert_clean(fails, report, f"Mixtral layer, route {route}")


@functools.lru_cache(maxsize=None)
def _mixtral_model():
    from atom_amd.e2e.mixtral import MixtralForCausalLM
    model = MixtralForCausalLM(_mixtral_config()).cuda()
    fusion = L._unfused()
    for mod in model.modules():                             # one launch per stage, without touching the process-wide DecodeFusion
        if hasattr(mod, "fusion"):
            mod.fusion = fusion
    return model


def _load_model_rest(model, fp16):
    model.model.embed_tokens.weight.data = _dev(fp16["embed"])
    model.lm_head.weight.data = _dev(fp16["head"])
    model.model.norm.weight.data = _dev(fp16["norm_w"])


@pytest.mark.parametrize("route", V.MODEL_ROUTES)
def test_mixtral_model(route):
    """MixtralForCausalLM, 2 layers: the embedding gather, every layer teacher-forced on its observed input and on ITS slice of the pool
    the layer before left, the final norm and the logits"""
    case = V.mixtral_model_case(route)
    model, req = _mixtral_model(), case["req"]
    _load_model_rest(model, case["fp16"])
    for layer, f, lay in zip(model.model.layers, case["fp16"]["layers"], case["mdl"]["layers"]):
        _load_mixtral(layer, f, lay)
    pool = L._device_pool(case["pool"], V.MIXTRAL_KV)
    tr, marks, after, calls = _model_forward(model, model.model.layers, case, pool, _moe_in_hook)
    for m, layer, pool_after in zip(marks, model.model.layers, after):
        tr["layers"].append(_mixtral_trace(calls[m["start"]:m["stop"]], layer, req, m["x"], m["out"], pool_after, m["moe_in"], m["moe_ptrs"]))
    report = []
    fails = R.check_model(tr, dict(req=req, mdl=case["mdl"], pool=case["pool"], ids=case["ids"]), report, layer_check=X.mixtral_check)
    L._assert_clean(fails, report, f"Mixtral model, route {route}")


# ==================================================================================================== LoRA
LORA_READS = dict(q="norm1", k="norm1", v="norm1", o="attn_q", gate="norm2", up="norm2", down="act")


class _NormSpy:
    """every call of atom_amd.e2e.llama_lora.rmsnorm_fp16: (launches captured so far, cloned output); ``calls_now``: a list whose only
    element is the growing list of captured launches"""

    def __init__(self, calls_now):
        self.calls_now, self.seen = calls_now, []

    def __enter__(self):
        from atom_amd.e2e import llama_lora
        self._orig = llama_lora.rmsnorm_fp16

        def spy(*args, **kw):
            out = self._orig(*args, **kw)
            self.seen.append((len(self.calls_now[0]), out.clone()))
            return out
        llama_lora.rmsnorm_fp16 = spy
        return self

    def __exit__(self, *exc):
        from atom_amd.e2e import llama_lora
        llama_lora.rmsnorm_fp16 = self._orig


@functools.lru_cache(maxsize=None)
def _manager(kv_heads):
    """the case's adapters through LlamaLoraManager.load: 3 adapters, all seven projections, alpha 24 on rank 16"""
    from atom_amd.utils.lora import LORA_MODULES, LlamaLoraManager
    lora = V.adapters(kv_heads)
    mgr = LlamaLoraManager(_config(kv_heads, V.LORA_THETA), V.NADAPT, V.RANK, target_modules=LORA_MODULES, device=torch.device("cuda"))
    for a, ad in enumerate(lora["adapters"]):
        w = mgr.alloc()
        assert w.idx == a
        for module, per_layer in ad.items():
            for layer, (A, B) in enumerate(per_layer):
                mgr.load(w, layer, module, _dev(A), _dev(B), alpha=lora["alpha"])
    return mgr


@functools.lru_cache(maxsize=None)
def _lora_model(kv_heads):
    from atom_amd.e2e import LlamaForCausalLMWithLora
    return LlamaForCausalLMWithLora(_config(kv_heads, V.LORA_THETA)).cuda()


def _load_lora_layer(layer, fp16, lay):
    for name, mod in L._projections(layer).items():
        _load_linear(mod, fp16[name], lay["w"][name], name)
    _load_norms(layer, fp16)


def _lora_trace(calls, norms, layer, mgr, req, x, out, pool_after):
    """The captured launches of ONE forward of the layer with adapters as a tests/variant_ref.py trace.  Asserts on the way: the
    documented op order, one launch each; every GEMM fed with its quantiser stage's very outputs; every adapter call given the GEMM's
    own output tensor (address and bytes) for its rows; kv_quant_u4, the cache writes, the attention ops, the residual add and the
    activation reading the adapted tensors."""
    rows, doff, nd, nkv = req.rows, req.doff, len(req.decodes), req.kv_heads
    n_lora = int(doff > 0) + int(nd > 0)
    by_weight = {mod.weight_int8.data_ptr(): name for name, mod in L._projections(layer).items()}
    by_pool = {mgr.mgr[m].wa_T.data_ptr(): p for m, p in V.LORA_MODULES.items()}
    assert len(norms) == 2 and norms[0][0] == 1, [n for n, _ in norms]
    tr = {"x": t2n(x), "xn": t2n(norms[0][1]), "n": t2n(norms[1][1])}
    seen, produced, recoded = [], {}, None
    base, base_ptr, y, xs, codes = {}, {}, {}, {}, {}          # per projection: GEMM output, its address, the adapted tensor, A's operand
    for call in calls:
        name, args, ptrs, outs, out_ptrs = call
        if name == "repack_act_f6":
            recoded = args
            continue
        if name in GEMMS:
            assert name == "dense_layer_gemm_i4_fp16"
            proj = _gemm_call(call, by_weight, produced, LORA_READS, recoded)
            recoded = None
            base[proj], base_ptr[proj], y[proj], xs[proj] = outs[0], out_ptrs[0], outs[0].clone(), []
            seen.append(proj)
            continue
        assert recoded is None, name
        if name == "add_lora":
            proj = by_pool[ptrs[2]]
            assert ptrs[3] == mgr.mgr[[m for m, p in V.LORA_MODULES.items() if p == proj][0]].wb_T.data_ptr()
            width = base[proj].size(1) * 2
            lo = {base_ptr[proj]: 0, base_ptr[proj] + doff * width: doff}.get(ptrs[0])
            assert lo is not None, f"{proj}: the adapter call was not given the GEMM's output tensor"
            sl = slice(0, doff) if lo == 0 and doff > 0 else slice(doff, rows)
            assert args[0].size(0) == sl.stop - sl.start and L._same(args[0], base[proj][sl]), f"{proj}: rows {sl} are not the GEMM's output"
            y[proj][sl] = outs[0]
            xs[proj].append(args[1])
            seen.append("add_lora:" + proj)
            continue
        seen.append(name)
        if name == "rmsnorm_fp16_i4":
            produced["norm1"], tr["norm1"] = outs, L._quant(outs, rows)
        elif name == "kv_quant_u4":
            proj = {base_ptr["k"]: "k", base_ptr["v"]: "v"}[ptrs[0]]
            assert proj not in codes and L._same(args[0].reshape(rows, -1), y[proj]), f"kv_quant_u4 did not read the adapted {proj}"
            codes[proj] = outs
            tr[proj] = dict(codes=t2n(outs[0]).reshape(rows, -1), sz=t2n(outs[1]).reshape(rows, nkv, 2))
        elif name in ("init_kv_i4", "append_kv_i4"):
            sl = slice(0, doff) if name == "init_kv_i4" else slice(doff, rows)
            want = (codes["k"][0][sl], codes["v"][0][sl], codes["k"][1][sl], codes["v"][1][sl])
            assert all(L._same(a.reshape(w.shape), w) for a, w in zip(args[1:5], want)), f"{name} did not write kv_quant_u4's output"
        elif name in ("batch_prefill_i4", "batch_decode_i4"):
            sl = slice(0, doff) if name == "batch_prefill_i4" else slice(doff, rows)
            assert L._same(args[0].reshape(sl.stop - sl.start, -1), y["q"][sl]), f"{name} did not read the adapted q"
        elif name == "reorder_fp16_i4":
            produced["attn_q"], tr["attn"], tr["attn_q"] = outs, t2n(args[0]), L._quant(outs, rows)
        elif name == "add_rmsnorm_fp16_i4":
            assert ptrs[0] == base_ptr["o"] and L._same(args[0], y["o"]) and L._same(args[1], x), "the residual add did not read the adapted o and x"
            produced["norm2"], tr["residual1"], tr["norm2"] = outs[1:], t2n(outs[0]), L._quant(outs[1:], rows)
        elif name == "activate_fp16_i4":
            assert [ptrs[0], ptrs[1]] == [base_ptr["gate"], base_ptr["up"]] and L._same(args[0], y["gate"]) and L._same(args[1], y["up"])
            produced["act"], tr["act"] = outs, L._quant(outs, rows)
    lora = lambda p: ["add_lora:" + p] * n_lora
    kv = (["init_kv_i4", "batch_prefill_i4"] if doff else []) + (["append_kv_i4", "batch_decode_i4"] if nd else [])
    assert seen == (["rmsnorm_fp16_i4", "q", "k", "v"] + lora("q") + lora("k") + lora("v") + ["kv_quant_u4"] * 2 + kv + ["reorder_fp16_i4", "o"]
                    + lora("o") + ["add_rmsnorm_fp16_i4", "gate", "up"] + lora("gate") + lora("up") + ["activate_fp16_i4", "down"] + lora("down")), seen
    for p, (after, before) in dict(q=("q", "q_base"), k=("k_lora", "k_base"), v=("v_lora", "v_base"), o=("o", "o_base"), gate=("gate", "gate_base"),
                                   up=("up", "up_base"), down=("d", "d_base")).items():
        tr[after], tr[before] = t2n(y[p]), t2n(base[p])
    tr["d_x"] = t2n(torch.cat(xs["down"], dim=0))
    tr["out"] = t2n(out)
    tr["cache"] = dict(buf=pool_after[0], param=pool_after[1])
    return tr


@pytest.mark.parametrize("route,kv_heads", V.LORA_CASES)
def test_lora_layer(route, kv_heads):
    """layer 1 of a LlamaForCausalLMWithLora with adapters set through LlamaLoraManager.load and set_adapters: two different adapters
    and one sequence without in every batch; A prefill, C decode, D mixed (other ids on the prefill requests than on the decode rows)"""
    case = V.lora_case(route, kv_heads)
    model, mgr, req = _lora_model(kv_heads), _manager(kv_heads), case["req"]
    layer = model.model.layers[1]
    _load_lora_layer(layer, case["fp16"], case["lay"])
    pool = L._device_pool(case["pool"], kv_heads)
    model.set_adapters(case["lay"]["lora_ids"], mgr)
    calls_now = []
    try:
        before = L._snapshot(pool)
        x = _dev(case["x"])
        with _NormSpy(calls_now) as norms:
            from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
            pre, dec = L._sequences(pool, req)
            blen = BatchLenInfo([n for _, n, _ in req.prefills], len(req.decodes), torch.device("cuda"))
            with _Spy() as spy:
                calls_now.append(spy.calls)
                out = layer(x, blen, BatchedKvCacheInt4(pre) if pre else None, BatchedKvCacheInt4(dec) if dec else None)
                torch.cuda.synchronize()
    finally:
        model.set_adapters(None)
    tr = _lora_trace(spy.calls, norms.seen, layer, mgr, req, x, out, L._snapshot(pool))
    report = []
    fails = X.lora_check(tr, dict(req=req, lay=case["lay"], pool=before, x=case["x"]), report)
    L._assert_clean(fails, report, f"LoRA layer, route {route}, {kv_heads} K/V heads, ids {case['lay']['lora_ids']}")


@pytest.mark.parametrize("route,kv_heads", V.LORA_MODEL_CASES)
def test_lora_model(route, kv_heads):
    """LlamaForCausalLMWithLora, 2 layers: as test_mixtral_model; layer i on layer i of the adapter pools"""
    case = V.lora_model_case(route, kv_heads)
    model, mgr, req = _lora_model(kv_heads), _manager(kv_heads), case["req"]
    _load_model_rest(model, case["fp16"])
    for layer, f, lay in zip(model.model.layers, case["fp16"]["layers"], case["mdl"]["layers"]):
        _load_lora_layer(layer, f, lay)
    pool = L._device_pool(case["pool"], kv_heads)
    model.set_adapters(case["mdl"]["layers"][0]["lora_ids"], mgr)
    calls_now = []
    try:
        with _NormSpy(calls_now) as norms:
            tr, marks, after, calls = _model_forward(model, model.model.layers, case, pool, calls_now=calls_now)
    finally:
        model.set_adapters(None)
    for m, layer, pool_after in zip(marks, model.model.layers, after):
        mine = [(n - m["start"], t) for n, t in norms.seen if m["start"] < n < m["stop"]]
        tr["layers"].append(_lora_trace(calls[m["start"]:m["stop"]], mine, layer, mgr, req, m["x"], m["out"], pool_after))
    report = []
    fails = R.check_model(tr, dict(req=req, mdl=case["mdl"], pool=case["pool"], ids=case["ids"]), report, layer_check=X.lora_check)
    L._assert_clean(fails, report, f"LoRA model, route {route}, {kv_heads} K/V heads, ids {case['mdl']['layers'][0]['lora_ids']}")
