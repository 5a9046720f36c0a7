"""Sliding-window attention through the model tree (``config.sliding_window`` -> LlamaAttention -> the attention ops' ``window=``): the
attention stage of the real-kernel LlamaDecoderLayer against the FP64 window reference of tests/attn_window_ref.py on the cache the layer
itself wrote, with the layer sizes, inputs and launch tracing of tests/test_gpu_layer_ref.py (the pattern of
tests/test_gpu_rope_model.py); the fused decode routes against the unfused layer; ``layer_types``; generate() by graph replay against
the eager loop with prompts shorter and longer than the window; one speculative run; and the refusals.

W = 8: every case holds rows at positions >= 8 (the cases' requests are 16 .. 37 tokens long), and every layer case also shows that
the reference WITHOUT a window misses the bound the layer is held to -- a layer that dropped the window would fail here."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_window_ref as W
from tests import layer_cases as C
from tests import layer_ref as R
from tests import test_gpu_generate as G
from tests import test_gpu_layer_ref as LR
from tests import test_gpu_rope_model as RM

pytestmark = pytest.mark.gpu

WINDOW = 8
GEN_WINDOW = 12                                              # test_gpu_generate's first two prompts hold 7 and 19 tokens


def _config(kv_heads, theta, window=WINDOW, **extra):
    c = LR._config(kv_heads, theta)
    c.sliding_window = window
    for k, v in extra.items():
        setattr(c, k, v)
    return c


@functools.lru_cache(maxsize=None)
def _layer(kv_heads, theta, fused=False):
    from atom_amd.e2e import LlamaDecoderLayer
    from atom_amd.e2e.llama import DecodeFusion
    layer = LlamaDecoderLayer(_config(kv_heads, theta), layer_idx=1, fusion=DecodeFusion() if fused else LR._unfused()).cuda()
    fp16, lay = C.layer_params(kv_heads, 1)
    LR._load(layer, fp16, lay)
    assert layer.self_attn.window == WINDOW and layer.self_attn.rope_kw == {"window": WINDOW}
    return layer


def _window_attention(req, q, pool, layer_idx, theta, window):
    """float64 [T, heads * 128]: the window reference over the described requests' caches (prefill rows first, then decode rows)"""
    nh, nkv = req.heads, req.kv_heads
    qf = np.asarray(q, dtype=np.float16).reshape(req.rows, nh, 128)
    out = np.zeros((req.rows, nh, 128))
    if req.prefills:
        indptr, indices, lpo, qo = req.prefill_tables()
        c = dict(data=pool[0], param=pool[1], indptr=indptr, indices=indices, lpo=lpo)
        out[:req.doff] = W.ref_prefill(qf[:req.doff], c, qo, window, G=nh // nkv, theta=theta, layer=layer_idx)
    if req.decodes:
        indptr, indices, lpo = req.decode_tables()
        c = dict(data=pool[0], param=pool[1], indptr=indptr, indices=indices, lpo=lpo)
        out[req.doff:] = W.ref_decode(qf[req.doff:], c, window, G=nh // nkv, theta=theta, layer=layer_idx)
    return out.reshape(req.rows, nh * 128)


# a windowed layer's prefill always attends through the op, so the routes with chunks from empty caches (A, D) are traced as op prefill
ROUTES = [("A", True), ("B", False), ("C", False), ("D", True)]


@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("route,hip_prefill", ROUTES)
def test_attention_stage_follows_the_window(route, hip_prefill, kv_heads):
    case = C.layer_case(route, kv_heads)
    theta, lay, req = case["lay"]["rope_theta"], case["lay"], case["req"]
    calls, x, out, after = RM._run_route(_layer(kv_heads, theta), case, hip_prefill)
    tr = LR._trace(calls, _layer(kv_heads, theta), req, x, out, after, hip_prefill, lay)
    ok, msg = R._check_attn(req, tr["attn"], _window_attention(req, tr["q"], after, lay["layer_idx"], theta, WINDOW))
    print(f"route {route} op prefill {hip_prefill} kv_heads {kv_heads} W {WINDOW}: {msg}")
    assert ok, msg
    plain_ok, plain_msg = R._check_attn(req, tr["attn"], R.attention(req, tr["q"], after, lay["layer_idx"], theta))
    print(f"    against plain causal attention: {plain_msg}")
    assert not plain_ok, "the un-windowed reference is within the bound too: this case would not notice a dropped window"


@pytest.mark.parametrize("route", ["A", "D"])
def test_windowed_prefill_never_takes_the_torch_route(route):
    """chunks from empty caches with DecodeFusion.prefill_attn off: the windowed layer still calls ops.batch_prefill_i4"""
    case = C.layer_case(route, 2)
    calls, _, _, _ = RM._run_route(_layer(2, case["lay"]["rope_theta"]), case, False)
    assert "batch_prefill_i4" in [c[0] for c in calls]
    calls, _, _, _ = RM._run_route(LR._layer(2, case["lay"]["rope_theta"]), case, False)
    assert "batch_prefill_i4" not in [c[0] for c in calls]   # (the layer without a window takes it, as ever)


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_fused_decode_routes_take_the_window(kv_heads):
    """the decode step through the fused launches (FP32 k / v sums quantised into the cache, then the windowed op: two launches): the
    bits and the cache of the one-launch-per-stage layer, which test_attention_stage_follows_the_window holds to the reference"""
    case = C.layer_case("C", kv_heads)
    theta = case["lay"]["rope_theta"]
    _, _, want, pool_want = RM._run_route(_layer(kv_heads, theta), case, False)
    calls, _, got, pool_got = RM._run_route(_layer(kv_heads, theta, fused=True), case, False)
    names = [c[0] for c in calls]
    assert "append_kv_i4" not in names and "quant_append_kv_i4" in names and "batch_decode_i4" in names, names
    assert torch.equal(got, want)
    assert np.array_equal(pool_got[0], pool_want[0]) and np.array_equal(pool_got[1].view(np.uint16), pool_want[1].view(np.uint16))


def test_layer_types_window_only_the_marked_layers():
    from atom_amd.e2e import LlamaDecoderLayer, LlamaForCausalLM
    types_ = ["sliding_attention", "full_attention"]
    model = LlamaForCausalLM(_config(2, 1e4, layer_types=types_))
    assert [layer.self_attn.window for layer in model.model.layers] == [WINDOW, None]
    assert model.model.layers[1].self_attn.rope_kw == {} and model.model.layers[0].self_attn.rope_kw == {"window": WINDOW}
    off = LlamaForCausalLM(_config(2, 1e4, layer_types=types_, use_sliding_window=False))
    assert [layer.self_attn.window for layer in off.model.layers] == [None, None]
    assert LlamaDecoderLayer(_config(2, 1e4, window=None), layer_idx=1).self_attn.window is None
    # ... and the unmarked layer computes what the layer of a config without a window computes
    case = C.layer_case("C", 2)
    theta = case["lay"]["rope_theta"]
    full = LlamaDecoderLayer(_config(2, theta, layer_types=types_), layer_idx=1, fusion=LR._unfused()).cuda()
    fp16, lay = C.layer_params(2, 1)
    LR._load(full, fp16, lay)
    _, _, got, _ = RM._run_route(full, case, False)
    _, _, want, _ = RM._run_route(LR._layer(2, theta), case, False)
    _, _, windowed, _ = RM._run_route(_layer(2, theta), case, False)
    assert torch.equal(got, want) and not torch.equal(windowed, want)


def _gen_model(kv_heads, seed, window=GEN_WINDOW):
    """test_gpu_generate._model with a sliding window"""
    from atom_amd.e2e import LlamaForCausalLM
    cfg = G._cfg(kv_heads)
    cfg.sliding_window = window
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    assert all(layer.self_attn.window == window for layer in model.model.layers)
    return model


@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_equals_the_eager_loop(kv_heads):
    """two prompts (7 tokens: shorter than the window of 12; 19: longer), 41 new tokens, a two-layer model: tokens and logits of the
    graph replay equal the eager loop's (tests/test_gpu_generate.py's pattern); and the window matters to this model"""
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _gen_model(kv_heads, G.SEED[kv_heads]), G._prompts(2)
    assert len(prompts[0]) < GEN_WINDOW < len(prompts[1])
    cap = max(-(-(len(p) + G.NEW - 1) // 16) for p in prompts)
    capacity = G._pages([len(p) for p in prompts], 16, G.NEW) + 2
    pe = G._pool(2, G._kv_heads(kv_heads), capacity, 16)
    se, first, first_logits = G._prefill(model, prompts, pe)
    toks, logs = G._eager_decode(model, se, first, G.NEW - 1, cap)
    want_tokens = torch.cat([first[None], toks]).t().tolist()
    want_logits = torch.cat([first_logits[None], logs])
    pg = G._pool(2, G._kv_heads(kv_heads), capacity, 16)
    caches = [KvCacheInt4(pg, 0) for _ in prompts]
    got_tokens, got_logits = generate(model, prompts, G.NEW, pg, caches=caches, return_logits=True)
    assert got_tokens == want_tokens
    assert got_logits.shape == want_logits.shape and torch.equal(got_logits, want_logits)
    G._assert_same_cache(caches, pg, se, pe)
    plain = _gen_model(kv_heads, G.SEED[kv_heads])
    for layer in plain.model.layers:
        layer.self_attn.window = None
    pp = G._pool(2, G._kv_heads(kv_heads), capacity, 16)
    _, _, plain_logits = G._prefill(plain, prompts, pp)
    assert not torch.equal(plain_logits[1], first_logits[1])  # (the prompt longer than the window)


def test_speculative_run_reproduces_the_eager_speculative_loop():
    """SpeculativeParams(num_draft_tokens=2) on the windowed model: the replayed speculative run equals the eager speculative loop of
    tests/test_gpu_generate_spec.py token for token (the verify step attends through the windowed prefill op on a static cache)"""
    from atom_amd.e2e import SpeculativeParams, generate
    from tests import spec_ref
    from tests import test_gpu_generate_spec as S
    K, batch, new, key = 2, 2, 24, "window"
    model, prompts = _gen_model(None, G.SEED[None]), G._prompts(batch)
    S._MODELS[None, key] = model
    try:
        want, accepted, steps, counts, _ = S._eager_spec(None, batch, K, new, lambda b, h, n: spec_ref.draft_rule(h, len(h), K, 3, 1), seed=key)
    finally:
        del S._MODELS[None, key]
    pool = S._spec_pool(prompts, 4, new, K)
    free = pool.num_free_blocks
    spec, stats = generate(model, prompts, new, pool, speculative=SpeculativeParams(num_draft_tokens=K, ngram_max=3), return_spec_stats=True)
    assert spec == want and stats.accepted == accepted and stats.steps == steps
    assert pool.num_free_blocks == free


def test_refusals():
    from atom_amd.e2e import LlamaDecoderLayer, LlamaForCausalLM
    from atom_amd.e2e.mixtral import MixtralDecoderLayer
    for bad in (0, -4096, 2.5):
        with pytest.raises(ValueError, match="sliding_window"):
            LlamaDecoderLayer(_config(2, 1e4, window=bad), layer_idx=0)
        with pytest.raises(ValueError, match="sliding_window"):
            LlamaForCausalLM(_config(2, 1e4, window=bad))
    cfg = _config(2, 1e4, window=4096, num_local_experts=4, num_experts_per_tok=2)
    with pytest.raises(NotImplementedError, match="sliding"):
        MixtralDecoderLayer(cfg, layer_idx=0)
    plain = LlamaDecoderLayer(LR._config(2, 5e5), layer_idx=0)  # no window: nothing passed
    assert plain.self_attn.window is None and plain.self_attn.rope_kw == {}
