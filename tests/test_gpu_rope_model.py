"""RoPE scaling through the model tree (atom_amd/e2e/rope.py -> LlamaAttention -> the attention ops' ``rope_table`` / ``attn_scale``):
the attention stage of the real-kernel LlamaDecoderLayer against the FP64 table reference of tests/rope_table_ref.py on the cache the
layer itself wrote, with the layer sizes, inputs and launch tracing of tests/test_gpu_layer_ref.py; generate() by graph replay against
the eager loop; one speculative run; and the refusal of an unsupported type.

The configs scale with ``original_max_position_embeddings = 64`` so that the scaling bites at the cases' lengths (<= 37 tokens): with
theta 1e4 the llama3 rule then divides the frequencies of pairs 17..63 by 8.  Every layer case also shows that the reference with PLAIN
theta misses the bound the layer is held to -- a layer that dropped the table would fail here."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import layer_cases as C
from tests import layer_ref as R
from tests import rope_table_ref as RT
from tests import test_gpu_generate as G
from tests import test_gpu_layer_ref as LR

pytestmark = pytest.mark.gpu

SCALING = {
    "llama3": dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64),
    "yarn": dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64),
}


def _table(kind, theta):
    return RT.config_table(dict(SCALING[kind], rope_theta=theta))


def _config(kv_heads, theta, kind, new_spelling):
    c = LR._config(kv_heads, theta)
    if new_spelling:                                          # transformers 5: everything in rope_parameters, rope_theta None
        c.rope_theta, c.rope_parameters = None, dict(SCALING[kind], rope_theta=theta)
    else:
        c.rope_scaling = dict(SCALING[kind])
    return c


@functools.lru_cache(maxsize=None)
def _layer(kv_heads, theta, kind, fused=False):
    from atom_amd.e2e import LlamaDecoderLayer
    from atom_amd.e2e.llama import DecodeFusion
    layer = LlamaDecoderLayer(_config(kv_heads, theta, kind, new_spelling=(kind == "llama3")), layer_idx=1,
                              fusion=DecodeFusion() if fused else LR._unfused()).cuda()
    fp16, lay = C.layer_params(kv_heads, 1)
    LR._load(layer, fp16, lay)
    at = layer.self_attn
    table, scale = _table(kind, theta)
    assert at.rope_table.is_cuda and at.rope_table.dtype == torch.float32 and np.array_equal(LR.t2n(at.rope_table), table)
    assert at.attn_scale == scale and at.rope_theta == theta and "self_attn.rope_table" not in layer.state_dict()
    return layer


def _table_attention(req, q, pool, layer_idx, table, scale):
    """float64 [T, heads * 128]: the table reference over the described requests' caches (prefill rows first, then decode rows)"""
    nh, nkv = req.heads, req.kv_heads
    qf = np.asarray(q, dtype=np.float16).reshape(req.rows, nh, 128)
    out = np.zeros((req.rows, nh, 128))
    if req.prefills:
        indptr, indices, lpo, qo = req.prefill_tables()
        c = dict(data=pool[0], param=pool[1], indptr=indptr, indices=indices, lpo=lpo)
        out[:req.doff] = RT.ref_prefill(qf[:req.doff], c, qo, table, G=nh // nkv, attn_scale=scale, layer=layer_idx)
    if req.decodes:
        indptr, indices, lpo = req.decode_tables()
        c = dict(data=pool[0], param=pool[1], indptr=indptr, indices=indices, lpo=lpo)
        out[req.doff:] = RT.ref_decode(qf[req.doff:], c, table, G=nh // nkv, attn_scale=scale, layer=layer_idx)
    return out.reshape(req.rows, nh * 128)


def _run_route(layer, case, hip_prefill):
    """test_gpu_layer_ref._layer_route up to the trace: (trace, x, out, pool after)"""
    dev = torch.device("cuda")
    kv_heads = case["req"].kv_heads
    pool = LR._device_pool(case["pool"], kv_heads)
    layer.fusion.prefill_attn = hip_prefill
    try:
        known = {}
        if case["first"] is not None:
            seqs = LR._sequences(pool, case["first"])
            LR._call(layer, pool, case["first"], torch.from_numpy(case["x_first"]).to(dev), seqs)
            known = {tuple(pages): seq for (_, _, pages), seq in zip(case["first"].prefills, seqs[0])}
        x = torch.from_numpy(case["x"]).to(dev)
        out, calls = LR._call(layer, pool, case["req"], x, LR._sequences(pool, case["req"], known))
    finally:
        layer.fusion.prefill_attn = False
    return calls, x, out, LR._snapshot(pool)


ROUTES = [("A", False), ("A", True), ("B", False), ("C", False), ("D", False)]   # eager prefill, op prefill, chunked, decode, mixed


@pytest.mark.parametrize("kind", sorted(SCALING))
@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("route,hip_prefill", ROUTES)
def test_attention_stage_follows_the_table(route, hip_prefill, kv_heads, kind):
    case = C.layer_case(route, kv_heads)
    theta, lay, req = case["lay"]["rope_theta"], case["lay"], case["req"]
    layer = _layer(kv_heads, theta, kind)
    calls, x, out, after = _run_route(layer, case, hip_prefill)
    tr = LR._trace(calls, layer, req, x, out, after, hip_prefill, lay)
    table, scale = _table(kind, theta)
    ok, msg = R._check_attn(req, tr["attn"], _table_attention(req, tr["q"], after, lay["layer_idx"], table, scale))
    print(f"route {route} op prefill {hip_prefill} kv_heads {kv_heads} {kind}: {msg}")
    assert ok, msg
    plain_ok, plain_msg = R._check_attn(req, tr["attn"], R.attention(req, tr["q"], after, lay["layer_idx"], theta))
    print(f"    against plain theta: {plain_msg}")
    assert not plain_ok, "the plain-theta reference is within the bound too: this case would not notice a dropped table"


@pytest.mark.parametrize("kind", sorted(SCALING))
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_fused_decode_routes_take_the_table(kv_heads, kind):
    """the decode step with the append inside the decode launch (MHA) and the other fused launches: the bits and the cache of the
    one-launch-per-stage layer, which test_attention_stage_follows_the_table holds to the reference"""
    case = C.layer_case("C", kv_heads)
    theta = case["lay"]["rope_theta"]
    _, _, want, pool_want = _run_route(_layer(kv_heads, theta, kind), case, False)
    calls, _, got, pool_got = _run_route(_layer(kv_heads, theta, kind, fused=True), case, False)
    names = [c[0] for c in calls]
    assert "append_kv_i4" not in names, names                # (the fused route ran)
    assert torch.equal(got, want)
    assert np.array_equal(pool_got[0], pool_want[0]) and np.array_equal(pool_got[1].view(np.uint16), pool_want[1].view(np.uint16))


def _gen_model(kv_heads, seed):
    """test_gpu_generate._model with the llama3 config"""
    from atom_amd.e2e import LlamaForCausalLM
    cfg = G._cfg(kv_heads)
    cfg.rope_scaling = dict(SCALING["llama3"])
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    assert all(layer.self_attn.rope_table is not None for layer in model.model.layers)
    return model


@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_equals_the_eager_loop(kv_heads):
    """two prompts, 41 new tokens, a two-layer model with the llama3 config: tokens and logits of the graph replay equal the eager
    loop's (tests/test_gpu_generate.py's pattern; the eager caches take the static cache's max_pages, which sizes the KV splits)"""
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _gen_model(kv_heads, G.SEED[kv_heads]), G._prompts(2)
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
    # and the table matters to this model: the same weights without scaling give other logits
    plain = _gen_model(kv_heads, G.SEED[kv_heads])
    for layer in plain.model.layers:
        layer.self_attn.rope_table = None
    pp = G._pool(2, G._kv_heads(kv_heads), capacity, 16)
    _, _, plain_logits = G._prefill(plain, prompts, pp)
    assert not torch.equal(plain_logits, first_logits)


def test_speculative_run_reproduces_greedy():
    """SpeculativeParams(num_draft_tokens=2) with the llama3 config: the replayed speculative run equals the eager speculative loop of
    tests/test_gpu_generate_spec.py (n-gram drafts by tests/spec_ref.py, the same kernels) token for token, as that suite asserts for
    the unscaled model.  Against PLAIN greedy generate() the verify step attends through the prefill op and the plain step through the
    decode op (different kernels, within rounding of each other): equality is asserted where the plain run's logits leave a margin
    between the best two tokens at every step, and only reported where they hold a near-tie."""
    from atom_amd.e2e import SpeculativeParams, generate
    from tests import spec_ref
    from tests import test_gpu_generate_spec as S
    K, batch, new, key = 2, 2, 24, "rope-llama3"
    model, prompts = _gen_model(None, G.SEED[None]), G._prompts(batch)
    S._MODELS[None, key] = model                              # the suite's eager loop on THIS model
    try:
        want, accepted, steps, counts, _ = S._eager_spec(None, batch, K, new, lambda b, h, n: spec_ref.draft_rule(h, len(h), K, 3, 1), seed=key)
    finally:
        del S._MODELS[None, key]
    pool = S._spec_pool(prompts, 4, new, K)
    free = pool.num_free_blocks
    spec, stats = generate(model, prompts, new, pool, speculative=SpeculativeParams(num_draft_tokens=K, ngram_max=3), return_spec_stats=True)
    assert spec == want and stats.accepted == accepted and stats.steps == steps
    assert pool.num_free_blocks == free
    plain, logits = generate(model, prompts, new, pool, return_logits=True)
    top2 = logits.float().topk(2, dim=-1).values
    margin = float((top2[..., 0] - top2[..., 1]).min())
    print(f"accepted {accepted}, steps {steps}; smallest top-2 margin of the plain run {margin:.4f}; speculative == plain greedy: {spec == plain}")
    if margin >= 0.125:
        assert spec == plain
    elif spec != plain:
        print("    near-tie in the plain run: the two kernels may choose differently there; not compared")


def test_unsupported_type_raises_at_construction():
    from atom_amd.e2e import LlamaDecoderLayer, LlamaForCausalLM
    cfg = LR._config(2, 1e4)
    cfg.rope_scaling = dict(rope_type="dynamic", factor=2.0)
    with pytest.raises(NotImplementedError, match="dynamic"):
        LlamaDecoderLayer(cfg, layer_idx=0)
    with pytest.raises(NotImplementedError, match="dynamic"):
        LlamaForCausalLM(cfg)
    plain = LlamaDecoderLayer(LR._config(2, 5e5), layer_idx=0)  # no scaling: nothing allocated, nothing passed
    assert plain.self_attn.rope_table is None and plain.self_attn.rope_kw == {} and list(plain.self_attn.named_buffers(recurse=False)) == []
