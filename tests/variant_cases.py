"""The inputs of the staged Mixtral and LoRA checks, shared by tests/test_variant_ref_cpu.py (which shows that tests/variant_ref.py's
checkers report every wiring error on them) and tests/test_gpu_variant_ref.py (which holds the HIP layers to the same checkers): numpy
only.  The geometry, the random-byte pool, the scrambled page lists and layer_idx 1 are those of tests/layer_cases.py; routes A
(prefill 37 / 16 / 1), C (decode 16 / 17 / 33) and D (mixed).  rope_theta is never the default (Mixtral-8x7B's 1e6, Llama 3's 5e5), so
that a layer which ignores it is seen on every route.

Mixtral: 2 K/V heads, 8 experts, top-2; expert weights fp16 N(0, 0.05^2), router weight N(0, 0.1^2); the reference side packs
concat(w1, w3) and w2 per expert with the oracle's packer.  On route A every expert receives a row, on route C (6 routed rows) some
receive none -- asserted in the CPU test.

LoRA: 4 and 1 K/V heads, rank 16, alpha 24 (alpha / r = 1.5), a pool of 3 adapters on all seven projections, stated directly in the
packed intermediate channel order.  A ~ N(0, 1.2^2 / in), B ~ N(0, 0.2^2): x A^T is about 1.2 rms(x) per rank, the delta
sqrt(16) * 1.2 * 0.3 = 1.4 rms(x) per output against a base output of 0.05 sqrt(in) rms(x) = 1.1 (1.9 for down_proj) -- the CPU test
asserts delta rms >= base rms / 2 on the reference's trace, so that the adapter tolerance cannot absorb a missing or foreign delta.
Ids per SEQUENCE: two different adapters and one -1 in every batch; on D the prefill ids (0, 2) and the decode ids (-1, 0) differ."""
import functools

import numpy as np

from oracle import atom_oracle as O
from tests import layer_cases as C

ROUTES = ("A", "C", "D")
EXPERTS, TOP_K, MIXTRAL_KV, MIXTRAL_THETA = 8, 2, 2, 1e6
RANK, ALPHA, NADAPT, LORA_KV, LORA_THETA = 16, 24.0, 3, (4, 1), 5e5
LORA_IDS = {"A": [2, -1, 0], "C": [0, -1, 2], "D": [0, 2, -1, 0]}
LORA_MODULES = dict(q_proj="q", k_proj="k", v_proj="v", o_proj="o", gate_proj="gate", up_proj="up", down_proj="down")

_pack = lambda w: O.quant_weight_sim(w, 0.85, 2)


# ---------------------------------------------------------------------------------------------------- Mixtral
@functools.lru_cache(maxsize=None)
def mixtral_params(seed):
    """One layer: ``fp16`` (what the GPU test loads: q / k / v / o, the norms, the indices, gate_w [E, H], experts = [(w1, w3, w2)]) and
    ``lay`` (what tests/variant_ref.py takes)"""
    g = np.random.default_rng(7000 + seed)
    shapes = C.proj_shapes(MIXTRAL_KV)
    fp16 = {name: (g.standard_normal(shapes[name]) * 0.05).astype(np.float16) for name in ("q", "k", "v", "o")}
    for name in ("norm1_w", "norm2_w"):
        fp16[name] = (1 + 0.1 * g.standard_normal(C.HIDDEN)).astype(np.float16)
    for name in ("norm1_idx", "norm2_idx", "attn_idx"):
        fp16[name] = g.permutation(C.HIDDEN).astype(np.int16)
    fp16["gate_w"] = (g.standard_normal((EXPERTS, C.HIDDEN)) * 0.1).astype(np.float16)
    w = lambda *shape: (g.standard_normal(shape) * 0.05).astype(np.float16)
    fp16["experts"] = [(w(C.INTER, C.HIDDEN), w(C.INTER, C.HIDDEN), w(C.HIDDEN, C.INTER)) for _ in range(EXPERTS)]
    lay = {name: fp16[name] for name in ("norm1_w", "norm2_w", "norm1_idx", "norm2_idx", "attn_idx")}
    lay["w"] = {name: _pack(fp16[name]) for name in ("q", "k", "v", "o")}
    lay["moe"] = dict(gate_w=fp16["gate_w"], top_k=TOP_K, w13=[_pack(np.concatenate([w1, w3], axis=0)) for w1, w3, _ in fp16["experts"]],
                      w2=[_pack(w2) for _, _, w2 in fp16["experts"]])
    lay["eps"] = C.EPS
    return fp16, lay


def _batch(route, kv_heads, seed):
    req, first = C.requests(route, kv_heads, seed)
    assert first is None
    x = (np.random.default_rng(seed + 100).standard_normal((req.rows, C.HIDDEN)) * 0.7).astype(np.float16)
    return req, x, C.random_pool(kv_heads, seed + 200)


def mixtral_case(route):
    """dict(req, fp16, lay, pool, x)"""
    fp16, lay = mixtral_params(1)
    req, x, pool = _batch(route, MIXTRAL_KV, 500 + 10 * ROUTES.index(route))
    return dict(req=req, fp16=fp16, lay=C._with(lay, rope_theta=MIXTRAL_THETA, layer_idx=1), pool=pool, x=x)


@functools.lru_cache(maxsize=None)
def _model_rest(seed):
    g = np.random.default_rng(seed)
    return dict(embed=g.standard_normal((C.VOCAB, C.HIDDEN)).astype(np.float16), head=(g.standard_normal((C.VOCAB, C.HIDDEN)) * 0.05).astype(np.float16),
                norm_w=(1 + 0.1 * g.standard_normal(C.HIDDEN)).astype(np.float16))


def _model_case(route, kv_heads, seed, rest, layers):
    """``layers``: [(fp16, lay with layer_idx and rope_theta)]"""
    req, first = C.requests(route, kv_heads, seed)
    assert first is None
    fp16 = dict(rest, layers=[f for f, _ in layers])
    mdl = dict(embed=rest["embed"], head=rest["head"], norm_w=rest["norm_w"], eps=C.EPS, layers=[lay for _, lay in layers])
    return dict(req=req, fp16=fp16, mdl=mdl, pool=C.random_pool(kv_heads, seed + 200), ids=np.random.default_rng(seed).integers(0, C.VOCAB, size=req.rows))


MODEL_ROUTES = ("A", "C")


def mixtral_model_case(route):
    params = [mixtral_params(2 + i) for i in range(C.LAYERS)]
    layers = [(f, C._with(lay, rope_theta=MIXTRAL_THETA, layer_idx=i)) for i, (f, lay) in enumerate(params)]
    return _model_case(route, MIXTRAL_KV, 600 + 10 * ROUTES.index(route), _model_rest(61), layers)


# ---------------------------------------------------------------------------------------------------- LoRA
@functools.lru_cache(maxsize=None)
def adapters(kv_heads):
    """dict(rank, alpha, adapters[id][module] = [(A fp16 [r, in], B fp16 [out, r]) per layer]): the whole pool, module names as the manager's"""
    g = np.random.default_rng(8000 + kv_heads)
    shapes = C.proj_shapes(kv_heads)
    pool = []
    for _ in range(NADAPT):
        ad = {}
        for module, p in LORA_MODULES.items():
            out, inp = shapes[p]
            ad[module] = [((g.standard_normal((RANK, inp)) * 1.2 / np.sqrt(inp)).astype(np.float16), (g.standard_normal((out, RANK)) * 0.2).astype(np.float16))
                          for _ in range(C.LAYERS)]
        pool.append(ad)
    return dict(rank=RANK, alpha=ALPHA, adapters=pool)


LORA_CASES = [(r, kv) for r in ROUTES for kv in LORA_KV]


def lora_case(route, kv_heads):
    """dict(req, fp16, lay, pool, x); lay["lora"] the pool, lay["lora_ids"] one id per sequence"""
    fp16, lay = C.layer_params(kv_heads, 1)
    req, x, pool = _batch(route, kv_heads, 700 + 10 * ROUTES.index(route) + kv_heads)
    return dict(req=req, fp16=fp16, pool=pool, x=x,
                lay=C._with(lay, rope_theta=LORA_THETA, layer_idx=1, lora=adapters(kv_heads), lora_ids=LORA_IDS[route]))


LORA_MODEL_CASES = [(r, kv) for r in MODEL_ROUTES for kv in LORA_KV]


def lora_model_case(route, kv_heads):
    params = [C.layer_params(kv_heads, 2 + i) for i in range(C.LAYERS)]
    layers = [(f, C._with(lay, rope_theta=LORA_THETA, layer_idx=i, lora=adapters(kv_heads), lora_ids=LORA_IDS[route])) for i, (f, lay) in enumerate(params)]
    return _model_case(route, kv_heads, 800 + 10 * ROUTES.index(route) + kv_heads, _model_rest(62 + kv_heads), layers)
