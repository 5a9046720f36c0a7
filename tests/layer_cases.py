"""The inputs of the staged layer / model checks, shared by tests/test_layer_ref_cpu.py (which shows that tests/layer_ref.py's checker
reports every wiring error on them) and tests/test_gpu_layer_ref.py (which holds the HIP layer to the same checker): numpy only.
Hidden 512, 4 query heads of 128, intermediate 1408, 2 layers, pages of 16 tokens; every layer case runs at layer_idx 1 over a pool
filled with random bytes, on page lists in a scrambled order.

Routes (``layer_case(route, kv_heads)``; kv_heads 4 = MHA, 2 and 1 = grouped-query, 2 being the one where h // G and h % kv_heads differ):
  A  prefill from empty caches, lengths 37, 16, 1
  B  chunked prefill: prefixes 16, 5, 0 in the cache from a first call (``first``), chunks 21, 12, 7
  C  decode only: lengths 16, 17, 33 (the last slot of a page, the first of a new one, the first of a third)
  D  mixed: prefills of 5 and 17 tokens plus decode requests of lengths 20 and 16, one batch
  E  rope_theta 5e5 on a mixed batch with cached prefixes: B's chunks plus D's decode requests
"""
import functools

import numpy as np

from oracle import atom_oracle as O
from tests.layer_ref import Requests

HIDDEN, HEADS, INTER, LAYERS, PAGE, VOCAB, EPS = 512, 4, 1408, 2, 16, 1000, 1e-5
CAPACITY = 12
ROUTES = ("A", "B", "C", "D", "E")
KV_HEADS = (4, 2, 1)

_PREFILLS = {"A": [(0, 37), (0, 16), (0, 1)], "B": [(16, 21), (5, 12), (0, 7)], "C": [], "D": [(0, 5), (0, 17)], "E": [(16, 21), (5, 12), (0, 7)]}
_DECODES = {"A": [], "B": [], "C": [16, 17, 33], "D": [20, 16], "E": [20, 16]}


def proj_shapes(kv_heads):
    kv = kv_heads * 128
    return dict(q=(HIDDEN, HIDDEN), k=(kv, HIDDEN), v=(kv, HIDDEN), o=(HIDDEN, HIDDEN), gate=(INTER, HIDDEN), up=(INTER, HIDDEN),
                down=(HIDDEN, INTER))


@functools.lru_cache(maxsize=None)
def layer_params(kv_heads, seed):
    """One layer's parameters: ``fp16`` (what the GPU test loads: projection weights, norm weights, the three reorder indices) and
    ``lay`` (what tests/layer_ref.py takes: the same with the weights through the oracle's packer; rope_theta / layer_idx set per case)."""
    g = np.random.default_rng(1000 * seed + kv_heads)
    fp16 = {name: (g.standard_normal(shape) * 0.05).astype(np.float16) for name, shape in proj_shapes(kv_heads).items()}
    for name in ("norm1_w", "norm2_w"):
        fp16[name] = (1 + 0.1 * g.standard_normal(HIDDEN)).astype(np.float16)
    for name in ("norm1_idx", "norm2_idx", "attn_idx"):
        fp16[name] = g.permutation(HIDDEN).astype(np.int16)
    lay = {name: fp16[name] for name in ("norm1_w", "norm2_w", "norm1_idx", "norm2_idx", "attn_idx")}
    lay["w"] = {name: O.quant_weight_sim(fp16[name], 0.85, 2) for name in proj_shapes(kv_heads)}
    lay["eps"] = EPS
    return fp16, lay


def _with(lay, **kw):
    out = dict(lay)
    out.update(kw)
    return out


def random_pool(kv_heads, seed):
    """(buf, param): random codes and (scale, zero) in every slot of every page and layer"""
    g = np.random.default_rng(seed)
    shape = (CAPACITY, LAYERS, 2, kv_heads, PAGE)
    buf = g.integers(0, 256, size=shape + (64,), dtype=np.uint8)
    param = (g.random(shape + (2,)) * 0.2 + 0.01).astype(np.float16)
    return buf, param


def requests(route, kv_heads, seed):
    """(the call's Requests, the Requests of the call that writes the prefixes or None)"""
    pages = [int(p) for p in np.random.default_rng(seed).permutation(CAPACITY)]
    take = lambda n: [pages.pop() for _ in range(-(-n // PAGE))]
    pre = [(a, n, take(a + n)) for a, n in _PREFILLS[route]]
    dec = [(s, take(s)) for s in _DECODES[route]]
    first = [(0, a, pg[:-(-a // PAGE)]) for a, n, pg in pre if a > 0]
    return (Requests(pre, dec, HEADS, kv_heads, PAGE), Requests(first, [], HEADS, kv_heads, PAGE) if first else None)


def layer_case(route, kv_heads):
    """dict(req, first, fp16, lay, pool, x, x_first): everything one layer call takes, on both sides"""
    seed = 7 + 10 * ROUTES.index(route) + kv_heads
    fp16, lay = layer_params(kv_heads, 1)
    req, first = requests(route, kv_heads, seed)
    g = np.random.default_rng(seed + 100)
    x = (g.standard_normal((req.rows, HIDDEN)) * 0.7).astype(np.float16)
    x_first = None if first is None else (g.standard_normal((first.rows, HIDDEN)) * 0.7).astype(np.float16)
    return dict(req=req, first=first, fp16=fp16, lay=_with(lay, rope_theta=5e5 if route == "E" else 1e4, layer_idx=1),
                pool=random_pool(kv_heads, seed + 200), x=x, x_first=x_first)


LAYER_CASES = [(r, kv) for r in ("A", "B", "C", "D") for kv in KV_HEADS] + [("E", 2)]


@functools.lru_cache(maxsize=None)
def model_params(kv_heads):
    g = np.random.default_rng(50 + kv_heads)
    fp16 = dict(embed=g.standard_normal((VOCAB, HIDDEN)).astype(np.float16), head=(g.standard_normal((VOCAB, HIDDEN)) * 0.05).astype(np.float16),
                norm_w=(1 + 0.1 * g.standard_normal(HIDDEN)).astype(np.float16))
    layers = [layer_params(kv_heads, 2 + i) for i in range(LAYERS)]
    mdl = dict(embed=fp16["embed"], head=fp16["head"], norm_w=fp16["norm_w"], eps=EPS,
               layers=[_with(lay, rope_theta=1e4, layer_idx=i) for i, (_, lay) in enumerate(layers)])
    fp16["layers"] = [f for f, _ in layers]
    return fp16, mdl


MODEL_CASES = [(r, kv) for r in ("A", "C") for kv in (4, 2)]


def model_case(route, kv_heads):
    seed = 300 + 10 * ROUTES.index(route) + kv_heads
    fp16, mdl = model_params(kv_heads)
    req, first = requests(route, kv_heads, seed)
    assert first is None
    ids = np.random.default_rng(seed).integers(0, VOCAB, size=req.rows)
    return dict(req=req, fp16=fp16, mdl=mdl, pool=random_pool(kv_heads, seed + 200), ids=ids)
