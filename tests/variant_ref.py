"""Staged restatements of the two other decoder layers that are served as they are -- MixtralDecoderLayer (atom_amd/e2e/mixtral.py)
and LlamaDecoderLayerWithLora with adapters set (atom_amd/e2e/llama_lora.py) -- and of the models around them (checker side only):
numpy, the oracle and FP64 on top of tests/layer_ref.py's attention half and, for the router and the combine, tests/moe_ref.py (torch
on the CPU).  Nothing of ``atom_amd``.  Written from the two modules' docstrings and the arithmetic they cite:

Mixtral (qMixtralLayer.py:283-436): the attention half of the Llama layer, then
    gate_in = w2 * f16(residual1 * rsqrt(mean(residual1^2) + eps))     the UN-quantised post-attention norm, original channel order
    router_logits = gate_in @ gate.weight^T (fp16)                     route = top_k of the softmax, renormalised, fp16; the tables
    gate, up [T * top_k, F]: routed row r = token row_token[r]'s norm2 codes against ITS expert's w13 (w1 rows, then w3 rows)
    act = quant(silu(gate) * up)      y = down per expert      out = residual1 + sum_k half(y[slot_row[t, k]] * w[t, k]) (fp16 adds)

LoRA: the layer docstring's op sequence; for a targeted projection y += f16(x A^T) B'^T on the rows of a sequence with an adapter id
>= 0 (prefill requests first, then decode rows), A / B' that adapter's at THIS layer, B' = f16(B * alpha / r) as LoraWeight.load
rounds it.  x: the un-quantised input norm in original order (q, k, v), the raw attention output (o), the un-quantised post-attention
norm (gate, up), fp16 silu(gate) * up of the adapted gate / up (down).  k / v are quantised AFTER their adapters: the cache holds them.

``*_forward`` computes a trace free-running, ``*_check`` recomputes every stage from the trace's own previous stage, as
tests/layer_ref.py does; ``wrong=name`` applies one wiring error (MIXTRAL_WRONG / LORA_WRONG: name -> the first stage that must
report it; the attention-half names of layer_ref.WRONG are taken too).  tests/test_variant_ref_cpu.py shows that each is reported.

Trace formats beyond layer_ref's.  ``route``: dict(ids int [T, top_k], w fp16 [T, top_k], expert_indptr [E + 1], row_token [R],
slot_row [T, top_k], tile_expert / tile_row0 [n_tiles], n_tiles).  LoRA: ``k_lora`` / ``v_lora`` are the fp16 rows after the adapter,
``k`` / ``v`` their codes as in layer_ref; ``d_x`` is the fp16 operand of down_proj's adapter (checked under stage ``d``).

Bounds and their sources:
  gate_in, xn, n         2 fp16 ulps of the FP64 value (layer_ref._final_norm: the same two roundings)
  router_logits          layer_ref._check_logits
  route                  ids and every table exact against moe_ref.route / moe_ref.tables on the observed logits, weights within one
                         fp16 ulp (tests/test_gpu_moe.py: _check_router)
  gate, up, y, *_base    layer_ref.gemm_bound on the exact sums of the whole stage
  act                    layer_ref._quant_close
  out (Mixtral)          bit for bit against moe_ref.combine on the observed operands (tests/test_gpu_moe.py, the combine tests)
  q, k_lora, v_lora, o, gate, up, d (LoRA)   rows without an adapter: the base rows bit for bit; the others |err| <= 5e-3 + 5e-3 |ref|
                         against FP64 base_observed + f16(x A^T) B'^T (tests/test_gpu_lora.py:
                         test_add_lora_random_inputs_within_the_reference_tests_tolerance); for d, x is the OBSERVED operand, which is
                         itself held within 2 fp16 ulps of FP64 silu(gate) * up (torch rounds silu and the product: 1 + 1/2 ulp)
  k, v (LoRA)            bit for bit against O.quant_o4 of the observed fp16 rows (tests/test_gpu_kv.py:
                         test_u4_head_quantiser_on_planted_vectors, the "kv_quant_u4 + append_kv_i4" entry)
  out (LoRA)             |out - (residual1 + d)| <= 2^-11 |residual1 + d|: one fp16 rounding of an exactly known sum
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import atom_oracle as O
from tests import layer_ref as R
from tests import moe_ref

f16, f32, f64 = R.f16, R.f32, R.f64

ATTN_WRONG = {n: s for n, s in R.WRONG.items() if s in R.ATTN_STAGES}

# ==================================================================================================== Mixtral
MOE_STAGES = ("gate_in", "router_logits", "route", "gate", "up", "act", "y", "out")
MIXTRAL_STAGES = R.ATTN_STAGES + MOE_STAGES
MIXTRAL_WRONG = {
    "router_reads_residual": "gate_in",             # no norm in front of the router
    "router_reads_reordered_norm": "gate_in",       # the norm in post_attention_layernorm's reorder_index order
    "router_reads_layer_input_norm": "gate_in",     # the norm of the layer input in place of residual1's
    "router_norm_without_weight": "gate_in",
    "weights_not_renormalised": "route",            # the full softmax's weights at the chosen experts
    "experts_on_token_order_rows": "gate",          # routed row r reads token r // top_k, not row_token[r]
    "moe_gate_up_swapped": "gate",                  # w3 rows first
    "combine_unweighted": "out",
    "combine_ignores_slot_row": "out",              # slot (t, k) reads row t * top_k + k
    "moe_residual_from_layer_input": "out",
}
TABLES = ("expert_indptr", "row_token", "slot_row", "tile_expert", "tile_row0")


def _norm16(x, w, eps):
    """(FP64 value, fp16 as the modules round it) of the un-quantised RMSNorm: layer_ref._final_norm"""
    return R._final_norm(x, w, eps)


def _check_ulps(got, ref, n):
    got = np.asarray(got, dtype=f16)
    if got.shape != ref.shape:
        return False, f"shape {got.shape}, expected {ref.shape}"
    d = np.abs(got.astype(f64) - ref) / R.ulp16(ref)
    return bool(d.max() <= n), f"up to {d.max():.3g} fp16 ulps off (bound {n})"


def _route(logits, top_k, experts, renormalise=True):
    lt = torch.from_numpy(np.ascontiguousarray(np.asarray(logits, dtype=f16)))
    ids, w = moe_ref.route(lt, top_k)
    if not renormalise:
        w = torch.gather(torch.softmax(lt.float(), dim=-1), 1, ids).half()
    tb = moe_ref.tables(ids, experts)
    out = dict(ids=ids.numpy().astype(np.int64), w=w.numpy(), n_tiles=int(tb["n_tiles"]))
    for key in TABLES:
        out[key] = np.asarray(tb[key], dtype=np.int64).reshape((-1, top_k) if key == "slot_row" else (-1,))
    return out


def routed_gemm(act, experts, indptr, rows):
    """float64 [R, N]: routed row r = the exact sums of row ``rows[r]`` of the quantiser stage ``act`` against the weight of the expert
    whose segment of ``indptr`` holds r"""
    rows = np.asarray(rows, dtype=np.int64)
    D = np.zeros((len(rows), experts[0]["q4"].shape[0]))
    for e, w in enumerate(experts):
        lo, hi = int(indptr[e]), int(indptr[e + 1])
        if hi > lo:
            D[lo:hi] = R.gemm({key: np.asarray(act[key])[rows[lo:hi]] for key in ("q4", "q8", "s4", "s8")}, w)
    return D


def _combine(y, route, w, slot_row, residual):
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)))
    return moe_ref.combine(t(y, f16), t(route["ids"], np.int64), t(w, f16), t(slot_row, np.int64), t(residual, f16)).numpy()


def moe_half(tr, lay, x, wrong=None):
    """the sparse MoE block's stages on the trace's residual1 / norm2, added to ``tr``.  ``lay["moe"]``: dict(gate_w fp16 [E, H],
    w13 / w2: the oracle's packed-weight dict per expert, top_k)"""
    moe, x = lay["moe"], np.asarray(x, dtype=f16)
    E, K = len(moe["w13"]), moe["top_k"]
    F = moe["w13"][0]["q4"].shape[0] // 2
    is_ = lambda name: wrong == name
    r1, T = tr["residual1"], x.shape[0]
    normed = _norm16(r1, lay["norm2_w"], lay["eps"])[1]
    if is_("router_reads_residual"):
        gate_in = r1
    elif is_("router_reads_reordered_norm"):
        gate_in = normed[:, np.asarray(lay["norm2_idx"]).astype(np.int64)]
    elif is_("router_reads_layer_input_norm"):
        gate_in = _norm16(x, lay["norm2_w"], lay["eps"])[1]
    elif is_("router_norm_without_weight"):
        gate_in = _norm16(r1, np.ones_like(lay["norm2_w"]), lay["eps"])[1]
    else:
        gate_in = normed
    tr["gate_in"] = np.ascontiguousarray(gate_in)
    tr["router_logits"] = (tr["gate_in"].astype(f64) @ np.asarray(moe["gate_w"], dtype=f16).astype(f64).T).astype(f16)
    rt = tr["route"] = _route(tr["router_logits"], K, E, renormalise=not is_("weights_not_renormalised"))
    rows = np.arange(T * K) // K if is_("experts_on_token_order_rows") else rt["row_token"]
    D = routed_gemm(tr["norm2"], moe["w13"], rt["expert_indptr"], rows)
    g, u = (D[:, F:], D[:, :F]) if is_("moe_gate_up_swapped") else (D[:, :F], D[:, F:])
    tr["gate"], tr["up"] = g.astype(f16), u.astype(f16)
    tr["act"] = O.silu_mul_quant(tr["gate"], tr["up"], "kernel", 1.0)
    tr["y"] = routed_gemm(tr["act"], moe["w2"], rt["expert_indptr"], np.arange(T * K)).astype(f16)
    w = np.ones_like(rt["w"]) if is_("combine_unweighted") else rt["w"]
    slot_row = np.arange(T * K).reshape(T, K) if is_("combine_ignores_slot_row") else rt["slot_row"]
    tr["out"] = _combine(tr["y"], rt, w, slot_row, x if is_("moe_residual_from_layer_input") else r1)
    return tr


def mixtral_forward(req, lay, pool, x, wrong=None):
    """One Mixtral decoder layer; arguments as layer_ref.forward, ``lay`` with "moe" (``moe_half``) and without the dense MLP's weights"""
    assert wrong is None or wrong in MIXTRAL_WRONG or wrong in R.WRONG
    return moe_half(R.attention_half(req, lay, pool, x, wrong), lay, x, wrong)


def check_moe_half(trace, inputs, put):
    lay, moe = inputs["lay"], inputs["lay"]["moe"]
    E, K = len(moe["w13"]), moe["top_k"]
    F = moe["w13"][0]["q4"].shape[0] // 2
    T = np.asarray(inputs["x"]).shape[0]
    put("gate_in", _check_ulps(trace["gate_in"], _norm16(trace["residual1"], lay["norm2_w"], lay["eps"])[0], 2))
    put("router_logits", R._check_logits(trace["router_logits"], trace["gate_in"], moe["gate_w"]))
    want, got = _route(trace["router_logits"], K, E), trace["route"]
    flat = lambda a: np.asarray(a).astype(np.int64).reshape(-1)
    bad = [key for key in ("ids",) + TABLES if not np.array_equal(flat(got[key]), flat(want[key]))]
    if int(got["n_tiles"]) != want["n_tiles"]:
        bad.append("n_tiles")
    gw = np.asarray(got["w"], dtype=f16)
    d = int(np.abs(R._ord16(gw) - R._ord16(want["w"])).max()) if gw.shape == want["w"].shape else -1
    put("route", (not bad and 0 <= d <= 1, f"tables that differ from the restated ones: {bad or 'none'}; weights up to {d} fp16 ulps off "
                  f"(bound 1); rows per expert {np.diff(want['expert_indptr']).tolist()}"))
    # (the later stages on the restated ids and tables -- the observed ones are these or the stage above has failed -- and the observed weights)
    D = routed_gemm(trace["norm2"], moe["w13"], want["expert_indptr"], want["row_token"])
    put("gate", R._check_gemm(trace["gate"], D[:, :F]))
    put("up", R._check_gemm(trace["up"], D[:, F:]))
    put("act", R._quant_close(trace["act"], O.silu_mul_quant(trace["gate"], trace["up"], "kernel", 1.0)))
    put("y", R._check_gemm(trace["y"], routed_gemm(trace["act"], moe["w2"], want["expert_indptr"], np.arange(T * K))))
    ref = _combine(trace["y"], want, gw if gw.shape == want["w"].shape else want["w"], want["slot_row"], trace["residual1"])
    same = R._bits_equal(trace["out"], ref)
    n = int((np.asarray(trace["out"], dtype=f16).view(np.uint16) != ref.view(np.uint16)).sum()) if np.shape(trace["out"]) == ref.shape else -1
    put("out", (same, f"against the fp16 combine of the observed y, weights and residual1: {n} elements differ (bound: none)"))


def mixtral_check(trace, inputs, report=None):
    """as layer_ref.check, for a Mixtral layer's trace"""
    missing = R.absent(trace, MIXTRAL_STAGES)
    if missing:
        return missing
    fails, put = R.reporter(report)
    R.check_attention_half(trace, inputs, put)
    check_moe_half(trace, inputs, put)
    return fails


# ==================================================================================================== LoRA
LORA_STAGES = ("norm1", "xn", "q_base", "q", "k_base", "k_lora", "v_base", "v_lora", "k", "v", "cache", "attn", "attn_q", "o_base", "o",
               "residual1", "norm2", "n", "gate_base", "gate", "up_base", "up", "act", "d_base", "d", "out")
LORA_WRONG = {
    "adapter_reads_reordered_norm": "q",            # A on the norm in input_layernorm's reorder_index order
    "adapter_reads_layer_input": "q",               # A on the layer input, no norm
    "alpha_ignored": "q",                           # B in place of B * alpha / r
    "adapter_of_layer_zero": "q",                   # every layer on layer 0 of the pools
    "prefill_ids_per_row": "q",                     # prefill row r takes ids[r] (no segment table)
    "decode_ids_from_front": "q",                   # the decode rows take ids[:decode] in place of ids[P:]
    "kv_delta_after_quantiser": "k",                # the cache holds the base k / v
    "o_adapter_reads_reordered_attn": "o",          # A of o_proj on the attention output in self_attn's reorder_index order
    "mlp_adapter_reads_residual": "gate",           # A of gate / up on residual1, no norm
    "down_adapter_reads_base_gate_up": "d",         # A of down_proj on silu(gate) * up from before the gate / up adapters
    "second_residual_from_layer_input": "out",
}
RTOL = ATOL = 5e-3


def row_ids(req, ids, wrong=None):
    """the adapter id of every row: ids[:P] per prefill request (its chunk's rows), then ids[P:] per decode row"""
    ids, P, D = [int(i) for i in ids], len(req.prefills), len(req.decodes)
    assert len(ids) >= P + D
    pre = [ids[s] for s, (_, n, _) in enumerate(req.prefills) for _ in range(n)]
    if wrong == "prefill_ids_per_row":
        pre = [ids[r] if r < len(ids) else -1 for r in range(req.doff)]
    dec = ids[:D] if wrong == "decode_ids_from_front" else ids[P:P + D]
    return np.array(pre + dec, dtype=np.int64)


def lora_delta(x, rids, lora, module, layer, scaled=True):
    """float64 [T, out]: f16(x A^T) B'^T per row, zero on rows without an adapter"""
    x = np.asarray(x, dtype=f16).astype(f64)
    s = lora["alpha"] / lora["rank"] if scaled else 1.0
    out = None
    for a in sorted(set(rids.tolist()) - {-1}):
        A, B = lora["adapters"][a][module][layer]
        Bs = (np.asarray(B, dtype=f16).astype(f64) * s).astype(f16).astype(f64)
        if out is None:
            out = np.zeros((x.shape[0], Bs.shape[0]))
        rows = np.nonzero(rids == a)[0]
        out[rows] = (x[rows] @ np.asarray(A, dtype=f16).astype(f64).T).astype(f16).astype(f64) @ Bs.T
    return out


def _adapted(base, delta, rids):
    y = np.array(base, dtype=f16)
    if delta is not None:
        rows = rids >= 0
        y[rows] = (y[rows].astype(f64) + delta[rows]).astype(f16)
    return y


def _silu_mul(gate, up):
    g, u = np.asarray(gate, dtype=f16).astype(f64), np.asarray(up, dtype=f16).astype(f64)
    return g / (1 + np.exp(-g)) * u


def lora_forward(req, lay, pool, x, wrong=None):
    """One Llama layer with adapters set.  ``lay``: layer_ref's, plus ``lora`` = dict(rank, alpha, adapters[id][module] = [(A fp16
    [r, in], B fp16 [out, r]) per layer]) and ``lora_ids`` (one id per sequence); every one of the seven projections is targeted."""
    assert wrong is None or wrong in LORA_WRONG or wrong in R.WRONG
    x = np.asarray(x, dtype=f16)
    W, nkv, hidden, lora = lay["w"], req.kv_heads, x.shape[1], lay["lora"]
    is_ = lambda name: wrong == name
    rids = row_ids(req, lay["lora_ids"], wrong)
    li = 0 if is_("adapter_of_layer_zero") else lay["layer_idx"]
    delta = lambda xin, module: lora_delta(xin, rids, lora, module, li, scaled=not is_("alpha_ignored"))
    tr = {}
    n1 = tr["norm1"] = O.rmsnorm_reorder_quant(x, lay["norm1_w"], lay["eps"], lay["norm1_idx"], "kernel", 1.0)
    xn = tr["xn"] = _norm16(x, lay["norm1_w"], lay["eps"])[1]
    xa = xn[:, np.asarray(lay["norm1_idx"]).astype(np.int64)] if is_("adapter_reads_reordered_norm") else x if is_("adapter_reads_layer_input") else xn
    for p, name in (("q", "q"), ("k", "k_lora"), ("v", "v_lora")):
        tr[p + "_base"] = R.gemm(n1, W[p]).astype(f16)
        tr[name] = _adapted(tr[p + "_base"], delta(xa, p + "_proj"), rids)
    late = is_("kv_delta_after_quantiser")
    tr["k"], tr["v"] = (R._o4(tr[p + ("_base" if late else "_lora")].astype(f64), nkv) for p in "kv")
    layer = 0 if is_("cache_layer_zero") else lay["layer_idx"]
    front = is_("mixed_rows_from_front")
    after = R.write_cache(req, pool, tr["k"], tr["v"], layer, swap=is_("kv_swapped"), decode_from_front=front)
    tr["cache"] = dict(buf=after[0], param=after[1])
    tr["attn"] = R.attention(req, tr["q"], after, layer, 1e4 if is_("theta_default") else lay["rope_theta"],
                             scale=1 / np.sqrt(hidden) if is_("softmax_scale_hidden") else None, swap=is_("kv_swapped"),
                             head_modulo=is_("gqa_head_modulo"), chunk_from_zero=is_("chunk_positions_from_zero"),
                             decode_plus_one=is_("decode_position_plus_one"), decode_from_front=front).astype(f16)
    aidx = np.asarray(lay["norm1_idx"] if is_("o_proj_uses_norm1_index") else lay["attn_idx"]).astype(np.int64)
    aq = tr["attn_q"] = O.reorder_quant(tr["attn"], aidx, "kernel", 1.0)
    tr["o_base"] = R.gemm(aq, W["o"]).astype(f16)
    oa = tr["attn"][:, np.asarray(lay["attn_idx"]).astype(np.int64)] if is_("o_adapter_reads_reordered_attn") else tr["attn"]
    tr["o"] = _adapted(tr["o_base"], delta(oa, "o_proj"), rids)
    r1 = tr["residual1"] = (tr["o"].astype(f32) + x.astype(f32)).astype(f16)
    n2 = tr["norm2"] = O.rmsnorm_reorder_quant(r1, lay["norm2_w"], lay["eps"], lay["norm2_idx"], "kernel", 1.0)
    n = tr["n"] = _norm16(r1, lay["norm2_w"], lay["eps"])[1]
    na = r1 if is_("mlp_adapter_reads_residual") else n
    for p in ("gate", "up"):
        tr[p + "_base"] = R.gemm(n2, W[p]).astype(f16)
        tr[p] = _adapted(tr[p + "_base"], delta(na, p + "_proj"), rids)
    act = tr["act"] = O.silu_mul_quant(tr["gate"], tr["up"], "kernel", 1.0)
    tr["d_base"] = R.gemm(act, W["down"]).astype(f16)
    b = "_base" if is_("down_adapter_reads_base_gate_up") else ""
    tr["d_x"] = _silu_mul(tr["gate" + b], tr["up" + b]).astype(f16)
    tr["d"] = _adapted(tr["d_base"], delta(tr["d_x"], "down_proj"), rids)
    res = x if is_("second_residual_from_layer_input") else r1
    tr["out"] = (tr["d"].astype(f32) + res.astype(f32)).astype(f16)
    return tr


def adapter_shares(trace, req, lay):
    """{module: rms(adapter delta) / rms(base output)} over the rows with an adapter, from a trace"""
    rows = row_ids(req, lay["lora_ids"]) >= 0
    rms = lambda a: float(np.sqrt((a ** 2).mean()))
    names = dict(q_proj=("q", "q_base"), k_proj=("k_lora", "k_base"), v_proj=("v_lora", "v_base"), o_proj=("o", "o_base"),
                 gate_proj=("gate", "gate_base"), up_proj=("up", "up_base"), down_proj=("d", "d_base"))
    return {m: rms(trace[a][rows].astype(f64) - trace[b][rows].astype(f64)) / rms(trace[b][rows].astype(f64)) for m, (a, b) in names.items()}


def _check_adapter(got, base, x, rids, lay, module):
    got, base = np.asarray(got, dtype=f16), np.asarray(base, dtype=f16)
    if got.shape != base.shape:
        return False, f"shape {got.shape}, expected {base.shape}"
    rows = rids >= 0
    plain = R._bits_equal(got[~rows], base[~rows])
    ref = base[rows].astype(f64) + lora_delta(x, rids, lay["lora"], module, lay["layer_idx"])[rows]
    err = np.abs(got[rows].astype(f64) - ref)
    used = (err / (ATOL + RTOL * np.abs(ref))).max()
    return bool(plain and used <= 1), (f"rows with an adapter: max|err| {err.max():.4g}, the largest err / (5e-3 + 5e-3 |ref|) is {used:.3g} (bound 1); "
                                       f"the {int((~rows).sum())} rows without one {'are' if plain else 'ARE NOT'} the base rows bit for bit")


def lora_check(trace, inputs, report=None):
    """as layer_ref.check, for a trace of the layer with adapters"""
    missing = R.absent(trace, LORA_STAGES + ("d_x",))
    if missing:
        return missing
    req, lay, x = inputs["req"], inputs["lay"], np.asarray(inputs["x"], dtype=f16)
    W, nkv = lay["w"], req.kv_heads
    rids = row_ids(req, lay["lora_ids"])
    fails, put = R.reporter(report)
    put("norm1", R._quant_exact(trace["norm1"], O.rmsnorm_reorder_quant(x, lay["norm1_w"], lay["eps"], lay["norm1_idx"], "kernel", 1.0)))
    put("xn", _check_ulps(trace["xn"], _norm16(x, lay["norm1_w"], lay["eps"])[0], 2))
    for p, name in (("q", "q"), ("k", "k_lora"), ("v", "v_lora")):
        put(p + "_base", R._check_gemm(trace[p + "_base"], R.gemm(trace["norm1"], W[p])))
        put(name, _check_adapter(trace[name], trace[p + "_base"], trace["xn"], rids, lay, p + "_proj"))
    for p in "kv":
        want = R._o4(np.asarray(trace[p + "_lora"], dtype=f16).astype(f64), nkv)
        same = (np.array_equal(np.asarray(trace[p]["codes"]).reshape(want["codes"].shape), want["codes"])
                and R._bits_equal(np.asarray(trace[p]["sz"]).reshape(want["sz"].shape), want["sz"]))
        put(p, (same, f"codes and (scale, zero) against the u4 quantiser of the observed adapted {p}: "
                f"{int((np.asarray(trace[p]['codes']).reshape(want['codes'].shape) != want['codes']).sum())} bytes differ (bound: none)"))
    R.check_attention_core(trace, inputs, put)
    put("o_base", R._check_gemm(trace["o_base"], R.gemm(trace["attn_q"], W["o"])))
    put("o", _check_adapter(trace["o"], trace["o_base"], trace["attn"], rids, lay, "o_proj"))
    r1 = (np.asarray(trace["o"], dtype=f16).astype(f32) + x.astype(f32)).astype(f16)
    put("residual1", (R._bits_equal(trace["residual1"], r1), "against the fp16 sum of the layer input and the adapted o_proj output"))
    put("norm2", R._quant_exact(trace["norm2"], O.rmsnorm_reorder_quant(trace["residual1"], lay["norm2_w"], lay["eps"], lay["norm2_idx"],
                                                                        "kernel", 1.0)))
    put("n", _check_ulps(trace["n"], _norm16(trace["residual1"], lay["norm2_w"], lay["eps"])[0], 2))
    for p in ("gate", "up"):
        put(p + "_base", R._check_gemm(trace[p + "_base"], R.gemm(trace["norm2"], W[p])))
        put(p, _check_adapter(trace[p], trace[p + "_base"], trace["n"], rids, lay, p + "_proj"))
    put("act", R._quant_close(trace["act"], O.silu_mul_quant(trace["gate"], trace["up"], "kernel", 1.0)))
    put("d_base", R._check_gemm(trace["d_base"], R.gemm(trace["act"], W["down"])))
    ok_x, msg_x = _check_ulps(trace["d_x"], _silu_mul(trace["gate"], trace["up"]), 2)
    ok_d, msg_d = _check_adapter(trace["d"], trace["d_base"], trace["d_x"], rids, lay, "down_proj")
    put("d", (ok_x and ok_d, f"the adapter's operand against silu(gate) * up: {msg_x}; {msg_d}"))
    ref = np.asarray(trace["d"], dtype=f16).astype(f64) + np.asarray(trace["residual1"], dtype=f16).astype(f64)
    err = np.abs(np.asarray(trace["out"], dtype=f16).astype(f64) - ref)
    over = err - 2.0 ** -11 * np.abs(ref)
    put("out", (bool(over.max() <= 0), f"{int((over > 0).sum())} elements outside 2^-11 |residual1 + d|, max|err| {err.max():.4g}"))
    return fails
