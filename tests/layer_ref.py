"""A staged restatement of the real-kernel Llama decoder layer and of the model around it (checker side only): numpy, the oracle and
FP64, nothing of ``atom_amd`` and no torch.  Written from the docstrings of ``atom_amd/e2e/llama.py`` and the reference's call order
(llama.py:247-292):

    norm1 = quant(reorder(RMSNorm(x)))        q = q_proj(norm1)   k, v = k_proj(norm1), v_proj(norm1) with the u4 epilogue
    cache: k / v codes of every row into the pages of its request, at the row's absolute position, in THIS layer's slice of the pool
    attn  = causal attention over the de-quantised cache: RoPE(rope_theta) on q and on every key at its own position, scale
            1 / sqrt(128), query head h on K/V head h // G; a chunk's rows at positions prefix .. prefix + len - 1, a decode row at
            length - 1
    attn_q = quant(reorder(attn)) with the ATTENTION's index      o = o_proj(attn_q)
    residual1 = x + o (fp16)     norm2 = quant(reorder(RMSNorm(residual1)))
    gate, up = gate_proj(norm2), up_proj(norm2)     act = quant(silu(gate) * up)     out = down_proj(act) + residual1

Rows of a batch: the prefill requests' chunks first, in order, then one row per decode request.  Which row sits at which position and
in which cache slot comes from a ``Requests`` description alone (prefix, chunk length and page list per prefill request; length and
page list per decode request), never from device-side page tables.

``forward`` computes a trace (stage name -> arrays) free-running; ``check`` takes a trace -- this module's or one captured from the
HIP ops -- and recomputes EVERY stage from the trace's own output of the stage before it (teacher forcing: a flipped INT4 code cannot
compound), compares with the stage's bound and returns the failures.  ``forward(..., wrong=name)`` applies one deliberate wiring
error; tests/test_layer_ref_cpu.py shows that ``check`` reports each of them, on the inputs the GPU tests use.

Both come in two halves that the other decoder layers reuse (tests/variant_ref.py: Mixtral, LoRA): the attention half, norm1 ..
residual1 and norm2 (``attention_half``, ``check_attention_half``), and the dense-MLP half, gate .. out (``mlp_half``,
``check_mlp_half``); ``model_forward`` / ``check_model`` take the layer-level pair as a parameter.

Trace formats.  A quantiser stage is the oracle's dict: q4 int8 [T, K - 128], q8 int8 [T, 128], s4 fp16 [T, G], s8 fp16 [T].  ``k`` /
``v``: dict(codes uint8 [T, kv_heads * 64], sz fp16 [T, kv_heads, 2] = (scale, zero)).  ``cache``: dict(buf, param), the WHOLE pool
after the call.  Every other stage is an fp16 array [T, features].

The bounds (``check``), with their sources:
  norm1, attn_q, residual1, norm2   bit for bit (tests/test_gpu_quant.py: _check_tail(exact=True), test_add_rmsnorm_is_add_then_rmsnorm)
  q, o, gate, up                    max|err| <= 2e-3 * rms(D) + 1e-3 * max|D| against the exact sums D (tests/test_gpu_e2e.py)
  k, v                              see ``_check_o4``
  cache                             bit for bit over the whole pool: bytes and (scale, zero), other layers and pages included
  attn                              4e-3 * max|ref| + 1e-3 on prefill rows (tests/test_gpu_prefill_i4.py: _bound), 2e-3 * max|ref| + 1e-3
                                    on decode rows (tests/test_gpu_kv.py), max|ref| over the rows of that kind
  act                               codes within 1, fewer than 2e-3 of them off, scales within one fp16 ulp (_check_tail(exact=False))
  out                               |out - (D_down + residual1)| <= (the GEMM bound on D_down) + 2^-11 * |D_down + residual1|: the
                                    projection's fp16 rounding is inside the GEMM bound, the add rounds to fp16 once more (half an ulp
                                    is at most 2^-11 relative)
Model level (``check_model``): see ``_final_norm`` and ``_check_logits``.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import atom_oracle as O

f16, f32, f64 = np.float16, np.float32, np.float64
HEAD = 128

LAYER_STAGES = ("norm1", "q", "k", "v", "cache", "attn", "attn_q", "o", "residual1", "norm2", "gate", "up", "act", "out")

# name -> the first stage at which ``check`` must report it (model-level stages: "final_norm", "logits")
WRONG = {
    "kv_swapped": "cache",                         # K and V exchanged in the cache write AND the cache read: attention is unchanged
    "cache_layer_zero": "cache",                   # every layer on layer 0 of the pool (the reference's "Hack for memory")
    "theta_default": "attn",                       # rope_theta ignored: 1e4
    "softmax_scale_hidden": "attn",                # 1 / sqrt(hidden) in place of 1 / sqrt(128)
    "o_proj_uses_norm1_index": "attn_q",           # the reorder quantiser in front of o_proj with input_layernorm's index
    "gate_up_swapped": "gate",
    "second_residual_from_layer_input": "out",     # down + x in place of down + residual1
    "chunk_positions_from_zero": "attn",           # a chunk's queries at 0 .. len - 1 although its cache holds a prefix
    "decode_position_plus_one": "attn",            # a decode query at position length
    "gqa_head_modulo": "attn",                     # query head h on K/V head h % kv_heads
    "mixed_rows_from_front": "cache",              # the decode requests' rows taken from the front of a mixed batch
    "no_final_norm": "final_norm",
    "head_before_norm": "logits",                  # lm_head on the un-normed stream, the norm on the returned hidden states only
}
MODEL_WRONG = ("no_final_norm", "head_before_norm")


@dataclasses.dataclass
class Requests:
    """prefills: (cached-prefix length, chunk length, page list) per prefill request; decodes: (length, page list) per decode request
    (the length counts the token of this step).  A page list holds exactly the pages of the request's length after the call."""
    prefills: list
    decodes: list
    heads: int
    kv_heads: int
    page: int = 16

    def __post_init__(self):
        for s, pages in [(a + n, pg) for a, n, pg in self.prefills] + list(self.decodes):
            assert s >= 1 and len(pages) == -(-s // self.page), (s, pages)
        assert self.heads % self.kv_heads == 0

    @property
    def doff(self):
        return sum(n for _, n, _ in self.prefills)

    @property
    def rows(self):
        return self.doff + len(self.decodes)

    def prefill_tables(self):
        """(indptr, indices, last_page_offset, append_indptr) of the prefill requests, from the description"""
        return _tables([(a + n, pg) for a, n, pg in self.prefills], self.page) + (np.cumsum([0] + [n for _, n, _ in self.prefills]),)

    def decode_tables(self):
        return _tables(self.decodes, self.page)


def _tables(seqs, page):
    indptr = np.cumsum([0] + [len(pg) for _, pg in seqs]).astype(np.int32)
    indices = np.array([p for _, pg in seqs for p in pg], dtype=np.int32)
    lpo = np.array([(s - 1) % page + 1 for s, _ in seqs], dtype=np.int32)
    return indptr, indices, lpo


# ---------------------------------------------------------------------------------------------------- small numerics
def ulp16(x):
    """the spacing of fp16 numbers at |x| (2^-24 below the smallest normal), float64"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, dtype=f64)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _ord16(a):
    """fp16 -> integers in the order of the values: neighbouring numbers differ by one"""
    b = np.ascontiguousarray(np.asarray(a, dtype=f16)).view(np.int16).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFF), b)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(np.asarray(a, dtype=f16)), np.ascontiguousarray(np.asarray(b, dtype=f16))
    return a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16))


def gemm(act, w):
    """the exact sums of a projection on a quantiser stage's codes, float64 [T, N]"""
    return O.gemm_w4a4_exact(act["q4"], w["q4"], act["s4"], w["s4"], act["q8"], w["q8"], act["s8"], w["s8"])


def gemm_abs(act, w):
    """sum over the G + 1 K steps of |integer dot x scales|, float64 [T, N]: what an FP32 accumulation error is relative to"""
    G = act["s4"].shape[1]
    A = np.zeros((act["q4"].shape[0], w["q4"].shape[0]))
    for g in range(G):
        sl = slice(g * 128, (g + 1) * 128)
        dot = act["q4"][:, sl].astype(f64) @ w["q4"][:, sl].astype(f64).T
        A += np.abs(dot) * act["s4"][:, g].astype(f64)[:, None] * w["s4"][g].astype(f64)[None, :]
    dot = act["q8"].astype(f64) @ w["q8"].astype(f64).T
    return A + np.abs(dot) * act["s8"].astype(f64)[:, None] * w["s8"].astype(f64)[None, :]


def gemm_bound(D):
    return 2e-3 * np.sqrt((D ** 2).mean()) + 1e-3 * np.abs(D).max()


def _o4(D, kv_heads):
    codes, sz = O.quant_o4(D.astype(f32))
    return dict(codes=codes, sz=sz.reshape(D.shape[0], kv_heads, 2))


def _nibbles(codes):
    """uint8 [.., 64] -> float64 [.., 128], element 2j in the low nibble"""
    c = np.asarray(codes, dtype=np.uint8)
    u = np.empty(c.shape[:-1] + (c.shape[-1] * 2,))
    u[..., 0::2] = c & 0xF
    u[..., 1::2] = c >> 4
    return u


def rope(x, pos, theta):
    """x float64 [S, 128] at absolute positions pos [S]: pairs (i, i + 64) turned by pos * theta^(-2i / 128)"""
    ang = np.asarray(pos, dtype=f64)[:, None] * theta ** (-np.arange(0, HEAD, 2) / HEAD)[None, :]
    c, s = np.cos(ang), np.sin(ang)
    a, b = x[:, :HEAD // 2], x[:, HEAD // 2:]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=1)


# ---------------------------------------------------------------------------------------------------- cache and attention
def write_cache(req, pool, k, v, layer, *, swap=False, decode_from_front=False):
    """(buf, param) after the call: the rows' k / v codes appended at the described slots (O.kv_append_i4) of ``layer``"""
    buf, param = pool[0].copy(), pool[1].copy()
    nkv = req.kv_heads
    parts = [t.reshape(req.rows, nkv, -1) for t in (k["codes"], v["codes"], k["sz"], v["sz"])]
    if swap:
        parts = [parts[1], parts[0], parts[3], parts[2]]
    doff, nd = req.doff, len(req.decodes)
    if req.prefills:
        indptr, indices, lpo, app = req.prefill_tables()
        O.kv_append_i4(buf, param, indptr, indices, lpo, *[t[:doff] for t in parts], layer, app)
    if nd:
        rows = slice(0, nd) if decode_from_front else slice(doff, doff + nd)
        O.kv_append_i4(buf, param, *req.decode_tables(), *[t[rows] for t in parts], layer, None)
    return buf, param


def attention(req, q, pool, layer, theta, *, scale=None, swap=False, head_modulo=False, chunk_from_zero=False, decode_plus_one=False,
              decode_from_front=False):
    """float64 [T, heads * 128]: causal attention of every row over its request's de-quantised cache (after this call's append)"""
    buf, param = pool
    nh, nkv, P = req.heads, req.kv_heads, req.page
    G = nh // nkv
    scale = 1 / np.sqrt(HEAD) if scale is None else scale
    qf = np.asarray(q, dtype=f16).astype(f64).reshape(req.rows, nh, HEAD)
    out = np.zeros((req.rows, nh, HEAD))
    jobs, r = [], 0                                               # (query rows, output rows, query positions, length, pages)
    for prefix, n, pages in req.prefills:
        pos = np.arange(n) + (0 if chunk_from_zero else prefix)
        jobs.append((np.arange(r, r + n), np.arange(r, r + n), pos, prefix + n, pages))
        r += n
    for i, (length, pages) in enumerate(req.decodes):
        jobs.append((np.array([i if decode_from_front else r + i]), np.array([r + i]), np.array([length - 1 + (1 if decode_plus_one else 0)]),
                     length, pages))
    ik, iv = (1, 0) if swap else (0, 1)
    for qrows, orows, pos, S, pages in jobs:
        pg = np.asarray(pages, dtype=np.int64)
        for h in range(nh):
            hk = h % nkv if head_modulo else h // G
            kc = buf[pg, layer, ik, hk].reshape(-1, HEAD // 2)[:S]
            vc = buf[pg, layer, iv, hk].reshape(-1, HEAD // 2)[:S]
            kp = param[pg, layer, ik, hk].reshape(-1, 2)[:S].astype(f64)
            vp = param[pg, layer, iv, hk].reshape(-1, 2)[:S].astype(f64)
            kf = rope(_nibbles(kc) * kp[:, :1] - kp[:, 1:], np.arange(S), theta)
            vf = _nibbles(vc) * vp[:, :1] - vp[:, 1:]
            s = rope(qf[qrows, h], pos, theta) @ kf.T * scale
            s[np.arange(S)[None, :] > pos[:, None]] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[orows, h] = (p / p.sum(axis=1, keepdims=True)) @ vf
    return out.reshape(req.rows, nh * HEAD)


# ---------------------------------------------------------------------------------------------------- the layer, free-running
ATTN_STAGES = LAYER_STAGES[:LAYER_STAGES.index("gate")]          # the attention half: norm1 .. residual1, norm2
MLP_STAGES = LAYER_STAGES[len(ATTN_STAGES):]                     # the dense-MLP half: gate, up, act, out


def attention_half(req, lay, pool, x, wrong=None):
    """norm1 .. residual1, norm2 of one decoder layer (what every variant of the layer shares); arguments as ``forward``"""
    x = np.asarray(x, dtype=f16)
    assert x.shape[0] == req.rows
    W, nkv, hidden = lay["w"], req.kv_heads, x.shape[1]
    is_ = lambda name: wrong == name
    tr = {}
    n1 = tr["norm1"] = O.rmsnorm_reorder_quant(x, lay["norm1_w"], lay["eps"], lay["norm1_idx"], "kernel", 1.0)
    tr["q"] = gemm(n1, W["q"]).astype(f16)
    tr["k"], tr["v"] = _o4(gemm(n1, W["k"]), nkv), _o4(gemm(n1, W["v"]), nkv)
    layer = 0 if is_("cache_layer_zero") else lay["layer_idx"]
    front = is_("mixed_rows_from_front")
    after = write_cache(req, pool, tr["k"], tr["v"], layer, swap=is_("kv_swapped"), decode_from_front=front)
    tr["cache"] = dict(buf=after[0], param=after[1])
    theta = 1e4 if is_("theta_default") else lay["rope_theta"]
    tr["attn"] = attention(req, tr["q"], after, layer, theta, scale=1 / np.sqrt(hidden) if is_("softmax_scale_hidden") else None,
                           swap=is_("kv_swapped"), head_modulo=is_("gqa_head_modulo"), chunk_from_zero=is_("chunk_positions_from_zero"),
                           decode_plus_one=is_("decode_position_plus_one"), decode_from_front=front).astype(f16)
    idx = lay["norm1_idx"] if is_("o_proj_uses_norm1_index") else lay["attn_idx"]
    aq = tr["attn_q"] = O.reorder_quant(tr["attn"], idx, "kernel", 1.0)
    tr["o"] = gemm(aq, W["o"]).astype(f16)
    tr["residual1"] = (tr["o"].astype(f32) + x.astype(f32)).astype(f16)
    tr["norm2"] = O.rmsnorm_reorder_quant(tr["residual1"], lay["norm2_w"], lay["eps"], lay["norm2_idx"], "kernel", 1.0)
    return tr


def mlp_half(tr, lay, x, wrong=None):
    """gate, up, act, out of the dense MLP on the trace's norm2 / residual1, added to ``tr``"""
    W, n2 = lay["w"], tr["norm2"]
    is_ = lambda name: wrong == name
    g, u = ("up", "gate") if is_("gate_up_swapped") else ("gate", "up")
    tr["gate"], tr["up"] = gemm(n2, W[g]).astype(f16), gemm(n2, W[u]).astype(f16)
    act = tr["act"] = O.silu_mul_quant(tr["gate"], tr["up"], "kernel", 1.0)
    res = np.asarray(x, dtype=f16) if is_("second_residual_from_layer_input") else tr["residual1"]
    tr["out"] = (gemm(act, W["down"]).astype(f16).astype(f32) + res.astype(f32)).astype(f16)
    return tr


def forward(req, lay, pool, x, wrong=None):
    """One decoder layer.  ``lay``: dict(w = {projection: the oracle's packed-weight dict}, norm1_w, norm1_idx, norm2_w, norm2_idx,
    attn_idx, eps, rope_theta, layer_idx); ``pool``: (buf, param) from before the call (not modified); ``x`` fp16 [T, hidden].
    Returns the trace.  ``wrong``: one name of WRONG (a model-level name changes nothing here)."""
    assert wrong is None or wrong in WRONG
    return mlp_half(attention_half(req, lay, pool, x, wrong), lay, x, wrong)


# ---------------------------------------------------------------------------------------------------- the checker
def _quant_exact(got, want):
    for key in ("q4", "q8"):
        if got[key].shape != want[key].shape or not np.array_equal(got[key], want[key]):
            n = int((np.asarray(got[key]) != want[key]).sum()) if got[key].shape == want[key].shape else -1
            return False, f"{key}: {n} codes differ"
    for key in ("s4", "s8"):
        if not _bits_equal(got[key], want[key]):
            return False, f"{key}: scales differ"
    return True, "bit for bit"


def _quant_close(got, want):
    """tests/helpers.py: _check_tail(exact=False)"""
    ok, text = True, []
    for key in ("q4", "q8"):
        d = np.abs(got[key].astype(np.int32) - want[key])
        ok = ok and d.max() <= 1 and (d > 0).mean() < 2e-3
        text.append(f"{key}: largest code distance {int(d.max())}, share off {(d > 0).mean():.3g} (bounds 1, 2e-3)")
    for key in ("s4", "s8"):
        d = np.abs(_ord16(got[key]) - _ord16(want[key])).max()
        ok = ok and d <= 1
        text.append(f"{key}: scales up to {int(d)} fp16 ulps off (bound 1)")
    return bool(ok), "; ".join(text)


def _check_gemm(got, D):
    err = np.abs(np.asarray(got, dtype=f16).astype(f64) - D).max()
    return bool(err <= gemm_bound(D)), f"max|err| {err:.4g}, bound {gemm_bound(D):.4g} (rms {np.sqrt((D ** 2).mean()):.4g}, max {np.abs(D).max():.4g})"


def _check_o4(got, D, A, steps):
    """The u4 epilogue of k_proj / v_proj on a stage whose FP32 sums D32 differ from the exact D in the last bits, so that a code at
    a rounding boundary may legitimately differ: a bound on VALUES, every element, no excluded share.  Per 128-group (one head of one row)
    the kernel takes scale32 = (max D32 - min D32) / 15, zero32 = -min D32, code = clamp(round((D32 + zero32) * (1 / scale32)), 0, 15) and
    stores scale = f16(scale32), zero = f16(zero32) (oracle.quant_o4).
      1. scale and zero are within ONE fp16 ulp of f16((max D - min D) / 15) and f16(-min D) (the accumulation error, far below half an
         fp16 ulp, can move a rounding by one).
      2. |code * scale - zero - D| <= scale / 2 + t for every element.  With u = (D32 + zero32) / scale32 the code is within
         1/2 + 45 * 2^-24 of u (three FP32 roundings on a number of at most 15), so |code * scale32 - zero32 - D32| <= scale32 / 2 up to
         2.7e-6 scale32.  Replacing scale32, zero32, D32 by what is stored and by D adds code * |scale - scale32| <= 15 * ulp16(scale) / 2,
         |zero - zero32| <= ulp16(zero) / 2, scale32 / 2 <= scale / 2 + ulp16(scale) / 4 and |D32 - D|.  The allowance is one whole ulp
         where half is owed -- it absorbs the FP32 terms above -- and for |D32 - D| the accumulation bound of G + 1 fused
         multiply-adds in any order, (G + 1) * 2^-24 * sum|term| (gemm_abs; the largest of the group):
             t = ulp16(zero) + 15 * ulp16(scale) + (G + 1) * 2^-24 * max_group sum|term|
         (the ulps taken at the larger of the stored and the restated number).  Nothing in it was measured on the GPU."""
    T, N = D.shape
    Dg, Ag = D.reshape(T, N // HEAD, HEAD), A.reshape(T, N // HEAD, HEAD)
    s_ref = ((Dg.max(-1) - Dg.min(-1)) / 15).astype(f16)
    z_ref = (-Dg.min(-1)).astype(f16)
    sz = np.asarray(got["sz"], dtype=f16).reshape(T, N // HEAD, 2)
    s, z = sz[..., 0], sz[..., 1]
    ds, dz = np.abs(_ord16(s) - _ord16(s_ref)).max(), np.abs(_ord16(z) - _ord16(z_ref)).max()
    if ds > 1 or dz > 1:
        return False, f"(scale, zero) ({int(ds)}, {int(dz)}) fp16 ulps from the restated ones (bound 1)"
    s64, z64 = s.astype(f64), z.astype(f64)
    t = (np.maximum(ulp16(z64), ulp16(z_ref)) + 15 * np.maximum(ulp16(s64), ulp16(s_ref)) + steps * 2.0 ** -24 * Ag.max(-1))
    code = _nibbles(np.asarray(got["codes"]).reshape(T, N // HEAD, HEAD // 2))
    over = np.abs(code * s64[..., None] - z64[..., None] - Dg) - (0.5 * s64 + t)[..., None]
    at = np.unravel_index(np.argmax(over), over.shape)
    used = (np.abs(code * s64[..., None] - z64[..., None] - Dg) - 0.5 * s64[..., None]) / t[..., None]
    return bool(over.max() <= 0), (f"(scale, zero) ({int(ds)}, {int(dz)}) ulps off; {int((over > 0).sum())} elements outside scale / 2 + t, largest "
                                   f"excess over scale / 2 is {used.max():.3g} t, at (row, head, d) {tuple(int(i) for i in at)}")


def _check_attn(req, got, ref):
    got = np.asarray(got, dtype=f16).astype(f64)
    ok, msgs = True, []
    for what, rows, rel in (("prefill", slice(0, req.doff), 4e-3), ("decode", slice(req.doff, req.rows), 2e-3)):
        if rows.stop > rows.start:
            err, top = np.abs(got[rows] - ref[rows]).max(), np.abs(ref[rows]).max()
            ok = ok and bool(err <= rel * top + 1e-3)
            msgs.append(f"{what} rows: max|err| {err:.4g}, bound {rel * top + 1e-3:.4g} ({rel:g} * {top:.4g} + 1e-3)")
    return ok, "; ".join(msgs)


def reporter(report):
    """(fails, put): ``put(stage, (ok, message))`` files a failure under ``fails`` and one line per stage under ``report`` (if given)"""
    fails = []

    def put(stage, res):
        ok, msg = res
        if not ok:
            fails.append((stage, msg))
        if report is not None:
            report.append(f"{stage}: {'ok' if ok else 'FAIL'}: {msg}")
    return fails, put


def absent(trace, stages):
    """[(stage, message)] for the stages a trace lacks: a stage cannot pass by being absent"""
    return [(s, "stage absent from the trace") for s in stages if s not in trace]


def check_attention_half(trace, inputs, put):
    """norm1 .. residual1, norm2 of ``trace``, each against its restatement on the trace's own previous stage"""
    req, lay, pool, x = inputs["req"], inputs["lay"], inputs["pool"], np.asarray(inputs["x"], dtype=f16)
    W, steps = lay["w"], x.shape[1] // 128
    put("norm1", _quant_exact(trace["norm1"], O.rmsnorm_reorder_quant(x, lay["norm1_w"], lay["eps"], lay["norm1_idx"], "kernel", 1.0)))
    n1 = trace["norm1"]
    put("q", _check_gemm(trace["q"], gemm(n1, W["q"])))
    for name in ("k", "v"):
        put(name, _check_o4(trace[name], gemm(n1, W[name]), gemm_abs(n1, W[name]), steps))
    check_attention_core(trace, inputs, put)
    check_attention_tail(trace, inputs, put)


def check_attention_core(trace, inputs, put):
    """cache, attn, attn_q: the pool against the append of the observed k / v codes, the attention of the observed q over that pool, the
    reorder quantiser of the observed attention output (whatever produced q and the k / v codes)"""
    req, lay, pool = inputs["req"], inputs["lay"], inputs["pool"]
    want = write_cache(req, pool, trace["k"], trace["v"], lay["layer_idx"])
    same = np.array_equal(trace["cache"]["buf"], want[0]), _bits_equal(trace["cache"]["param"], want[1])
    put("cache", (all(same), "the pool against the append of the observed codes at the described slots: "
                  f"{int((trace['cache']['buf'] != want[0]).sum())} bytes differ, "
                  f"{int((np.ascontiguousarray(trace['cache']['param']).view(np.uint16) != want[1].view(np.uint16)).sum())} (scale, zero) halves"))
    put("attn", _check_attn(req, trace["attn"], attention(req, trace["q"], want, lay["layer_idx"], lay["rope_theta"])))
    put("attn_q", _quant_exact(trace["attn_q"], O.reorder_quant(trace["attn"], lay["attn_idx"], "kernel", 1.0)))


def check_attention_tail(trace, inputs, put):
    """o, residual1, norm2"""
    lay, x = inputs["lay"], np.asarray(inputs["x"], dtype=f16)
    put("o", _check_gemm(trace["o"], gemm(trace["attn_q"], lay["w"]["o"])))
    r1 = (np.asarray(trace["o"], dtype=f16).astype(f32) + x.astype(f32)).astype(f16)
    put("residual1", (_bits_equal(trace["residual1"], r1), "against the fp16 sum of the layer input and o_proj's output"))
    put("norm2", _quant_exact(trace["norm2"], O.rmsnorm_reorder_quant(trace["residual1"], lay["norm2_w"], lay["eps"], lay["norm2_idx"],
                                                                      "kernel", 1.0)))


def check_mlp_half(trace, inputs, put):
    """gate, up, act, out of the dense MLP"""
    W = inputs["lay"]["w"]
    for name in ("gate", "up"):
        put(name, _check_gemm(trace[name], gemm(trace["norm2"], W[name])))
    put("act", _quant_close(trace["act"], O.silu_mul_quant(trace["gate"], trace["up"], "kernel", 1.0)))
    D = gemm(trace["act"], W["down"])
    ref = D + np.asarray(trace["residual1"], dtype=f16).astype(f64)
    over = np.abs(np.asarray(trace["out"], dtype=f16).astype(f64) - ref) - (gemm_bound(D) + 2.0 ** -11 * np.abs(ref))
    err = np.abs(np.asarray(trace["out"], dtype=f16).astype(f64) - ref).max()
    put("out", (bool(over.max() <= 0), f"{int((over > 0).sum())} elements outside the bound, max|err| {err:.4g} (GEMM part of the bound "
                f"{gemm_bound(D):.4g})"))


def check(trace, inputs, report=None):
    """Every stage of ``trace`` against its restatement on the trace's own previous stage.  ``inputs``: dict(req, lay, pool, x) as
    ``forward`` takes them.  Returns [(stage, message)], empty when all is well.  ``report``: a list that receives one line per stage
    with the measured figure."""
    missing = absent(trace, LAYER_STAGES)
    if missing:
        return missing
    fails, put = reporter(report)
    check_attention_half(trace, inputs, put)
    check_mlp_half(trace, inputs, put)
    return fails


# ---------------------------------------------------------------------------------------------------- the model
def _final_norm(h, w, eps):
    """The un-quantised final RMSNorm, float64: x * rsqrt(mean(x^2) + eps) (the module takes the statistics in FP32), cast to fp16,
    then times the fp16 weight, rounded to fp16 again.  Returns (w * x * r in float64, the two roundings applied in order).
    Bound 2 fp16 ulps of the float64 value: the cast errs by at most 2^-11 relative, which the weight carries into the product as less
    than one ulp of it; the product's own rounding is half an ulp, one where it lands in the next binade; the FP32 statistic's 2^-22
    relative is far inside the rest."""
    x = np.asarray(h, dtype=f16).astype(f64)
    r = 1 / np.sqrt((x ** 2).mean(-1, keepdims=True) + eps)
    wf = np.asarray(w, dtype=f16).astype(f64)
    return wf * x * r, (wf * (x * r).astype(f16).astype(f64)).astype(f16)


def _check_logits(got, xn, head):
    """lm_head on the observed normed stream: fp16 operands, FP32 accumulation over K = hidden in any order, one rounding to fp16.
    |err| <= 2^-10 * |ref| + K * 2^-24 * (|x| @ |W|^T): K additions, each 2^-24 relative to a partial sum of at most sum|term|, then the
    fp16 rounding -- half an ulp, at most 2^-11 relative to the FP32 sum; 2^-10 of the exact value covers it where the sum and the
    exact value sit in different binades."""
    xf, wf = np.asarray(xn, dtype=f16).astype(f64), np.asarray(head, dtype=f16).astype(f64)
    ref = xf @ wf.T
    over = np.abs(np.asarray(got, dtype=f16).astype(f64) - ref) - (2.0 ** -10 * np.abs(ref) + xf.shape[1] * 2.0 ** -24 * (np.abs(xf) @ np.abs(wf).T))
    return bool(over.max() <= 0), f"{int((over > 0).sum())} logits outside the bound, largest err - bound {over.max():.4g}"


def model_forward(req, mdl, pool, ids, wrong=None, layer_forward=None):
    """``mdl``: dict(embed fp16 [V, hidden], layers [lay ...], norm_w, eps, head fp16 [V, hidden]).  Trace: embed, layers (each with its
    observed input under "x"), final_norm, logits.  ``layer_forward``: the layer (``forward`` unless given; a variant's has its signature)."""
    layer_forward = layer_forward or forward
    tr = {"embed": np.asarray(mdl["embed"], dtype=f16)[np.asarray(ids, dtype=np.int64)], "layers": []}
    h = tr["embed"]
    for lay in mdl["layers"]:
        t = layer_forward(req, lay, pool, h, wrong)
        t["x"] = h
        tr["layers"].append(t)
        pool, h = (t["cache"]["buf"], t["cache"]["param"]), t["out"]
    normed = _final_norm(h, mdl["norm_w"], mdl["eps"])[1]
    tr["final_norm"] = h if wrong == "no_final_norm" else normed
    xin = h if wrong == "head_before_norm" else tr["final_norm"]
    tr["logits"] = (xin.astype(f64) @ np.asarray(mdl["head"], dtype=f16).astype(f64).T).astype(f16)
    return tr


def check_model(trace, inputs, report=None, layer_check=None):
    """``inputs``: dict(req, mdl, pool, ids).  Every layer teacher-forced on its observed input and the pool the layer before left.
    ``layer_check``: the layer's checker (``check`` unless given; a variant's has its signature)."""
    layer_check = layer_check or check
    req, mdl, pool = inputs["req"], inputs["mdl"], inputs["pool"]
    fails = []
    want = np.asarray(mdl["embed"], dtype=f16)[np.asarray(inputs["ids"], dtype=np.int64)]
    if not _bits_equal(trace["embed"], want):
        fails.append(("embed", "not the rows of the embedding table"))
    if len(trace["layers"]) != len(mdl["layers"]):
        return fails + [("layers", f"{len(trace['layers'])} layers in the trace, {len(mdl['layers'])} in the model")]
    h = trace["embed"]
    for i, (t, lay) in enumerate(zip(trace["layers"], mdl["layers"])):
        if not _bits_equal(t["x"], h):
            fails.append((f"layer{i}.x", "the layer's input is not the output of the stage before it"))
        rep = None if report is None else []
        fails += [(f"layer{i}.{s}", m) for s, m in layer_check(t, dict(req=req, lay=lay, pool=pool, x=t["x"]), rep)]
        if report is not None:
            report += [f"layer{i}.{line}" for line in rep]
        pool, h = (t["cache"]["buf"], t["cache"]["param"]), t["out"]
    ref, _ = _final_norm(h, mdl["norm_w"], mdl["eps"])
    over = np.abs(np.asarray(trace["final_norm"], dtype=f16).astype(f64) - ref) - 2 * ulp16(ref)
    d = (np.abs(np.asarray(trace["final_norm"], dtype=f16).astype(f64) - ref) / ulp16(ref)).max()
    res = [("final_norm", (bool(over.max() <= 0), f"up to {d:.3g} fp16 ulps off (bound 2)")),
           ("logits", _check_logits(trace["logits"], trace["final_norm"], mdl["head"]))]
    for stage, (ok, msg) in res:
        if not ok:
            fails.append((stage, msg))
        if report is not None:
            report.append(f"{stage}: {'ok' if ok else 'FAIL'}: {msg}")
    return fails
