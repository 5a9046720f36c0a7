"""The MX form of the mixed-precision linear layer: MXFP4 channels, an MXFP8 keeper, both on the scaled MFMA."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops


WEIGHT_GROUPS = ("qkv", "o_proj", "gate_up", "down_proj")      # the four weight operands of LlamaDecoderLayerMxfp4


def weight_formats(config) -> dict:
    """``config.weight_format`` as {group: "mxfp4" | "mxfp6"} over WEIGHT_GROUPS: a string names all four, a mapping its keys (missing
    keys are "mxfp4"); anything else is a ``ValueError``."""
    wf = getattr(config, "weight_format", "mxfp4")
    if isinstance(wf, str):
        wf = dict.fromkeys(WEIGHT_GROUPS, wf)
    if not hasattr(wf, "keys") or any(k not in WEIGHT_GROUPS or wf[k] not in ("mxfp4", "mxfp6") for k in wf.keys()):
        raise ValueError(f"config.weight_format must be \"mxfp4\", \"mxfp6\" or a mapping of {WEIGHT_GROUPS} to one of them, got {wf!r}")
    return {g: wf.get(g, "mxfp4") for g in WEIGHT_GROUPS}


class LinearMxfp4(nn.Module):
    """``forward(x_fp16, reorder_index)`` = quantise the reordered activation to MX, then the MXFP4 GEMM against the MX weight.
    ``act_format``: "mxfp4" (W4A4) or "mxfp6" (W4A6: E2M3 activations, same weight).  ``weight_format``: "mxfp4" or "mxfp6" (E2M3
    bulk codes, W6A4 / W6A6, DESIGN.md 4.30: ``weight_fp4`` then holds [R, S, 96, 16])."""

    def __init__(self, in_features, out_features, act_format="mxfp4", weight_format="mxfp4"):
        super().__init__()
        if act_format not in ("mxfp4", "mxfp6"):
            raise ValueError(f"act_format must be \"mxfp4\" or \"mxfp6\", got {act_format!r}")
        if weight_format not in ("mxfp4", "mxfp6"):
            raise ValueError(f"weight_format must be \"mxfp4\" or \"mxfp6\", got {weight_format!r}")
        self.act_format, self.weight_format = act_format, weight_format
        if in_features % 128 or in_features < 256 or out_features % 64 or out_features < 64:
            raise ValueError("LinearMxfp4: in_features a multiple of 128 (>= 256), out_features a multiple of 64")
        self.in_features, self.out_features = in_features, out_features
        r, s = out_features // 16, in_features // 128 - 1
        self.weight_fp4 = nn.Parameter(torch.empty(r, s, 96 if weight_format == "mxfp6" else 64, 16, dtype=torch.uint8), requires_grad=False)
        self.weight_scale = nn.Parameter(torch.empty(r, s + 1, 64, dtype=torch.uint8), requires_grad=False)
        self.weight_fp8 = nn.Parameter(torch.empty(r, 2, 64, 16, dtype=torch.uint8), requires_grad=False)

    @torch.no_grad()
    def load_fp16_weight(self, weight: torch.Tensor):
        """Fill the parameters from a (column-reordered) fp16 weight [out, in]."""
        if tuple(weight.shape) != (self.out_features, self.in_features):
            raise ValueError(f"weight must be [{self.out_features}, {self.in_features}], got {tuple(weight.shape)}")
        w = ops.quant_weight_mx(weight.contiguous(), self.weight_format)
        self.weight_fp4.data, self.weight_scale.data, self.weight_fp8.data = w.q4, w.sc, w.q8
        return self

    def weight_mx(self) -> ops.MxOperand:
        return ops.MxOperand(self.weight_fp4.data, self.weight_scale.data, self.weight_fp8.data, self.out_features, self.in_features)

    def forward(self, x, reorder_index=None):
        lead = x.shape[:-1]
        y = ops.gemm_mxfp4(ops.reorder_quant_mx(x.reshape(-1, self.in_features).contiguous(), reorder_index, self.act_format), self.weight_mx())
        return y.view(*lead, self.out_features)


def _mx_key(mods):
    """what a fused operand is keyed by (as the INT4 fusions): the storage and version of every parameter it was built from"""
    return tuple((p.data_ptr(), p._version) for m in mods for p in (m.weight_fp4, m.weight_scale, m.weight_fp8))


class LlamaAttentionMxfp4(nn.Module):
    """The attention block of the MX decoder layer: q | k | v from ONE MXFP4 GEMM over the row-stacked weight, fp16 out; k and v take
    the fp16 road into the INT4 paged cache (ops.kv_quant_u4 -> init_kv_i4 / append_kv_i4), attention is the INT4 paged-KV ops'
    (prefill always through ops.batch_prefill_i4), o_proj an MXFP4 GEMM on the reordered, MX-quantised attention output.  Head size
    128, no sliding window, no attention sinks."""

    window = None                                                # (what generate() looks for on an attention layer)

    def __init__(self, config, layer_idx: int):
        super().__init__()
        from .rope import rope_init
        self.config, self.layer_idx = config, layer_idx
        self.act_format = getattr(config, "activation_format", "mxfp4")
        self.hidden_size, self.num_heads = config.hidden_size, config.num_attention_heads
        explicit = getattr(config, "head_dim", None)
        self.head_dim = self.hidden_size // self.num_heads if explicit is None else int(explicit)
        if self.head_dim != 128 or self.head_dim * self.num_heads != self.hidden_size:
            raise NotImplementedError(f"the MXFP4 decoder layer is built for head_dim 128 (hidden_size = heads x 128), got {self.head_dim}")
        if getattr(config, "sliding_window", None) is not None and getattr(config, "use_sliding_window", True) is not False:
            raise NotImplementedError("the MXFP4 decoder layer has no sliding-window attention: config.sliding_window must be None")
        nkv = getattr(config, "num_key_value_heads", None)
        self.num_kv_heads = self.num_heads if nkv is None else int(nkv)
        if self.num_kv_heads < 1 or self.num_heads % self.num_kv_heads:
            raise ValueError(f"num_key_value_heads {self.num_kv_heads} does not divide num_attention_heads {self.num_heads}")
        self.kv_dim = self.num_kv_heads * self.head_dim
        wf = weight_formats(config)
        self.q_proj = LinearMxfp4(self.hidden_size, self.hidden_size, weight_format=wf["qkv"])
        self.k_proj = LinearMxfp4(self.hidden_size, self.kv_dim, weight_format=wf["qkv"])
        self.v_proj = LinearMxfp4(self.hidden_size, self.kv_dim, weight_format=wf["qkv"])
        self.o_proj = LinearMxfp4(self.hidden_size, self.hidden_size, weight_format=wf["o_proj"])
        self.reorder_index = nn.Parameter(torch.randperm(self.hidden_size).to(torch.int16), requires_grad=False)
        self.rope_theta, self.rope_scale, inv_freq, attention_factor = rope_init(config, self.head_dim)
        self.attn_scale = float(attention_factor) ** 2
        self.register_buffer("rope_table", None if inv_freq is None else ops.rope_table(inv_freq, "cpu", self.head_dim), persistent=False)

    @property
    def rope_kw(self) -> dict:
        kw = {}
        if self.rope_scale != 1.0:
            kw["rope_scale"] = self.rope_scale
        if self.rope_table is not None or self.attn_scale != 1.0:
            kw.update(rope_table=self.rope_table, attn_scale=self.attn_scale)
        return kw

    def qkv_mx(self) -> ops.MxOperand:
        """q_proj, k_proj and v_proj row-stacked: one weight operand (built once per set of parameters)"""
        mods = [self.q_proj, self.k_proj, self.v_proj]
        key = _mx_key(mods)
        if getattr(self, "_qkv", None) is None or self._qkv[0] != key:
            ws = [m.weight_mx() for m in mods]
            self._qkv = (key, ops.MxOperand(*(torch.cat([getattr(w, f) for w in ws]) for f in ("q4", "sc", "q8")),
                                            self.hidden_size + 2 * self.kv_dim, self.hidden_size))
        return self._qkv[1]

    def forward(self, x_mx, blen, prefill_kv, decode_kv):
        """``x_mx``: the MX operand of the input norm.  Returns the fp16 o_proj output (the caller adds the residual)."""
        nh, hd, nkv, hs = self.num_heads, self.head_dim, self.num_kv_heads, self.hidden_size
        for kv in (prefill_kv, decode_kv):
            if kv is not None and (ops._kv_dims(kv)[1], ops._kv_dims(kv)[3]) != (nkv, hd):
                raise ValueError(f"a paged KV cache of {ops._kv_dims(kv)[1]} heads of {ops._kv_dims(kv)[3]} for a layer of {nkv} K/V heads of {hd}")
        qkv = ops.gemm_mxfp4(x_mx, self.qkv_mx())
        rows, doff = qkv.size(0), blen.doff
        q = qkv[:, :hs].contiguous().view(rows, nh, hd)
        k_u4, k_sz = ops.kv_quant_u4(qkv[:, hs:hs + self.kv_dim].contiguous().view(rows, nkv, hd))
        v_u4, v_sz = ops.kv_quant_u4(qkv[:, hs + self.kv_dim:].contiguous().view(rows, nkv, hd))
        outs = []
        if len(blen.prefills) > 0:
            assert prefill_kv is not None
            ops.init_kv_i4(prefill_kv, k_u4[:doff], v_u4[:doff], k_sz[:doff], v_sz[:doff], blen.indptr, self.layer_idx)
            o = ops.batch_prefill_i4(q[:doff], blen.indptr, prefill_kv, self.layer_idx, rope_theta=self.rope_theta, max_q_len=max(blen.prefills),
                                     **self.rope_kw)
            outs.append(o.view(doff, hs))
        if blen.decode > 0:
            assert decode_kv is not None
            ops.append_kv_i4(decode_kv, k_u4[doff:], v_u4[doff:], k_sz[doff:], v_sz[doff:], self.layer_idx)
            o = ops.batch_decode_i4(q[doff:], decode_kv, self.layer_idx, rope_theta=self.rope_theta, **self.rope_kw)
            outs.append(o.view(blen.decode, hs))
        attn = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return ops.gemm_mxfp4(ops.reorder_quant_mx(attn.contiguous(), self.reorder_index, self.act_format), self.o_proj.weight_mx())


class LlamaMLPMxfp4(nn.Module):
    """down( silu(gate(x)) * up(x) ) + residual in two launches: the fused gate/up SiLU-quantising GEMM, then down_proj's GEMM with
    the residual add in its store."""

    def __init__(self, config):
        super().__init__()
        self.hidden_size, self.intermediate_size = config.hidden_size, config.intermediate_size
        self.act_format = getattr(config, "activation_format", "mxfp4")
        if self.intermediate_size % 128 or self.intermediate_size < 256:
            raise ValueError(f"the MXFP4 MLP needs intermediate_size a multiple of 128 (>= 256), got {self.intermediate_size}")
        wf = weight_formats(config)
        self.gate_proj = LinearMxfp4(self.hidden_size, self.intermediate_size, weight_format=wf["gate_up"])
        self.up_proj = LinearMxfp4(self.hidden_size, self.intermediate_size, weight_format=wf["gate_up"])
        self.down_proj = LinearMxfp4(self.intermediate_size, self.hidden_size, weight_format=wf["down_proj"])

    def gate_up_mx(self) -> ops.MxOperand:
        mods = [self.gate_proj, self.up_proj]
        key = _mx_key(mods)
        if getattr(self, "_gu", None) is None or self._gu[0] != key:
            self._gu = (key, ops.fuse_gate_up_mx(self.gate_proj.weight_mx(), self.up_proj.weight_mx(), self.gate_proj.weight_format))
        return self._gu[1]

    def forward(self, x_mx, residual):
        return ops.gemm_mxfp4(ops.gate_up_silu_quant_mx(x_mx, self.gate_up_mx(), self.act_format), self.down_proj.weight_mx(), add=residual)


class LlamaDecoderLayerMxfp4(nn.Module):
    """The dense Llama decoder layer on MX operands (``config.linear_format = "mxfp4"``), launch by launch:
    rmsnorm_quant_mx -> gemm_mxfp4 (q | k | v) -> the INT4 paged-KV attention -> reorder_quant_mx -> gemm_mxfp4 (o_proj) ->
    add_rmsnorm_quant_mx (the residual add of the attention block; the stream is updated in place) -> gate_up_silu_quant_mx ->
    gemm_mxfp4(add=residual).  No host work: a decode step captures.  ``hidden_states`` is overwritten with the post-attention stream.
    ``config.activation_format = "mxfp6"`` makes the four quantising launches (both norms, o_proj's reorder quantiser, the fused
    gate/up output) write MXFP6 activations; every GEMM then runs W4A6.  ``config.weight_format`` ("mxfp4", "mxfp6"
    or a mapping over ``WEIGHT_GROUPS``) gives the four weight operands E2M3 bulk codes, all or some; the launches are
    the same, the ops read each format off its operand."""

    def __init__(self, config, layer_idx: int, fusion=None):
        super().__init__()
        from .llama import LlamaRMSNormInt4
        if fusion is not None:
            raise NotImplementedError("DecodeFusion names launches of the INT4 routes; the MXFP4 decoder layer takes none")
        self.hidden_size = config.hidden_size
        self.act_format = getattr(config, "activation_format", "mxfp4")
        if self.act_format not in ("mxfp4", "mxfp6"):
            raise ValueError(f"config.activation_format must be \"mxfp4\" or \"mxfp6\", got {self.act_format!r}")
        self.self_attn = LlamaAttentionMxfp4(config, layer_idx)
        self.mlp = LlamaMLPMxfp4(config)
        self.input_layernorm = LlamaRMSNormInt4(config.hidden_size, eps=config.rms_norm_eps)            # (its parameters; the MX ops read them)
        self.post_attention_layernorm = LlamaRMSNormInt4(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, hidden_states, blen, prefill_kv, decode_kv) -> torch.Tensor:
        il, pl = self.input_layernorm, self.post_attention_layernorm
        h = hidden_states if hidden_states.is_contiguous() else hidden_states.contiguous()
        attn = self.self_attn(ops.rmsnorm_quant_mx(h, il.weight, il.reorder_index, il.variance_epsilon, self.act_format), blen, prefill_kv, decode_kv)
        x_mx = ops.add_rmsnorm_quant_mx(attn, h, pl.weight, pl.reorder_index, pl.variance_epsilon, self.act_format)      # h += attn
        return self.mlp(x_mx, h)
