"""Mixtral on the native W4A4 path: the sparse mixture-of-experts block as five launches with no host work between them -- router
tables, one routed GEMM for gate and up, the SiLU x up quantiser, one routed GEMM for down, the weighted combine (csrc/moe_w4a4.hip) --
under the Llama attention (grouped-query) and the Llama model skeleton, so ``generate()`` and ``DecodeGraph`` take the model as it is.
The reference quantises Mixtral on its simulated path only and runs the block as a Python loop over the experts with a host read per
expert (model/qMixtralLayer.py:302-350): the arithmetic here is that loop's -- activations quantised once per token in front of the
experts (:309-311), every expert output scaled by its fp16 routing weight, added in expert order, the residual last.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .llama import GROUP, DecodeFusion, LlamaAttention, LlamaForCausalLM, LlamaModel, LlamaRMSNormInt4


class MixtralSparseMoeInt4(nn.Module):
    """reference qMixtralLayer.py:283-350.  ``gate.weight`` fp16 [E, H] in the model's original channel order (the router sees
    un-quantised states); the experts' packed weights stacked: ``w13_*`` = gate (w1) rows then up (w3) rows of each expert, ``w2_*`` =
    down, in the layout of ``LinearInt4``'s parameters with a leading expert dimension (scales exactly [E, G, N] / [E, N])."""

    def __init__(self, config):
        super().__init__()
        h, f = config.hidden_size, config.intermediate_size
        e = self.num_experts = int(config.num_local_experts)
        self.top_k = int(config.num_experts_per_tok)
        self.hidden_size, self.intermediate_size = h, f
        if h % GROUP or f % GROUP or h < 2 * GROUP or f < 2 * GROUP:
            raise ValueError("hidden_size and intermediate_size must be multiples of 128, at least 256")
        if not (2 <= e <= 64 and 1 <= self.top_k <= min(8, e)):
            raise ValueError(f"{e} experts, top-{self.top_k}: the router takes 2..64 experts and top-1..8")
        self.gate = nn.Linear(h, e, bias=False, dtype=torch.float16)
        par = lambda *shape, dtype: nn.Parameter(torch.empty(*shape, dtype=dtype), requires_grad=False)
        self.w13_int4 = par(e, 2 * f, (h - GROUP) // 2, dtype=torch.uint8)
        self.w13_int8 = par(e, 2 * f, GROUP, dtype=torch.int8)
        self.w13_scale_int4 = par(e, h // GROUP - 1, 2 * f, dtype=torch.float16)
        self.w13_scale_int8 = par(e, 2 * f, dtype=torch.float16)
        self.w2_int4 = par(e, h, (f - GROUP) // 2, dtype=torch.uint8)
        self.w2_int8 = par(e, h, GROUP, dtype=torch.int8)
        self.w2_scale_int4 = par(e, f // GROUP - 1, h, dtype=torch.float16)
        self.w2_scale_int8 = par(e, h, dtype=torch.float16)

    @torch.no_grad()
    def load_expert_fp16(self, j: int, w1: torch.Tensor, w3: torch.Tensor, w2: torch.Tensor, w_clip: float = 0.85, channel_group: int = 2):
        """Fill expert ``j`` from its (column-reordered) fp16 weights: w1 / w3 [F, H] (gate / up), w2 [H, F] (down)."""
        f, h = self.intermediate_size, self.hidden_size
        assert w1.shape == (f, h) and w3.shape == (f, h) and w2.shape == (h, f)
        for name, w in (("w13", torch.cat([w1, w3], 0)), ("w2", w2)):
            b4, b8, sb, sb8 = ops.quant_weight_w4(w.contiguous(), w_clip, channel_group)
            getattr(self, name + "_int4").data[j].copy_(b4.view(torch.uint8))
            getattr(self, name + "_int8").data[j].copy_(b8)
            getattr(self, name + "_scale_int4").data[j].copy_(sb)
            getattr(self, name + "_scale_int8").data[j].copy_(sb8)
        return self

    def forward(self, x_q, gate_in: torch.Tensor, residual: torch.Tensor = None) -> torch.Tensor:
        """``x_q``: the quantised operand (outlier, norms, outlier_scales, norm_scales) of the tokens, ``gate_in`` fp16 [T, H]: the
        router's un-quantised input, ``residual`` fp16 [T, H] or None.  Returns residual + moe(x) fp16 [T, H]."""
        outlier, norms, outlier_scales, norm_scales = x_q
        route = ops.moe_route_topk(nn.functional.linear(gate_in, self.gate.weight), self.top_k)
        gate, up = ops.moe_gemm_i4(norms, norm_scales, outlier, outlier_scales,
                                   (self.w13_int4, self.w13_int8, self.w13_scale_int4, self.w13_scale_int8), route, gather=True, nseg=2)
        a8, a4, s8, s4 = ops.activate_fp16_i4(gate, up)
        (y,) = ops.moe_gemm_i4(a4, s4, a8, s8, (self.w2_int4, self.w2_int8, self.w2_scale_int4, self.w2_scale_int8), route, gather=False)
        return ops.moe_combine(y, route, residual)


class MixtralDecoderLayer(nn.Module):
    """reference qMixtralLayer.py:353-436: Llama's attention block (grouped-query), then the sparse MoE block on the quantised
    post-attention norm; the router's input is the same norm un-quantised (its gate is a QLinearLayer with enable_quant=False)."""

    def __init__(self, config, layer_idx: int, fusion: DecodeFusion = None):
        super().__init__()
        if getattr(config, "sliding_window", None) is not None:
            raise NotImplementedError("sliding-window attention is not implemented: config.sliding_window must be None (Mixtral-8x7B ships null)")
        self.hidden_size = config.hidden_size
        self.self_attn = LlamaAttention(config=config, layer_idx=layer_idx, fusion=fusion)
        self.block_sparse_moe = MixtralSparseMoeInt4(config)
        self.input_layernorm = LlamaRMSNormInt4(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNormInt4(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, hidden_states, blen, prefill_kv, decode_kv) -> torch.Tensor:
        attn = self.self_attn(self.input_layernorm(hidden_states), blen, prefill_kv, decode_kv)
        pl = self.post_attention_layernorm
        residual, normed = pl.forward_add(attn, hidden_states)
        h = residual.float()                                     # LlamaRMSNorm's arithmetic: fp32 statistics, weight after the cast back
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + pl.variance_epsilon)
        gate_in = pl.weight * h.to(residual.dtype)
        return self.block_sparse_moe(normed, gate_in, residual)


class MixtralModel(LlamaModel):
    layer_class = MixtralDecoderLayer


class MixtralForCausalLM(LlamaForCausalLM):
    """(logits, hidden_states) with the forward signature of ``LlamaForCausalLM``."""
    model_class = MixtralModel
