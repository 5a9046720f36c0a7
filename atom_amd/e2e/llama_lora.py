"""Llama with fp16 LoRA adapters on the frozen 4-bit base, one adapter per SEQUENCE of a batch (the role of the reference's
punica/models/llama_lora.py, on ``ops.add_lora`` over ``utils.lora``'s pools).  The forward signature is the base model's, so
``generate()`` and ``DecodeGraph`` take the model as it is."""
from __future__ import annotations

from typing import Sequence

import torch

from .. import ops
from ..utils.lora import LlamaLoraManager
from .llama import LlamaDecoderLayer, LlamaForCausalLM, LlamaModel


def linear_fp16(lin, x_q):
    """A projection's packed weight on the quantised operand ``x_q`` with fp16 output, whatever the module's own out_dtype."""
    outlier, norms, outlier_scales, norm_scales = x_q
    return ops.dense_layer_gemm_i4_fp16(norms, lin.weight_int4, norm_scales, lin.scale_int4, outlier, lin.weight_int8, outlier_scales,
                                        lin.scale_int8)


def rmsnorm_fp16(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """The un-quantised norm output in the model's original channel order (LlamaRMSNorm's arithmetic, as MixtralDecoderLayer computes
    its router input): what an adapter's A reads."""
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return weight * h.to(x.dtype)


class LlamaDecoderLayerWithLora(LlamaDecoderLayer):
    """``lora`` is None (``set_adapters(None)``): ``LlamaDecoderLayer.forward``, bit for bit.  With adapters set the layer runs the
    un-fused op order below; ``P`` = number of prefill requests, ids[:P] their adapters (segments of ``blen.indptr``), ids[P:] the
    decode rows' (one-row segments); ``lora(y, x, m)`` = for a targeted module ``m``: ``ops.add_lora(y[:doff], x[:doff], wa_T, wb_T,
    ids[:P], layer_idx, 1.0, seg_indptr=blen.indptr)`` when P > 0, then ``ops.add_lora(y[doff:], x[doff:], wa_T, wb_T, ids[P:P + decode],
    layer_idx, 1.0)`` when there are decode rows -- nothing for an untargeted module.

        x_q   = input_layernorm(h)                                   (ops.rmsnorm_fp16_i4)
        xn    = rmsnorm_fp16(h, input_layernorm.weight, eps)         (torch)
        q, k, v = linear_fp16(q_proj | k_proj | v_proj, x_q);  lora(q, xn, "q_proj"), lora(k, xn, "k_proj"), lora(v, xn, "v_proj")
        (k_u4, k_sz), (v_u4, v_sz) = ops.kv_quant_u4(k.view(T, kv_heads, 128)), ops.kv_quant_u4(v.view(...))
        prefill rows: ops.init_kv_i4(prefill_kv, ..., blen.indptr, layer_idx); ops.batch_prefill_i4(q, blen.indptr, prefill_kv,
                      layer_idx, rope_theta=..., max_q_len=max(blen.prefills))
        decode rows:  ops.append_kv_i4(decode_kv, ..., layer_idx); ops.batch_decode_i4(q, decode_kv, layer_idx, rope_theta=...)
        attn  = the two outputs concatenated [T, hidden]
        o     = o_proj(ops.reorder_fp16_i4(attn, self_attn.reorder_index));  lora(o, attn, "o_proj")
        res, n_q = post_attention_layernorm.forward_add(o, h)        (ops.add_rmsnorm_fp16_i4: res = o + h)
        n     = rmsnorm_fp16(res, post_attention_layernorm.weight, eps)
        gate, up = linear_fp16(gate_proj | up_proj, n_q);  lora(gate, n, "gate_proj"), lora(up, n, "up_proj")
        d     = linear_fp16(down_proj, ops.activate_fp16_i4(gate, up));  lora(d, silu(gate) * up (torch, fp16), "down_proj")
        out   = res + d
    """

    lora = None          # (manager, ids int32 device buffer) while adapters are set

    def _lora(self, y, x, module, blen):
        mgr, ids = self.lora
        m = mgr.mgr.get(module)
        if m is None:
            return
        layer_idx, p, doff = self.self_attn.layer_idx, len(blen.prefills), blen.doff
        if p > 0:
            ops.add_lora(y[:doff], x[:doff], m.wa_T, m.wb_T, ids[:p], layer_idx, 1.0, seg_indptr=blen.indptr)
        if blen.decode > 0:
            ops.add_lora(y[doff:], x[doff:], m.wa_T, m.wb_T, ids[p:p + blen.decode], layer_idx, 1.0)

    def forward(self, hidden_states, blen, prefill_kv, decode_kv) -> torch.Tensor:
        if self.lora is None:
            return super().forward(hidden_states, blen, prefill_kv, decode_kv)
        at, mlp, il, pl = self.self_attn, self.mlp, self.input_layernorm, self.post_attention_layernorm
        nh, nkv, hd, layer_idx = at.num_heads, at.num_kv_heads, at.head_dim, at.layer_idx
        at._check_cache(prefill_kv)
        at._check_cache(decode_kv)
        rows, doff = hidden_states.size(0), blen.doff
        if doff + blen.decode != rows or len(blen.prefills) + blen.decode > self.lora[1].numel():
            raise ValueError(f"{rows} rows for prefill requests of {list(blen.prefills)} and {blen.decode} decode rows with "
                             f"{self.lora[1].numel()} adapter ids set")
        x_q = il(hidden_states)
        xn = rmsnorm_fp16(hidden_states, il.weight, il.variance_epsilon)
        q, k, v = linear_fp16(at.q_proj, x_q), linear_fp16(at.k_proj, x_q), linear_fp16(at.v_proj, x_q)
        self._lora(q, xn, "q_proj", blen)
        self._lora(k, xn, "k_proj", blen)
        self._lora(v, xn, "v_proj", blen)
        k_u4, k_sz = ops.kv_quant_u4(k.view(rows, nkv, hd))
        v_u4, v_sz = ops.kv_quant_u4(v.view(rows, nkv, hd))
        outs = []
        if len(blen.prefills) > 0:
            assert prefill_kv is not None
            ops.init_kv_i4(prefill_kv, k_u4[:doff], v_u4[:doff], k_sz[:doff], v_sz[:doff], blen.indptr, layer_idx)
            o = ops.batch_prefill_i4(q[:doff].view(-1, nh, hd), blen.indptr, prefill_kv, layer_idx, rope_theta=at.rope_theta,
                                     max_q_len=max(blen.prefills), **at.rope_kw)
            outs.append(o.view(doff, at.hidden_size))
        if blen.decode > 0:
            assert decode_kv is not None
            ops.append_kv_i4(decode_kv, k_u4[doff:], v_u4[doff:], k_sz[doff:], v_sz[doff:], layer_idx)
            o = ops.batch_decode_i4(q[doff:].view(blen.decode, nh, hd), decode_kv, layer_idx, rope_theta=at.rope_theta, **at.rope_kw)
            outs.append(o.view(blen.decode, at.hidden_size))
        attn = (outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)).contiguous()
        o = at.o_proj(ops.reorder_fp16_i4(attn, at.reorder_index))
        self._lora(o, attn, "o_proj", blen)
        res, n_q = pl.forward_add(o, hidden_states)
        n = rmsnorm_fp16(res, pl.weight, pl.variance_epsilon)
        gate, up = linear_fp16(mlp.gate_proj, n_q), linear_fp16(mlp.up_proj, n_q)
        self._lora(gate, n, "gate_proj", blen)
        self._lora(up, n, "up_proj", blen)
        d = linear_fp16(mlp.down_proj, ops.activate_fp16_i4(gate, up))
        if "down_proj" in self.lora[0].mgr:
            self._lora(d, torch.nn.functional.silu(gate) * up, "down_proj", blen)
        return res + d


class LlamaModelWithLora(LlamaModel):
    layer_class = LlamaDecoderLayerWithLora


class LlamaForCausalLMWithLora(LlamaForCausalLM):
    """(logits, hidden_states) with the forward signature of ``LlamaForCausalLM`` and its state dict."""
    model_class = LlamaModelWithLora

    MIN_IDS = 64          # the id buffer's first size: batches up to this many sequences never replace it

    def set_adapters(self, ids: Sequence[int] | None, manager: LlamaLoraManager = None):
        """One adapter id (``LlamaLoraWeight.idx``; -1: none) per SEQUENCE of the next batches, prefill requests first, then the decode
        rows.  The ids are copied IN PLACE into a persistent int32 device buffer, so a captured decode step sees a later call (the
        buffer is replaced only when a batch has more sequences than it holds).  ``None``: every layer runs the base model's forward."""
        if ids is None:
            for layer in self.model.layers:
                layer.lora = None
            return
        if manager is None:
            raise ValueError("set_adapters(ids, manager): the adapter pools are missing")
        ids = [int(i) for i in ids]
        if any(i < -1 or i >= manager.capacity for i in ids):
            raise ValueError(f"adapter ids {ids}: -1 or 0 .. {manager.capacity - 1}")
        if manager.num_layers != len(self.model.layers):
            raise ValueError("the adapter pools were built for another number of layers")
        buf = getattr(self, "_lora_ids", None)
        if buf is None or buf.numel() < len(ids) or buf.device != manager.device:
            buf = self._lora_ids = torch.full((max(self.MIN_IDS, len(ids)),), -1, dtype=torch.int32, device=manager.device)
        buf[:len(ids)].copy_(torch.tensor(ids, dtype=torch.int32))
        view = buf[:len(ids)]
        for layer in self.model.layers:
            layer.lora = (manager, view)
