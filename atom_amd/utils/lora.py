"""Adapter pools for multi-adapter LoRA beside the 4-bit base (roles and names of the reference's punica/utils/lora.py: LoraManager,
LoraWeight, a Llama-level manager), laid out for ``ops.add_lora``: ``wa_T`` fp16 [capacity, L, r, in], ``wb_T`` fp16 [capacity, L, out, r].

What grouped-query models and real adapters force to differ from the reference:
  * one ``LoraManager`` per TARGET MODULE (the reference shares three pools by shape): ``k_proj`` / ``v_proj`` are ``kv_dim`` wide;
  * ``target_modules`` -- any subset of the seven projections, ("q_proj", "v_proj") by default; a projection that is not targeted has
    no pool and costs nothing in the model;
  * ``load(layer_idx, module, A, B, alpha)`` folds ``alpha / r`` into B in FP32 before the fp16 cast, so the ops' single scalar
    ``scale`` stays 1 in the model;
  * one adapter id addresses the adapter's slot in EVERY pool, so a batch carries one id per sequence (-1: no adapter).

Channel order.  The base model's quantisers reorder channels internally, so every LoRA input here is in the model's ORIGINAL order:
``A`` of q / k / v / gate / up reads the un-reordered norm output, ``A`` of o_proj the attention output; ``B`` rows of q / k / v / o /
down are the original output channels.  The intermediate dimension is different: ``B`` rows of gate_proj / up_proj and ``A`` columns
of down_proj follow the rows of ``gate_proj`` / ``up_proj`` AS PACKED (the exporter may have permuted them by down_proj's reorder
index).  ``permute_intermediate`` turns a PEFT-order adapter into that order with the caller's index."""
from __future__ import annotations

import dataclasses
from typing import Sequence

import torch

__all__ = ["LORA_MODULES", "LoraManager", "LoraWeight", "LlamaLoraWeight", "LlamaLoraManager", "permute_intermediate"]

LORA_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


class LoraManager:
    """The pool of one projection: ``capacity`` adapters x ``num_layers`` layers of rank ``lora_rank``.  Slots start as zeros (an
    adapter that was never loaded adds nothing)."""

    def __init__(self, capacity: int, num_layers: int, in_features: int, out_features: int, lora_rank: int,
                 dtype: torch.dtype = torch.float16, device="cuda"):
        if dtype != torch.float16:
            raise TypeError("the LoRA kernels are fp16 only")
        if lora_rank % 8 or not 8 <= lora_rank <= 64:
            raise ValueError(f"lora_rank {lora_rank}: a multiple of 8 in 8 .. 64")
        if in_features % 64 or out_features % 64:
            raise ValueError("in_features and out_features must be multiples of 64")
        self._wa_T = torch.zeros((capacity, num_layers, lora_rank, in_features), dtype=dtype, device=device)
        self._wb_T = torch.zeros((capacity, num_layers, out_features, lora_rank), dtype=dtype, device=device)
        self._free = set(range(capacity))

    device = property(lambda self: self._wa_T.device)
    dtype = property(lambda self: self._wa_T.dtype)
    capacity = property(lambda self: self._wa_T.size(0))
    num_layers = property(lambda self: self._wa_T.size(1))
    lora_rank = property(lambda self: self._wa_T.size(2))
    in_features = property(lambda self: self._wa_T.size(3))
    out_features = property(lambda self: self._wb_T.size(2))
    wa_T = property(lambda self: self._wa_T)
    wb_T = property(lambda self: self._wb_T)

    def alloc(self, idx: int = None) -> "LoraWeight":
        """A free slot (``idx``: that one)."""
        if idx is None:
            idx = min(self._free)
        self._free.remove(idx)
        return LoraWeight(self, idx)

    def free(self, lora_weight: "LoraWeight"):
        assert lora_weight.mgr is self and 0 <= lora_weight.idx < self.capacity and lora_weight.idx not in self._free
        self._wa_T[lora_weight.idx].zero_()
        self._wb_T[lora_weight.idx].zero_()
        self._free.add(lora_weight.idx)


@dataclasses.dataclass
class LoraWeight:
    mgr: LoraManager
    idx: int

    @torch.no_grad()
    def load(self, layer_idx: int, A: torch.Tensor, B: torch.Tensor, alpha: float = None):
        """A [r, in], B [out, r] (PEFT's lora_A.weight / lora_B.weight); ``alpha / r`` (None: 1) goes into B in FP32."""
        m = self.mgr
        assert A.shape == (m.lora_rank, m.in_features) and B.shape == (m.out_features, m.lora_rank)
        s = 1.0 if alpha is None else float(alpha) / m.lora_rank
        m.wa_T[self.idx, layer_idx].copy_(A.to(m.device, torch.float32).to(m.dtype))
        m.wb_T[self.idx, layer_idx].copy_((B.to(m.device, torch.float32) * s).to(m.dtype))


@dataclasses.dataclass
class LlamaLoraWeight:
    """One adapter of a Llama model: its id (the slot in every targeted projection's pool) and the slots themselves."""
    idx: int
    modules: dict

    def load(self, layer_idx: int, module: str, A: torch.Tensor, B: torch.Tensor, alpha: float = None):
        self.modules[module].load(layer_idx, A, B, alpha)


class LlamaLoraManager:
    """The pools of a Llama model's targeted projections.  ``config``: hidden_size, intermediate_size, num_hidden_layers,
    num_attention_heads, num_key_value_heads (optional)."""

    def __init__(self, config, capacity: int, lora_rank: int, target_modules: Sequence[str] = ("q_proj", "v_proj"),
                 dtype: torch.dtype = torch.float16, device="cuda"):
        bad = [m for m in target_modules if m not in LORA_MODULES]
        if bad or not target_modules:
            raise ValueError(f"target_modules {tuple(target_modules)}: a non-empty subset of {LORA_MODULES}")
        h, f = config.hidden_size, config.intermediate_size
        nkv = getattr(config, "num_key_value_heads", None)
        kv = h if nkv is None else h // config.num_attention_heads * int(nkv)
        dims = {"q_proj": (h, h), "k_proj": (h, kv), "v_proj": (h, kv), "o_proj": (h, h), "gate_proj": (h, f), "up_proj": (h, f),
                "down_proj": (f, h)}
        self.target_modules = tuple(m for m in LORA_MODULES if m in target_modules)
        self.capacity, self.lora_rank, self.num_layers = capacity, lora_rank, config.num_hidden_layers
        self.mgr = {m: LoraManager(capacity, config.num_hidden_layers, *dims[m], lora_rank, dtype, device) for m in self.target_modules}
        self._free = set(range(capacity))

    @property
    def device(self):
        return next(iter(self.mgr.values())).device

    def alloc(self) -> LlamaLoraWeight:
        idx = min(self._free)
        self._free.remove(idx)
        return LlamaLoraWeight(idx, {m: mgr.alloc(idx) for m, mgr in self.mgr.items()})

    def free(self, weight: LlamaLoraWeight):
        for m, w in weight.modules.items():
            self.mgr[m].free(w)
        self._free.add(weight.idx)

    def load(self, weight: LlamaLoraWeight, layer_idx: int, module: str, A: torch.Tensor, B: torch.Tensor, alpha: float = None):
        """``A`` [r, in], ``B`` [out, r] of one projection of one layer, in the channel order of the module docstring."""
        if module not in self.mgr:
            raise KeyError(f"{module} is not a target module of this manager {self.target_modules}")
        weight.load(layer_idx, module, A, B, alpha)


def permute_intermediate(module: str, A: torch.Tensor, B: torch.Tensor, index: torch.Tensor):
    """A PEFT-order adapter of ``module`` in the order of the packed intermediate channels: packed row j of gate_proj / up_proj is
    original row ``index[j]``.  gate_proj / up_proj: B's rows are gathered; down_proj: A's columns; every other projection is returned
    as it is (its channels are in the original order on both sides)."""
    idx = index.to(torch.long)
    if module in ("gate_proj", "up_proj"):
        return A, B[idx.to(B.device)]
    if module == "down_proj":
        return A[:, idx.to(A.device)], B
    return A, B
