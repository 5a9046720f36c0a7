"""The MX form of the mixed-precision linear layer: MXFP4 channels, an MXFP8 keeper, both on the scaled MFMA."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops


class LinearMxfp4(nn.Module):
    """``forward(x_fp16, reorder_index)`` = quantise the reordered activation to MX, then the MXFP4 GEMM against the MX weight."""

    def __init__(self, in_features, out_features):
        super().__init__()
        if in_features % 128 or in_features < 256 or out_features % 64 or out_features < 64:
            raise ValueError("LinearMxfp4: in_features a multiple of 128 (>= 256), out_features a multiple of 64")
        self.in_features, self.out_features = in_features, out_features
        r, s = out_features // 16, in_features // 128 - 1
        self.weight_fp4 = nn.Parameter(torch.empty(r, s, 64, 16, dtype=torch.uint8), requires_grad=False)
        self.weight_scale = nn.Parameter(torch.empty(r, s + 1, 64, dtype=torch.uint8), requires_grad=False)
        self.weight_fp8 = nn.Parameter(torch.empty(r, 2, 64, 16, dtype=torch.uint8), requires_grad=False)

    @torch.no_grad()
    def load_fp16_weight(self, weight: torch.Tensor):
        """Fill the parameters from a (column-reordered) fp16 weight [out, in]."""
        if tuple(weight.shape) != (self.out_features, self.in_features):
            raise ValueError(f"weight must be [{self.out_features}, {self.in_features}], got {tuple(weight.shape)}")
        w = ops.quant_weight_mx(weight.contiguous())
        self.weight_fp4.data, self.weight_scale.data, self.weight_fp8.data = w.q4, w.sc, w.q8
        return self

    def weight_mx(self) -> ops.MxOperand:
        return ops.MxOperand(self.weight_fp4.data, self.weight_scale.data, self.weight_fp8.data, self.out_features, self.in_features)

    def forward(self, x, reorder_index=None):
        lead = x.shape[:-1]
        y = ops.gemm_mxfp4(ops.reorder_quant_mx(x.reshape(-1, self.in_features).contiguous(), reorder_index), self.weight_mx())
        return y.view(*lead, self.out_features)
