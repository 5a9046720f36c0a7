"""MXFP6 weights without a device: the new entry points' argument checks, the fused operand, the config switch."""
import pytest
import torch

from atom_amd import _lib, ops
from tests.test_gpu_llama_mx import _cfg


def test_entry_points_check_arguments_before_any_launch():
    L = _lib.lib()
    P, ODD = 0x10000, 0x10001                                 # never dereferenced: every call below fails its checks
    wq = lambda N, K, x=P, q=P: L.atom_quant_weight_mx6_f16(x, N, K, q, P, P, None)                                                  # noqa: E731
    mm = lambda M, N, K, a=P, r=None, o=P, ab=6, wb=6: L.atom_gemm_mx_f16(a, P, P, P, P, P, r, o, M, N, K, ab, wb, None)              # noqa: E731
    gu = lambda M, F, K, a=P, o=P, ab=6, wb=6, ob=6: L.atom_gemm_mx_silu_mul_quant(a, P, P, P, P, P, o, P, P, M, F, K, ab, wb, ob, None)   # noqa: E731
    for bad in (128, 320, 0):
        assert wq(64, bad) == mm(4, 64, bad) == gu(4, 256, bad) == _lib.ERR_SHAPE
    assert wq(0, 256) == mm(0, 64, 256) == mm(4, 96, 256) == gu(4, 320, 256) == gu(0, 256, 256) == _lib.ERR_SHAPE
    assert wq(64, 256, x=None) == wq(64, 256, q=None) == mm(4, 64, 256, a=None) == mm(4, 64, 256, o=None) == gu(4, 256, 256, a=None) == _lib.ERR_INVALID_ARG
    assert mm(4, 64, 256, ab=5) == mm(4, 64, 256, wb=8) == gu(4, 256, 256, ab=0) == gu(4, 256, 256, wb=5) == gu(4, 256, 256, ob=8) == _lib.ERR_INVALID_ARG
    assert wq(64, 256, q=ODD) == mm(4, 64, 256, r=ODD) == mm(4, 64, 256, a=ODD, wb=4) == gu(4, 256, 256, o=ODD) == _lib.ERR_ALIGN


def test_fused_gate_up_operand_needs_the_keyword():
    g, s = torch.Generator().manual_seed(3), 2
    w6 = [ops.mx_from_plain(*(torch.randint(0, 256, (64, w), dtype=torch.uint8, generator=g) for w in (96 * s, 4 * s, 128, 4))) for _ in range(2)]
    w4 = ops.mx_from_plain(*(torch.randint(0, 256, (64, w), dtype=torch.uint8, generator=g) for w in (64 * s, 4 * s, 128, 4)))
    for call in (lambda: ops.fuse_gate_up_mx(*w6), lambda: ops.fuse_gate_up_mx(w4, w4, weight_format="mxfp6"),
                 lambda: ops.fuse_gate_up_mx(*w6, weight_format="fp6"), lambda: ops.quant_weight_mx(torch.zeros(64, 256), weight_format="fp6")):
        with pytest.raises(ValueError):
            call()
    gu = ops.fuse_gate_up_mx(*w6, weight_format="mxfp6")
    assert (gu.rows, gu.k) == (128, 384) and tuple(gu.q4.shape) == (8, s, 96, 16) and ops._mx_native(gu)
    for f in range(8):                                        # [g0 g1 u0 u1 g2 g3 u2 u3]
        assert all(torch.equal(getattr(gu, n)[f], getattr(w6[(f // 2) % 2], n)[2 * (f // 4) + f % 2]) for n in ("q4", "sc", "q8")), f


@pytest.mark.parametrize("kw", [dict(weight_format="mxfp6"), dict(weight_format={"o_proj": "mxfp6"}), dict(linear_format="mxfp4", weight_format="fp6"),
                                dict(linear_format="mxfp4", weight_format={"q_proj": "mxfp6"}), dict(linear_format="mxfp4", weight_format={"qkv": "int4"}),
                                dict(linear_format="mxfp4", weight_format={"o_proj": "mxfp6", "down_proj": "mxfp6"})])
def test_weight_format_is_checked_and_reaches_its_groups(kw):
    from atom_amd.e2e import LlamaForCausalLM
    if "down_proj" not in kw["weight_format"]:
        with pytest.raises(ValueError):
            LlamaForCausalLM(_cfg(**kw))
        return
    at, mlp = (lambda layer: (layer.self_attn, layer.mlp))(LlamaForCausalLM(_cfg(**kw)).model.layers[1])
    assert [m.weight_fp4.shape[2] for m in (at.q_proj, at.k_proj, at.v_proj, at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj)] == [64, 64, 64, 96, 64, 64, 96]
