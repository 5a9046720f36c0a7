"""Dense Llama on MXFP4 without a device: the argument checks and route query of the new entry points, the fused weight's interleave."""
import pytest
import torch

from atom_amd import _lib, ops


def test_entry_points_check_arguments_before_any_launch():
    L = _lib.lib()
    P, ODD = 0x10000, 0x10001                                 # never dereferenced: every call below fails its checks
    gu = lambda M, F, K, a=P, o=P: L.atom_gemm_mxfp4_silu_mul_quant(a, P, P, P, P, P, P, o, P, M, F, K, None)            # noqa: E731
    rms = lambda M, K, x=P, w=P, q4=P: L.atom_rmsnorm_quant_mx_f16(x, w, P, M, K, 1e-5, q4, P, P, None)                  # noqa: E731
    arms = lambda M, K, x=P, r=P, q4=P: L.atom_add_rmsnorm_quant_mx_f16(x, r, P, P, M, K, 1e-5, q4, P, P, None)          # noqa: E731
    add = lambda M, N, K, a=P, r=P, o=P: L.atom_gemm_mxfp4_add_f16(a, P, P, P, P, P, r, o, M, N, K, None)                # noqa: E731
    for bad in (128, 320, 0):
        assert gu(4, 256, bad) == rms(4, bad) == arms(4, bad) == add(4, 64, bad) == _lib.ERR_SHAPE
    assert gu(0, 256, 256) == rms(0, 256) == arms(0, 256) == add(0, 64, 256) == _lib.ERR_SHAPE
    assert gu(4, 128, 256) == gu(4, 320, 256) == gu(4, 0, 256) == add(4, 96, 256) == rms(4, 16384 + 128) == _lib.ERR_SHAPE
    assert gu(4, 256, 256, a=None) == gu(4, 256, 256, o=None) == rms(4, 256, x=None) == rms(4, 256, w=None) == _lib.ERR_INVALID_ARG
    assert arms(4, 256, r=None) == arms(4, 256, q4=None) == add(4, 64, 256, r=None) == add(4, 64, 256, o=None) == _lib.ERR_INVALID_ARG
    assert gu(4, 256, 256, a=ODD) == gu(4, 256, 256, o=ODD) == rms(4, 256, x=ODD) == rms(4, 256, q4=ODD) == _lib.ERR_ALIGN
    assert arms(4, 256, r=ODD) == add(4, 64, 256, r=ODD) == add(4, 64, 256, a=ODD) == _lib.ERR_ALIGN


def test_route_query():
    route = _lib.lib().atom_gemm_mxfp4_silu_mul_quant_route
    assert [route(m, f, k) for m in (1, 16, 17, 129) for k in (256, 640) for f in (256, 384)] == [1] * 8 + [2] * 8
    assert [route(m, 11008, 4096) for m in (1, 16, 256, 2048)] == [1, 1, 2, 2]
    assert route(0, 256, 256) == route(4, 128, 256) == route(4, 320, 256) == route(4, 256, 128) == route(4, 256, 300) == 0
    assert ops.gate_up_silu_quant_mx_route(16, 256, 256) == "decode" and ops.gate_up_silu_quant_mx_route(17, 256, 256) == "tile"
    assert ops.gate_up_silu_quant_mx_route(4, 192, 256) is None


@pytest.mark.parametrize("F,K", [(256, 256), (384, 640)])
def test_fuse_gate_up_mx_interleaves_fragment_pairs(F, K):
    g = torch.Generator().manual_seed(F + K)
    r, s = F // 16, K // 128 - 1
    mk = lambda: ops.MxOperand(*(torch.randint(0, 256, sh, dtype=torch.uint8, generator=g)                             # noqa: E731
                                 for sh in ((r, s, 64, 16), (r, s + 1, 64), (r, 2, 64, 16))), F, K)
    gate, up = mk(), mk()
    fused = ops.fuse_gate_up_mx(gate, up)
    assert (fused.rows, fused.k) == (2 * F, K)
    for f in range(2 * r):                                    # fused fragment f: pair f // 4, gate (f % 4 < 2) or up, member f % 2
        src, frag = (gate if f % 4 < 2 else up), 2 * (f // 4) + f % 2
        assert all(torch.equal(getattr(fused, n)[f], getattr(src, n)[frag]) for n in ("q4", "sc", "q8"))
    with pytest.raises(ValueError):
        ops.fuse_gate_up_mx(gate, ops.MxOperand(up.q4[:-1], up.sc[:-1], up.q8[:-1], F - 16, K))
