"""The MoE-on-MX entry points without a device: their argument checks, with pointers that are never dereferenced."""
import pytest

from atom_amd import _lib

P, ODD = 0x10000, 0x10001
GOOD = dict(a=P, w=P, idx=P, tab=P, out0=P, out1=P, A_rows=4, R=8, E=4, N_seg=64, nseg=2, K=256)


def gemm(**kw):
    a = {**GOOD, **kw}
    return _lib.lib().atom_moe_gemm_mxfp4_f16(a["a"], P, P, a["w"], P, P, a["idx"], a["tab"], P, P, P, a["out0"], a["out1"], a["A_rows"], a["R"],
                                              a["E"], a["N_seg"], a["nseg"], a["K"], None)


def silu(rows=4, K=256, gate=P, up=P, q4=P):
    return _lib.lib().atom_silu_mul_quant_mx_f16(gate, up, rows, K, q4, P, P, None)


@pytest.mark.parametrize("kw,err", [
    (dict(K=128), _lib.ERR_SHAPE), (dict(K=320), _lib.ERR_SHAPE), (dict(N_seg=96), _lib.ERR_SHAPE), (dict(N_seg=0), _lib.ERR_SHAPE),
    (dict(E=0), _lib.ERR_SHAPE), (dict(E=65), _lib.ERR_SHAPE), (dict(R=0), _lib.ERR_SHAPE), (dict(A_rows=0), _lib.ERR_SHAPE),
    (dict(nseg=3), _lib.ERR_INVALID_ARG), (dict(nseg=0), _lib.ERR_INVALID_ARG), (dict(out1=None), _lib.ERR_INVALID_ARG),
    (dict(a=None), _lib.ERR_INVALID_ARG), (dict(w=None), _lib.ERR_INVALID_ARG), (dict(tab=None), _lib.ERR_INVALID_ARG),
    (dict(out0=None), _lib.ERR_INVALID_ARG),
    (dict(a=ODD), _lib.ERR_ALIGN), (dict(w=ODD), _lib.ERR_ALIGN), (dict(out0=ODD), _lib.ERR_ALIGN), (dict(out1=ODD), _lib.ERR_ALIGN),
    (dict(idx=ODD), _lib.ERR_ALIGN), (dict(tab=ODD), _lib.ERR_ALIGN),
])
def test_routed_gemm_checks_arguments_before_any_launch(kw, err):
    assert gemm(**kw) == err


def test_silu_quantiser_checks_arguments_before_any_launch():
    assert silu(K=128) == silu(K=320) == silu(rows=0) == _lib.ERR_SHAPE
    assert silu(gate=None) == silu(up=None) == silu(q4=None) == _lib.ERR_INVALID_ARG
    assert silu(gate=ODD) == silu(up=ODD) == silu(q4=ODD) == _lib.ERR_ALIGN
