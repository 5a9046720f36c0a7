"""MXFP6 activations without a device: the E2M3 reference, the plain <-> native conversion, the new entry points' argument checks."""
import numpy as np
import pytest
import torch

from atom_amd import _lib, ops
from tests import mx6_ref as R6
from tests import mx_ref as R


def test_e2m3_reference_round_trips_all_codes():
    codes = np.arange(64, dtype=np.uint8).reshape(2, 32)
    v = R.decode(codes, "e2m3")
    assert v.max() == 7.5 and v[0, 1] == 0.125 and v[0, 8] == 1.0 and v[1, 0] == 0 and v[1, 31] == -7.5
    got, scale = R.quantise(v, "e2m3")                        # amax 7.5: scale byte 127; -0 (code 0x20) comes back as code 0
    assert (scale == 127).all() and np.array_equal(got, np.where(codes == 0x20, 0, codes))
    assert np.array_equal(R6.unpack6(R6.pack6(codes)), codes) and R6.pack6(codes).shape == (2, 24)
    assert R6.pack6(np.array([[1] + [0] * 30 + [0x20]]))[0].tolist() == [1] + [0] * 22 + [0x80]


@pytest.mark.parametrize("rows,K", [(1, 256), (17, 384), (32, 640)])
def test_plain_native_conversion_is_an_inverse_for_mxfp6(rows, K):
    g, s = torch.Generator().manual_seed(rows + K), K // 128 - 1
    plain = tuple(torch.randint(0, 256, (rows, w), dtype=torch.uint8, generator=g) for w in (96 * s, 4 * s, 128, 4))
    o = ops.mx_from_plain(*plain)
    assert tuple(o.q4.shape) == ((rows + 15) // 16, s, 96, 16) and ops._mx_native(o) and (o.rows, o.k) == (rows, K)
    assert all(torch.equal(a, b) for a, b in zip(ops.mx_to_plain(o), plain))
    # row 0, block 1 of step 0 is lane 16: head piece 16, the first half of tail piece 64 + 8
    assert torch.equal(torch.cat([o.q4[0, 0, 16], o.q4[0, 0, 72, :8]]), plain[0][0, 24:48])
    for call in (lambda: ops.mx_from_plain(plain[0][:, :-1], *plain[1:]), lambda: ops.fuse_gate_up_mx(o, o), lambda: ops.reorder_quant_mx(plain[0], act_format="fp6")):
        with pytest.raises(ValueError):
            call()


def test_entry_points_check_arguments_before_any_launch():
    L = _lib.lib()
    P, ODD = 0x10000, 0x10001                                 # never dereferenced: every call below fails its checks
    rq = lambda M, K, x=P, q=P: L.atom_reorder_quant_mx6_f16(x, None, M, K, q, P, P, None)                               # noqa: E731
    rms = lambda M, K, x=P, q=P: L.atom_rmsnorm_quant_mx6_f16(x, P, P, M, K, 1e-5, q, P, P, None)                       # noqa: E731
    arms = lambda M, K, r=P, q=P: L.atom_add_rmsnorm_quant_mx6_f16(P, r, P, P, M, K, 1e-5, q, P, P, None)               # noqa: E731
    mm = lambda M, N, K, a=P, r=None, o=P: L.atom_gemm_mxfp4_a6_f16(a, P, P, P, P, P, r, o, M, N, K, None)               # noqa: E731
    gu = lambda M, F, K, a=P, o=P, ab=6, ob=6: L.atom_gemm_mxfp4_a6_silu_mul_quant(a, P, P, P, P, P, o, P, P, M, F, K, ab, ob, None)   # noqa: E731
    for bad in (128, 320, 0):
        assert rq(4, bad) == rms(4, bad) == arms(4, bad) == mm(4, 64, bad) == gu(4, 256, bad) == _lib.ERR_SHAPE
    assert rq(0, 256) == rms(0, 256) == arms(0, 256) == mm(0, 64, 256) == mm(4, 96, 256) == gu(4, 320, 256) == gu(0, 256, 256) == _lib.ERR_SHAPE
    assert rq(4, 256, x=None) == rms(4, 256, q=None) == arms(4, 256, r=None) == mm(4, 64, 256, a=None) == mm(4, 64, 256, o=None) == _lib.ERR_INVALID_ARG
    assert gu(4, 256, 256, a=None) == gu(4, 256, 256, ab=5) == gu(4, 256, 256, ob=8) == _lib.ERR_INVALID_ARG
    assert rq(4, 256, q=ODD) == rms(4, 256, x=ODD) == arms(4, 256, r=ODD) == mm(4, 64, 256, r=ODD) == gu(4, 256, 256, o=ODD) == _lib.ERR_ALIGN
