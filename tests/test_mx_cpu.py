"""MXFP4 W4A4 without a device: the layout converters of atom_amd.ops and the argument checks of the three C entry points."""
import pytest
import torch

from atom_amd import _lib, ops


def _plain(rows, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    u8 = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, generator=g)   # noqa: E731
    return u8(rows, (k - 128) // 2), u8(rows, (k - 128) // 32), u8(rows, 128), u8(rows, 4)


@pytest.mark.parametrize("rows,k", [(1, 256), (16, 384), (37, 640)])
def test_plain_native_round_trip(rows, k):
    plain = _plain(rows, k)
    o = ops.mx_from_plain(*plain)
    r, s = (rows + 15) // 16, k // 128 - 1
    assert (o.rows, o.k) == (rows, k) and o.q4.shape == (r, s, 64, 16) and o.sc.shape == (r, s + 1, 64) and o.q8.shape == (r, 2, 64, 16)
    for a, b in zip(ops.mx_to_plain(o), plain):
        assert torch.equal(a, b)
    # the fragment order itself: lane = row % 16 + 16 * (block % 4) holds that block's 16 E2M1 code bytes and its scale byte
    codes, scales, k8, s8 = plain
    for row, blk in [(0, 0), (rows - 1, 4 * s - 1), (rows // 2, 2)]:
        t, lane, st = row // 16, row % 16 + 16 * (blk % 4), blk // 4
        assert torch.equal(o.q4[t, st, lane], codes[row, 16 * blk:16 * blk + 16]) and o.sc[t, st, lane] == scales[row, blk]
        kb = blk % 4                                          # keeper: half h of the lane holds channels 64 h + 16 kb .. + 15
        assert torch.equal(torch.cat([o.q8[t, 0, lane], o.q8[t, 1, lane]]), torch.cat([k8[row, 16 * kb:16 * kb + 16], k8[row, 64 + 16 * kb:80 + 16 * kb]]))
        assert o.sc[t, s, lane] == s8[row, kb]
    if rows % 16:                                             # padding rows: zero codes, unit scales
        assert int(o.q4[-1, :, 15::16].max()) == 0 and int(o.q8[-1, :, 15::16].max()) == 0 and bool((o.sc[-1, :, 15::16] == 127).all())


def test_entry_points_check_arguments_before_any_launch():
    L = _lib.lib()
    P, ODD = 0x10000, 0x10001                                 # never dereferenced: every call below fails its checks
    quant = lambda M, K, x=P, q4=P: L.atom_reorder_quant_mx_f16(x, P, M, K, q4, P, P, None)        # noqa: E731
    wq = lambda N, K, w=P, sc=P: L.atom_quant_weight_mx_f16(w, N, K, P, sc, P, None)               # noqa: E731
    gemm = lambda M, N, K, a=P, o=P: L.atom_gemm_mxfp4_f16(a, P, P, P, P, P, o, M, N, K, None)     # noqa: E731
    for bad in (128, 320, 0):
        assert quant(4, bad) == wq(64, bad) == gemm(4, 64, bad) == _lib.ERR_SHAPE
    assert quant(0, 256) == gemm(0, 64, 256) == wq(0, 256) == _lib.ERR_SHAPE
    assert wq(96, 256) == gemm(4, 96, 256) == gemm(4, 32, 256) == _lib.ERR_SHAPE
    assert quant(4, 256, x=None) == wq(64, 256, w=None) == gemm(4, 64, 256, a=None) == gemm(4, 64, 256, o=None) == _lib.ERR_INVALID_ARG
    assert quant(4, 256, q4=ODD) == quant(4, 256, x=ODD) == wq(64, 256, sc=ODD) == gemm(4, 64, 256, a=ODD) == gemm(4, 64, 256, o=ODD) == _lib.ERR_ALIGN
    route = L.atom_gemm_mxfp4_route
    assert [route(m, 4096, 4096) for m in (1, 16, 17, 4096)] == [1, 1, 2, 2]
    assert route(0, 64, 256) == route(4, 64, 128) == route(4, 96, 256) == route(4, 64, 300) == 0
    assert ops.gemm_mxfp4_route(16, 64, 256) == "decode" and ops.gemm_mxfp4_route(17, 64, 256) == "tile" and ops.gemm_mxfp4_route(1, 64, 128) is None
