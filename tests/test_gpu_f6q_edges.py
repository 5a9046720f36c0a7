"""Edges of the 256x256 BF6 kernel (gemm_w4a4_f6q_kernel, the instantiation for weights whose channel pairs share their scales).

f6_pick_cfg sends a shape there from 129 tiles of 256 x 256, so the shapes here have 9 x 15 = 135 tiles: M = 2304, N = 3840.
Every number of int4 groups G from 1 to 10 (K = 128 (G + 1)) walks the prologue with and without the early second stage, all three
residues of the K loop that is unrolled by 3, and both generic tail steps; the ragged shapes put whole tiles (the store path with a
scalar base) and ragged ones (the checked stores) into one launch.  Every shape runs twice back to back on different operands, so
that what the first launch left in LDS differs from what the second one must read."""
import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests.helpers import bits16, f6_codes, rand_gemm_operands, t2n, to_device

pytestmark = pytest.mark.gpu

M0, N0 = 2304, 3840
SHAPES = [(M0, N0, 128 * (G + 1)) for G in range(1, 11)] + [(2100, 3840, 896), (2304, 3776, 640)]


def _ops():
    from atom_amd import ops
    return ops


def _f6_run(ops, d, t):
    a6 = torch.from_numpy(f6_codes(d["qa4"], d["sA"])).cuda()
    b6 = ops.repack_weight_f6(t[1], t[3])
    assert getattr(b6, "atom_f6s", None) is not None and b6.atom_pairs          # fp32 weight scales, shared by channel pairs
    return ops.dense_layer_gemm_i4_fp16(a6, b6, *t[2:], scale_layout="plain", a_wide="f6")


def _int8_run(ops, t, M, N, K):
    """atom_gemm_w4a4_f16 itself (no workspace): the INT8 MFMA tile kernel on the packed operands."""
    D = torch.empty((M, N), dtype=torch.float16, device="cuda")
    st = ops.L.lib().atom_gemm_w4a4_f16(*[x.data_ptr() for x in t], D.data_ptr(), M, N, K, 128, 128, ops.L.SCALE_LAYOUT_PLAIN,
                                        ops.L.current_stream(D.device))
    ops.L.check(st, "atom_gemm_w4a4_f16")
    return D


def _sample_rows(M, seed):
    """24 rows: the first and last rows of the output and of one tile row, both rows of a record pair, the rest drawn."""
    fixed = [0, 1, 30, 31, 32, 33, 127, 128, 255, 256, M - 257, M - 256, M - 2, M - 1]
    rest = np.random.default_rng(seed).permutation(M)
    rows = list(dict.fromkeys(fixed + [int(r) for r in rest]))[:24]
    return np.sort(np.array(rows))


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_f6q_every_loop_residue_and_store_path_bit_exact(M, N, K):
    from tests import c_oracle
    ops = _ops()
    assert ((M + 255) // 256) * ((N + 255) // 256) == 135
    for seed in (K + M, 7 * K + N + 1):                                       # twice, back to back, on different operands
        d = rand_gemm_operands(M, N, K, seed=seed)
        t = to_device(d, "plain")
        out = _f6_run(ops, d, t)
        int8 = _int8_run(ops, t, M, N, K)
        assert out.shape == (M, N) and torch.equal(out, int8), (M, N, K, seed)
        rows = _sample_rows(M, seed)
        want = c_oracle.gemm(O.pack_int4(d["qa4"][rows]), O.pack_int4(d["qb4"]), np.ascontiguousarray(d["sA"][rows].T), d["sB"],
                             d["qa8"][rows], d["qb8"], d["sA8"][rows], d["sB8"])
        assert np.array_equal(bits16(t2n(out)[rows]), bits16(want)), (M, N, K, seed)


def _planted(M, N, K):
    """All int4 codes +1, keeper codes 0, scales that differ between adjacent token rows, between the 32 rows of a record group,
    between groups of consecutive stages and between channel pairs -- all exact in fp16, every product and sum exact in fp32."""
    G = (K - 128) // 128
    m, g, n = np.arange(M), np.arange(G), np.arange(N)
    d = dict(
        qa4=np.ones((M, K - 128), np.int8), qb4=np.ones((N, K - 128), np.int8),
        qa8=np.zeros((M, 128), np.int8), qb8=np.zeros((N, 128), np.int8),
        sA=((1 + m % 32)[:, None] * (1 + g % 3)[None, :] * 2.0 ** -8).astype(np.float16),      # [M, G]
        sB=np.broadcast_to(((1 + (n // 2) % 16) * 2.0 ** -6)[None, :], (G, N)).astype(np.float16).copy(),
        sA8=np.full((M,), 0.25, np.float16), sB8=np.full((N,), 0.5, np.float16),
    )
    return d


def test_f6q_planted_scales_cannot_be_swapped():
    """With every integer dot product equal to 128, an output is 128 * sum_g sA[g][m] * sB[g][n]: a token scale taken from the partner
    row of its record pair, from another block pair or from the wrong stage changes it.  Expected value: float64, rounded to fp16 once
    (every intermediate is exact in fp32, so this IS the contract's value), and the C restatement of the contract on 64 rows."""
    from tests import c_oracle
    ops = _ops()
    M, N, K = M0, N0, 128 * 8                                                 # G = 7: early second stage, loop once, one regular tail step, both generic ones
    d = _planted(M, N, K)
    G = (K - 128) // 128
    assert np.array_equal(d["sA"].astype(np.float64), (1 + np.arange(M) % 32)[:, None] * (1 + np.arange(G) % 3)[None, :] * 2.0 ** -8)
    want64 = 128.0 * (d["sA"].astype(np.float64) @ d["sB"].astype(np.float64))
    want = want64.astype(np.float16)
    assert np.isfinite(want).all()
    assert (want[0::2] != want[1::2]).all()                                   # the two rows of a record pair never agree
    w1 = (128.0 * (d["sA"][:, :G - 1].astype(np.float64) @ d["sB"][:G - 1].astype(np.float64))).astype(np.float16)
    assert (w1 != want).all()                                                 # ... and neither does a sum that misses a stage
    t = to_device(d, "plain")
    # a random launch first: LDS holds other scales when the planted one starts
    d0 = rand_gemm_operands(M, N, K, seed=99)
    _f6_run(ops, d0, to_device(d0, "plain"))
    out = _f6_run(ops, d, t)
    assert np.array_equal(bits16(t2n(out)), bits16(want))
    rows = np.r_[0:32, M - 32:M]
    ref = c_oracle.gemm(O.pack_int4(d["qa4"][rows]), O.pack_int4(d["qb4"]), np.ascontiguousarray(d["sA"][rows].T), d["sB"],
                        d["qa8"][rows], d["qb8"], d["sA8"][rows], d["sB8"])
    assert np.array_equal(bits16(t2n(out)[rows]), bits16(ref))
