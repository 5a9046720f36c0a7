"""The scale-product tiles of the 256x256 BF6 kernel (gemm_w4a4_f6q_kernel: scale_tile4, one v_mfma_f32_16x16x1 per four pair slots
in place of sixteen multiplies; lane l supplies the scales of token l % 16 and of channel pair l % 16 of slot l / 16) on planted
scales, bit for bit, through atom_gemm_w4a4_f16 with ATOM_AB_F6 | ATOM_B_F6S, with and without ATOM_B_SCALE_PAIRS.

Shapes.  One workgroup tile of that kernel is 256 x 256, and K = 7 * 128 + 128 (G = 7 >= 6) walks the regular first step, the
compile-time-slot bodies and both generic tail steps.  f6_pick_cfg sends a shape to that kernel only from 129 of its tiles, so every
case runs at 256 x 256 (whatever kernel the dispatch picks for one tile: the mid-size one today) AND at 768 x 11008 = 3 x 43 = 129
tiles, which the 256x256 kernel takes; the random case likewise at 512 x 512 and at 768 x 11008 with K = 12 * 128 + 128 (the main loop
runs twice).

References: the exact value (float64 on exact integer dot products, rounded to fp16 once -- tests/gemm_planted.expected) wherever
every partial sum is an FP32 number whatever the order, and the C restatement of the contract (tests/c_oracle.gemm in the order
atom_gemm_w4a4_f6_order names) -- on every row of the one-tile shape, on sampled rows of the large one."""
import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import c_oracle as CO
from tests import gemm_planted as P
from tests import gemm_route_cases as C
from tests.helpers import bits16, rand_gemm_operands

pytestmark = pytest.mark.gpu

K7 = 7 * 128 + 128
K12 = 12 * 128 + 128
ONE_TILE = (256, 256)
Q_TILES = (768, 11008)                                           # 129 tiles of 256 x 256: the 256x256 kernel's own shape
POS = 5                                                          # the one code position of a group that is not zero
FLAGS = {"pairs": C.AB_F6 | C.B_F6S | C.PAIRS, "own": C.AB_F6 | C.B_F6S}


def _lib():
    from atom_amd import _lib
    return _lib.lib()


def _takes_q_kernel(M, N, K):
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    return t256 >= 129 and (t256 + 255) // 256 == 1 and ((M + 63) // 64) * (N // 64) > 512


def _run(d, M, N, K, flags):
    """D of atom_gemm_w4a4_f16 on the operand dict d (numpy, fp16 [M, N])"""
    src = dict(A4=O.pack_int4(d["qa4"]), B4=O.pack_int4(d["qb4"]), A8=d["qa8"], B8=d["qb8"], sA=np.ascontiguousarray(d["sA"].T),
               sA8=d["sA8"], sB=np.ascontiguousarray(d["sB"]), sB8=d["sB8"])
    st, dev, outs = C.call(("f6q_scale_tile", "f16", M, N, K, dict(flags=flags)), src=src)
    assert st == 0, f"status {st}"
    return dev.get("D")


def _oracle(d, M, N, K, rows):
    order = {1: 1, 2: -2, 4: -4}[_lib().atom_gemm_w4a4_f6_order(M, N, K)]
    return CO.gemm(O.pack_int4(d["qa4"][rows]), O.pack_int4(d["qb4"]), np.ascontiguousarray(d["sA"][rows].T), d["sB"], d["qa8"][rows],
                   d["qb8"], d["sA8"][rows], d["sB8"], nsplit=order)


def _rows(M):
    """every row of one tile; of a larger shape the first and last 32 (both rows of 16 record pairs, blocks 0-1 and 6-7 of a wave
    tile) and 16 rows inside the second tile row"""
    return np.arange(M) if M <= 256 else np.r_[0:32, 356:372, M - 32:M]


def _empty(M, N, K):
    G = K // 128 - 1
    return dict(qa4=np.zeros((M, K - 128), np.int8), qb4=np.zeros((N, K - 128), np.int8), qa8=np.zeros((M, 128), np.int8),
                qb8=np.zeros((N, 128), np.int8), sA=np.zeros((M, G), np.float16), sB=np.zeros((G, N), np.float16),
                sA8=np.ones((M,), np.float16), sB8=np.ones((N,), np.float16))


def _sb_planted(n, g, paired):
    """the weight scale that names its channel pair (16 values), or its channel (32 values), rotated by g"""
    return 1 + ((n // 2 + g) % 16) / 16.0 if paired else 1 + ((n + g) % 32) / 32.0


def _decode(v, idot, paired):
    """what a planted output names: (token within its block, channel pair or channel within its 16 / 32)"""
    if idot == 0 or not np.isfinite(v) or v == 0:
        return "nothing (%r)" % float(v)
    m, e = np.frexp(abs(float(v)) / abs(int(idot)))              # m in [0.5, 1)
    return "token %d of its block, %s %g" % (e - 1 + 12, "pair" if paired else "channel", (2 * m - 1) * (16 if paired else 32))


def _first_wrong(got, want, d_idot, paired, what):
    bad = np.argwhere(bits16(got) != bits16(want))
    if len(bad) == 0:
        return None
    m, n = (int(x) for x in bad[0])
    idot = d_idot(m, n)
    return (f"{what}: {len(bad)} of {got.size} outputs differ; first at (m, n) = ({m}, {n}): got {float(got[m, n])!r} = "
            f"{_decode(got[m, n], idot, paired)}, expected {float(want[m, n])!r} = {_decode(want[m, n], idot, paired)}")


# ------------------------------------------------------------------------------------------------ planted scales, one group
def _planted(M, N, K, g0, paired):
    """codes zero except position POS of group g0, where idot is a small signed integer that depends on (m / 16, n / 16);
    sA[g0, m] = 2^((m % 16) - 12), sB[g0, .] = 1 + (pair % 16) / 16 (own scales: 1 + (n % 32) / 32): every output is exact in fp16,
    its exponent names the token within its block and its mantissa the channel pair.  The other groups carry other scales on zero
    codes."""
    d = _empty(M, N, K)
    G = K // 128 - 1
    m, n, g = np.arange(M), np.arange(N), np.arange(G)
    a = (1 + (m // 16) % 3).astype(np.int8)
    b = ((1 + (n // 16) % 2) * np.where((n // 16) % 3 == 1, -1, 1)).astype(np.int8)
    d["qa4"][:, 128 * g0 + POS] = a
    d["qb4"][:, 128 * g0 + POS] = b
    d["sA"][:] = np.ldexp(1.0, -((m[:, None] + g[None, :]) % 8)) * 3
    d["sB"][:] = 1.5
    d["sA"][:, g0] = np.ldexp(1.0, (m % 16) - 12)
    d["sB"][g0] = _sb_planted(n, 0, paired)
    return d, (lambda i, j: int(a[i]) * int(b[j]))


@pytest.mark.parametrize("M,N", [ONE_TILE, Q_TILES])
@pytest.mark.parametrize("g0", [0, 1, 4, 5, 6])     # the first step, a compile-time-slot body, the last such step, the two generic tail steps
@pytest.mark.parametrize("tag", ["pairs", "own"])
def test_planted_scales_name_their_token_and_channel_pair(M, N, g0, tag):
    K, paired = K7, tag == "pairs"
    assert _takes_q_kernel(*Q_TILES, K) and _lib().atom_gemm_w4a4_f6_order(*Q_TILES, K) == 1
    d, idot = _planted(M, N, K, g0, paired)
    assert P.pairs_shared(d) == paired
    want64 = P.sums(d).numpy()
    want = want64.astype(np.float16)
    assert np.array_equal(want.astype(np.float64), want64) and (want != 0).all()          # every output exact in fp16
    assert (want[0::2] != want[1::2]).all() and (want[:, 0:-2] != want[:, 2:]).all()      # neighbouring tokens and pairs never agree
    got = _run(d, M, N, K, FLAGS[tag])
    msg = _first_wrong(got, want, idot, paired, f"{M}x{N} group {g0} [{tag}]")
    assert msg is None, msg
    rows = _rows(M)
    assert np.array_equal(bits16(got[rows]), bits16(_oracle(d, M, N, K, rows)))


# ------------------------------------------------------------------------------------------------ ring timing: every group its own scales
def _ring(M, N, K, paired):
    """idot = +-1 in every group, sA[g, m] and sB[g, .] the planted values rotated by g: a token scale or a weight scale that arrives
    one slot, one block or one stage early or late changes the sum.  Every term is a multiple of u = 2^-16 (own scales: 2^-17) and the
    terms' absolute sum stays below 2^24 u (asserted), so every order of summation gives the exact sum."""
    d = _empty(M, N, K)
    G = K // 128 - 1
    m, n = np.arange(M), np.arange(N)
    for g in range(G):
        d["qa4"][:, 128 * g + POS] = 1
        d["qb4"][:, 128 * g + POS] = np.where((n // 16 + g) % 2 == 1, -1, 1)
        d["sA"][:, g] = np.ldexp(1.0, ((m + g) % 16) - 12)
        d["sB"][g] = _sb_planted(n, g, paired)
    u = 2.0 ** (-17 if not paired else -16)
    assert (np.abs(d["sA"].astype(np.float64)) @ np.abs(d["sB"].astype(np.float64))).max() / u < 2.0 ** 24
    return d


@pytest.mark.parametrize("M,N", [ONE_TILE, Q_TILES])
@pytest.mark.parametrize("tag", ["pairs", "own"])
def test_scales_rotated_by_group_arrive_in_their_own_slot(M, N, tag):
    K, paired = K7, tag == "pairs"
    d = _ring(M, N, K, paired)
    assert P.pairs_shared(d) == paired
    want = P.expected(d).numpy()
    G = K // 128 - 1
    for miss in (0, G - 1):                                      # a sum that takes one group's scales from its neighbour differs everywhere
        w = dict(d, sA=np.roll(d["sA"], 1, axis=1)) if miss == 0 else dict(d, sB=np.roll(d["sB"], 1, axis=0))
        assert (P.expected(w).numpy() != want).mean() > 0.9
    got = _run(d, M, N, K, FLAGS[tag])
    bad = np.argwhere(bits16(got) != bits16(want))
    assert len(bad) == 0, f"{len(bad)} of {got.size} outputs differ, first at (m, n) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    rows = _rows(M)
    assert np.array_equal(bits16(got[rows]), bits16(_oracle(d, M, N, K, rows)))


# ------------------------------------------------------------------------------------------------ zero rows and extremes
_SA = np.array([0.0, -0.0, 65504.0, 2.0 ** -24, 1.0, 0.375, 2.0 ** -14, -0.0], np.float16)      # by (m + 3 g) % 8
_SB = np.array([0.0, 65504.0, 2.0 ** -24, 1.0, -0.0, 2.0 ** -14, 0.0, 0.046875], np.float16)    # by (pair + g) % 8 (own: (n + g) % 8)


def _extremes(M, N, K, paired, seed=11):
    """random codes in [-2, 2]; token scales and weight scales from palettes that hold +0, -0, the fp16 maximum and the smallest
    subnormal: every +-0 product, the largest (65504^2, finite in FP32) and the smallest (2^-48, normal in FP32) occur in every tile;
    one token of every block and one channel pair of every 16 have all their scales zero (their outputs are +0)"""
    g = np.random.default_rng(seed)
    G = K // 128 - 1
    d = _empty(M, N, K)
    d["qa4"] = g.integers(-2, 3, size=(M, K - 128)).astype(np.int8)
    d["qb4"] = g.integers(-2, 3, size=(N, K - 128)).astype(np.int8)
    d["qa8"] = g.integers(-3, 4, size=(M, 128)).astype(np.int8)
    d["qb8"] = g.integers(-3, 4, size=(N, 128)).astype(np.int8)
    m, n, gi = np.arange(M), np.arange(N), np.arange(G)
    d["sA"] = _SA[(m[:, None] + 3 * gi[None, :]) % 8]
    d["sB"] = _SB[((n // 2 if paired else n)[None, :] + gi[:, None]) % 8]
    d["sA8"] = np.full((M,), 2.0 ** -7, np.float16)
    d["sB8"] = np.full((N,), 2.0 ** -6, np.float16)
    zm, zn = m % 16 == 3, (n // 2) % 16 == 5                     # zero rows: a token per block and a channel pair per 16 with no scale at all
    d["sA"][zm], d["sA8"][zm], d["sB"][:, zn], d["sB8"][zn] = 0, 0, 0, 0
    return d


@pytest.mark.parametrize("M,N", [ONE_TILE, Q_TILES])
@pytest.mark.parametrize("tag", ["pairs", "own"])
def test_zero_scales_and_extremes_give_the_oracles_bits(M, N, tag):
    K, paired = K7, tag == "pairs"
    d = _extremes(M, N, K, paired)
    assert P.pairs_shared(d) == paired
    for k in ("sA", "sB"):
        b = d[k].view(np.uint16)
        assert all((b == x).any() for x in (0x0000, 0x8000, 0x7BFF, 0x0001))             # +0, -0, the maximum, the smallest subnormal
    got = _run(d, M, N, K, FLAGS[tag])
    rows = _rows(M)
    want = _oracle(d, M, N, K, rows)
    assert not np.isnan(want.astype(np.float32)).any() and np.isinf(want.astype(np.float32)).any()
    assert (bits16(want[rows % 16 == 3]) == 0).all() and (bits16(want[:, (np.arange(N) // 2) % 16 == 5]) == 0).all()
    bad = np.argwhere(bits16(got[rows]) != bits16(want))
    assert len(bad) == 0, f"{len(bad)} of {want.size} outputs differ, first at row {rows[bad[0][0]]}, column {bad[0][1]}"


# ------------------------------------------------------------------------------------------------ random
@pytest.mark.parametrize("M,N", [(512, 512), Q_TILES])
@pytest.mark.parametrize("tag", ["pairs", "own"])
def test_random_operands_bit_exact(M, N, tag):
    K = K12
    assert _takes_q_kernel(*Q_TILES, K)
    d = rand_gemm_operands(M, N, K, seed=20261 + M)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    if tag == "own":                                             # every channel its own scale
        d["sB"] = np.random.default_rng(5).uniform(0.005, 0.05, size=d["sB"].shape).astype(np.float16)
    assert P.pairs_shared(d) == (tag == "pairs")
    got = _run(d, M, N, K, FLAGS[tag])
    rows = np.arange(M) if M <= 512 and N <= 512 else np.r_[0:8, 250:262, M - 4:M]
    want = _oracle(d, M, N, K, rows)
    bad = np.argwhere(bits16(got[rows]) != bits16(want))
    assert len(bad) == 0, f"{len(bad)} of {want.size} outputs differ, first at row {rows[bad[0][0]]}, column {bad[0][1]}"
