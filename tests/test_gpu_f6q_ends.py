"""The ends of the 256x256 BF6 kernel (gemm_w4a4_f6q_kernel, the instantiation for weights whose channel pairs share their scales)
and the scale tiles of its K step, bit for bit: the front (tile index, first fetch) on whole, ragged and two-band shapes, the two
scale-tile register sets (a tile is made two pair slots ahead of its first reader) in every slot group, loop depth and tail form, and
the two keeper halves, the second of which is fetched last of all.

Shapes.  f6_pick_cfg sends a shape to that kernel from 129 tiles of 256 x 256, so the smallest one is 768 x 11008 = 3 x 43 tiles.
K = 7 * 128 (G = 6 int4 groups) is the shortest K whose first step is a regular one: three regular steps, one compile-time tail step,
the two generic ones.  K = 9 * 128 and 13 * 128 run the unrolled loop once and twice and end in the two forms the tail has (without
and with a compile-time tail step).  700 x 10880 is still 3 x 43 tiles, every one of the last tile row and tile column ragged (the
entry point takes N in multiples of 64 only, so 10880 = 170 * 64 stands for the 10900 first planned).
1280 x 6912 = 5 x 27 tiles has a full band of four tile rows and a band of one: both forms of the tile index in one launch.

References.  The planted operands make every partial sum an FP32 number whatever the order (tests/gemm_planted.expected asserts it),
so the whole output is compared with the exact value rounded to fp16 once; sampled rows are compared with the C restatement of the
contract (tests/c_oracle.gemm) as well."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from oracle import atom_oracle as O
from tests import c_oracle as CO
from tests import gemm_planted as P
from tests import gemm_route_cases as C
from tests.helpers import bits16, rand_gemm_operands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_TILES = (768, 11008)
RAGGED = (700, 10880)
TWO_BANDS = (1280, 6912)
K7, K9, K13 = 7 * 128, 9 * 128, 13 * 128
POS = 5                                                          # the one code position of a group that is not zero
FLAGS = C.AB_F6 | C.B_F6S | C.PAIRS


def _lib():
    from atom_amd import _lib
    return _lib.lib()


def _takes_q_kernel(M, N, K):
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    return t256 >= 129 and (t256 + 255) // 256 == 1 and ((M + 63) // 64) * (N // 64) > 512 and _lib().atom_gemm_w4a4_f6_order(M, N, K) == 1


def _run(d, M, N, K):
    src = dict(A4=O.pack_int4(d["qa4"]), B4=O.pack_int4(d["qb4"]), A8=d["qa8"], B8=d["qb8"], sA=np.ascontiguousarray(d["sA"].T),
               sA8=d["sA8"], sB=np.ascontiguousarray(d["sB"]), sB8=d["sB8"])
    st, dev, outs = C.call(("f6q_ends", "f16", M, N, K, dict(flags=FLAGS)), src=src)
    assert st == 0, f"status {st}"
    return dev.get("D")


def _oracle(d, rows):
    return CO.gemm(O.pack_int4(d["qa4"][rows]), O.pack_int4(d["qb4"]), np.ascontiguousarray(d["sA"][rows].T), d["sB"], d["qa8"][rows],
                   d["qb8"], d["sA8"][rows], d["sB8"])


def _rows(M):
    """the first and last 32 rows (both rows of 16 record pairs, token blocks 0-1 and the last ones of a wave tile) and 16 rows
    inside the second tile row"""
    return np.r_[0:32, 356:372, M - 32:M]


def _empty(M, N, K):
    G = K // 128 - 1
    return dict(qa4=np.zeros((M, K - 128), np.int8), qb4=np.zeros((N, K - 128), np.int8), qa8=np.zeros((M, 128), np.int8),
                qb8=np.zeros((N, 128), np.int8), sA=np.zeros((M, G), np.float16), sB=np.zeros((G, N), np.float16),
                sA8=np.ones((M,), np.float16), sB8=np.ones((N,), np.float16))


def _assert_same(got, want, what):
    bad = np.argwhere(bits16(got) != bits16(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} outputs differ, first at (m, n) = {tuple(int(x) for x in bad[0])}: "
                           f"{float(got[tuple(bad[0])])!r} != {float(want[tuple(bad[0])])!r}")


# ------------------------------------------------------------------------------------------------ scale tiles
def _tiles(M, N, K):
    """idot = +-1 in every group.  The token scale is 2^((token block + g) % 8 - 10) (1 + (m % 16) / 16), the weight scale
    2^((n / 32 + g) % 4) (1 + ((n / 2 + g) % 16) / 16): one value per (group, token block of the wave tile, token) and per (group,
    feature-block pair, channel pair).  A pair slot of the K step is (token block, feature-block pair), a scale tile holds the products
    of four slots: a tile, or one of its two operands, that is read a slot, a tile or a stage early or late changes the sum.
    Every term is a multiple of 2^-18 and at most 2^3, G <= 12 of them: every order of summation gives the exact sum."""
    d = _empty(M, N, K)
    G = K // 128 - 1
    m, n = np.arange(M), np.arange(N)
    for g in range(G):
        d["qa4"][:, 128 * g + POS] = 1
        d["qb4"][:, 128 * g + POS] = np.where((n // 16 + g) % 2 == 1, -1, 1)
        d["sA"][:, g] = np.ldexp(1 + (m % 16) / 16.0, ((m // 16 + g) % 8) - 10)
        d["sB"][g] = np.ldexp(1 + ((n // 2 + g) % 16) / 16.0, (n // 32 + g) % 4)
    assert G <= 12 and P.pairs_shared(d)
    return d


def _check_tiles(M, N, K):
    assert _takes_q_kernel(M, N, K)
    d = _tiles(M, N, K)
    G = K // 128 - 1
    want = P.expected(d).numpy()                                 # (asserts that every sum is an FP32 number)
    sa = d["sA"][:128].astype(np.float64)
    for g in range(G):                                           # distinct over the 128 tokens of a wave tile and its 32 channel pairs
        assert len(np.unique(sa[:, g])) == 128 and len(np.unique(d["sB"][g, 0:64:2].astype(np.float64))) == 32
    for w in (dict(d, sA=np.roll(d["sA"], 16, axis=0)),          # the token scales of the neighbouring block (a tile one slot pair off)
              dict(d, sB=np.roll(d["sB"], 32, axis=1)),          # the weight scales of the other feature-block pair (one slot off)
              dict(d, sA=np.roll(d["sA"], 1, axis=1)),           # the token scales, the weight scales of the neighbouring stage
              dict(d, sB=np.roll(d["sB"], 1, axis=0))):
        assert (P.expected(w).numpy() != want).mean() > 0.9
    got = _run(d, M, N, K)
    _assert_same(got, want, f"{M}x{N}x{K} planted scale tiles")
    rows = _rows(M)
    _assert_same(got[rows], _oracle(d, rows), f"{M}x{N}x{K} planted scale tiles vs the C contract")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [K7, K9, K13])
def test_scale_tiles_in_every_slot_group_and_loop_depth(K):
    _check_tiles(*Q_TILES, K)


@pytest.mark.gpu
def test_ragged_tiles_take_the_same_front_and_the_checked_stores():
    _check_tiles(*RAGGED, K7)


@pytest.mark.gpu
def test_tile_index_in_a_full_band_and_a_short_one():
    _check_tiles(*TWO_BANDS, K7)


@pytest.mark.gpu
def test_ragged_random_operands_bit_exact():
    M, N, K = (*RAGGED, K9)
    assert _takes_q_kernel(M, N, K)
    d = rand_gemm_operands(M, N, K, seed=20277)
    assert P.pairs_shared(d)
    got = _run(d, M, N, K)
    rows = np.r_[0:8, 250:262, M - 4:M]
    _assert_same(got[rows], _oracle(d, rows), f"{M}x{N}x{K} random")


# ------------------------------------------------------------------------------------------------ keeper
@pytest.mark.gpu
@pytest.mark.parametrize("K", [K7, K9])
def test_keeper_halves_differ_and_both_have_landed(K):
    """Zero int4 codes under non-zero scales; keeper codes in [-3, 3] in the first 64 columns and odd ones in [-7, 7] in the second 64,
    keeper scales powers of two by row and channel.  Every output is the keeper's alone, exact in FP32; a half read before it has
    landed holds the int4 records of the stage that used its slot before."""
    M, N = Q_TILES
    assert _takes_q_kernel(M, N, K)
    g = np.random.default_rng(K)
    d = _empty(M, N, K)
    d["sA"][:], d["sB"][:] = 0.75, 1.5
    d["qa8"][:, :64] = g.integers(-3, 4, size=(M, 64))
    d["qb8"][:, :64] = g.integers(-3, 4, size=(N, 64))
    d["qa8"][:, 64:] = 2 * g.integers(-4, 4, size=(M, 64)) + 1
    d["qb8"][:, 64:] = 2 * g.integers(-4, 4, size=(N, 64)) + 1
    d["sA8"] = np.ldexp(1.0, -(np.arange(M) % 5)).astype(np.float16)
    d["sB8"] = np.ldexp(1.0, -((np.arange(N) // 2) % 7)).astype(np.float16)
    want = P.expected(d).numpy()
    h0 = P.expected(dict(d, qa8=np.where(np.arange(128) < 64, d["qa8"], 0).astype(np.int8))).numpy()
    h1 = P.expected(dict(d, qa8=np.where(np.arange(128) >= 64, d["qa8"], 0).astype(np.int8))).numpy()
    assert (h0 != want).mean() > 0.9 and (h1 != want).mean() > 0.9 and (h0 != h1).mean() > 0.9   # each half matters, and they differ
    got = _run(d, M, N, K)
    _assert_same(got, want, f"{M}x{N}x{K} keeper")
    rows = _rows(M)
    _assert_same(got[rows], _oracle(d, rows), f"{M}x{N}x{K} keeper vs the C contract")


# ------------------------------------------------------------------------------------------------ resources (CPU, needs hipcc)
def test_headline_instantiation_holds_two_scale_tiles_without_a_spill():
    spec = importlib.util.spec_from_file_location("insn_model", os.path.join(ROOT, "tools", "insn_model.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    hipcc, _ = tool.makefile_flags()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    body, f = tool.kernel_text(tool.build_asm())
    assert tool.check_resources(body, f) == []
    assert f["ScratchSize"] == 0 and f["private_segment_fixed_size"] == 0
    assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0
    assert f["Occupancy"] == 2 and f["NumVgprs"] <= 256 and f.get("NumAgprs", 0) == 0
    # the second tile: no scale-product MFMA of the main loop writes the register tuple its predecessor wrote, whose last block still
    # has a reader (with one tile they all write the same one)
    loop = tool.regions(body)["loop"]
    dst = [l.split()[1].rstrip(",") for l in loop if l.strip().startswith("v_mfma_f32_16x16x1_")]
    assert len(dst) == 12 and all(a != b for a, b in zip(dst, dst[1:] + dst[:1]))
