"""The output write of the 256x256 BF6 kernel (gemm_w4a4_f6q_kernel, the instantiation for weights whose channel pairs share their
scales), bit for bit: a token block's fp16 outputs leave from inside the keeper step, once the de-quantisation of its second pair slot
has made the block final, as write-through stores through one helper for the whole-tile and the checked path.

Shapes (tests/test_gpu_f6q_ends.py explains them): 768 x 11008 = 3 x 43 whole tiles; 700 x 10880, the last tile row and column ragged
(checked stores); 1280 x 6912 = 5 x 27 tiles, a full band of tile rows and a band of one.  K = 7 * 128 and 9 * 128 end the K loop in its
two tail forms.

References.  Every planted sum is an FP32 number whatever the order (tests/gemm_planted.expected asserts it); the whole output is compared
with the exact value rounded to fp16 once, sampled rows with the C restatement of the contract (tests/c_oracle.gemm) as well.

Wave tile.  A wave owns 128 tokens x 64 features of a tile.  Token block tb of the keeper is rows 32 (tb >> 1) + (tb & 1) + 2 l, l < 16
(the even or the odd rows of a run of 32); a pair slot is (token block, 32-feature half); lane (l, kb) stores features 8 kb .. 8 kb + 7 of
each half of row 2 l + (tb & 1)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from tests import gemm_planted as P
from tests import gemm_route_cases as C
from tests import test_gpu_f6q_ends as E
from tests.helpers import bits16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_TILES, RAGGED, TWO_BANDS = E.Q_TILES, E.RAGGED, E.TWO_BANDS
K7, K9 = E.K7, E.K9
POS = E.POS
SENTINEL = 0x7E55                                                # a NaN no kernel writes


def _token_block(m):
    return 2 * ((m % 128) // 32) + (m & 1)


# ------------------------------------------------------------------------------------------------ a block stored before it is final
def _three_parts(M, N, K):
    """Three contributions to every output, each one value per (token block tb, feature half hf) of a wave tile:
        the last int4 group   (1 + 2 hf) 2^(tb - 6)        one code of 1 against one of 1 + 2 hf, token scale 2^(tb - 6)
        keeper half 0         (tb + 1) (17 + 4 hf) 2^-6    one code pair in columns 0..63 of the keeper
        keeper half 1         (tb + 9) (23 + 8 hf) 2^-6    one code pair in columns 64..127
    The earlier int4 groups have zero codes under non-zero scales.  Every term is a multiple of 2^-6, their sum is below 32: exact in FP32
    and an fp16 number.  The block's outputs are final only after the de-quantisation of its second pair slot (hf = 1), and the last
    int4 group's last pair only after the K loop: stores issued one de-quantisation early, or from the neighbouring block's registers,
    give another value."""
    d = E._empty(M, N, K)
    G = K // 128 - 1
    m, n = np.arange(M), np.arange(N)
    tb, hf = _token_block(m), (n % 64) // 32
    d["sA"][:], d["sB"][:] = 0.75, 1.5
    d["qa4"][:, 128 * (G - 1) + POS] = 1
    d["qb4"][:, 128 * (G - 1) + POS] = 1 + 2 * hf
    d["sA"][:, G - 1] = np.ldexp(1.0, tb - 6)
    d["sB"][G - 1] = 1.0
    d["qa8"][:, 3], d["qb8"][:, 3] = tb + 1, 17 + 4 * hf
    d["qa8"][:, 64 + 5], d["qb8"][:, 64 + 5] = tb + 9, 23 + 8 * hf
    d["sA8"][:], d["sB8"][:] = 2.0 ** -6, 1.0
    assert P.pairs_shared(d)
    return d


def _check_three_parts(M, N, K, host_checks):
    assert E._takes_q_kernel(M, N, K)
    d = _three_parts(M, N, K)
    want = P.expected(d).numpy()
    if host_checks:
        tb, hf = np.meshgrid(np.arange(8), np.arange(2), indexing="ij")
        parts = np.stack([(1 + 2 * hf) * np.ldexp(1.0, tb - 6), (tb + 1) * (17 + 4 * hf) / 64.0, (tb + 9) * (23 + 8 * hf) / 64.0])
        assert (parts != 0).all() and len(np.unique(parts)) == parts.size           # distinct per block and half, and from each other
        assert len(np.unique(parts.sum(axis=0))) == 16
        z = lambda a, sl: np.where(sl, 0, a).astype(np.int8)
        k = np.arange(128)
        for w in (dict(d, qa4=np.zeros_like(d["qa4"])), dict(d, qa8=z(d["qa8"], k < 64)), dict(d, qa8=z(d["qa8"], k >= 64))):
            assert (P.expected(w).numpy() != want).mean() > 0.9                     # dropping any one contribution shows
    got = E._run(d, M, N, K)
    E._assert_same(got, want, f"{M}x{N}x{K} three contributions per block and half")
    rows = E._rows(M)
    E._assert_same(got[rows], E._oracle(d, rows), f"{M}x{N}x{K} three contributions vs the C contract")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [K7, K9])
def test_no_block_leaves_before_its_last_dequantisation(K):
    _check_three_parts(*Q_TILES, K, host_checks=K == K7)


@pytest.mark.gpu
def test_no_block_leaves_early_through_the_checked_stores():
    _check_three_parts(*RAGGED, K7, host_checks=False)


@pytest.mark.gpu
def test_no_block_leaves_early_in_two_bands():
    _check_three_parts(*TWO_BANDS, K7, host_checks=False)


# ------------------------------------------------------------------------------------------------ store placement
def _placed(M, N, K, coarse):
    """One non-zero term per output, value a(m) b(n) with a and b odd integers times powers of two, at most 10 significant bits: an fp16
    number, so nothing is rounded away.  An fp16 output cannot hold all of (m, n); two operand sets do.
      fine    a = (65 + 2 (m % 32)) 2^((m / 32) % 4 - 8), b = +-(1 + 2 ((n / 2) % 4)) 2^((n / 8) % 8), + for even n: the place inside a
              wave tile (row of the token block, token block, channel of the pair, 8-feature piece, half)
      coarse  a = (65 + 2 ((m / 128) % 32)) 2^-8, b = +-(1 + 2 ((n / 64) % 4)) 2^((n / 512) % 32 - 8), + for even n / 256: the wave
              tile inside the tile, and the tile
    The term sits in one int4 group (fine: the last, coarse: the first), one code of 1 against one of +-1, 3, 5, 7; the other groups have
    zero codes under non-zero scales, the keeper zero codes."""
    d = E._empty(M, N, K)
    G = K // 128 - 1
    m, n = np.arange(M), np.arange(N)
    d["sA"][:], d["sB"][:] = 0.75, 1.5
    if coarse:
        g, a = 0, np.ldexp(65.0 + 2 * ((m // 128) % 32), -8)
        code, sb = (1 + 2 * ((n // 64) % 4)) * np.where((n // 256) % 2 == 1, -1, 1), np.ldexp(1.0, (n // 512) % 32 - 8)
    else:
        g, a = G - 1, np.ldexp(65.0 + 2 * (m % 32), (m // 32) % 4 - 8)
        code, sb = (1 + 2 * ((n // 2) % 4)) * np.where(n % 2 == 1, -1, 1), np.ldexp(1.0, (n // 8) % 8)
    d["qa4"][:, 128 * g + POS] = 1
    d["qb4"][:, 128 * g + POS] = code
    d["sA"][:, g], d["sB"][g] = a, sb
    assert P.pairs_shared(d)
    assert np.array_equal(d["sA"][:, g].astype(np.float64), a) and np.array_equal(d["sB"][g].astype(np.float64), sb)
    va, vb = a, code * sb
    want = np.outer(va, vb)
    assert np.array_equal(want.astype(np.float16).astype(np.float64), want)        # every output is an fp16 number
    for r in ((128, 256, 384) if coarse else (1, 2, 16, 32, 64)):                    # a row off by this much holds another value
        assert (np.outer(np.roll(va, r), vb) != want).mean() > 0.9
    for r in ((64, 128, 256, 512, 1024) if coarse else (1, 2, 8, 16, 32)):           # ... a column
        assert (np.outer(va, np.roll(vb, r)) != want).mean() > 0.9
    return d, want.astype(np.float16)


def _run_padded(d, M, N, K):
    """E._run with the output inside a larger buffer of SENTINEL: (the output, the halves in front of it, the halves behind it).  Behind
    it there is room for the rows a ragged last tile row would have below M."""
    import torch
    from atom_amd import _lib
    from oracle import atom_oracle as O
    lib = _lib.lib()
    G = K // 128 - 1
    stream = _lib.current_stream(torch.device("cuda"))
    dev = C._Dev({})
    for k, a in dict(A4=O.pack_int4(d["qa4"]), B4=O.pack_int4(d["qb4"]), A8=d["qa8"], B8=d["qb8"], sA=np.ascontiguousarray(d["sA"].T),
                     sA8=d["sA8"], sB=np.ascontiguousarray(d["sB"]), sB8=d["sB8"]).items():
        dev.put(k, a)
    assert lib.atom_scale_size(M, C.PLAIN) == M
    rows = (M + 255) // 256 * 256
    dev.put("A6", np.zeros((G, rows, 104), dtype=np.uint8))
    _lib.check(lib.atom_repack_act_f6(dev.ptr("A4"), dev.ptr("sA"), M, K, C.PLAIN, dev.ptr("A6"), stream), "atom_repack_act_f6")
    dev.put("B6", np.zeros(lib.atom_f6_weight_bytes(N, K), dtype=np.uint8))
    _lib.check(lib.atom_repack_weight_f6s(dev.ptr("B4"), dev.ptr("sB"), N, K, dev.ptr("B6"), stream), "atom_repack_weight_f6s")
    pad = (rows - M + 8) * N                                     # halves; a multiple of 64, so the output stays 16-byte aligned
    buf = torch.full((pad + M * N + pad,), SENTINEL, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    st = lib.atom_gemm_w4a4_f16(*(dev.ptr(k) for k in ("A6", "B6", "sA", "sB", "A8", "B8", "sA8", "sB8")), buf.data_ptr() + 2 * pad,
                                M, N, K, 128, 128, C.PLAIN | E.FLAGS, stream)
    torch.cuda.synchronize()
    assert st == 0, f"status {st}"
    h = buf.cpu().numpy().view(np.uint16)
    return h[pad:pad + M * N].view(np.float16).reshape(M, N), h[:pad], h[pad + M * N:]


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", [False, True], ids=["fine", "coarse"])
@pytest.mark.parametrize("shape", [Q_TILES, RAGGED], ids=["whole", "ragged"])
def test_every_output_lands_in_its_place_and_nowhere_else(shape, coarse):
    M, N = shape
    assert E._takes_q_kernel(M, N, K7)
    d, want = _placed(M, N, K7, coarse)
    assert np.array_equal(bits16(P.expected(d).numpy()), bits16(want))
    got, front, behind = _run_padded(d, M, N, K7)
    assert (bits16(got) != SENTINEL).all(), f"{int((bits16(got) == SENTINEL).sum())} outputs were never written"
    E._assert_same(got, want, f"{M}x{N}x{K7} placement ({'coarse' if coarse else 'fine'})")
    for name, pad in (("in front of the output", front), ("behind row M - 1", behind)):
        bad = np.flatnonzero(pad != SENTINEL)
        assert len(bad) == 0, f"{len(bad)} halves written {name}, first at {int(bad[0])}"


# ------------------------------------------------------------------------------------------------ resources (CPU, needs hipcc)
def test_no_instantiation_spills_or_uses_scratch():
    """Resource counts of every gemm_w4a4_f6q_kernel instantiation, from the compiler's own figures.  None uses scratch memory or spills a
    vector register, and the headline one (plain output, shared scale pairs) keeps two waves per SIMD without any spill.  The four gate/up
    instantiations move two scalar registers into lanes of a vector register (sgpr_spill_count 2, as before this test was written): that
    costs no memory access, so the bound for them is that figure, not zero."""
    spec = importlib.util.spec_from_file_location("insn_model", os.path.join(ROOT, "tools", "insn_model.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    hipcc, _ = tool.makefile_flags()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    asm = tool.build_asm()
    keys = ["gemm_w4a4_f6q_kernelINS0_3CfgILi256ELi256ELi4ELi3ELi2ELi0EEELi%dELb0ELb%dEEE" % (gu, pair) for gu in (0, 1, 2) for pair in (0, 1)]
    assert tool.HEADLINE in keys
    for key in keys:
        body, f = tool.kernel_text(asm, key)
        print(key, {k: f.get(k) for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy", "vgpr_spill_count", "sgpr_spill_count")})
        gate_up = "EEELi0E" not in key
        assert f["ScratchSize"] == 0 and f["private_segment_fixed_size"] == 0, key
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] <= (2 if gate_up else 0), key
        assert tool.n_ops(body, "scratch_") == 0, key
        assert f["NumVgprs"] <= 256 and f.get("NumAgprs", 0) == 0 and f["Occupancy"] == 2, key
    body, f = tool.kernel_text(asm)
    assert tool.check_resources(body, f) == [] and f["Occupancy"] == 2 and f["sgpr_spill_count"] == 0
