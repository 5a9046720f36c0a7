"""CPU-only checks of the planted GEMM operands (tests/gemm_planted.py), at every shape the GPU test (tests/test_gpu_gemm_planted.py)
uses -- the operand shapes of the covered cases of tests/gemm_route_cases.py:
  * every exact family meets the exactness bound on the operands it generated (printed: log2 of the largest |term| sum in units of
    the smallest scale product; below 24);
  * on the exact families oracle/atom_oracle.c in every summation order it knows (1, 8, -2, -4, "lanes") returns expected(d) bit for
    bit -- the reference and the oracle agree, and the order does not matter -- on sampled rows and columns (the C loop is O(M N K));
  * every family tells each of its wrong rules (printed: how many elements each rule changes), in every output row for the channel-pair
    rules of own_scales, on all rows and at most 64 columns (whole channel pairs, evenly spread, first and last pair included);
  * the pair structure of the weight scales is what the family says."""
import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import c_oracle as C
from tests import gemm_planted as P

SHAPES = list(P.shapes())
EXACT = [f for f in P.FAMILIES.values() if f.exact]
ORDERS = (1, 8, -2, -4, "lanes")


def _rows(M, n):
    return np.unique(np.concatenate([[0, M - 1, M // 2, min(M - 1, 8), min(M - 1, 63)], np.arange(M)[:: max(1, M // n)]]))[: n + 5]


def test_covered_cases_are_all_that_are_taken():
    from tests import gemm_route_cases as R
    cases = P.covered_cases()
    left = [c[0] for c in R.CASES if c[0] not in [k[0] for k in cases]]
    assert len(cases) == 72 + len(P.EXTRA) and len(R.CASES) == 76
    assert left == ["decode_output_off_16", "f32_scales_off_8", "multi_scales_off_8", "multi_q_scales_off_8"]
    assert set(c[1] for c in cases) <= set(P.ENTRY_FAMILIES) | {"multi_q", "merge_q"}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%dx%d" % s)
def made(request):
    """every family's operands at one shape, made once for the tests below (pytest runs them shape by shape)"""
    M, N, K = request.param
    return (M, N, K), {name: f(M, N, K) for name, f in P.FAMILIES.items()}


def test_exactness_bound_and_pair_structure(made):
    (M, N, K), ds = made
    for family in EXACT:
        d = ds[family.name]
        mg = P.margin(d)
        print(f"{family.name} {M}x{N}x{K}: spread {d['spread']}, margin 2^{mg:.2f} units, unequal pairs {P.unequal_pair_share(d):.3f}")
        assert P.is_exact(d) and mg < P.LIMIT, (family.name, M, N, K, mg)
        assert P.pairs_shared(d) == family.paired
        if family.name.startswith("own_scales"):
            assert P.unequal_pair_share(d) > 0.5
            assert (d["sB8"][0::2] != d["sB8"][1::2]).all()
        if family.name.startswith("one_pair_off"):
            g, j = d["planted"]
            off = np.argwhere(d["sB"][:, 0::2] != d["sB"][:, 1::2])
            assert off.tolist() == [[g, j]] and (g, j) in ((0, 0), (d["sB"].shape[0] - 1, N // 2 - 1))


def test_free_own_scales_are_unpaired(made):
    """(atom_amd.ops.scale_pairs_shared needs a device: tests/test_gpu_gemm_planted.py asks it)"""
    d = made[1]["own_scales_free"]
    assert not P.pairs_shared(d) and P.unequal_pair_share(d) > 0.9


def test_c_oracle_in_every_order_equals_expected(made):
    """sampled so that one C call stays near 10^6 multiply-adds: up to 4 + 5 rows, 8 columns"""
    (M, N, K), ds = made
    for family in EXACT:
        d = ds[family.name]
        s = P.take(d, _rows(M, 4), P.pair_columns(N, 8))
        want = P.expected(s)
        assert torch.equal(P.bits(P.round_f16(P.sums(s))), P.bits(want))          # the float64 rounding routine == the conversion
        a4, b4 = O.pack_int4(s["qa4"]), O.pack_int4(s["qb4"])
        for order in ORDERS:
            got = C.gemm(a4, b4, s["sA"].T, s["sB"], s["qa8"], s["qb8"], s["sA8"], s["sB8"], nsplit=order)
            bad = got.view(np.uint16) != want.numpy().view(np.uint16)
            assert not bad.any(), f"{family.name} {M}x{N}x{K} order {order}: {bad.sum()} of {bad.size} differ"
        got = C.gemm(a4, b4, s["sA"].T, s["sB"], s["qa8"], s["qb8"], s["sA8"], s["sB8"], fp32=True)
        assert np.array_equal(got.view(np.uint32), P.expected(s, entry="f32").numpy().view(np.uint32))


def test_family_tells_its_rules(made):
    (M, N, K), ds = made
    for family in EXACT:
        d = ds[family.name]
        G = d["sB"].shape[0]
        s = P.take(d, np.arange(M), P.pair_columns(N, 64))
        exact = P.sums(s)
        want = P.expected(s, exact=exact)
        if "target" in d:
            assert np.array_equal(exact.numpy(), d["target"][:, P.pair_columns(N, 64)])     # the planted sums are what was planted
        for rule in family.tells_at(G):
            diff = P.differ(want, P.expected(s, wrong=rule, exact=exact))
            rows = int(diff.any(dim=1).sum())
            print(f"{family.name} {M}x{N}x{K} {rule}: {int(diff.sum())} of {diff.numel()} elements differ, in {rows} of {M} rows")
            assert diff.any(), (family.name, M, N, K, rule)
            if family.name.startswith("own_scales") and rule.startswith("pair_"):
                assert rows == M, (family.name, M, N, K, rule, rows)
            if family.name.startswith("one_pair_off"):
                col = int(np.argwhere(P.pair_columns(N, 64) == 2 * d["planted"][1] + 1)[0, 0])
                assert not diff[:, [c for c in range(diff.shape[1]) if c != col]].any()
        if family.name == "ties":                                 # both parities of the lower neighbour, and both sides of a tie
            up = P.differ(want, P.round_f16(exact, "rtz")).any() and P.differ(want, P.round_f16(exact, "half_away")).any()
            assert up
        if family.name.startswith("tiny"):
            w = want.float().abs()
            assert ((w > 0) & (w < 2.0 ** -14)).any() and (w == 0).any()
        if family.name == "huge":
            w = want.float().abs()
            assert torch.isinf(w).any() and (w == 65504).any() and not torch.isnan(w).any()
