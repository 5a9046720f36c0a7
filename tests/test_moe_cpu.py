"""CPU-only checks of the sparse mixture-of-experts entry points (include/atom_hip.h): the tile bound, the argument validation
(it precedes every launch, so no GPU is needed), and the checker's own restatement of the block (tests/moe_ref.py)."""
import random

import torch

from tests import moe_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def test_max_tiles_is_the_formula_and_bounds_every_split():
    L, lib = _lib()
    rnd = random.Random(3)
    for R, E in [(0, 8), (1, 8), (2, 8), (63, 8), (64, 8), (65, 2), (260, 6), (4096, 8), (3, 64), (10 ** 6, 64)]:
        assert lib.atom_moe_max_tiles(R, E) == R // 64 + min(E, R)
    for _ in range(200):
        E = rnd.randrange(2, 65)
        R = rnd.choice([1, 2, 5, 63, 64, 65, 127, 128, 129, 500, rnd.randrange(1, 5000)])
        cuts = sorted(rnd.randrange(0, R + 1) for _ in range(E - 1))
        m = [b - a for a, b in zip([0] + cuts, cuts + [R])]
        if rnd.random() < 0.3:                                # everything on few experts
            m = [0] * E
            for _ in range(min(R, rnd.randrange(1, 4))):
                m[rnd.randrange(E)] += 1
            m[rnd.randrange(E)] += R - sum(m)
        assert sum(m) == R and len(m) == E
        assert sum(-(-x // 64) for x in m) <= lib.atom_moe_max_tiles(R, E), (R, E, m)
        assert len(moe_ref.tables_from_counts(m)[1]) == sum(-(-x // 64) for x in m)


def _route(lib, T=4, E=8, K=2, ptrs=None):
    ptrs = [P] * 9 if ptrs is None else ptrs
    return lib.atom_moe_route_topk(ptrs[0], T, E, K, *ptrs[1:], None)


def _gemm(lib, ptrs=None, A_rows=16, R=32, E=8, N_seg=128, nseg=2, K=384, group=128, keeper=128, layout=0):
    ptrs = [P] * 15 if ptrs is None else ptrs
    return lib.atom_moe_gemm_w4a4_f16(*ptrs, A_rows, R, E, N_seg, nseg, K, group, keeper, layout, None)


def _combine(lib, ptrs=None, T=4, K=2, H=512):
    ptrs = [P] * 6 if ptrs is None else ptrs
    return lib.atom_moe_combine_f16(*ptrs, T, K, H, None)


def test_router_rejects_bad_arguments():
    L, lib = _lib()
    for i in range(9):
        assert _route(lib, ptrs=[P] * i + [None] + [P] * (8 - i)) == L.ERR_INVALID_ARG
    assert _route(lib, E=65) == L.ERR_SHAPE and _route(lib, E=1, K=1) == L.ERR_SHAPE
    assert _route(lib, E=4, K=5) == L.ERR_SHAPE and _route(lib, E=64, K=9) == L.ERR_SHAPE and _route(lib, K=0) == L.ERR_SHAPE
    assert _route(lib, T=0) == L.ERR_SHAPE and _route(lib, T=2 ** 30, K=2) == L.ERR_SHAPE
    assert _route(lib, ptrs=[P] + [P + 2] + [P] * 7) == L.ERR_ALIGN


def test_routed_gemm_rejects_bad_arguments():
    L, lib = _lib()
    for i in range(15):
        if i in (8, 14):                                      # row_index may be NULL (identity); out1 is unused with one segment
            continue
        assert _gemm(lib, ptrs=[P] * i + [None] + [P] * (14 - i)) == L.ERR_INVALID_ARG, i
    assert _gemm(lib, ptrs=[P] * 14 + [None], nseg=2) == L.ERR_INVALID_ARG
    assert _gemm(lib, nseg=3) == L.ERR_INVALID_ARG and _gemm(lib, layout=2) == L.ERR_INVALID_ARG
    assert _gemm(lib, E=65) == L.ERR_SHAPE and _gemm(lib, E=0) == L.ERR_SHAPE
    assert _gemm(lib, N_seg=96) == L.ERR_SHAPE and _gemm(lib, N_seg=100) == L.ERR_SHAPE and _gemm(lib, N_seg=0) == L.ERR_SHAPE
    assert _gemm(lib, K=200) == L.ERR_SHAPE and _gemm(lib, K=128) == L.ERR_SHAPE and _gemm(lib, K=400) == L.ERR_SHAPE
    assert _gemm(lib, group=64) == L.ERR_SHAPE and _gemm(lib, keeper=64) == L.ERR_SHAPE
    assert _gemm(lib, R=0) == L.ERR_SHAPE and _gemm(lib, R=2 ** 31) == L.ERR_SHAPE and _gemm(lib, A_rows=0) == L.ERR_SHAPE
    assert _gemm(lib, A_rows=2 ** 21, K=4096 + 128) == L.ERR_SHAPE           # A_rows * K4 / 2 = 2^32: beyond a 32-bit lane offset
    assert _gemm(lib, ptrs=[P + 8] + [P] * 14) == L.ERR_ALIGN and _gemm(lib, ptrs=[P] * 8 + [P + 2] + [P] * 6) == L.ERR_ALIGN


def test_combine_rejects_bad_arguments():
    L, lib = _lib()
    for i in (0, 1, 2, 3, 5):
        assert _combine(lib, ptrs=[P] * i + [None] + [P] * (5 - i)) == L.ERR_INVALID_ARG
    assert _combine(lib, H=500) == L.ERR_SHAPE and _combine(lib, H=0) == L.ERR_SHAPE and _combine(lib, K=9) == L.ERR_SHAPE
    assert _combine(lib, K=0) == L.ERR_SHAPE and _combine(lib, T=0) == L.ERR_SHAPE
    assert _combine(lib, ptrs=[P + 8] + [P] * 5) == L.ERR_ALIGN


def _expert_fn(E, H, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn((E, H), generator=g) * 2).half()
    b = torch.randn((E, H), generator=g).half()
    return lambda e, rows: moe_ref.hadd(moe_ref.hmul(rows, a[e][None, :]), b[e][None, :])      # elementwise: a row's result is its own


def test_reference_block_equals_its_direct_formulation():
    T, E, K, H = 37, 8, 2, 64
    g = torch.Generator().manual_seed(0)
    x = torch.randn((T, H), generator=g).half()
    res = torch.randn((T, H), generator=g).half()
    logits = moe_ref.distinct_logits(T, E, 1)
    fn = _expert_fn(E, H, 2)
    for r in (None, res):
        a, b = moe_ref.block(x, logits, K, E, fn, r), moe_ref.block_direct(x, logits, K, E, fn, r)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    tb = moe_ref.tables(moe_ref.route(logits, K)[0], E)
    assert sorted(tb["row_token"]) == sorted(list(range(T)) * K) and tb["expert_indptr"][-1] == T * K
    for e in range(E):
        seg = tb["row_token"][tb["expert_indptr"][e]:tb["expert_indptr"][e + 1]]
        assert seg == sorted(seg) and len(set(seg)) == len(seg)


def test_reference_routing_equals_the_entry_points_formula():
    """softmax -> topk -> renormalise -> half against exp(l_k - l_max) / sum over the selected, on logits without ties: the same
    experts and the same fp16 weights bit for bit"""
    n = 0
    for T, E, K in [(5000, 8, 2), (300, 3, 1), (300, 16, 4), (300, 64, 8), (37, 8, 2), (200, 5, 5), (100, 64, 1), (400, 32, 3)]:
        logits = moe_ref.distinct_logits(T, E, 10 + E + K)
        ids, w = moe_ref.route(logits, K)
        ids2, w2 = moe_ref.route_formula(logits, K)
        assert torch.equal(ids, ids2)
        assert torch.equal(w.view(torch.int16), w2.view(torch.int16))
        n += w.numel()
    assert n > 16000


PLANTED = [(600, 8, 2), (600, 2, 2), (600, 3, 1), (600, 16, 4), (600, 64, 8), (600, 5, 5)]      # the GPU router test's cases
PLANTED_SEED = 500


def _ids_are_a_selection(ids, E):
    """every row: top_k different experts of 0 .. E - 1"""
    return bool(((ids >= 0) & (ids < E)).all()) and all(len(set(r)) == len(r) for r in ids.tolist())


def test_planted_logits_tell_the_tie_rule_from_its_opposite():
    """on the planted logits, "the lower index of equal logits" and "the higher index" select different experts (or the same in
    another order) on at least 50 rows of every case, and the tables built from them differ: a router with the opposite rule, or
    with no rule, cannot pass the GPU test on these inputs.  torch.topk is such a router: it promises no order among equal values,
    and on the CPU build this was written with it leaves the lower-index rule on 354 to 597 of the 600 rows at E >= 5 (none at
    E = 2 and 3, where it happens to keep it) -- which is why moe_ref.route sorts stably instead.  The count is printed, not asserted:
    it is a property of the torch build."""
    for T, E, K in PLANTED:
        logits, exact_rows = moe_ref.planted_logits(T, E, K, PLANTED_SEED + E + K)
        assert logits.shape == (T, E) and logits.dtype == torch.float16
        lo, w_lo = moe_ref.route(logits, K)
        hi, w_hi = moe_ref.route(logits, K, tie="high")
        rows = int((lo != hi).any(-1).sum())
        topk_rows = int((torch.topk(logits.float(), K, dim=-1).indices != lo).any(-1).sum())
        print(f"T {T} E {E} top_k {K}: low / high differ on {rows} rows, torch.topk leaves the lower-index rule on {topk_rows}")
        assert rows >= 50
        assert torch.equal(lo.sort(-1).values, hi.sort(-1).values) == (E == K)      # E > K: other experts, not only another order
        t_lo, t_hi = moe_ref.tables(lo, E), moe_ref.tables(hi, E)
        assert t_lo["slot_row"] != t_hi["slot_row"]
        assert E == K or (t_lo["row_token"] != t_hi["row_token"] and t_lo["expert_indptr"] != t_hi["expert_indptr"])
        # both select a multiset of the same logits, largest first: only the indices of equal ones differ
        l = logits.float()
        assert torch.equal(torch.gather(l, 1, lo), torch.gather(l, 1, hi))
        assert bool((torch.gather(l, 1, lo).diff(dim=-1) <= 0).all())
        tied = torch.gather(l, 1, lo).diff(dim=-1) == 0
        assert bool((lo.diff(dim=-1)[tied] > 0).all()) and bool((hi.diff(dim=-1)[tied] < 0).all())
        assert _ids_are_a_selection(lo, E) and _ids_are_a_selection(hi, E)


def test_exact_weight_rows_have_exact_weights():
    """the rows planted from {0, -128, -256}: both formulations give half(1 / m) on the m tied maxima and 0 elsewhere, bit for bit"""
    n = 0
    for T, E, K in PLANTED:
        logits, exact_rows = moe_ref.planted_logits(T, E, K, PLANTED_SEED + E + K)
        assert len(exact_rows) == T // 8
        ids, w = moe_ref.route(logits, K)
        ids2, w2 = moe_ref.route_formula(logits, K)
        assert torch.equal(ids, ids2)
        l = torch.gather(logits.float(), 1, ids)[exact_rows]
        m = (l == 0).sum(-1, keepdim=True)
        assert bool((m >= 1).all()) and bool((m <= K).all())
        want = torch.where(l == 0, (1.0 / m.float()).half(), torch.zeros((), dtype=torch.float16))
        assert torch.equal(w[exact_rows].view(torch.int16), want.view(torch.int16))
        assert torch.equal(w2[exact_rows].view(torch.int16), want.view(torch.int16))
        n += int((m > 1).sum())
        # on all planted rows the two formulations stay within one fp16 ulp of each other (the bound the GPU test gives the kernel)
        assert (w.view(torch.int16).int() - w2.view(torch.int16).int()).abs().max().item() <= 1
    assert n >= 100                                           # rows whose maximum is tied


def test_route_on_signed_zeros_and_saturated_rows():
    """+0 / -0 compare equal and all-65504 rows are one tie: experts 0 .. K - 1 in order, equal weights"""
    for T, E, K in PLANTED:
        logits, _ = moe_ref.planted_logits(T, E, K, PLANTED_SEED + E + K)
        ids, w = moe_ref.route(logits, K)
        hi, _ = moe_ref.route(logits, K, tie="high")
        for r in range(4):
            assert ids[r].tolist() == list(range(K)) and hi[r].tolist() == list(range(E - 1, E - 1 - K, -1))
            assert torch.equal(w[r].view(torch.int16), torch.full((K,), 1.0 / K).half().view(torch.int16))
