"""GPU tests of the LoRA ops (ops.bgmv, ops.add_lora, ops.kv_quant_u4; csrc/lora_f16.hip).  The core comparisons are BIT FOR BIT
against tests/lora_ref.py on exact-arithmetic inputs (small integers, a power-of-two scale: every sum is exact in FP32 whatever the
order, the helper asserts it), so a wrong lane map, a masked row that leaks, a tile that crosses a segment or an id that is not
honoured shows as a wrong integer, not as noise.  One planted row shows the one thing exact inputs cannot otherwise see (t rounded
to fp16 between the passes), and the reference test's own random case runs within its own tolerance."""
import pytest
import torch

from tests import lora_ref
from tests.lora_ref import bits

pytestmark = pytest.mark.gpu

H1, H2, CAP, LAYERS, LAYER = 320, 192, 3, 2, 1
SEG_LENS = [1, 15, 16, 17, 0, 33]            # 82 rows: tile boundaries inside, at and next to segment ends; an empty segment
SEG_IDS = [2, -1, 0, 2, 1, 1]
GUARD = 8
SENTINEL = 0x7BFF                            # fp16 65504: survives only if the guard rows are never written


def _row_ids(rows):
    """non-monotonic, repeated, with -1"""
    return [(2, 0, -1, 1, 0, 2, 2, -1, 1)[i % 9] for i in range(rows)]


def _indptr(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


_CASES = {}


def _case(rank):
    """exact inputs of (82 + 8 guard rows, 320 -> rank -> 192), made once per rank and never modified"""
    if rank not in _CASES:
        y, x, wa, wb = lora_ref.exact_inputs(sum(SEG_LENS), H1, H2, rank, CAP, LAYERS, seed=10 + rank, guard=GUARD)
        y[sum(SEG_LENS):] = torch.tensor([SENTINEL], dtype=torch.int16).view(torch.float16)
        _CASES[rank] = (y, x, wa, wb, x.cuda(), wa.cuda(), wb.cuda())
    return _CASES[rank]


@pytest.mark.parametrize("id_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("rank", [8, 16, 24, 32, 64])
@pytest.mark.parametrize("rows", [1, 3, 17, 70])
def test_add_lora_one_row_segments(rows, rank, id_dtype):
    from atom_amd import ops
    y, x, wa, wb, xd, wad, wbd = _case(rank)
    ids = _row_ids(rows)
    want = lora_ref.add_lora(y[:rows], x[:rows], wa, wb, ids, LAYER, 0.25, exact=True)
    got = y.cuda()
    ops.add_lora(got[:rows], xd[:rows], wad, wbd, torch.tensor(ids, dtype=id_dtype, device="cuda"), LAYER, 0.25)
    assert torch.equal(bits(got[:rows].cpu()), bits(want))
    assert torch.equal(bits(got[rows:].cpu()), bits(y[rows:]))                                   # nothing behind the batch moved
    none = [i for i, a in enumerate(ids) if a < 0]
    assert torch.equal(bits(got[none].cpu()), bits(y[none]))


@pytest.mark.parametrize("rank", [8, 16, 24, 32, 64])
def test_add_lora_segments(rank):
    from atom_amd import ops
    y, x, wa, wb, xd, wad, wbd = _case(rank)
    ptr, rows = _indptr(SEG_LENS), sum(SEG_LENS)
    want = lora_ref.add_lora(y, x, wa, wb, SEG_IDS, LAYER, 0.25, seg_indptr=ptr, exact=True)
    got = y.cuda()
    ops.add_lora(got, xd, wad, wbd, torch.tensor(SEG_IDS, dtype=torch.int32, device="cuda"), LAYER, 0.25,
                 seg_indptr=torch.tensor(ptr, dtype=torch.int32, device="cuda"))
    got = got.cpu()
    assert torch.equal(bits(got[:rows]), bits(want[:rows]))
    assert torch.equal(bits(got[1:16]), bits(y[1:16]))                                           # the -1 segment, as bits
    assert bool((bits(got[rows:]) == SENTINEL).all())                                            # the guard rows behind seg_indptr[S]
    assert not torch.equal(got[16:32], y[16:32]) and not torch.equal(got[49:82], y[49:82])


@pytest.mark.parametrize("rank", [8, 64])
def test_segment_table_longer_than_one_search_pass(rank):
    """lora_ref.long_table: 200 segments, so the kernels' search of 64 segments at a time runs four passes and carries its tile
    count over a block of 64 empty segments into the third; the first segment starts at row 5.  add_lora 320 -> rank -> 192 and
    each pass alone, bit for bit on exact inputs (tests/test_lora_cpu.py: a lost count changes every non-empty segment behind 128)"""
    from atom_amd import ops
    ptr, ids = lora_ref.long_table()
    y, x, wa, wb, y_s, x_e = lora_ref.long_case(rank)
    rows, layer = ptr[-1], lora_ref.LONG_LAYER
    assert y.size(0) == rows + lora_ref.LONG_GUARD >= lora_ref.LONG_S
    idt = torch.tensor(ids, dtype=torch.int32, device="cuda")
    ptrt = torch.tensor(ptr, dtype=torch.int32, device="cuda")
    xd, wad, wbd = x.cuda(), wa.cuda(), wb.cuda()
    runs = [(y, lora_ref.add_lora(y, x, wa, wb, ids, layer, 0.25, seg_indptr=ptr, exact=True),
             lambda o: ops.add_lora(o, xd, wad, wbd, idt, layer, 0.25, seg_indptr=ptrt)),
            (y_s, lora_ref.bgmv(y_s, x, wa, ids, layer, 0.25, seg_indptr=ptr, exact=True),
             lambda o: ops.bgmv(o, xd, wad, idt, layer, 0.25, seg_indptr=ptrt)),
            (y, lora_ref.bgmv(y, x_e, wb, ids, layer, 0.25, seg_indptr=ptr, exact=True),
             lambda o: ops.bgmv(o, x_e.cuda(), wbd, idt, layer, 0.25, seg_indptr=ptrt))]
    for y0, want, run in runs:
        got = y0.cuda()
        run(got)
        got = got.cpu()
        assert torch.equal(bits(got[:rows]), bits(want[:rows]))
        assert torch.equal(bits(got[:ptr[0]]), bits(y0[:ptr[0]]))                                # the rows in front of the first segment
        assert bool((bits(got[rows:]) == lora_ref.LONG_SENTINEL).all())                          # the guard rows behind seg_indptr[S]
        for s, a in enumerate(ids):
            if not 0 <= a < lora_ref.LONG_CAP:
                assert torch.equal(bits(got[ptr[s]:ptr[s + 1]]), bits(y0[ptr[s]:ptr[s + 1]])), s  # segments without an adapter
        assert not torch.equal(got[ptr[128]:rows], y0[ptr[128]:rows])


def test_add_lora_ids_outside_the_pool_touch_nothing():
    from atom_amd import ops
    y, x, wa, wb, xd, wad, wbd = _case(8)
    got = y.cuda()
    ops.add_lora(got[:5], xd[:5], wad, wbd, torch.tensor([CAP, -7, 2 ** 31 - 1, -2 ** 31, CAP + 1000], dtype=torch.int64, device="cuda"), LAYER, 0.25)
    ops.add_lora(got, xd, wad, wbd, torch.tensor([CAP] * 6, dtype=torch.int32, device="cuda"), LAYER, 0.25,
                 seg_indptr=torch.tensor(_indptr(SEG_LENS), dtype=torch.int32, device="cuda"))
    assert torch.equal(bits(got.cpu()), bits(y))


@pytest.mark.parametrize("segmented", [False, True])
def test_add_lora_long_sums_rank_64(segmented):
    """H1 4096 (every K step of every wave), rank 64 (two K steps of the second pass), 33 rows"""
    from atom_amd import ops
    rows = 33
    y, x, wa, wb = lora_ref.exact_inputs(rows, 4096, 1024, 64, 2, 1, seed=4)
    ids, ptr = ([1, 0], [0, 16, 33]) if segmented else ([i % 2 for i in range(rows)], None)
    want = lora_ref.add_lora(y, x, wa, wb, ids, 0, 0.125, seg_indptr=ptr, exact=True)
    got = y.cuda()
    ops.add_lora(got, x.cuda(), wa.cuda(), wb.cuda(), torch.tensor(ids, device="cuda"), 0, 0.125,
                 seg_indptr=None if ptr is None else torch.tensor(ptr, dtype=torch.int32, device="cuda"))
    assert torch.equal(bits(got.cpu()), bits(want))


@pytest.mark.parametrize("segmented", [False, True])
@pytest.mark.parametrize("rank", [8, 16, 24, 32, 40, 48, 56, 64])
def test_bgmv_alone_in_both_shape_regimes(rank, segmented):
    """shrink (H2 = rank) and expand (H1 = rank), each on rows and on the segment table"""
    from atom_amd import ops
    y, x, wa, wb, xd, wad, wbd = _case(8)
    g = torch.Generator().manual_seed(rank)
    rows = sum(SEG_LENS)
    ids, ptr = (SEG_IDS, _indptr(SEG_LENS)) if segmented else (_row_ids(rows), None)
    idt = torch.tensor(ids, dtype=torch.int32, device="cuda")
    ptrt = None if ptr is None else torch.tensor(ptr, dtype=torch.int32, device="cuda")
    w_s = torch.randint(-1, 2, (CAP, LAYERS, rank, H1), generator=g).half()
    y_s = torch.randint(-8, 9, (rows, rank), generator=g).half()
    want = lora_ref.bgmv(y_s, x[:rows], w_s, ids, LAYER, 0.25, seg_indptr=ptr, exact=True)
    got = y_s.cuda()
    ops.bgmv(got, xd[:rows], w_s.cuda(), idt, LAYER, 0.25, seg_indptr=ptrt)
    assert torch.equal(bits(got.cpu()), bits(want))
    w_e = torch.randint(-1, 2, (CAP, LAYERS, H2, rank), generator=g).half()
    x_e = torch.randint(-2, 3, (rows, rank), generator=g).half()
    want = lora_ref.bgmv(y[:rows], x_e, w_e, ids, LAYER, 0.25, seg_indptr=ptr, exact=True)
    got = y[:rows].cuda()
    ops.bgmv(got, x_e.cuda(), w_e.cuda(), idt, LAYER, 0.25, seg_indptr=ptrt)
    assert torch.equal(bits(got.cpu()), bits(want))


@pytest.mark.parametrize("segmented", [False, True])
def test_t_is_rounded_to_fp16_between_the_passes(segmented):
    """row 0: t_0 = 2049 (1024 products 2 * 1 and one 1 * 1), t_1 = -2048, B[n, 0] = B[n, 1] = 1.  fp16 rounds 2049 to 2048: the
    delta is 0; a kernel that keeps t in FP32 adds `scale`"""
    from atom_amd import ops
    h1, h2, r, rows, scale = 1088, 64, 8, 3, 0.25
    x = torch.zeros(rows, h1).half()
    x[0, :1024], x[0, 1024] = 2, 1
    wa, wb = torch.zeros(1, 1, r, h1).half(), torch.zeros(1, 1, h2, r).half()
    wa[0, 0, 0, :1025] = 1
    wa[0, 0, 1, :1024] = -1
    wb[0, 0, :, 0:2] = 1
    y = torch.arange(rows * h2).reshape(rows, h2).remainder(17).half()
    ids, ptr = ([0], [0, rows]) if segmented else ([0] * rows, None)
    want = lora_ref.add_lora(y, x, wa, wb, ids, 0, scale, seg_indptr=ptr)          # (not exact=True: t = 2049 is the plant)
    fp32_t = lora_ref.add_lora(y, x, wa, wb, ids, 0, scale, seg_indptr=ptr, round_t=False, exact=True)
    assert torch.equal(want, y) and torch.equal(fp32_t[0], y[0] + scale)                         # the plant tells the two apart
    got = y.cuda()
    ops.add_lora(got, x.cuda(), wa.cuda(), wb.cuda(), torch.tensor(ids, device="cuda"), 0, scale,
                 seg_indptr=None if ptr is None else torch.tensor(ptr, dtype=torch.int32, device="cuda"))
    assert torch.equal(bits(got.cpu()), bits(want))


def _random_case(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, nl, h1, h2, r, bs = 4, 2, 4096, 11008, 8, 32
    rn = lambda *s: torch.randn(s, device="cuda", generator=g).half()
    return rn(n, nl, r, h1), rn(n, nl, h2, r), rn(bs, h1), rn(bs, h2), torch.randint(0, n, (bs,), device="cuda", generator=g)


def test_add_lora_random_inputs_within_the_reference_tests_tolerance():
    """the reference test's own case (tests/test_bgmv.py there): rows 32, 4096 -> 8 -> 11008, scale 0.123, normal inputs, one id per
    row, against the float32 restatement with t rounded to fp16, rtol = atol = 5e-3.  (t is about 64 here, where an fp16 step is
    1/16: a t that the two summation orders round to different neighbours moves a whole row by 0.123 / 16 * |B[n, j]| -- the reference's
    own kernel has that exposure against this restatement too; the inputs are seeded, and the kernel's order is fixed.)"""
    from atom_amd import ops
    wa, wb, x, y, ids = _random_case(0xabcd)
    scale = 0.123
    for layer in range(wa.size(1)):
        ref = y.clone()
        for i, a in enumerate(ids.tolist()):
            t = (x[i:i + 1].float() @ wa[a, layer].float().t()).half().float()
            ref[i] += ((t @ wb[a, layer].float().t()).squeeze(0) * torch.tensor(scale, dtype=torch.float32, device="cuda"))
        got = y.clone()
        ops.add_lora(got, x, wa, wb, ids, layer, scale)
        print("max abs diff", (got.float() - ref.float()).abs().max().item())
        torch.testing.assert_close(got, ref, rtol=5e-3, atol=5e-3)


def test_segmented_passes_on_random_inputs_each_within_that_tolerance():
    """the same operands through the segment table (the MFMA kernels), pass by pass, so that no comparison crosses the rounding of t:
    the shrink pass against half(float32 x A^T), then the expand pass FROM THE KERNEL'S t against the float32 restatement, both with
    rtol = atol = 5e-3 (an fp16 step is 2^-10 relative); test_add_lora_is_two_bgmv_passes_bit_for_bit ties add_lora to the two passes"""
    from atom_amd import ops
    wa, wb, x, y, ids = _random_case(0xabce)
    ptr, scale, layer = [0, 5, 21, 32], 0.123, 1
    ids = ids[:3].contiguous()
    ptrd = torch.tensor(ptr, dtype=torch.int32, device="cuda")
    t = torch.zeros((x.size(0), wa.size(2)), dtype=torch.float16, device="cuda")
    ops.bgmv(t, x, wa, ids, layer, 1.0, seg_indptr=ptrd)
    got = y.clone()
    ops.bgmv(got, t, wb, ids, layer, scale, seg_indptr=ptrd)
    t_ref, ref = torch.empty_like(t), y.clone()
    for s, a in enumerate(ids.tolist()):
        sl = slice(ptr[s], ptr[s + 1])
        t_ref[sl] = (x[sl].float() @ wa[a, layer].float().t()).half()
        ref[sl] += ((t[sl].float() @ wb[a, layer].float().t()) * torch.tensor(scale, dtype=torch.float32, device="cuda"))
    print("max abs diff t", (t.float() - t_ref.float()).abs().max().item(), "y", (got.float() - ref.float()).abs().max().item())
    torch.testing.assert_close(t, t_ref, rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(got, ref, rtol=5e-3, atol=5e-3)
    assert not torch.equal(got, y)


@pytest.mark.parametrize("segmented", [False, True])
def test_add_lora_is_two_bgmv_passes_bit_for_bit(segmented):
    """normal inputs, where the order of every sum matters: add_lora (one launch on one-row segments, t in LDS) leaves the bits of
    bgmv into a zeroed t with scale 1 followed by bgmv into y"""
    from atom_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    n, nl, h1, h2, r, bs = 3, 2, 1088, 2112, 24, 45
    rn = lambda *s: torch.randn(s, device="cuda", generator=g).half()
    wa, wb, x, y = rn(n, nl, r, h1), rn(n, nl, h2, r), rn(bs, h1), rn(bs, h2)
    if segmented:
        ids = torch.tensor([1, -1, 2, 0], dtype=torch.int32, device="cuda")
        ptr = torch.tensor([0, 7, 20, 36, 45], dtype=torch.int32, device="cuda")
    else:
        ids, ptr = torch.tensor(_row_ids(bs), dtype=torch.int32, device="cuda"), None
    one, two, t = y.clone(), y.clone(), torch.zeros((bs, r), dtype=torch.float16, device="cuda")
    ops.add_lora(one, x, wa, wb, ids, 1, 0.37, seg_indptr=ptr)
    ops.bgmv(t, x, wa, ids, 1, 1.0, seg_indptr=ptr)
    ops.bgmv(two, t, wb, ids, 1, 0.37, seg_indptr=ptr)
    assert torch.equal(bits(one), bits(two)) and not torch.equal(one, y)


def _slots(seqs, pool):
    block = pool.block_len
    out = []
    for c in seqs:
        for k in range(-(-c.seqlen // block)):
            n = min(block, c.seqlen - k * block)
            out.append((pool.buf[c.indicies[k], :, :, :, :n].clone(), pool.param[c.indicies[k], :, :, :, :n].clone().view(torch.int16)))
    return out


def test_kv_quant_u4_then_append_equals_the_fused_quantising_append():
    """random fp16 k / v: kv_quant_u4 + append_kv_i4 leaves the cache bytes of quant_append_kv_i4 on k.float() (the cast is exact);
    two sequences whose appended tokens end a page, start one and sit inside one"""
    from atom_amd import ops
    from atom_amd.utils import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    heads, layers, block = 3, 2, 16
    g = torch.Generator(device="cuda").manual_seed(7)
    pools = [KvPoolInt4(layers, heads, 128, 8, block, torch.device("cuda")) for _ in range(2)]
    for p in pools:
        p.buf.zero_()
        p.param.zero_()
    seqs = [[KvCacheInt4(p, n) for n in (15, 31)] for p in pools]
    for step in range(3):                                    # lengths 16 / 32 (last slot of a page), 17 / 33 (first of the next), 18 / 34
        k = (torch.randn((2, heads, 128), device="cuda", generator=g) * (1 + step)).half()
        v = torch.randn((2, heads, 128), device="cuda", generator=g).half()
        k[1, 0] = 0.5                                        # an all-equal head vector: scale 0
        for s in seqs:
            for c in s:
                c.acquire_one()
        for layer in range(layers):
            ops.quant_append_kv_i4(BatchedKvCacheInt4(seqs[0]), k.float().view(2, -1), v.float().view(2, -1), layer)
            (k4, ks), (v4, vs) = ops.kv_quant_u4(k), ops.kv_quant_u4(v)
            assert k4.shape == (2, heads, 64) and k4.dtype == torch.uint8 and ks.shape == (2, heads, 2) and ks.dtype == torch.float16
            ops.append_kv_i4(BatchedKvCacheInt4(seqs[1]), k4, v4, ks, vs, layer)
    a, b = _slots(seqs[0], pools[0]), _slots(seqs[1], pools[1])
    assert len(a) == len(b) == 2 + 3
    for (da, pa), (db, pb) in zip(a, b):
        assert torch.equal(da, db) and torch.equal(pa, pb)
    assert bool(a[0][0].any()) and bool(a[-1][0][..., 1, :].any())


def test_add_lora_in_a_captured_graph_follows_the_id_buffer():
    from atom_amd import ops
    y, x, wa, wb, xd, wad, wbd = _case(24)
    rows = sum(SEG_LENS)
    ptr = _indptr(SEG_LENS)
    ptrd = torch.tensor(ptr, dtype=torch.int32, device="cuda")
    ids_rows = torch.tensor(_row_ids(rows), dtype=torch.int32, device="cuda")
    ids_seg = torch.tensor(SEG_IDS, dtype=torch.int32, device="cuda")
    y0 = y[:rows].cuda()
    ya, yb = y0.clone(), y0.clone()

    def step():
        ya.copy_(y0)
        yb.copy_(y0)
        ops.add_lora(ya, xd[:rows], wad, wbd, ids_rows, LAYER, 0.25)
        ops.add_lora(yb, xd[:rows], wad, wbd, ids_seg, LAYER, 0.25, seg_indptr=ptrd)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    new_rows = [(a + 2) % 4 - 1 for a in _row_ids(rows)]     # every id changes (-1 -> 0, 0 -> 1, 1 -> 2, 2 -> -1)
    new_seg = [1, 2, -1, 0, 0, 2]
    ids_rows.copy_(torch.tensor(new_rows, dtype=torch.int32))
    ids_seg.copy_(torch.tensor(new_seg, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(ya.cpu()), bits(lora_ref.add_lora(y[:rows], x[:rows], wa, wb, new_rows, LAYER, 0.25, exact=True)))
    assert torch.equal(bits(yb.cpu()), bits(lora_ref.add_lora(y[:rows], x[:rows], wa, wb, new_seg, LAYER, 0.25, seg_indptr=ptr, exact=True)))
