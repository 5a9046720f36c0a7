"""GPU tests of the two beam-search kernels (csrc/beam.hip) against their host restatement (tests/beam_ref.py, itself checked on the CPU
by tests/test_beam_cpu.py): ops.beam_select bit for bit -- random and tie-heavy inputs, finished rows, -inf rows, an eos among the
winners, refused arguments -- and StaticBeamKvCacheInt4.fork over 40 rounds of step + fork with planted and random parents: tables,
spares and every row's visible slots.  Every comparison is EXACT."""
import numpy as np
import pytest
import torch

from tests import beam_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NEG = float("-inf")


# ------------------------------------------------------------------------------------------------ 1. beam_select
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _select_both(ids, lp, cum, fin, length, eos, w_in, w_out):
    from atom_amd import ops
    got = ops.beam_select(_dev(ids), _dev(lp), _dev(cum), _dev(fin), _dev(length), eos, w_out, w_in=w_in)
    want = beam_ref.select(ids, lp, cum, fin, length, eos, w_in, w_out)
    names = ("parent", "token", "cum", "finished", "length")
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if name == "cum":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (name, g.tolist(), w.tolist())
    return want


def _random_case(rng, G, w_in, C, coarse):
    rows = G * w_in
    lp = -np.sort(rng.random((rows, C)).astype(np.float32) * 12, axis=1)
    cum = -(rng.random(rows).astype(np.float32) * 30)
    if coarse:                                               # few distinct values: ties across rows and within rows
        lp, cum = np.round(lp), np.round(cum / 2) * 2
    ids = rng.integers(0, 1000, (rows, C)).astype(np.int64)
    fin = (rng.random(rows) < 0.35).astype(np.int32) if w_in > 1 else np.zeros(rows, np.int32)
    if rows > 1:
        lp[rng.integers(rows)] = NEG                         # a row whose candidates are all -inf
        fin[rng.integers(rows)] = 0
    length = rng.integers(1, 50, rows).astype(np.int32)
    return ids, lp.astype(np.float32), cum.astype(np.float32), fin, length


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_beam_select_equals_the_reference_bit_for_bit(W):
    rng = np.random.default_rng(W)
    live_eos = 0
    for G in (1, 3):
        for w_in in sorted({1, W}):
            for C in sorted({W, 32}):
                for coarse in (False, True):
                    case = _random_case(rng, G, w_in, C, coarse)
                    token = _select_both(*case, None, w_in, W)[1]
                    eos = int(token[-1])                      # an eos that appears among the winners
                    nfin = _select_both(*case, eos, w_in, W)[3]
                    assert nfin[-1] == 1 or case[3].any()
                    live_eos += int(nfin.sum() > case[3].sum() or not case[3].any())
    assert live_eos > 0


def test_beam_select_planted_ties_and_frozen_rows():
    z = np.zeros(3, np.int32)
    ids = np.arange(12, dtype=np.int64).reshape(3, 4) + 10
    lp = np.array([[-1, -2, -5, -6], [-1, -4, -5, -6], [0, -7, -8, -9]], dtype=np.float32)
    want = _select_both(ids, lp, np.array([-1, -2, -3], np.float32), z, z + 2, None, 3, 3)       # equal scores across rows
    assert want[0].tolist() == [0, 0, 1] and want[1].tolist() == [10, 11, 14]
    lp = np.array([[-1, -1, -1, -1], [-1, -1, -3, -3], [-9, -9, -9, -9]], dtype=np.float32)
    want = _select_both(ids, lp, np.zeros(3, np.float32), z, z, None, 3, 3)                      # equal log-probabilities in a row
    assert want[0].tolist() == [0, 0, 0] and want[1].tolist() == [10, 11, 12]
    lp = np.full((3, 4), NEG, dtype=np.float32)
    want = _select_both(ids, lp, np.array([NEG, -1, 0], np.float32), z, z, None, 3, 3)           # all -inf
    assert want[0].tolist() == [0, 0, 0] and np.isneginf(want[2]).all()
    _select_both(ids, lp, np.array([-0.0, 0.0, -0.0], np.float32), np.ones(3, np.int32), z + 5, 4, 3, 3)   # -0 == +0: parent order
    # all rows finished; a finished row beside live ones; one finished row into two outputs (padding)
    ids2, lp2 = np.array([[5, 6], [7, 5]], dtype=np.int64), np.array([[-1, -2], [-0.5, -3]], dtype=np.float32)
    _select_both(ids2, lp2, np.array([-3, -1], np.float32), np.array([1, 1], np.int32), np.array([4, 9], np.int32), 5, 2, 2)
    want = _select_both(ids2, lp2, np.array([-1.25, -1], np.float32), np.array([1, 0], np.int32), np.array([4, 9], np.int32), 5, 2, 2)
    assert want[0].tolist() == [0, 1] and want[1].tolist() == [5, 7] and want[3].tolist() == [1, 0] and want[4].tolist() == [4, 10]
    want = _select_both(ids2[:1], lp2[:1], np.array([-2], np.float32), np.array([1], np.int32), np.array([3], np.int32), 5, 1, 2)
    assert want[2].tolist() == [-2, NEG]


def test_beam_select_updates_the_state_in_place():
    """out = the inputs of the same name (what the captured step does): the same result as with fresh outputs"""
    from atom_amd import ops
    rng = np.random.default_rng(9)
    ids, lp, cum, fin, length = _random_case(rng, 3, 4, 7, True)
    want = beam_ref.select(ids, lp, cum, fin, length, int(ids[0, 0]), 4, 4)
    d = [_dev(x) for x in (ids, lp, cum, fin, length)]
    parent, token = torch.zeros(12, dtype=torch.int32, device=DEV), torch.zeros(12, dtype=torch.int64, device=DEV)
    ops.beam_select(*d, int(ids[0, 0]), 4, out=(parent, token, d[2], d[3], d[4]))
    for g, w in zip((parent, token, d[2], d[3], d[4]), want):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), w.view(np.uint8))


def test_beam_select_rejects_bad_arguments():
    from atom_amd import _lib as L
    from atom_amd import ops
    G, W, C = 2, 4, 8
    ins = [torch.zeros((G * W, C), dtype=torch.int64, device=DEV), torch.zeros((G * W, C), dtype=torch.float32, device=DEV),
           torch.zeros(G * W, dtype=torch.float32, device=DEV), torch.zeros(G * W, dtype=torch.int32, device=DEV),
           torch.zeros(G * W, dtype=torch.int32, device=DEV)]
    outs = [torch.full((G * W + 2,), 77, dtype=d, device=DEV) for d in (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32)]
    ip, op = [t.data_ptr() for t in ins], [t.data_ptr() for t in outs]
    call = lambda i, o, g=G, w_in=W, w_out=W, c=C: L.lib().atom_beam_select(*i, g, w_in, w_out, c, -1, *o, None)
    for k in range(5):
        assert call(ip[:k] + [None] + ip[k + 1:], op) == L.ERR_INVALID_ARG
        assert call(ip, op[:k] + [None] + op[k + 1:]) == L.ERR_INVALID_ARG
        assert call(ip[:k] + [ip[k] + 2] + ip[k + 1:], op) == L.ERR_ALIGN
        assert call(ip, op[:k] + [op[k] + 2] + op[k + 1:]) == L.ERR_ALIGN
    assert call(ip[:1] + ip[1:], [op[0], op[1] + 4] + op[2:]) == L.ERR_ALIGN          # int64 tokens off 8 bytes
    assert call(ip, op, w_in=0, w_out=0) == L.ERR_SHAPE and call(ip, op, w_in=17, w_out=17) == L.ERR_SHAPE
    assert call(ip, op, w_in=1, w_out=17) == L.ERR_SHAPE and call(ip, op, w_in=2, w_out=4) == L.ERR_SHAPE
    assert call(ip, op, c=3) == L.ERR_SHAPE and call(ip, op, c=33) == L.ERR_SHAPE and call(ip, op, g=0) == L.ERR_SHAPE
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in outs)                # none of the refused calls launched anything
    with pytest.raises(ValueError):
        ops.beam_select(*ins, None, 0)
    with pytest.raises(ValueError):
        ops.beam_select(*ins, None, 17)
    with pytest.raises(ValueError):
        ops.beam_select(ins[0][:, :3], ins[1][:, :3], *ins[2:], None, 4)
    with pytest.raises(L.AtomHipError):
        ops.beam_select(*[t.cpu() for t in ins], None, 4)


# ------------------------------------------------------------------------------------------------ 2. the fork
def _pool(heads, capacity, block):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(1, heads, 128, capacity, block, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def _beam_cache(heads, P, W, starts, reserve, capacity=None):
    """a pool whose prompts' slots hold a pattern, the beam cache over them and the reference built from the device's state"""
    from atom_amd.utils import KvCacheInt4, StaticBeamKvCacheInt4
    need = sum(-(-n // P) + W * (-(-(n + reserve) // P) - n // P + 1) for n in starts)
    pool = _pool(heads, need + 3 if capacity is None else capacity, P)
    seqs = [KvCacheInt4(pool, n) for n in starts]
    for g, c in enumerate(seqs):
        for i in range(c.seqlen):
            pool.buf[c.indicies[i // P], :, :, :, i % P] = 200 + g
            pool.param[c.indicies[i // P], :, :, :, i % P] = 1000 + 10 * g + i
    free = pool.num_free_blocks
    skv = StaticBeamKvCacheInt4(seqs, W, reserve)
    return pool, seqs, skv, free


def _ref_of(pool, skv):
    arrays = [pool.buf.cpu().numpy(), pool.param.view(torch.int16).cpu().numpy()]
    return beam_ref.RefBeamCache(skv.page_table.tolist(), skv.spare.tolist(), skv.row_pages.tolist(),
                                 [n for n in skv.seqlens], skv.page_size, skv.num_beams, arrays)


def _assert_same_state(pool, skv, ref):
    assert skv.page_table.tolist() == ref.tables and skv.spare.tolist() == ref.spare
    buf, param = pool.buf.cpu().numpy(), pool.param.view(torch.int16).cpu().numpy()
    for r, n in enumerate(ref.lens):
        for j in range(-(-n // ref.P)):
            page, m = ref.tables[r][j], min(ref.P, n - j * ref.P)
            assert np.array_equal(buf[page][..., :m, :], ref.arrays[0][page][..., :m, :]), (r, j)
            assert np.array_equal(param[page][..., :m, :], ref.arrays[1][page][..., :m, :]), (r, j)


@pytest.mark.parametrize("heads,P,W", [(1, 16, 2), (2, 16, 4), (2, 32, 2), (1, 32, 4)])
def test_fork_follows_the_reference_over_40_rounds(heads, P, W):
    """start lengths 5 and 16: a partial and a full first page; 40 tokens: every row crosses page boundaries, forks meet off == 0"""
    starts, rounds, G = [5, 16], 40, 2
    pool, seqs, skv, free = _beam_cache(heads, P, W, starts, rounds)
    all_pages = {i for c in seqs for i in c.indicies} | set(skv._pages)
    ref = _ref_of(pool, skv)
    ref.check_ownership(all_pages)
    # the construction: beam 0 sits on the prompt's own pages, every beam reads the prompt's pattern
    for g, c in enumerate(seqs):
        assert ref.tables[g * W][:len(c.indicies)] == c.indicies
        for b in range(W):
            assert ref.tables[g * W + b][:c.seqlen // P] == c.indicies[:c.seqlen // P]
            for i in range(c.seqlen):
                page, off = ref.slot(g * W + b, i)
                assert int(ref.arrays[0][page, 0, 0, 0, off, 0]) == 200 + g and int(pool.param[page, 0, 1, 0, off, 1]) == 1000 + 10 * g + i
    assert skv.indptr.tolist() == [sum(-(-n // P) for n in ref.lens[:r]) for r in range(G * W + 1)]
    rng = np.random.default_rng(heads * 100 + P + W)
    planted = [list(range(W)), [0] * W, [1, 0] + list(range(2, W)), [(b + 1) % W for b in range(W)]]
    for step in range(rounds):
        skv.step()
        ref.step()
        for r in range(G * W):                               # what the forward does: every row writes its new slot
            page, off = ref.slot(r, ref.lens[r] - 1)
            pool.buf[page, :, :, :, off] = (17 * r + step) % 256
            pool.param[page, :, :, :, off] = r * 64 + step
            ref.arrays[0][page, :, :, :, off] = (17 * r + step) % 256
            ref.arrays[1][page, :, :, :, off] = torch.tensor(float(r * 64 + step), dtype=torch.float16).view(torch.int16).item()
        parent = planted[step % 5] * G if step % 5 < 4 else rng.integers(0, W, G * W).tolist()
        before = ref.writable()
        skv.fork(torch.tensor(parent, dtype=torch.int32, device=DEV))
        ref.fork(parent)
        assert ref.writable() == before
        ref.check_ownership(all_pages)
        _assert_same_state(pool, skv, ref)
    # the tables the attention ops read after the next rebuild: each row's pages in order
    skv.step(0)
    indptr, ind = skv.indptr.tolist(), skv.indicies.tolist()
    for r, n in enumerate(ref.lens):
        assert ind[indptr[r]:indptr[r + 1]] == ref.tables[r][:-(-n // P)]
    skv.close()
    assert skv.seqlens == [n + rounds for n in starts for _ in range(W)] and pool.num_free_blocks == free


def test_fork_keeps_rows_with_a_bad_parent_and_flags_them():
    W, P = 4, 16
    pool, seqs, skv, free = _beam_cache(1, P, W, [5, 16], 8)
    all_pages = {i for c in seqs for i in c.indicies} | set(skv._pages)
    skv.step()
    ref = _ref_of(pool, skv)
    ref.step()
    assert int(skv.state[0].item()) == 0
    parent = [-1, 0, W, 1, 2, 2 ** 30, 0, -2 ** 31]
    skv.fork(torch.tensor(parent, dtype=torch.int32, device=DEV))
    rows_before = [list(t) for t in ref.tables]
    ref.fork(parent)
    assert ref.status == beam_ref.BAD_PARENT and int(skv.state[0].item()) == beam_ref.BAD_PARENT
    for r in (0, 2, 5, 7):
        assert ref.tables[r] == rows_before[r]
    _assert_same_state(pool, skv, ref)
    ref.check_ownership(all_pages)
    with pytest.raises(RuntimeError, match="parent"):
        skv.sync_host()
    skv.close()                                              # the status word was cleared by the read that raised
    assert pool.num_free_blocks == free


def test_fork_refuses_aliased_tables_and_bad_arguments():
    from atom_amd import _lib as L
    pool, seqs, skv, free = _beam_cache(1, 16, 2, [5], 4)
    parent = torch.zeros(2, dtype=torch.int32, device=DEV)
    before = skv.tables.tolist()
    t = dict(data=pool.buf.data_ptr(), param=pool.param.data_ptr(), tin=skv.page_table.data_ptr(), tout=skv.table_out.data_ptr(),
             sin=skv.spare.data_ptr(), sout=skv.spare_out.data_ptr(), rows=skv.row_pages.data_ptr(), lens=skv.lengths.data_ptr(),
             state=skv.state.data_ptr(), parent=parent.data_ptr())
    dims = dict(batch=2, w=2, cap=skv.max_pages, capacity=pool.buf.size(0), layers=1, heads=1, page=16, dim=128)

    def call(**kw):
        a = {**t, **dims, **kw}
        return L.lib().atom_kv_beam_fork_i4(*(a[k] for k in list(t) + list(dims)), None)
    assert call(tout=t["tin"]) == L.ERR_INVALID_ARG and call(sout=t["sin"]) == L.ERR_INVALID_ARG
    assert call(tout=t["tin"] + 4) == L.ERR_INVALID_ARG                       # overlapping, not only equal
    for k in t:
        assert call(**{k: None}) == L.ERR_INVALID_ARG, k
        assert call(**{k: t[k] + 2}) == L.ERR_ALIGN, k
    assert call(param=t["param"] + 4) == L.ERR_ALIGN                          # the page copy moves 16 bytes at a time
    assert call(w=0) == L.ERR_SHAPE and call(w=17) == L.ERR_SHAPE and call(batch=3) == L.ERR_SHAPE and call(batch=0) == L.ERR_SHAPE
    assert call(cap=0) == L.ERR_SHAPE and call(page=24) == L.ERR_SHAPE and call(dim=64) == L.ERR_SHAPE and call(capacity=0) == L.ERR_SHAPE
    torch.cuda.synchronize()
    assert skv.tables.tolist() == before
    with pytest.raises(L.AtomHipError):
        skv.fork(parent.cpu())
    skv.close()
    assert pool.num_free_blocks == free


def test_beam_cache_raises_before_keeping_a_page_when_the_pool_is_too_small():
    from atom_amd.utils import KvCacheInt4, StaticBeamKvCacheInt4
    pool = _pool(1, 12, 16)
    seqs = [KvCacheInt4(pool, 5), KvCacheInt4(pool, 16)]
    free = pool.num_free_blocks
    with pytest.raises(RuntimeError, match="pages needed"):
        StaticBeamKvCacheInt4(seqs, 4, 40)
    assert pool.num_free_blocks == free
