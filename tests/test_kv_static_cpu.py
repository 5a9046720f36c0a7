"""CPU-only checks of the bookkeeping behind StaticBatchedKvCacheInt4: KvCacheInt4.reserve (pages up front, no token), acquire_one on
reserved pages, KvCacheInt4.trim (the spare pages back to the pool), and the page-table step op's refusal of CPU tensors."""
import types

import pytest
import torch


def _pool(capacity=64, block=16):
    from atom_amd.utils.kvcache import KvPoolInt4
    return KvPoolInt4(2, 4, 128, capacity, block, torch.device("cpu"))


@pytest.mark.parametrize("block", [16, 32])
@pytest.mark.parametrize("seqlen,n", [(0, 0), (0, 1), (1, 15), (1, 16), (16, 0), (16, 1), (17, 40), (33, 31), (250, 100)])
def test_reserve_allocates_pages_and_leaves_the_length_alone(block, seqlen, n):
    from atom_amd.utils.kvcache import KvCacheInt4
    pool = _pool(block=block)
    c = KvCacheInt4(pool, seqlen)
    before, free = list(c.indicies), pool.num_free_blocks
    c.reserve(n)
    want = -(-(seqlen + n) // block)
    assert len(c.indicies) == want and c.indicies[:len(before)] == before and len(set(c.indicies)) == want
    assert c.seqlen == seqlen
    assert pool.num_free_blocks == free - (want - len(before))
    c.reserve(n)                                             # already reserved: nothing more
    assert len(c.indicies) == want and pool.num_free_blocks == free - (want - len(before))
    with pytest.raises(ValueError):
        c.reserve(-1)


@pytest.mark.parametrize("block", [16, 32])
def test_acquire_one_after_reserve_allocates_nothing_until_the_reserve_is_used_up(block):
    from atom_amd.utils.kvcache import KvCacheInt4
    pool = _pool(block=block)
    c = KvCacheInt4(pool, 17)
    c.reserve(40)
    pages, free = list(c.indicies), pool.num_free_blocks
    room = len(pages) * block - 17
    assert room >= 40
    for i in range(room):
        c.acquire_one()
        assert c.seqlen == 18 + i and c.indicies == pages and pool.num_free_blocks == free
    c.acquire_one()                                          # the reserve is used up: a new page, as without a reserve
    assert c.seqlen == 18 + room and c.indicies[:-1] == pages and len(c.indicies) == len(pages) + 1
    assert pool.num_free_blocks == free - 1


@pytest.mark.parametrize("block", [16, 32])
def test_trim_returns_exactly_the_spare_pages(block):
    from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4
    pool = _pool(block=block)
    free0 = pool.num_free_blocks
    other = KvCacheInt4(pool, 40)                            # a neighbour whose pages must not move
    other_pages = list(other.indicies)
    c = KvCacheInt4(pool, 33)
    c.reserve(100)
    c.acquire(5)
    need = -(-38 // block)
    keep, spare = c.indicies[:need], c.indicies[need:]
    assert len(spare) == -(-133 // block) - need > 0
    c.trim()
    assert c.indicies == keep and c.seqlen == 38
    assert pool.num_free_blocks == free0 - need - len(other_pages)
    for idx in spare:                                        # they are free again: freeing one twice is refused
        with pytest.raises(AssertionError):
            pool.free_block(idx)
    c.trim()                                                 # nothing spare: nothing happens
    assert c.indicies == keep and pool.num_free_blocks == free0 - need - len(other_pages)
    kv = BatchedKvCacheInt4([c, other])                      # an ordinary sequence again
    assert kv.indptr.tolist() == [0, need, need + len(other_pages)] and kv.indicies.tolist() == keep + other_pages
    assert kv.last_page_offset.tolist() == [(38 - 1) % block + 1, (40 - 1) % block + 1] and kv.max_pages == max(need, len(other_pages))
    c.release()
    other.release()
    assert pool.num_free_blocks == free0


def test_trim_on_a_page_boundary_and_of_an_empty_sequence():
    from atom_amd.utils.kvcache import KvCacheInt4
    pool = _pool()
    free0 = pool.num_free_blocks
    a, b = KvCacheInt4(pool, 16), KvCacheInt4(pool, 0)
    a.reserve(1)
    b.reserve(5)
    assert len(a.indicies) == 2 and len(b.indicies) == 1 and pool.num_free_blocks == free0 - 3
    a.trim()
    b.trim()
    assert len(a.indicies) == 1 and a.seqlen == 16 and b.indicies == [] and b.seqlen == 0
    assert pool.num_free_blocks == free0 - 1
    a.release()
    assert pool.num_free_blocks == free0


def test_kv_step_refuses_cpu_tensors():
    """no CPU fallback: the page tables are stepped by the HIP kernel or not at all"""
    from atom_amd import ops
    from atom_amd._lib import AtomHipError
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    kv = types.SimpleNamespace(page_table=z(2, 3), row_pages=z(2), lengths=z(4), indptr=z(3), indicies=z(6), last_page_offset=z(2),
                               state=z(4), page_size=16)
    with pytest.raises(AtomHipError):
        ops.kv_step_i4(kv, 1)


def test_generate_is_exported():
    from atom_amd import e2e, utils
    assert callable(e2e.generate) and isinstance(e2e.DecodeGraph, type) and isinstance(utils.StaticBatchedKvCacheInt4, type)
