"""GPU tests of token generation by graph replay: the device-side page-table step (atom_kv_step_i4), StaticBatchedKvCacheInt4 under
every attention op, DecodeGraph and generate().  Every comparison is EXACT: the replayed step runs the same kernels on the same
inputs as the eager step.  The one thing that changes a sum's order is the KV-split count, sized by ``max_pages``; the eager side
therefore sets ``max_pages`` of its host-built BatchedKvCacheInt4 to the static cache's (its row width ``cap``).  The eager side
keeps its own, un-reserved sequences in a second pool, so page NUMBERS differ between the sides: tables are compared through each
side's own page list, cache contents slot by slot."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _pool(layers, heads, capacity, block):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(layers, heads, 128, capacity, block, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def _pages(lens, block, extra=0):
    return sum(-(-(n + extra) // block) for n in lens)


# ------------------------------------------------------------------------------------------------ 1. tables
def _assert_tables(skv, static_seqs, eager_seqs):
    """the device tables of ``skv`` against a BatchedKvCacheInt4 built on the host from ``eager_seqs`` (another pool): equal indptr and
    last_page_offset; sequence b's entries are the FIRST pages of its own list, in order, on both sides"""
    from atom_amd.utils import BatchedKvCacheInt4
    ref = BatchedKvCacheInt4(eager_seqs)
    indptr = skv.indptr.tolist()
    assert indptr == ref.indptr.tolist()
    assert skv.last_page_offset.tolist() == ref.last_page_offset.tolist()
    got, want = skv.indicies[:indptr[-1]].tolist(), ref.indicies.tolist()
    for b, (cs, ce) in enumerate(zip(static_seqs, eager_seqs)):
        n = indptr[b + 1] - indptr[b]
        assert got[indptr[b]:indptr[b + 1]] == cs.indicies[:n], b
        assert want[indptr[b]:indptr[b + 1]] == ce.indicies[:n] and n == len(ce.indicies), b


def _run_tables(lens, block, steps):
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    pa = _pool(1, 1, _pages(lens, block, steps) + 2, block)
    pb = _pool(1, 1, _pages(lens, block, steps) + 2, block)
    sa, sb = [KvCacheInt4(pa, n) for n in lens], [KvCacheInt4(pb, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(sa, reserve=steps)
    assert skv.max_pages == max(-(-(n + steps) // block) for n in lens) and skv.page_size == block and skv.seqlens == lens
    _assert_tables(skv, sa, sb)                              # the constructor's step(0): the tables of the current lengths
    for _ in range(steps):
        skv.step()
        for c in sb:
            c.acquire_one()
        _assert_tables(skv, sa, sb)
    skv.step(0)                                              # add = 0 rebuilds the same tables
    _assert_tables(skv, sa, sb)
    skv.sync_host()
    assert skv.seqlens == [n + steps for n in lens] == [c.seqlen for c in sa]
    free = pa.num_free_blocks
    skv.close()
    assert [len(c.indicies) for c in sa] == [len(c.indicies) for c in sb] and pa.num_free_blocks >= free
    assert pa.num_free_blocks == pb.num_free_blocks


@pytest.mark.parametrize("block", [16, 32])
def test_tables_follow_the_host_bookkeeping_across_page_boundaries(block):
    """40 steps: every sequence crosses at least one page boundary, the third starts on one"""
    _run_tables([1, 15, 16, 17, 33, 250], block, 40)


def test_tables_of_1024_sequences():
    """16 groups of 64 sequences: every workgroup sums the page counts in front of its group itself"""
    _run_tables([(i * 7) % 40 + 1 for i in range(1024)], 16, 4)


def test_tables_with_sliced_rows():
    """rows wider than 256 pages: the copy of a group's rows is split over several workgroups (and 70 sequences: two groups)"""
    lens = [(i * 37) % 300 + 1 for i in range(70)]
    lens[3], lens[66] = 5000, 4100
    _run_tables(lens, 16, 3)


def test_step_rejects_bad_arguments():
    from atom_amd import _lib as L
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    pool = _pool(1, 1, 8, 16)
    skv = StaticBatchedKvCacheInt4([KvCacheInt4(pool, 5), KvCacheInt4(pool, 20)], reserve=4)
    t = [x.data_ptr() for x in (skv.page_table, skv.row_pages, skv.lengths, skv.indptr, skv.indicies, skv.last_page_offset, skv.state)]
    call = lambda ptrs, batch=2, cap=skv.max_pages, page=16, add=1: L.lib().atom_kv_step_i4(*ptrs, batch, cap, page, add, None)
    assert call(t, batch=0) == L.ERR_SHAPE and call(t, cap=0) == L.ERR_SHAPE and call(t, page=24) == L.ERR_SHAPE
    assert call(t, page=0) == L.ERR_SHAPE and call(t, add=-1) == L.ERR_INVALID_ARG
    for i in range(len(t)):
        assert call(t[:i] + [None] + t[i + 1:]) == L.ERR_INVALID_ARG
        assert call(t[:i] + [t[i] + 2] + t[i + 1:]) == L.ERR_ALIGN
    torch.cuda.synchronize()
    skv.sync_host()                                          # none of the refused calls launched anything
    assert skv.seqlens == [5, 20]
    skv.close()


# ------------------------------------------------------------------------------------------------ 2. overflow
def test_overflow_sets_the_status_word_and_stays_inside_the_rows():
    """reserve 3, 8 steps: the first sequence (10 tokens, one page) stops at 16 tokens, the others have room in their last page"""
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    lens, block = [10, 16, 30], 16
    pool = _pool(1, 1, 12, block)
    seqs = [KvCacheInt4(pool, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(seqs, reserve=3)
    reserved = [list(c.indicies) for c in seqs]
    assert [len(r) for r in reserved] == [1, 2, 3]
    for i in range(8):
        skv.step()
        indptr, ind = skv.indptr.tolist(), skv.indicies.tolist()
        for b, r in enumerate(reserved):                     # after EVERY step: counts within the reserve, entries from the row's own pages
            assert 0 < indptr[b + 1] - indptr[b] <= len(r) and ind[indptr[b]:indptr[b + 1]] == r[:indptr[b + 1] - indptr[b]]
        assert int(skv.state[0].item()) == (1 if i >= 6 else 0)
    assert skv.last_page_offset.tolist() == [16, 8, 6]
    with pytest.raises(RuntimeError, match="reserved pages"):
        skv.sync_host()
    assert skv.seqlens == [16, 24, 38] == [c.seqlen for c in seqs]      # the over-full sequence kept its last legal length
    skv.sync_host()                                          # the status word was cleared by the read that raised
    skv.close()
    assert [len(c.indicies) for c in seqs] == [1, 2, 3] and pool.num_free_blocks == 12 - 6


# ------------------------------------------------------------------------------------------------ 3. ops take the static cache
def _mirror_pair(lens, heads, block, reserve, seed):
    """two pools holding the same K/V per (sequence, position): (static cache over reserved sequences, its sequences, pool) and
    (un-reserved sequences, pool)"""
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    g = torch.Generator(device="cuda").manual_seed(seed)
    cap = _pages(lens, block, reserve) + 2
    pa, pb = _pool(2, heads, cap, block), _pool(2, heads, cap, block)
    pb.buf.copy_(torch.randint(0, 256, pb.buf.shape, device="cuda", generator=g, dtype=torch.uint8))
    pb.param.copy_((torch.rand(pb.param.shape, device="cuda", generator=g) * 0.2 + 0.01).half())
    sb = [KvCacheInt4(pb, n) for n in lens]
    sa = [KvCacheInt4(pa, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(sa, reserve=reserve)
    for ca, cb in zip(sa, sb):
        for i, j in zip(ca.indicies, cb.indicies):
            pa.buf[i].copy_(pb.buf[j])
            pa.param[i].copy_(pb.param[j])
    return skv, sa, pa, sb, pb, g


def _assert_same_cache(seqs_a, pool_a, seqs_b, pool_b):
    block = pool_a.block_len
    for ca, cb in zip(seqs_a, seqs_b):
        assert ca.seqlen == cb.seqlen
        for k in range(-(-ca.seqlen // block)):
            n = min(block, ca.seqlen - k * block)
            i, j = ca.indicies[k], cb.indicies[k]
            assert torch.equal(pool_a.buf[i, :, :, :, :n], pool_b.buf[j, :, :, :, :n])
            assert torch.equal(pool_a.param[i, :, :, :, :n].view(torch.int16), pool_b.param[j, :, :, :, :n].view(torch.int16))


@pytest.mark.parametrize("lens,heads,qheads", [([37, 5, 16, 300], 4, 4), ([600], 32, 32), ([20, 33, 1000], 2, 8), ([900] * 6, 32, 32)])
def test_attention_ops_take_the_static_cache(lens, heads, qheads):
    from atom_amd import ops
    from atom_amd.utils import BatchedKvCacheInt4
    skv, sa, pa, sb, pb, g = _mirror_pair(lens, heads, 16, 5, seed=len(lens) + heads)
    B = len(lens)
    skv.step()
    for c in sb:
        c.acquire_one()
    ref = BatchedKvCacheInt4(sb)
    ref.max_pages = skv.max_pages
    q = torch.randn((B, qheads, 128), device="cuda", generator=g).half()
    for layer in (0, 1):
        if heads == qheads:                                  # MHA: the step's K/V quantised and appended inside the attention launch
            k32 = torch.randn((B, heads * 128), device="cuda", generator=g)
            v32 = torch.randn((B, heads * 128), device="cuda", generator=g)
            assert torch.equal(ops.batch_decode_i4(q, skv, layer, append_kv=(k32, v32)), ops.batch_decode_i4(q, ref, layer, append_kv=(k32, v32)))
        else:
            k32 = torch.randn((B, heads * 128), device="cuda", generator=g)
            ops.quant_append_kv_i4(skv, k32, k32, layer)
            ops.quant_append_kv_i4(ref, k32, k32, layer)
        assert ops.decode_splits(B, skv, qheads) == ops.decode_splits(B, ref, qheads)
        assert torch.equal(ops.batch_decode_i4(q, skv, layer), ops.batch_decode_i4(q, ref, layer))
    # prefill: the last tokens of every sequence as a chunk
    qlens = [min(n + 1, 7 + 3 * b) for b, n in enumerate(lens)]
    qo = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    qp = torch.randn((sum(qlens), qheads, 128), device="cuda", generator=g).half()
    assert torch.equal(ops.batch_prefill_i4(qp, qo, skv, 1, max_q_len=max(qlens)), ops.batch_prefill_i4(qp, qo, ref, 1, max_q_len=max(qlens)))
    skv.close()
    _assert_same_cache(sa, pa, sb, pb)


# ------------------------------------------------------------------------------------------------ 4. replay equals eager
VOCAB = 1000
PROMPT_LENS = [7, 19, 16, 33, 2]
NEW = 41
SEED = {None: 0, 2: 0}          # model seeds per num_key_value_heads: the EAGER loop alone yields >= 8 distinct tokens per run with them


def _cfg(kv_heads, layers=2):
    c = types.SimpleNamespace(hidden_size=512, num_attention_heads=4, intermediate_size=1408, rms_norm_eps=1e-5, rope_theta=1e4,
                              num_hidden_layers=layers, vocab_size=VOCAB, pad_token_id=None)
    if kv_heads is not None:
        c.num_key_value_heads = kv_heads
    return c


def _model(kv_heads, seed):
    from atom_amd.e2e import LlamaForCausalLM
    torch.manual_seed(seed)                                   # embedding, lm_head and the reorder indices come from the global generator
    model = LlamaForCausalLM(_cfg(kv_heads)).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    return model


def _prompts(batch, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS[:batch]]


def _prefill(model, prompts, pool):
    """eager prefill of fresh sequences: (sequences, first tokens [batch], their logits [batch, vocab])"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    logits, _ = model(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    first = logits[torch.tensor(lens).cumsum(0) - 1]
    return seqs, first.argmax(-1), first


def _eager_decode(model, seqs, ids, steps, cap):
    """the loop a user writes without this feature: acquire_one on every sequence, a new BatchedKvCacheInt4, one forward, argmax"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    toks, logs = [], []
    for _ in range(steps):
        for c in seqs:
            c.acquire_one()
        kv = BatchedKvCacheInt4(seqs)
        kv.max_pages = cap
        logits, _ = model(ids, BatchLenInfo([], len(seqs), DEV), None, kv)
        ids = logits.argmax(-1)
        toks.append(ids)
        logs.append(logits)
    return torch.stack(toks), torch.stack(logs)


def _kv_heads(kv_heads):
    return 4 if kv_heads is None else kv_heads


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_equals_the_eager_loop(kv_heads, batch):
    """MHA and 4-on-2 GQA; one and two prompts (quantisers inside the GEMMs) and five (the generic path); 41 new tokens on pages of 16:
    every sequence fills pages during replay"""
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _model(kv_heads, SEED[kv_heads]), _prompts(batch)
    cap = max(-(-(len(p) + NEW - 1) // 16) for p in prompts)
    capacity = _pages([len(p) for p in prompts], 16, NEW) + 2
    pe = _pool(2, _kv_heads(kv_heads), capacity, 16)
    se, first, first_logits = _prefill(model, prompts, pe)
    toks, logs = _eager_decode(model, se, first, NEW - 1, cap)
    want_tokens = torch.cat([first[None], toks]).t().tolist()
    want_logits = torch.cat([first_logits[None], logs])
    print("distinct tokens per run:", len({t for row in want_tokens for t in row}), [len(set(row)) for row in want_tokens])
    assert len({t for row in want_tokens for t in row}) >= 8, "the tiny model collapsed: pick another seed for the EAGER loop"

    pg = _pool(2, _kv_heads(kv_heads), capacity, 16)
    free = pg.num_free_blocks
    caches = [KvCacheInt4(pg, 0) for _ in prompts]
    got_tokens, got_logits = generate(model, prompts, NEW, pg, caches=caches, return_logits=True)
    assert got_tokens == want_tokens
    assert got_logits.shape == want_logits.shape and torch.equal(got_logits, want_logits)
    assert [c.seqlen for c in caches] == [len(p) + NEW - 1 for p in prompts]
    assert [len(c.indicies) for c in caches] == [len(c.indicies) for c in se]         # trimmed: ordinary sequences again
    _assert_same_cache(caches, pg, se, pe)
    for c in caches:
        c.release()
    # the default form: its own caches, released at the end; tokens cut after the first eos
    eos = want_tokens[0][5]
    cut = generate(model, prompts, NEW, pg, eos_token_id=eos)
    assert cut == [row[:row.index(eos) + 1] if eos in row else row for row in want_tokens]
    assert pg.num_free_blocks == free


# ------------------------------------------------------------------------------------------------ 5. two graphs, one pool
def test_two_decode_graphs_over_one_pool_replay_interleaved():
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    model, prompts, steps = _model(None, SEED[None]), _prompts(5), 14
    groups = [prompts[:2], prompts[2:]]
    capacity = _pages([len(p) for p in prompts], 16, steps) + 2
    pe, pg = _pool(2, 4, capacity, 16), _pool(2, 4, capacity, 16)
    runs = []
    for grp in groups:                                       # captured one after the other, sequences of ONE pool
        sg, first, _ = _prefill(model, grp, pg)
        skv = StaticBatchedKvCacheInt4(sg, reserve=steps)
        dg = DecodeGraph(model, skv, steps, keep_logits=True)
        dg.input_ids.copy_(first)
        dg.step()
        dg.step()
        runs.append((dg, skv, sg))
    order = [0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0]
    for i in order + [1 - i for i in order]:                 # 12 more steps each, interleaved
        runs[i][0].step()
    for grp, (dg, skv, sg) in zip(groups, runs):
        se, first, _ = _prefill(model, grp, pe)
        toks, logs = _eager_decode(model, se, first, steps, skv.max_pages)
        assert dg.steps_done == steps and torch.equal(dg.tokens, toks) and torch.equal(dg.logits, logs)
        skv.close()
        _assert_same_cache(sg, pg, se, pe)
        for c in se:
            c.release()
    with pytest.raises(RuntimeError):
        runs[0][0].step()                                    # all steps taken: refused on the host, nothing is launched


# ------------------------------------------------------------------------------------------------ 6. no hidden synchronisation
def test_replay_loop_does_not_synchronise():
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device="cuda").item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): a synchronising .item() passed under it")
    model, prompts, steps = _model(2, SEED[2]), _prompts(2), 20
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    dg = DecodeGraph(model, skv, steps)
    dg.input_ids.copy_(first)
    dg.step()
    dg.step()                                                # eager warm-up and the capture are allowed to synchronise
    torch.cuda.set_sync_debug_mode("error")
    try:
        while dg.steps_done < steps:
            dg.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    skv.close()
    assert skv.seqlens == [len(p) + steps for p in prompts]
