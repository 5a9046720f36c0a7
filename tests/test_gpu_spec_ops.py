"""GPU tests of the speculative-decoding ops: ops.spec_draft_ngram, ops.spec_accept, ops.kv_step_rows_i4 /
StaticBatchedKvCacheInt4.step_rows and ops.sample(rows_per_seq=).  Every comparison is EXACT against tests/spec_ref.py (the sampler's
against its own one-element form)."""
import numpy as np
import pytest
import torch

from tests import spec_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
LENGTHS = [1, 2, 63, 64, 65, 257, 1025, 5000]               # across a lane stride (1 .. 65), a wave, a workgroup pass (512) and a trip (2048)


def _draft(hist, hist_len, K, nmax, nmin):
    """the op into columns 1 .. K of an input_ids-shaped buffer: (drafts [batch, K], the buffer)"""
    from atom_amd import ops
    batch = hist.shape[0]
    ids = torch.full((batch, K + 1), -7, dtype=torch.int64, device=DEV)
    ops.spec_draft_ngram(torch.from_numpy(hist).to(DEV), torch.tensor(hist_len, dtype=torch.int32, device=DEV), ids[:, 1:],
                         ngram_max=nmax, ngram_min=nmin)
    got = ids.cpu().numpy()
    assert (got[:, 0] == -7).all()                           # column 0 belongs to the last emitted token
    return got[:, 1:]


# ------------------------------------------------------------------------------------------------ 1. draft
@pytest.mark.parametrize("nmin,nmax", [(1, 1), (1, 3), (2, 8)])
@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("batch", [1, 3, 65])
def test_draft_equals_the_rule(batch, K, nmin, nmax):
    rng = np.random.default_rng(batch * 100 + K * 10 + nmax)
    lens = [LENGTHS[(b + K + nmax) % len(LENGTHS)] for b in range(batch)]
    if batch == 1:
        lens = [5000]
    cap = max(lens) + 3
    hist = rng.integers(0, 3, size=(batch, cap)).astype(np.int32) + 40     # three symbols: matches abound; behind len: more of the same
    want = spec_ref.draft(hist, lens, K, nmax, nmin)
    assert np.array_equal(_draft(hist, lens, K, nmax, nmin), want)


@pytest.mark.parametrize("length", LENGTHS)
def test_draft_at_every_length(length):
    """batch 3 of one length each: the lengths 1 and 2 too, where nothing (1) or only a run (2) can match"""
    rng = np.random.default_rng(length)
    hist = rng.integers(0, 3, size=(3, length + 1)).astype(np.int32) + 1
    for nmin, nmax in ((1, 1), (1, 3), (2, 8)):
        assert np.array_equal(_draft(hist, [length] * 3, 4, nmax, nmin), spec_ref.draft(hist, [length] * 3, 4, nmax, nmin))


def test_draft_planted_matches():
    L, K = 5000, 4
    base = (np.arange(L, dtype=np.int32) % 997) * 3 + 1000                     # no token of `base` equals a planted one
    rows, lens = [], []
    # the only match at s = 0: the last three tokens occur at the very start
    h = base.copy(); h[:3] = [7, 8, 9]; h[3:7] = [11, 12, 13, 14]; h[L - 3:] = [7, 8, 9]
    rows.append(h); lens.append(L)
    # the only match ending at len - 2, the last end the kernel visits (a run of three with ngram_min .. max covering 2): s + n =
    # len - 1, so the continuation is the last token itself and the rest is padding -- nothing behind the history is read
    h = base.copy(); h[L - 3:] = [6, 6, 6]
    rows.append(h); lens.append(L)
    # two equal-n matches 4,000 tokens apart: the later one wins
    h = base.copy(); h[100:103] = [7, 8, 9]; h[103] = 21; h[4100:4103] = [7, 8, 9]; h[4103] = 22; h[L - 3:] = [7, 8, 9]
    rows.append(h); lens.append(L)
    hist = np.stack(rows)
    want = spec_ref.draft(hist, lens, K, 3, 1)
    assert want[0].tolist() == [11, 12, 13, 14] and want[1].tolist() == [6] * K and want[2].tolist()[0] == 22
    assert np.array_equal(_draft(hist, lens, K, 3, 1), want)                  # hist_cap == len for every row
    # lengths outside the buffer: drafts of token 0, nothing is read
    assert np.array_equal(_draft(hist, [0, -5, L + 1], K, 3, 1), np.zeros((3, K), np.int64))


def test_draft_refuses_bad_operands():
    from atom_amd import _lib as L, ops
    hist = torch.zeros((2, 16), dtype=torch.int32, device=DEV)
    hl = torch.ones(2, dtype=torch.int32, device=DEV)
    out = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    with pytest.raises(L.AtomHipError):
        ops.spec_draft_ngram(hist.cpu(), hl, out)
    with pytest.raises(TypeError):
        ops.spec_draft_ngram(hist.long(), hl, out)
    with pytest.raises(TypeError):
        ops.spec_draft_ngram(hist, hl[:1], out)
    with pytest.raises(TypeError):
        ops.spec_draft_ngram(hist, hl, out.int())
    with pytest.raises(ValueError):
        ops.spec_draft_ngram(hist, hl, torch.zeros((2, 9), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.spec_draft_ngram(hist, hl, out, ngram_max=9)
    with pytest.raises(ValueError):
        ops.spec_draft_ngram(hist, hl, out, ngram_max=2, ngram_min=3)


# ------------------------------------------------------------------------------------------------ 2. accept
SENT = -99


def _accept_case(K, batch, seed):
    """rows that plant every a in 0 .. K and every budget clamp of {0, 1, a, a + 1, a + 2}, finished rows among them"""
    rng = np.random.default_rng(seed)
    Q, max_new, cap = K + 1, 40, 64
    targets = rng.integers(0, 50, size=(batch, Q)).astype(np.int64)
    ids = np.empty((batch, Q), np.int64)
    ids[:, 0] = rng.integers(0, 50, size=batch)
    n_out = rng.integers(1, 20, size=batch).astype(np.int32)
    budget = np.empty(batch, np.int32)
    for b in range(batch):
        a = b % (K + 1)
        ids[b, 1:] = targets[b, :K]
        if a < K:
            ids[b, 1 + a] = targets[b, a] + 1                # the first disagreement; drafts behind it agree again (and do not count)
        room = [a + 2, 0, 1, a, a + 1][(b // (K + 1)) % 5]
        budget[b] = n_out[b] + room
    hist_len = (n_out + rng.integers(1, 10, size=batch)).astype(np.int32)
    return dict(targets=targets, input_ids=ids, n_out=n_out, budget=budget, tokens=np.full((batch, max_new), SENT, np.int64),
                hist=np.full((batch, cap), SENT, np.int32), hist_len=hist_len, adds=np.full(batch, SENT, np.int32),
                draw=np.full(batch, SENT, np.int64), accepted=rng.integers(0, 9, size=batch).astype(np.int32),
                steps=rng.integers(0, 9, size=batch).astype(np.int32))


def _run_accept(c):
    from atom_amd import ops
    order = ("targets", "input_ids", "n_out", "budget", "tokens", "hist", "hist_len", "adds", "draw", "accepted", "steps")
    dev = {k: torch.from_numpy(c[k].copy()).to(DEV) for k in order}
    dev["done"] = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    ops.spec_accept(*(dev[k] for k in order), dev["done"])
    want = spec_ref.accept(*(c[k] for k in order))
    for k, w in want.items():                                # every output buffer, whole: the sentinels outside the written ranges too
        assert np.array_equal(dev[k].cpu().numpy(), w), k
    assert np.array_equal(dev["targets"].cpu().numpy(), c["targets"]) and np.array_equal(dev["budget"].cpu().numpy(), c["budget"])
    return want


@pytest.mark.parametrize("batch", [1, 70])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_accept_equals_the_rule(K, batch):
    c = _accept_case(K, batch, seed=K * 100 + batch)
    want = _run_accept(c)
    if batch == 70:
        emitted = want["adds"]
        assert set(range(K + 2)) <= set(emitted.tolist())    # every e of 0 .. K + 1 occurred
        assert (want["adds"] == 0).any() and want["done"][0] == 0


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_accept_plants_every_count(K):
    """one row per a = 0 .. K with room to spare: adds = a + 1"""
    c = _accept_case(K, K + 1, seed=K)
    c["budget"][:] = c["n_out"] + 20
    want = _run_accept(c)
    assert want["adds"].tolist() == [a + 1 for a in range(K + 1)] and want["done"][0] == 0


def test_accept_done_word_in_both_states():
    K, batch = 4, 70
    c = _accept_case(K, batch, seed=3)
    c["budget"][:] = c["n_out"]                              # every row already finished: nothing changes, done = 1
    want = _run_accept(c)
    assert want["done"][0] == 1 and (want["adds"] == 0).all() and (want["tokens"] == SENT).all() and (want["hist"] == SENT).all()
    c["budget"][:] = c["n_out"] + 1                          # every row finishes in this launch
    assert _run_accept(c)["done"][0] == 1
    c["budget"][-1] += 9                                     # all but the last row done
    assert _run_accept(c)["done"][0] == 0
    c["budget"][:] = c["n_out"] + 1
    c["budget"][0] += 9                                      # ... and all but the first
    assert _run_accept(c)["done"][0] == 0


def test_accept_stays_inside_its_buffers():
    """positions at the end of ``tokens`` and ``hist``: what does not fit is skipped, the counters still move"""
    c = _accept_case(4, 5, seed=11)
    c["input_ids"][:, 1:] = c["targets"][:, :4]              # all accepted: e = 5
    c["budget"][:] = 100
    c["n_out"][:] = [38, 39, 40, 35, 1]
    c["hist_len"][:] = [62, 64, 60, 63, 70]
    want = _run_accept(c)
    assert want["adds"].tolist() == [5] * 5 and want["n_out"].tolist() == [43, 44, 45, 40, 6]


def test_accept_refuses_bad_operands():
    from atom_amd import _lib as L, ops
    order = ("targets", "input_ids", "n_out", "budget", "tokens", "hist", "hist_len", "adds", "draw", "accepted", "steps")
    c = _accept_case(2, 3, seed=1)
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in order}
    dev["done"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = lambda **kw: [kw.get(k, dev[k]) for k in order + ("done",)]
    with pytest.raises(L.AtomHipError):
        ops.spec_accept(*args(n_out=dev["n_out"].cpu()))
    with pytest.raises(TypeError):
        ops.spec_accept(*args(n_out=dev["n_out"].long()))
    with pytest.raises(TypeError):
        ops.spec_accept(*args(input_ids=dev["input_ids"][:, :2]))
    with pytest.raises(TypeError):
        ops.spec_accept(*args(done=torch.zeros(2, dtype=torch.int32, device=DEV)))
    with pytest.raises(ValueError):
        ops.spec_accept(*args(targets=torch.zeros((3, 10), dtype=torch.int64, device=DEV)))
    torch.cuda.synchronize()
    assert np.array_equal(dev["tokens"].cpu().numpy(), c["tokens"])          # none of the refused calls launched anything


# ------------------------------------------------------------------------------------------------ 3. step_rows
def _pool(capacity, block):
    from atom_amd.utils import KvPoolInt4
    return KvPoolInt4(1, 1, 128, capacity, block, DEV)


_HOST = {}


def _HOST_POOL(like, block):
    """one host-side pool per static pool, as large"""
    if id(like) not in _HOST:
        _HOST.clear()
        _HOST[id(like)] = _pool(like.buf.size(0), block)
    return _HOST[id(like)]


def _assert_tables(skv, static_seqs, host_seqs):
    """the device tables against a host-built BatchedKvCacheInt4 over ``host_seqs`` (a pool of their own)"""
    from atom_amd.utils import BatchedKvCacheInt4
    ref = BatchedKvCacheInt4(host_seqs)
    indptr = skv.indptr.tolist()
    assert indptr == ref.indptr.tolist() and skv.last_page_offset.tolist() == ref.last_page_offset.tolist()
    got = skv.indicies[:indptr[-1]].tolist()
    for b, c in enumerate(static_seqs):
        assert got[indptr[b]:indptr[b + 1]] == c.indicies[:indptr[b + 1] - indptr[b]], b


@pytest.mark.parametrize("batch", [1, 64, 65, 130])
@pytest.mark.parametrize("block", [16, 32])
def test_step_rows_follows_the_host_bookkeeping(block, batch):
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    rounds, look = 40, 9
    rng = np.random.default_rng(block + batch)
    lens = [[1, 15, 16, 17, 250][b % 5] for b in range(batch)]
    adds = rng.integers(0, 10, size=(rounds, batch)).astype(np.int32)
    reserve = int(adds.sum(0).max()) + look
    pool = _pool(sum(-(-(n + reserve) // block) for n in lens) + 1, block)
    seqs = [KvCacheInt4(pool, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(seqs, reserve=reserve)
    ref = spec_ref.StepRows(lens, skv.row_pages.tolist(), block)
    host = [KvCacheInt4(_HOST_POOL(pool, block), n + look) for n in lens]     # a second pool: sequences of committed + lookahead tokens
    for r in range(rounds):
        skv.step_rows(torch.from_numpy(adds[r]).to(DEV), lookahead=look)
        ref.step(adds[r], look)
        for c, a in zip(host, adds[r]):
            c.acquire(int(a))
        assert skv.indptr.tolist() == ref.indptr and skv.last_page_offset.tolist() == ref.last_page_offset
        _assert_tables(skv, seqs, host)
    skv.sync_host()                                          # the committed lengths, without the look-ahead; no status bit
    assert skv.seqlens == ref.lens == [n + int(a) for n, a in zip(lens, adds.sum(0))] and ref.status == 0
    skv.close()


def test_step_rows_without_lookahead_is_the_scalar_step():
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    lens, block = [1, 15, 16, 17, 33, 250] * 12, 16
    pa, pb = _pool(sum(-(-(n + 12) // block) for n in lens) + 1, block), _pool(sum(-(-(n + 12) // block) for n in lens) + 1, block)
    sa, sb = [KvCacheInt4(pa, n) for n in lens], [KvCacheInt4(pb, n) for n in lens]
    ka, kb = StaticBatchedKvCacheInt4(sa, reserve=12), StaticBatchedKvCacheInt4(sb, reserve=12)
    for add in (1, 0, 3, 1, 2):
        ka.step(add)
        kb.step_rows(torch.full((len(lens),), add, dtype=torch.int32, device=DEV), lookahead=0)
        assert torch.equal(ka.indptr, kb.indptr) and torch.equal(ka.last_page_offset, kb.last_page_offset)
        n = int(ka.indptr[-1])
        for b, (ca, cb) in enumerate(zip(sa, sb)):           # the same positions of each side's own page list
            lo, hi = int(ka.indptr[b]), int(ka.indptr[b + 1])
            assert ka.indicies[lo:hi].tolist() == ca.indicies[:hi - lo] and kb.indicies[lo:hi].tolist() == cb.indicies[:hi - lo]
        assert n == int(kb.indptr[-1])
    ka.close(), kb.close()
    assert ka.seqlens == kb.seqlens == [n + 7 for n in lens]


def test_step_rows_flags_a_negative_count_and_an_overflow():
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    lens, block = [10, 16, 30], 16
    pool = _pool(12, block)
    seqs = [KvCacheInt4(pool, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(seqs, reserve=3)          # pages 1, 2, 3: room for 16, 32, 48 tokens
    t = lambda *x: torch.tensor(x, dtype=torch.int32, device=DEV)
    skv.step_rows(t(2, -4, 1), lookahead=2)                  # the negative count is 0 and flagged
    assert int(skv.state[0]) == 2 and skv.last_page_offset.tolist() == [14, 2, 1] and skv.indptr.tolist() == [0, 1, 3, 6]
    with pytest.raises(RuntimeError):
        skv.sync_host()
    assert skv.seqlens == [12, 16, 31]
    before = (skv.indptr.clone(), skv.indicies.clone(), skv.last_page_offset.clone())
    skv.step_rows(t(3, 1, 1), lookahead=2)                   # 12 + 3 + 2 > 16: the whole request of row 0 is refused
    assert int(skv.state[0]) == 1 and skv.last_page_offset.tolist() == [12, 3, 2] and skv.indptr.tolist() == [0, 1, 3, 6]
    assert skv.indicies[:1].tolist() == before[1][:1].tolist()
    with pytest.raises(RuntimeError):
        skv.sync_host()
    assert skv.seqlens == [12, 17, 32]
    skv.step_rows(t(2, 0, 0), lookahead=2)                   # 12 + 2 + 2 = 16 fits exactly
    skv.close()
    assert skv.seqlens == [14, 17, 32]


def test_scalar_and_row_steps_interleave_on_one_cache():
    """both entries flip the one parity word: after any mix the current lengths are the ones the next launch reads"""
    from atom_amd.utils import KvCacheInt4, StaticBatchedKvCacheInt4
    lens, block = [5, 20, 31], 16
    pool = _pool(16, block)
    seqs = [KvCacheInt4(pool, n) for n in lens]
    skv = StaticBatchedKvCacheInt4(seqs, reserve=20)
    ref = spec_ref.StepRows(lens, skv.row_pages.tolist(), block)
    t = lambda *x: torch.tensor(x, dtype=torch.int32, device=DEV)
    for kind, arg in (("s", 1), ("r", (2, 0, 3)), ("r", (1, 1, 1)), ("s", 2), ("s", 0), ("r", (0, 4, 0)), ("s", 1)):
        if kind == "s":
            skv.step(arg)
            ref.step([arg] * 3, 0)
        else:
            skv.step_rows(t(*arg), lookahead=4)
            ref.step(arg, 4)
        assert skv.indptr.tolist() == ref.indptr and skv.last_page_offset.tolist() == ref.last_page_offset
    skv.close()
    assert skv.seqlens == ref.lens == [12, 29, 39]


# ------------------------------------------------------------------------------------------------ 4. sampler rows
@pytest.mark.parametrize("q", [1, 3, 9])
def test_sample_rows_equals_the_one_element_form(q):
    from atom_amd import ops
    rows, vocab = 64 * q, 1000                               # 64 sequences of q rows
    g = torch.Generator(device="cuda").manual_seed(q)
    logits = (torch.randn((rows, vocab), device=DEV, generator=g) * 3).half()
    temp = torch.full((rows,), 0.9, device=DEV)
    temp[::7] = 0.0                                          # some greedy rows
    top_k = torch.full((rows,), 50, dtype=torch.int32, device=DEV)
    top_p = torch.full((rows,), 0.95, device=DEV)
    seeds = torch.arange(rows, dtype=torch.int64, device=DEV) // q + 5          # one seed per sequence
    base = torch.arange(rows // q, dtype=torch.int64, device=DEV) * 11 + 3
    got = ops.sample(logits, temp, top_k, top_p, seeds, step=base, rows_per_seq=q, step_offset=2)
    want = torch.empty_like(got)
    for r in range(rows):
        one = torch.tensor([int(base[r // q]) + r % q], dtype=torch.int64, device=DEV)
        want[r] = ops.sample(logits[r:r + 1], temp[r:r + 1], top_k[r:r + 1], top_p[r:r + 1], seeds[r:r + 1], step=one, step_offset=2)[0]
    assert torch.equal(got, want)
    assert len(set(got.tolist())) > 8                        # the draws differ: the rows are not all their argmax
    # step of one element: today's entry, unchanged by the keyword's existence -- every row takes draw number 4
    one = torch.tensor([4], dtype=torch.int64, device=DEV)
    same = ops.sample(logits, temp, top_k, top_p, seeds, step=one)
    fours = torch.full((rows,), 4, dtype=torch.int64, device=DEV)
    assert torch.equal(same, ops.sample(logits, temp, top_k, top_p, seeds, step=fours, rows_per_seq=1))
    with pytest.raises(TypeError):
        ops.sample(logits, temp, top_k, top_p, seeds, step=one, rows_per_seq=q)          # step must be [64] with the keyword
    with pytest.raises(ValueError):
        ops.sample(logits, temp, top_k, top_p, seeds, step=base, rows_per_seq=rows + 1)
