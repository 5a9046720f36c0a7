"""GPU tests of the rolling INT4 paged KV cache: the ring step of the page tables (atom_kv_step_ring_i4) against
tests/kv_ring_ref.ring_step bit for bit; the attention ops over a page list that starts at kv_start (atom_batch_decode_gqa_i4_ring,
atom_batch_prefill_gqa_i4_ring) against the FP64 windowed reference of the UN-RELEASED cache and, wherever the two plans agree, bit for
bit against the _win ops on that cache; ``utils.RollingKvCacheInt4`` and ``generate(rolling_kv=True)`` end to end.

The rolling caches come from kv_ring_ref.ring_cache: every byte no correct kernel may read is 0xFF (a NaN scale).
tests/test_kv_ring_cpu.py proves on the CPU, for exactly these cases, that the reference reads none of them and that each mutant of
the reader moves it by >= 10 x the bound applied here (attn_window_ref.REL: 4e-3 max|ref| + 1e-3 per (query row, head))."""
import types

import numpy as np
import pytest
import torch

from tests import attn_planted as A
from tests import attn_window_ref as W
from tests import kv_ring_ref as K
from tests.helpers import t2n

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FULL_PAGES = 1 << 15            # max_pages of the un-released side: large, so that the window bound governs its plan (as it does the ring's)


# ------------------------------------------------------------------------------------------------ the step kernel
class _Tables:
    """the device buffers of one atom_kv_step_ring_i4 problem and the host's copy of what the reference expects"""

    def __init__(self, table, rows, lens, P, window):
        self.B, self.cap = table.shape
        self.P, self.window = P, window
        self.table_h, self.rows_h, self.lens_h, self.status_h = table, list(rows), np.asarray(lens), 0
        i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)
        self.table, self.rows = i32(table), i32(rows)
        self.dev = i32(list(lens) + [0] * self.B + [0, 0, 0, 0])
        self.lens, self.state = self.dev[:2 * self.B], self.dev[2 * self.B:]
        self.out = torch.full((self.B + 1 + self.B * self.cap + 2 * self.B,), -7, dtype=torch.int32, device=DEV)
        self.indptr, self.indices = self.out[:self.B + 1], self.out[self.B + 1:self.B + 1 + self.B * self.cap]
        self.lpo, self.start = self.out[-2 * self.B:-self.B], self.out[-self.B:]

    def step(self, add, window=None, start=0):
        from atom_amd._lib import current_stream, lib
        ptrs = [t.data_ptr() for t in (self.table, self.rows, self.lens, self.indptr, self.indices, self.lpo, self.state)]
        return lib().atom_kv_step_ring_i4(*ptrs, self.B, self.cap, self.P, add, self.window if window is None else window,
                                          self.start.data_ptr() if start == 0 else start, current_stream(DEV))

    def step_and_compare(self, add):
        assert self.step(add) == 0
        lens2, indptr, indices, lpo, start, status = K.ring_step(self.table_h, self.rows_h, self.lens_h, add, self.window, self.P)
        self.status_h |= status
        dev, out = self.dev.tolist(), self.out.cpu().numpy()
        B, parity = self.B, dev[2 * self.B + 1] & 1
        assert dev[2 * B] == self.status_h and dev[2 * B + 2] == 0
        assert dev[parity * B:(parity + 1) * B] == lens2.tolist()
        assert np.array_equal(out[:B + 1], indptr) and np.array_equal(out[B + 1:B + 1 + indptr[-1]], indices)
        assert np.array_equal(out[-2 * B:-B], lpo) and np.array_equal(out[-B:], start)
        kept = lens2 == self.lens_h
        self.lens_h = lens2
        return kept, status


def _problem(batch, P, window, extra, max_add, seed):
    R = K.ring_size(window, P, max_add)
    cap = R + extra
    rng = np.random.default_rng(seed)
    table = rng.permutation(batch * cap + 5)[:batch * cap].reshape(batch, cap).astype(np.int32)
    rows = [R + extra] * batch
    # one row with a ring one page short of what its window needs: W - 1 + max_add consecutive keys touch ceil((W - 2 + max_add) / P) + 1
    # pages at the worst alignment (R itself where W - 2 + max_add is no multiple of P; W = 1: a row with no slot at all)
    short = 1 if batch >= 3 else None
    if short is not None:
        rows[short] = -(-(window - 2 + max_add) // P)
    starts = [0, window - 1, 2 * cap * P + P // 2 + 3]        # empty, the last length without a released key, mid-wrap
    lens = [starts[b % 3] for b in range(batch)]
    if short is not None:
        lens[short] = 0
    return _Tables(table, rows, lens, P, window), R, short


# (batch, page size, window, slots beyond R): every batch size (1, 3; 65 and 130 cross the 64-sequence group), page size and window of
# the grid at least twice, rings of exactly R and of R + 2
STEP_CASES = [(1, 16, 1, 0), (3, 16, 16, 2), (65, 16, 17, 0), (130, 16, 1, 2), (3, 48, 63, 0), (1, 48, 100, 2), (65, 48, 16, 2),
              (130, 48, 17, 0), (3, 16, 100, 0), (1, 16, 63, 2), (130, 16, 63, 0), (65, 48, 100, 0)]


@pytest.mark.parametrize("batch,P,window,extra", STEP_CASES)
def test_ring_step_equals_the_reference_bit_for_bit(batch, P, window, extra):
    """3 R P steps of one token from lengths 0, W - 1 and mid-wrap, then a rebuild (add = 0): lengths, kv_indptr, kv_indices,
    last_page_offset, kv_start and the status word after every launch.  The row whose ring is one page short stops with the overflow
    bit and keeps its length; the rows around it stay exact."""
    t, R, short = _problem(batch, P, window, extra, 1, seed=batch + window)
    refused = False
    for _ in range(3 * R * P):
        kept, status = t.step_and_compare(1)
        if short is not None and kept[short]:
            refused = True
            assert status & K.OVERFLOW
        assert not np.delete(kept, [] if short is None else [short]).any()
    t.step_and_compare(0)
    assert refused == (short is not None)
    assert t.status_h == (K.OVERFLOW if short is not None else 0)


@pytest.mark.parametrize("batch,P,window,extra", [(3, 16, 17, 0), (65, 48, 100, 2), (130, 16, 63, 0), (1, 48, 16, 2)])
def test_ring_step_of_several_tokens(batch, P, window, extra):
    """rings sized for max_add = 5: steps of 5, 1 and 0 tokens mixed, through three wraps"""
    t, R, short = _problem(batch, P, window, extra, 5, seed=7 * batch + window)
    n = 0
    while n < 3 * R * P:
        for add in (5, 5, 1, 0, 5, 1):
            t.step_and_compare(add)
            n += add
    assert t.status_h in ((0, K.OVERFLOW) if short is not None else (0,))


@pytest.mark.parametrize("P,window", [(16, 16), (48, 100)])
def test_ring_step_clamps_corrupted_lengths(P, window):
    """stored lengths below 0, at and next to INT_MAX, a length no ring of that size can describe, a row without a slot: the bits of the
    reference (BAD_LENGTH, OVERFLOW), its tables, and never an index from outside a row"""
    R = K.ring_size(window, P)
    table = np.random.default_rng(3).permutation(70 * (R + 2))[:7 * (R + 2)].reshape(7, R + 2).astype(np.int32)
    rows = [R, 1, R + 2, 0, R, R, R]
    lens = [5, 40 * P, 9, 0, -3, K.INT_MAX, K.INT_MAX - 1]
    t = _Tables(table, rows, lens, P, window)
    for add in (1, 1, 0, 1):
        t.step_and_compare(add)
        out = t.out.cpu().numpy()
        indptr = out[:8]
        for b in range(7):
            assert set(out[8 + indptr[b]:8 + indptr[b + 1]]) <= set(table[b, :rows[b]])
    assert t.status_h == K.OVERFLOW | K.BAD_LENGTH


def test_ring_step_rejects_bad_arguments():
    from atom_amd import _lib
    t, _, _ = _problem(3, 16, 16, 0, 1, seed=1)
    assert t.step(1, window=0) == t.step(1, window=-5) == t.step(-1) == t.step(1, start=None) == _lib.ERR_INVALID_ARG
    assert t.step(1, start=t.start.data_ptr() + 2) == _lib.ERR_ALIGN
    torch.cuda.synchronize()
    assert t.dev.tolist()[-4:] == [0, 0, 0, 0]                # nothing was launched


# ------------------------------------------------------------------------------------------------ attention over a ring
def _dev_kv(c, max_pages, **more):
    return types.SimpleNamespace(data=torch.from_numpy(c["data"]).to(DEV), param=torch.from_numpy(c["param"]).to(DEV),
                                 indptr=torch.from_numpy(c["indptr"]).to(DEV), indicies=torch.from_numpy(c["indices"]).to(DEV),
                                 last_page_offset=torch.from_numpy(c["lpo"]).to(DEV), max_pages=max_pages, **more)


def _ring_kv(rc):
    return _dev_kv(rc, rc["R"], kv_start=torch.from_numpy(rc["kv_start"]).to(DEV), window=rc["window"])


def _plans(case, prefill, win):
    """(plan of the ring call, plan of the _win call on the un-released cache): the splits (decode) or the workspace bytes (prefill)"""
    from atom_amd._lib import lib
    _, P, nkv, G, _ = case
    lens, qo, _, max_q, _, max_add = K.case_shape(case, prefill)
    R, B, L = K.ring_size(win, P, max_add), len(lens), lib()
    if prefill:
        args = (int(qo[-1]), B, nkv * G, nkv, P, max_q)
        return (L.atom_batch_prefill_gqa_i4_ring_workspace_bytes(*args, R, win), L.atom_batch_prefill_gqa_i4_win_workspace_bytes(*args, FULL_PAGES, win))
    args = (B, nkv * G, nkv, P)
    return L.atom_batch_decode_gqa_i4_ring_splits(*args, R, win), L.atom_batch_decode_gqa_i4_win_splits(*args, FULL_PAGES, win)


ATTN = [(c, False) for c in K.DECODE_CASES] + [(c, True) for c in K.PREFILL_CASES]


def _attn_id(cp):
    return ("prefill-" if cp[1] else "decode-") + K.case_id(cp[0])


def test_at_least_half_of_the_cases_are_compared_bit_for_bit():
    """a condition, not a measurement: the bit comparison below runs wherever the two plans agree, and that must be most of the grid"""
    pairs = [(_plans(case, prefill, win)) for case, prefill in ATTN for win in case[4]]
    same = sum(a == b for a, b in pairs)
    print(f"{same} of {len(pairs)} (case, window) pairs plan alike on the ring and on the un-released cache")
    assert 2 * same >= len(pairs)
    assert any(a == b and a > 1 for a, b in pairs)           # ... and some of them with a split KV range


def _run(kv, q, qo_d, max_q, win, **rope):
    from atom_amd import ops
    if qo_d is None:
        return ops.batch_decode_i4(q, kv, A.LAYER, window=win, **rope)
    return ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, window=win, **rope)


@pytest.mark.parametrize("cp", ATTN, ids=_attn_id)
def test_attention_over_the_ring(cp):
    """(a) within the windowed op's bound of the FP64 reference on the un-released cache; (b) bit-identical to the _win op on that
    cache wherever the plans agree.  The last window of every case also runs with a frequency table (the kTable instantiation)."""
    from atom_amd import ops
    case, prefill = cp
    _, P, nkv, G, windows = case
    lens, qo_ref, qo, max_q, adds, max_add = K.case_shape(case, prefill)
    qo_d = None if qo is None else torch.from_numpy(qo).to(DEV)
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 5)
    q, full, memo = torch.from_numpy(qn).to(DEV), _dev_kv(c, FULL_PAGES), {}
    table = ops.rope_table(1e4 ** (-np.arange(64) / 64.0), DEV)
    for win in windows:
        rc = K.ring_cache(c, win, K.ring_size(win, P, max_add), adds)
        ring = _ring_kv(rc)
        ref = W.ref_prefill(qn, c, qo_ref, win, G=G, memo=memo)
        ring_plan, full_plan = _plans(case, prefill, win)
        for rope in ({}, dict(rope_table=table)) if win == windows[-1] else ({},):
            got = _run(ring, q, qo_d, max_q, win, **rope)
            r = A.error_ratio(t2n(got), ref, K.REL)
            row, head = np.unravel_index(np.argmax(r), r.shape)
            print(f"{_attn_id(cp)} W={win} table={bool(rope)} plan {ring_plan}/{full_plan}: worst error / bound {r.max():.3f} (row {row}, head {head})")
            assert r.max() <= 1.0, (win, bool(rope), int(row), int(head), r.max())      # (a NaN fails this too)
            if ring_plan == full_plan:
                assert torch.equal(got, _run(full, q, qo_d, max_q, win, **rope)), (win, bool(rope))


def test_unmerged_partial_states_of_the_ring_merge_inside_o_proj():
    """merge=False on a rolling cache -> dense_layer_gemm_i4_merge_q gives the bits of merge=True + reorder + o_proj"""
    from atom_amd import ops
    from atom_amd.e2e.llama import LinearInt4
    G, nkv, seqlens, win, P = 2, 2, [2500], 700, 16
    c = A.build_needle(seqlens, nkv, P, seed=11)
    ring = _ring_kv(K.ring_cache(c, win, K.ring_size(win, P)))
    nq, batch = G * nkv, 1
    q = torch.from_numpy(A.needle_queries(batch, nq, 11)).to(DEV)
    o = ops.batch_decode_i4(q, ring, A.LAYER, window=win)
    assert A.error_ratio(t2n(o), W.ref_decode(t2n(q), c, win, G=G), K.REL).max() <= 1.0
    splits = ops.decode_splits(batch, ring, nq, window=win)
    assert splits >= 2
    part = ops.batch_decode_i4(q, ring, A.LAYER, merge=False, window=win)
    assert part.shape == (batch, nq, splits, 130)
    hs = nq * 128
    assert ops.merge_q_gemm_fits(batch, hs, 1, hs, splits)
    proj = LinearInt4(hs, hs, "fp16").cuda()
    gw = torch.Generator().manual_seed(2)
    proj.load_fp16_weight((torch.randn(hs, hs, generator=gw) * 0.05).half().cuda())
    ridx = torch.randperm(hs, generator=gw).to(torch.int16).cuda()
    (fused,) = ops.dense_layer_gemm_i4_merge_q(part, splits, proj.single(), reorder_index=ridx)
    (sep,), _ = ops.dense_layer_gemm_i4_multi_q("reorder", o.view(batch, hs), proj.single(), reorder_index=ridx)
    assert torch.equal(fused, sep)


def test_entries_report_a_bad_kv_start_behind_every_older_fault():
    from atom_amd._lib import current_stream, lib
    c = A.build_needle([40, 3], 2, 16, seed=1)
    kv = _ring_kv(K.ring_cache(c, 8, K.ring_size(8, 16)))
    q = torch.from_numpy(A.needle_queries(2, 4, 1)).to(DEV)
    o = torch.empty_like(q)
    ptrs = [t.data_ptr() for t in (kv.data, kv.param, kv.indptr, kv.indicies, kv.last_page_offset)]
    call = lambda window, start: lib().atom_batch_decode_gqa_i4_ring(o.data_ptr(), q.data_ptr(), *ptrs, 2, A.LAYERS, A.LAYER, 4, 2, 16, 128, 1e4,
                                                                      1.0, None, 1.0, window, start, kv.max_pages, None, 0, current_stream(DEV))
    ok, null, misaligned, bad_window = call(8, kv.kv_start.data_ptr()), call(8, None), call(8, kv.kv_start.data_ptr() + 2), call(0, None)
    from atom_amd import _lib
    assert ok == 0 and null == _lib.ERR_INVALID_ARG and misaligned == _lib.ERR_ALIGN
    assert bad_window == null                                 # window < 1 is reported first, and is INVALID_ARG as a null kv_start is
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the Python layers
def _cfg(heads, kv_heads, window, layers=2, vocab=1000):
    c = types.SimpleNamespace(hidden_size=128 * heads, num_attention_heads=heads, num_key_value_heads=kv_heads, intermediate_size=512,
                              rms_norm_eps=1e-5, rope_theta=1e4, num_hidden_layers=layers, vocab_size=vocab, pad_token_id=None)
    if window is not None:
        c.sliding_window = window
    return c


_MODELS = {}


def _model(heads, kv_heads, window=40, **extra):
    """a tiny windowed Llama, weights as the generate tests load them (tests/test_gpu_generate._model)"""
    key = (heads, kv_heads, window, tuple(sorted(extra.items())))
    if key not in _MODELS:
        from atom_amd.e2e import LlamaForCausalLM
        cfg = _cfg(heads, kv_heads, window)
        for k, v in extra.items():
            setattr(cfg, k, v)
        torch.manual_seed(0)
        model = LlamaForCausalLM(cfg).cuda()
        g = torch.Generator().manual_seed(100)
        for mod in model.modules():
            if type(mod).__name__ == "LinearInt4":
                mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
            elif type(mod).__name__ == "LlamaRMSNormInt4":
                mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
        _MODELS[key] = model
    return _MODELS[key]


WINDOW, PAGE, NEW = 40, 16, 200
PROMPT_LENS = (5, 90)


def _prompts(vocab=1000):
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in PROMPT_LENS]


def _pool(kv_heads, capacity):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(2, kv_heads, 128, capacity, PAGE, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def _lp_tensors(lp):
    return [x for x in (lp.token_logprobs, lp.token_ranks, lp.top_ids, lp.top_logprobs) if x is not None]


def test_value_errors():
    from atom_amd import ops
    from atom_amd.e2e import SpeculativeParams, generate
    from atom_amd.utils import KvCacheInt4, RollingKvCacheInt4
    pool = _pool(1, 16)
    seqs = [KvCacheInt4(pool, 50), KvCacheInt4(pool, 3)]
    kv = RollingKvCacheInt4(seqs, WINDOW, max_add=2)
    assert kv.max_pages == K.ring_size(WINDOW, PAGE, 2) and pool.num_free_blocks == 16 - 2 * kv.max_pages
    q = torch.zeros((2, 2, 128), dtype=torch.float16, device=DEV)
    qo = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    for bad in (None, WINDOW + 1):
        with pytest.raises(ValueError, match="rolling cache serves only windowed calls"):
            ops.batch_decode_i4(q, kv, 0, window=bad)
        with pytest.raises(ValueError, match="rolling cache serves only windowed calls"):
            ops.batch_prefill_i4(q, qo, kv, 0, window=bad)
        with pytest.raises(ValueError, match="rolling cache serves only windowed calls"):
            ops.decode_splits(2, kv, 2, window=bad)
    assert ops.decode_splits(2, kv, 2, window=WINDOW) >= 1 and ops.decode_splits(2, kv, 2, window=WINDOW - 1) >= 1
    kv.step(2)
    with pytest.raises(ValueError, match="max_add"):
        kv.step(3)
    kv.close()
    assert pool.num_free_blocks == 16 and all(c.seqlen == 0 and not c.indicies for c in seqs)
    model, prompts = _model(2, 1), _prompts()
    for kw, what in ((dict(caches=[]), "caches"), (dict(num_beams=2), "num_beams"), (dict(speculative=SpeculativeParams()), "speculative")):
        with pytest.raises(ValueError, match=f"rolling_kv does not combine with {what}"):
            generate(model, prompts, 4, pool, rolling_kv=True, **kw)
    with pytest.raises(ValueError, match="layer 0 has none"):
        generate(_model(2, 1, None), prompts, 4, pool, rolling_kv=True)
    mixed = _model(2, 1, WINDOW, layer_types=("sliding_attention", "full_attention"))
    with pytest.raises(ValueError, match="layer 1 has none"):
        generate(mixed, prompts, 4, pool, rolling_kv=True)
    assert pool.num_free_blocks == 16                         # every refusal came before a page was taken


def test_rolling_cache_steps_like_the_reference_and_returns_its_pages():
    """RollingKvCacheInt4 over sequences of 0, 50 and 200 tokens: the pages behind the window go back at construction, the rows are
    rings with logical page g in slot g % R, and 70 steps walk the tables the reference gives"""
    from atom_amd.utils import KvCacheInt4, RollingKvCacheInt4
    pool = _pool(1, 40)
    lens = [0, 50, 200]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    before = [list(c.indicies) for c in seqs]
    R = K.ring_size(WINDOW, PAGE)
    kv = RollingKvCacheInt4(seqs, WINDOW)
    assert pool.num_free_blocks == 40 - 3 * R and kv.max_pages == R
    table = kv.page_table.cpu().numpy()
    for b, n in enumerate(lens):
        f, cnt = K.live_pages(n, 1, WINDOW, PAGE)
        assert [table[b, g % R] for g in range(f, f + cnt)] == before[b][f:f + cnt]
    host = np.asarray(lens)
    for i in range(70):
        want = K.ring_step(table, [R] * 3, host, 0 if i == 0 else 1, WINDOW, PAGE)
        if i:
            kv.step()
        got = (kv.indptr, kv.indicies[:int(want[1][-1])], kv.last_page_offset, kv.kv_start)
        for g, w in zip(got, want[1:5]):
            assert g.cpu().tolist() == w.tolist()
        host = want[0]
    kv.sync_host()
    assert kv.seqlens == [n + 69 for n in lens]
    kv.close()
    assert pool.num_free_blocks == 40


@pytest.mark.parametrize("heads,kv_heads", [(2, 1), (4, 2)])
def test_generate_on_a_ring_of_pages(heads, kv_heads):
    """prompts of 5 and 90 tokens, W = 40 on pages of 16: the pool holds the prompts' pages plus R per sequence and not one more, and
    200 new tokens come out of it -- the default cache runs the same pool dry.  On a large pool the rolling run equals the default
    bit for bit (tokens and every step's logits), greedy, sampled with penalties and log-probabilities, and guided."""
    from atom_amd import ops
    from atom_amd.e2e import SamplingParams, TokenAutomaton, generate
    from atom_amd.utils import KvCacheInt4, RollingKvCacheInt4, StaticBatchedKvCacheInt4
    model, prompts = _model(heads, kv_heads), _prompts()
    R = K.ring_size(WINDOW, PAGE)
    tight = sum(-(-n // PAGE) for n in PROMPT_LENS) + R * len(prompts)
    pool = _pool(kv_heads, tight)
    out = generate(model, prompts, NEW, pool, rolling_kv=True)
    assert [len(row) for row in out] == [NEW, NEW] and pool.num_free_blocks == tight
    with pytest.raises(KeyError):                             # the default reserves prompt + 199 tokens per sequence: the pool runs dry
        generate(model, prompts, NEW, _pool(kv_heads, tight))
    # both caches plan the decode step alike (else the comparison below would be between two summation orders)
    big = sum(-(-(n + NEW) // PAGE) for n in PROMPT_LENS) + 2
    probe = _pool(kv_heads, big)
    seqs = [KvCacheInt4(probe, n) for n in PROMPT_LENS]
    static = StaticBatchedKvCacheInt4(seqs, reserve=NEW - 1)
    splits = ops.decode_splits(2, static, heads, window=WINDOW)
    static.close()
    rolling = RollingKvCacheInt4(seqs, WINDOW)
    assert ops.decode_splits(2, rolling, heads, window=WINDOW) == splits
    rolling.close()
    assert probe.num_free_blocks == big
    want, want_logits = generate(model, prompts, NEW, _pool(kv_heads, big), return_logits=True)
    got, got_logits = generate(model, prompts, NEW, _pool(kv_heads, big), return_logits=True, rolling_kv=True)
    assert got == want == out and torch.equal(got_logits, want_logits)
    assert len({t for row in want for t in row}) >= 8         # (not a model stuck on one token)
    params = [SamplingParams(temperature=0.8, top_k=50, seed=3, repetition_penalty=1.2, presence_penalty=0.3),
              SamplingParams(temperature=1.1, top_p=0.9, seed=4, frequency_penalty=0.2, logit_bias={7: 2.0})]
    a = generate(model, prompts, NEW, _pool(kv_heads, big), sampling=params, logprobs=2, return_logits=True)
    b = generate(model, prompts, NEW, _pool(kv_heads, big), sampling=params, logprobs=2, return_logits=True, rolling_kv=True)
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    for x, y in zip(_lp_tensors(a[2]), _lp_tensors(b[2])):
        assert torch.equal(x, y)
    auto = TokenAutomaton.from_sequences([[3, 1, 4, 1, 5, 9, 2, 6], [3, 1, 4, 2, 7]], 0, 1000)
    a = generate(model, prompts, 12, _pool(kv_heads, big), guide=[auto, None], return_logits=True)
    b = generate(model, prompts, 12, _pool(kv_heads, big), guide=[auto, None], return_logits=True, rolling_kv=True)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[0][0][:3] == [3, 1, 4]
