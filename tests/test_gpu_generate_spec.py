"""GPU tests of speculative decoding by graph replay: SpecDecodeGraph / generate(speculative=) on the tiny models, prompts and pools of
tests/test_gpu_generate.py, 41 new tokens on pages of 16.  Every comparison is EXACT: the eager side is the loop a user writes without
this feature -- host-built BatchedKvCacheInt4 over un-reserved sequences of a second pool, the verify forward as a chunked prefill of
Q = K + 1 tokens per sequence, drafting and acceptance by tests/spec_ref.py on the host, rejected slots dropped by trimming the host
sequence.  Its caches take the static cache's row width as ``max_pages``, so the KV-split count is the same on both sides.

Speculative output is NOT compared with plain generate() token for token: a verify row runs the multi-row GEMM routes and the
f16-operand prefill attention, a one-token step the dot-product kernels and the FP32 decode attention, so near-ties may resolve
differently.  test_report_* print where the two first differ, and whether the eager speculative output equals the all-rejected run
(row-position independence of the verify forward); profiles/spec/README.md records what they printed."""
import pytest
import torch

from tests import spec_ref
from tests.test_gpu_generate import NEW, SEED, VOCAB, _eager_decode, _kv_heads, _model, _pages, _pool, _prefill, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_MODELS, _EAGER = {}, {}
SAMPLED = "sampled"
# model seeds per num_key_value_heads for the n-gram test: with SEED's models no 41-token run repeats an n-gram it can continue; with
# these the EAGER loop alone accepts drafts ([1, 0] and [2, 2] per sequence) and rejects others
NGRAM_SEED = {None: 7, 2: 12}


def _get_model(kv_heads, seed=None):
    seed = SEED[kv_heads] if seed is None else seed
    if (kv_heads, seed) not in _MODELS:
        _MODELS[kv_heads, seed] = _model(kv_heads, seed)
    return _MODELS[kv_heads, seed]


def _sampling():
    from atom_amd.e2e import SamplingParams
    return [SamplingParams(temperature=0.8, top_k=50, top_p=0.95, seed=1), SamplingParams(temperature=0.0)]


def _cap(prompts, new, K):
    """the static cache's row width: prompt + (new + K) reserved tokens"""
    return max(-(-(len(p) + new + K) // 16) for p in prompts)


def _spec_pool(prompts, heads, new, K):
    return _pool(2, heads, _pages([len(p) for p in prompts], 16, new + K) + 2, 16)


class _Choose:
    """the token of every verify row: argmax, or ops.sample with ONE-element draw numbers, row by row"""

    def __init__(self, sampling, batch):
        from atom_amd.e2e import Sampler
        self.s = None if sampling is None else Sampler(batch, DEV, sampling)

    def first(self, logits):
        return logits.argmax(-1) if self.s is None else self.s.sample(logits.contiguous())

    def rows(self, logits, n_out, Q):
        from atom_amd import ops
        if self.s is None:
            return logits.argmax(-1).view(-1, Q).tolist()
        s, out = self.s, []
        for r in range(logits.size(0)):
            b, j = divmod(r, Q)
            step = torch.tensor([n_out[b] + j], dtype=torch.int64, device=DEV)
            out.append(int(ops.sample(logits[r:r + 1], s.temperature[b:b + 1], s.top_k[b:b + 1], s.top_p[b:b + 1], s.seeds[b:b + 1], step=step)[0]))
        return [out[b * Q:(b + 1) * Q] for b in range(len(n_out))]


def _eager_spec(kv_heads, batch, K, new, propose, sampling=None, reject_all=False, seed=None):
    """the eager loop: (tokens per sequence, accepted, steps, accept counts per step and sequence, final lengths).
    ``propose(b, history, n_out)`` gives K drafts; ``reject_all``: a step whose first draft is right by accident is run again with
    that draft replaced -- row 0 of a sequence does not see the drafts, so its token stays and the new draft is wrong for certain."""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    model, prompts = _get_model(kv_heads, seed), _prompts(batch)
    Q, cap = K + 1, _cap(prompts, new, K)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    seqs, _, first_logits = _prefill(model, prompts, pool)
    choose = _Choose(sampling, batch)
    first = choose.first(first_logits).tolist()
    hist = [list(p) + [t] for p, t in zip(prompts, first)]
    n_out, accepted, steps, counts = [1] * batch, [0] * batch, [0] * batch, []
    blen = BatchLenInfo([Q] * batch, 0, DEV)
    while min(n_out) < new:
        drafts = [[int(t) for t in propose(b, hist[b], n_out[b])] for b in range(batch)]
        while True:
            for c in seqs:
                c.acquire(Q)
            kv = BatchedKvCacheInt4(seqs)
            kv.max_pages = cap
            ids = torch.tensor([t for b in range(batch) for t in [hist[b][-1]] + drafts[b]], dtype=torch.int64, device=DEV)
            logits, _ = model(ids, blen, kv, None)
            targets = choose.rows(logits, n_out, Q)
            acc = [spec_ref.accept_count(drafts[b], targets[b], K) for b in range(batch)]
            if not (reject_all and any(acc)):
                break
            for b, c in enumerate(seqs):                     # once more, the accidentally right first drafts replaced
                c._seqlen -= Q
                c.trim()
                if acc[b]:
                    drafts[b][0] = (targets[b][0] + 1) % VOCAB
        for b, c in enumerate(seqs):
            e = spec_ref.emit_count(acc[b], new, n_out[b])
            hist[b] += targets[b][:e]
            c._seqlen -= Q - e                               # the rejected slots are dropped: the sequence keeps its e verified tokens
            c.trim()
            if e:
                n_out[b], accepted[b], steps[b] = n_out[b] + e, accepted[b] + e - 1, steps[b] + 1
        counts.append(acc)
    lens = [c.seqlen for c in seqs]
    for c in seqs:
        c.release()
    return [h[len(p):] for h, p in zip(hist, prompts)], accepted, steps, counts, lens


def _truth(kv_heads, batch, K, new, sampling=None):
    """the all-rejected eager run (computed once per case): every token comes from row 0 of a verify step"""
    key = (kv_heads, batch, K, new, SAMPLED if sampling else None)
    if key not in _EAGER:
        toks, accepted, steps, _, _ = _eager_spec(kv_heads, batch, K, new, lambda b, h, n: [(h[-1] + 1) % VOCAB] * K, sampling, reject_all=True)
        assert accepted == [0] * batch and steps == [new - 1] * batch
        _EAGER[key] = toks
    return _EAGER[key]


def _pattern(K):
    """1 = a right draft: runs of 0, 1, .., K right ones and one of 2 K + 1, each closed by a wrong one"""
    out = []
    for run in list(range(K + 1)) + [2 * K + 1]:
        out += [1] * run + [0]
    return out


def _table(truth, K, new):
    """drafts per token index: the truth, corrupted as (t + 1) % vocab where the pattern says so (sequence b starts b places into it)"""
    pat = _pattern(K)
    rows = []
    for b, toks in enumerate(truth):
        row = [0] * (new + K)
        for i in range(1, new + K):
            t = toks[i] if i < len(toks) else 0
            row[i] = t if pat[(i - 1 + b) % len(pat)] else (t + 1) % VOCAB
        rows.append(row)
    return rows


class TableDrafter:
    """drafts from a [batch, max_new + K] table at n_out + j: a gather, capturable"""

    def __init__(self, table, K):
        self.table = torch.tensor(table, dtype=torch.int64, device=DEV)
        self.cols = torch.arange(K, dtype=torch.int64, device=DEV).unsqueeze(0)

    def propose(self, hist, hist_len, n_out, out):
        out.copy_(self.table.gather(1, n_out.to(torch.int64).unsqueeze(1) + self.cols))


def _replay(kv_heads, batch, K, new, drafter, sampling=None, params=None):
    """SpecDecodeGraph over a static cache: (tokens per sequence, accepted, steps, final lengths, graph)"""
    from atom_amd.e2e import SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    model, prompts = _get_model(kv_heads), _prompts(batch)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    free = pool.num_free_blocks
    seqs, _, first_logits = _prefill(model, prompts, pool)
    first = _Choose(sampling, batch).first(first_logits)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    assert skv.max_pages == _cap(prompts, new, K)
    sg = SpecDecodeGraph(model, skv, new, params=params or SpeculativeParams(num_draft_tokens=K), drafter=drafter, sampler=sampling)
    sg.start(prompts, first)
    toks, counts = sg.run().tolist(), sg.n_out.tolist()
    skv.close()                                              # raises if the overflow bit was ever set
    lens = [c.seqlen for c in seqs]
    assert [len(c.indicies) for c in seqs] == [-(-n // 16) for n in lens]
    for c in seqs:
        c.release()
    assert pool.num_free_blocks == free
    return [row[:n] for row, n in zip(toks, counts)], sg.accepted.tolist(), sg.steps.tolist(), lens, sg


def _eager_table(kv_heads, batch, K, new, sampling=None):
    """the eager loop under the table drafter (computed once per case): (truth, table, tokens, accepted, steps, counts, lengths)"""
    key = ("table", kv_heads, batch, K, new, SAMPLED if sampling else None)
    if key not in _EAGER:
        truth = _truth(kv_heads, batch, K, new, sampling)
        table = _table(truth, K, new)
        _EAGER[key] = (truth, table) + _eager_spec(kv_heads, batch, K, new, lambda b, h, n: table[b][n:n + K], sampling)
    return _EAGER[key]


def _check_table_case(kv_heads, batch, K, new, sampling=None):
    truth, table, want, accepted, steps, counts, lens = _eager_table(kv_heads, batch, K, new, sampling)
    seen = {a for step in counts for a in step}
    distinct = len({t for row in want for t in row})
    print(f"kv_heads={kv_heads} batch={batch} K={K} new={new} sampled={bool(sampling)}: accept counts seen {sorted(seen)}, steps {steps}, "
          f"accepted {accepted}, distinct tokens {distinct}, equals the all-rejected run: {want == truth}")
    assert seen == set(range(K + 1)), "not every accept count 0 .. K occurred in the EAGER loop: pick another pattern/seed"
    assert distinct >= 8, "the tiny model collapsed in the EAGER loop: pick another pattern/seed"
    assert all(len(row) == new for row in want) and [1 + a + s for a, s in zip(accepted, steps)] == [new] * batch
    got, g_acc, g_steps, g_lens, _ = _replay(kv_heads, batch, K, new, TableDrafter(table, K), sampling)
    assert got == want
    assert g_acc == accepted and g_steps == steps
    assert g_lens == lens == [len(p) + new - 1 for p in _prompts(batch)]


# ------------------------------------------------------------------------------------------------ 1. replay equals the eager loop
@pytest.mark.parametrize("kv_heads", [None, 2])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_speculative_replay_equals_the_eager_loop(K, batch, kv_heads):
    _check_table_case(kv_heads, batch, K, NEW)


def test_speculative_replay_with_eight_drafts():
    """K = 8: the pattern of runs 0 .. 8 and 17 needs 63 tokens behind the first"""
    _check_table_case(None, 2, 8, 1 + len(_pattern(8)) + 2)


# ------------------------------------------------------------------------------------------------ 2. the n-gram drafter
@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_with_the_ngram_drafter_equals_the_eager_loop(kv_heads):
    from atom_amd.e2e import SpeculativeParams, generate
    K, batch = 4, 2
    propose = lambda b, h, n: spec_ref.draft_rule(h, len(h), K, 3, 1)
    want, accepted, steps, counts, _ = _eager_spec(kv_heads, batch, K, NEW, propose, seed=NGRAM_SEED[kv_heads])
    flat = [a for step in counts for a in step]
    print(f"ngram kv_heads={kv_heads}: accepted {accepted}, steps {steps}, accept counts {sorted(set(flat))}")
    assert sum(accepted) >= 1 and any(a < K for a in flat), "no draft accepted, or none rejected, in the EAGER loop: pick another seed (NGRAM_SEED)"
    model, prompts = _get_model(kv_heads, NGRAM_SEED[kv_heads]), _prompts(batch)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), NEW, K)
    free = pool.num_free_blocks
    got, stats = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K, ngram_max=3), return_spec_stats=True)
    assert got == want and stats.accepted == accepted and stats.steps == steps
    assert pool.num_free_blocks == free
    eos = want[0][5]                                         # cut after the first EOS on the host, as without the feature
    cut = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K, ngram_max=3), eos_token_id=eos)
    assert cut == [row[:row.index(eos) + 1] if eos in row else row for row in want]


# ------------------------------------------------------------------------------------------------ 3. sampled
def test_sampled_speculative_replay_equals_the_eager_loop():
    _check_table_case(None, 2, 4, NEW, sampling=_sampling())


def test_sampled_generate_takes_the_table_drafter():
    from atom_amd.e2e import SpeculativeParams, generate
    K, batch = 4, 2
    _, table, want, accepted, steps, _, _ = _eager_table(None, batch, K, NEW, _sampling())
    model, prompts = _get_model(None), _prompts(batch)
    pool = _spec_pool(prompts, 4, NEW, K)
    got, stats = generate(model, prompts, NEW, pool, sampling=_sampling(), speculative=SpeculativeParams(num_draft_tokens=K),
                          drafter=TableDrafter(table, K), return_spec_stats=True)
    assert got == want and stats.accepted == accepted and stats.steps == steps


# ------------------------------------------------------------------------------------------------ 4. budgets
@pytest.mark.parametrize("K", [1, 4])
def test_budgets_are_kept_and_the_pool_is_restored(K):
    from atom_amd.e2e import SpeculativeParams, generate
    model, prompts = _get_model(None), _prompts(2)
    pool = _spec_pool(prompts, 4, K + 2, K)
    free = pool.num_free_blocks
    longest = None
    for new in sorted({1, 2, K, K + 2}, reverse=True):
        got, stats = generate(model, prompts, new, pool, speculative=SpeculativeParams(num_draft_tokens=K), return_spec_stats=True)
        assert [len(row) for row in got] == [new] * 2        # never more than the budget (and, without an EOS, never fewer)
        assert [1 + a + s for a, s in zip(stats.accepted, stats.steps)] == [new] * 2
        assert pool.num_free_blocks == free
        longest = got if longest is None else longest
        assert [row[:1] for row in got] == [row[:1] for row in longest]      # the first token is the prefill's
    plain = generate(model, prompts, 1, pool)
    assert plain == generate(model, prompts, 1, pool, speculative=SpeculativeParams(num_draft_tokens=K))   # no step at all


# ------------------------------------------------------------------------------------------------ 5. no hidden synchronisation
def test_speculative_step_does_not_synchronise():
    from atom_amd.e2e import SpecDecodeGraph, SpeculativeParams
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
    K, new, batch = 4, 21, 2
    model, prompts = _get_model(2), _prompts(batch)
    pool = _spec_pool(prompts, 2, new, K)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K))
    sg.start(prompts, first)
    sg.step()
    sg.step()                                                # eager warm-up and the capture are allowed to synchronise
    torch.cuda.set_sync_debug_mode("error")
    try:
        while sg.steps_done < sg.max_steps:
            sg.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sg.commit()
    skv.close()
    assert sg.n_out.tolist() == [new] * batch and int(sg.done[0]) == 1
    assert skv.seqlens == [len(p) + new - 1 for p in prompts]
    want, accepted, steps, _, _ = _eager_spec(2, batch, K, new, lambda b, h, n: spec_ref.draft_rule(h, len(h), K, 3, 1))
    assert [row[:new] for row in sg.tokens.tolist()] == want and sg.accepted.tolist() == accepted and sg.steps.tolist() == steps
    with pytest.raises(RuntimeError):
        sg.step()                                            # all steps taken: refused on the host, nothing is launched
    for c in seqs:
        c.release()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_generate_refuses_what_speculative_decoding_does_not_cover():
    from atom_amd.e2e import SamplingParams, SpeculativeParams, generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _get_model(None), _prompts(1)
    pool = _spec_pool(prompts, 4, 8, 4)
    free = pool.num_free_blocks
    spec = SpeculativeParams()
    cases = [("num_beams", dict(num_beams=2)), ("logprobs", dict(logprobs=0)), ("return_logits", dict(return_logits=True)),
             ("caches", dict(caches=[KvCacheInt4(pool, 0)])),
             ("repetition_penalty", dict(sampling=SamplingParams(repetition_penalty=1.3))),
             ("presence_penalty", dict(sampling=SamplingParams(presence_penalty=0.5))),
             ("frequency_penalty", dict(sampling=[SamplingParams(frequency_penalty=0.5)])),
             ("logit_bias", dict(sampling=SamplingParams(logit_bias={3: 1.0})))]
    for name, kw in cases:
        with pytest.raises(ValueError, match=name):
            generate(model, prompts, 4, pool, speculative=spec, **kw)
    with pytest.raises(ValueError, match="speculative"):
        generate(model, prompts, 4, pool, return_spec_stats=True)
    for kw in (dict(num_draft_tokens=0), dict(num_draft_tokens=9), dict(ngram_max=9), dict(ngram_min=0), dict(ngram_min=3, ngram_max=2)):
        with pytest.raises(ValueError):
            SpeculativeParams(**kw)
    assert pool.num_free_blocks == free


# ------------------------------------------------------------------------------------------------ 7. without the argument
def test_generate_without_speculative_is_unchanged():
    from atom_amd.e2e import generate
    model, prompts = _get_model(None), _prompts(2)
    cap = max(-(-(len(p) + NEW - 1) // 16) for p in prompts)
    capacity = _pages([len(p) for p in prompts], 16, NEW) + 2
    pe, pg = _pool(2, 4, capacity, 16), _pool(2, 4, capacity, 16)
    se, first, _ = _prefill(model, prompts, pe)
    toks, _ = _eager_decode(model, se, first, NEW - 1, cap)
    assert generate(model, prompts, NEW, pg) == torch.cat([first[None], toks]).t().tolist()
    assert generate(model, prompts, NEW, pg, speculative=None) == torch.cat([first[None], toks]).t().tolist()


# ------------------------------------------------------------------------------------------------ 8. the two printed comparisons
def test_report_first_difference_from_plain_generate():
    """prints, never asserts on, where speculative output first differs from plain generate() (different kernels: see the module
    docstring) and whether the eager speculative run equals the all-rejected run"""
    from atom_amd.e2e import generate
    for kv_heads in (None, 2):
        for batch in (1, 2):
            model, prompts = _get_model(kv_heads), _prompts(batch)
            pool = _spec_pool(prompts, _kv_heads(kv_heads), NEW, 4)
            plain = generate(model, prompts, NEW, pool)
            for K in (1, 3, 4):
                truth, _, spec = _eager_table(kv_heads, batch, K, NEW)[:3]
                first = [next((i for i, (x, y) in enumerate(zip(s, p)) if x != y), "none") for s, p in zip(spec, plain)]
                print(f"REPORT kv_heads={kv_heads} batch={batch} K={K}: first token differing from plain generate() per sequence {first}; "
                      f"eager speculative == all-rejected run: {spec == truth}")
