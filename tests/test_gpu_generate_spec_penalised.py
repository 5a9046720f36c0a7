"""GPU tests of penalties under speculative decoding: SpecDecodeGraph(penalties=) / generate(speculative=
SpeculativeParams(penalised=True)) on the tiny models, prompts, pools and helpers of tests/test_gpu_generate_spec.py.  Every comparison
is EXACT.  The eager side is the loop a user writes without this feature: the host loop of tests/test_gpu_generate_spec.py (verify
forward as a chunked prefill, accept and emit by tests/spec_ref.py) with, per verify row, ``ops.penalize`` on a CLONE of the sequence's
state row through which drafts 1 .. j are fed one at a time, and, per emitted token, ``ops.penalize(fed=)`` on the state row itself."""
import importlib

import numpy as np
import pytest
import torch

from tests import guide_ref, guide_walk_ref, spec_ref
from tests.test_gpu_generate import NEW, VOCAB, _kv_heads, _prefill, _prompts
from tests.test_gpu_generate_spec import TableDrafter, _Choose, _cap, _get_model, _spec_pool, _table
from tests.test_gpu_generate_spec_guided import ConstDrafter, WRONG, _auto, _in_language, _masked, _tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BATCH = 2
_CACHE = {}


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


def _plain_sampling():
    from atom_amd.e2e import SamplingParams
    return [SamplingParams(temperature=0.8, top_k=50, top_p=0.95, seed=1), SamplingParams(temperature=0.0)]


def _unpenalised(kv_heads, K):
    """the unpenalised speculative run (computed once per case) and the token to ban: the one sequence 1 first emits at a position >= 2"""
    key = ("plain", kv_heads, K)
    if key not in _CACHE:
        from atom_amd.e2e import SpeculativeParams, generate
        model, prompts = _get_model(kv_heads), _prompts(BATCH)
        pool = _spec_pool(prompts, _kv_heads(kv_heads), NEW, K)
        rows = generate(model, prompts, NEW, pool, sampling=_plain_sampling(), speculative=SpeculativeParams(num_draft_tokens=K))
        banned = [t for i, t in enumerate(rows[1]) if i >= 2 and t not in rows[1][:i]]
        assert banned, "sequence 1 emits nothing new behind its second token: pick another model seed"
        _CACHE[key] = (rows, banned[0])
    return _CACHE[key]


def _sampling(kv_heads, K):
    from atom_amd.e2e import SamplingParams
    _, t = _unpenalised(kv_heads, K)
    return [SamplingParams(temperature=0.8, top_k=50, top_p=0.95, seed=1, repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=0.4),
            SamplingParams(temperature=0.0, logit_bias={t: float("-inf")})]


def _host_state(prompts, tokens):
    """prompt flags plus a count per emitted token, as the state words"""
    want = np.zeros((len(prompts), VOCAB), dtype=np.uint16)
    for b, (p, row) in enumerate(zip(prompts, tokens)):
        for t in p:
            want[b, t] |= 0x8000
        for t in row:
            want[b, t] += 1
    return want


def _state_of(pen):
    return pen.state[:, :VOCAB].cpu().numpy().view(np.uint16)


def _eager(kv_heads, K, new, propose, sampling, reject_all=False, names=None, force=True):
    """the eager loop: dict of tokens, accepted, steps, accept counts per step, final lengths, the final penalty state and, with
    guides (``names``), the status bits"""
    from atom_amd import ops
    from atom_amd.e2e import LogitPenalties
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    model, prompts = _get_model(kv_heads), _prompts(BATCH)
    autos = [None] * BATCH if names is None else [None if n is None else _auto(n) for n in names]
    Q, cap = K + 1, _cap(prompts, new, K)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    seqs, _, first_logits = _prefill(model, prompts, pool)
    choose = _Choose(sampling, BATCH)
    pen = LogitPenalties(BATCH, VOCAB, DEV, sampling)
    pen.reset(prompts)
    has_bias = pen.max_bias > 0
    dummy = torch.zeros((1, VOCAB), dtype=torch.float16, device=DEV)

    def row_kw(b):
        return dict(repetition=pen.repetition[b:b + 1], presence=pen.presence[b:b + 1], frequency=pen.frequency[b:b + 1],
                    bias_ids=pen.bias_ids[b:b + 1] if has_bias else None, bias_vals=pen.bias_vals[b:b + 1] if has_bias else None)

    def penalised_row(b, row, fed):
        """``row`` [1, vocab] under a clone of sequence b's state through which ``fed`` went one token at a time"""
        scratch, got = pen.state[b:b + 1].clone(), None
        for t in fed:
            got = ops.penalize(row, scratch, _i64([t]), **row_kw(b))
        return ops.penalize(row, scratch, None, **row_kw(b)) if got is None else got

    def emit(b, tokens):
        for t in tokens:                                      # counted into the state itself; the output is not used
            ops.penalize(dummy, pen.state[b:b + 1], _i64([t]))

    gstate = [guide_ref.FREE if a is None else a.start for a in autos]
    row0 = _masked(pen.apply(first_logits.contiguous()), gstate, autos)
    first = choose.first(row0).tolist()
    hist = [list(p) + [t] for p, t in zip(prompts, first)]
    for b in range(BATCH):
        emit(b, [first[b]])
    n_out, accepted, steps, counts, bits = [1] * BATCH, [0] * BATCH, [0] * BATCH, [], 0
    adds, prev = [0] * BATCH, [[0] * Q for _ in range(BATCH)]
    blen = BatchLenInfo([Q] * BATCH, 0, DEV)
    while min(n_out) < new:
        drafts = [[int(t) for t in propose(b, hist[b], n_out[b])] for b in range(BATCH)]
        if names is not None:                                 # the walk: every row's automaton state, the forced drafts
            for b, a in enumerate(autos):
                indptr, tok, nxt = _tables(a)
                gstate[b], prev[b], row, st = guide_walk_ref.walk(gstate[b], adds[b], prev[b], [hist[b][-1]] + drafts[b], indptr, tok, nxt,
                                                                 indptr.size - 1, tok.size, force)
                bits |= st
                drafts[b] = row[1:]
        while True:
            for c in seqs:
                c.acquire(Q)
            kv = BatchedKvCacheInt4(seqs)
            kv.max_pages = cap
            ids = _i64([t for b in range(BATCH) for t in [hist[b][-1]] + drafts[b]])
            logits, _ = model(ids, blen, kv, None)
            rows = torch.cat([penalised_row(b, logits[b * Q + j:b * Q + j + 1], drafts[b][:j]) for b in range(BATCH) for j in range(Q)])
            if names is not None:
                rows = _masked(rows, [s for b in range(BATCH) for s in prev[b]], [a for a in autos for _ in range(Q)])
            targets = choose.rows(rows, n_out, Q)
            acc = [spec_ref.accept_count(drafts[b], targets[b], K) for b in range(BATCH)]
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
            emit(b, targets[b][:e])
            c._seqlen -= Q - e
            c.trim()
            adds[b] = e
            if e:
                n_out[b], accepted[b], steps[b] = n_out[b] + e, accepted[b] + e - 1, steps[b] + 1
        counts.append(acc)
    if names is not None:
        for b in range(BATCH):
            gstate[b], st = guide_walk_ref.commit(gstate[b], adds[b], prev[b], Q)
            bits |= st
    lens = [c.seqlen for c in seqs]
    for c in seqs:
        c.release()
    return dict(tokens=[h[len(p):] for h, p in zip(hist, prompts)], accepted=accepted, steps=steps, counts=counts, lens=lens,
                state=_state_of(pen), bits=bits)


def _replay(kv_heads, K, new, drafter, sampling, names=None, force=True):
    """SpecDecodeGraph(penalties=) over a static cache: the same dict (without the counts), and the graph"""
    from atom_amd.e2e import LogitGuide, LogitPenalties, SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    model, prompts = _get_model(kv_heads), _prompts(BATCH)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    free = pool.num_free_blocks
    seqs, _, first_logits = _prefill(model, prompts, pool)
    pen = LogitPenalties(BATCH, VOCAB, DEV, sampling)
    pen.reset(prompts)
    guide = None if names is None else LogitGuide(BATCH, VOCAB, DEV, [None if n is None else _auto(n) for n in names])
    row0 = pen.apply(first_logits.contiguous())
    first = _Choose(sampling, BATCH).first(row0 if guide is None else guide.mask(row0))
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K, guided=names is not None, force_drafts=force, penalised=True),
                         drafter=drafter, sampler=sampling, guide=guide, penalties=pen)
    assert sg.penalised.shape == (BATCH * (K + 1), VOCAB) and sg.guided is None
    sg.start(prompts, first)
    toks, n_out = sg.run().tolist(), sg.n_out.tolist()
    skv.close()                                              # raises if the overflow bit was ever set
    lens = [c.seqlen for c in seqs]
    for c in seqs:
        c.release()
    assert pool.num_free_blocks == free
    return dict(tokens=[row[:n] for row, n in zip(toks, n_out)], accepted=sg.accepted.tolist(), steps=sg.steps.tolist(), lens=lens,
                state=_state_of(pen), bits=0 if guide is None else guide.status_bits()), sg


def _eager_table(kv_heads, K):
    """the penalised eager loop under the table drafter (computed once per case): (table, its dict)"""
    key = ("table", kv_heads, K)
    if key not in _CACHE:
        sampling = _sampling(kv_heads, K)
        truth = _eager(kv_heads, K, NEW, lambda b, h, n: [(h[-1] + 1) % VOCAB] * K, sampling, reject_all=True)
        assert truth["accepted"] == [0] * BATCH and truth["steps"] == [NEW - 1] * BATCH
        table = _table(truth["tokens"], K, NEW)
        _CACHE[key] = (table, _eager(kv_heads, K, NEW, lambda b, h, n: table[b][n:n + K], sampling))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. replay equals the eager loop
@pytest.mark.parametrize("kv_heads", [None, 2])
@pytest.mark.parametrize("K", [1, 4])
def test_penalised_speculative_replay_equals_the_eager_loop(K, kv_heads):
    from atom_amd.e2e import SpeculativeParams, generate
    prompts, sampling = _prompts(BATCH), _sampling(kv_heads, K)
    plain, banned = _unpenalised(kv_heads, K)
    table, want = _eager_table(kv_heads, K)
    seen = {a for step in want["counts"] for a in step}
    print(f"kv_heads={kv_heads} K={K}: banned token {banned}, accept counts seen {sorted(seen)}, steps {want['steps']}, accepted {want['accepted']}")
    assert {0, K} <= seen and (K == 1 or seen - {0, K}), "all-accepted, none-accepted and mixed steps must occur in the EAGER loop"
    assert all(len(row) == NEW for row in want["tokens"]) and [1 + a + s for a, s in zip(want["accepted"], want["steps"])] == [NEW] * BATCH
    # the penalties take effect in verify rows: with them ignored the outputs below would be the unpenalised ones
    assert banned in plain[1][2:] and banned not in want["tokens"][1]
    assert want["tokens"][0] != plain[0] and want["tokens"][1] != plain[1]
    assert np.array_equal(want["state"], _host_state(prompts, want["tokens"]))
    got, sg = _replay(kv_heads, K, NEW, TableDrafter(table, K), sampling)
    assert got["tokens"] == want["tokens"]
    assert got["accepted"] == want["accepted"] and got["steps"] == want["steps"]
    assert got["lens"] == want["lens"] == [len(p) + NEW - 1 for p in prompts]
    assert np.array_equal(got["state"], _host_state(prompts, got["tokens"]))
    sg.commit()                                              # a second commit counts nothing
    assert np.array_equal(_state_of(sg.penalties), got["state"])
    model = _get_model(kv_heads)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), NEW, K)
    free = pool.num_free_blocks
    out, stats = generate(model, prompts, NEW, pool, sampling=sampling, speculative=SpeculativeParams(num_draft_tokens=K, penalised=True),
                          drafter=TableDrafter(table, K), return_spec_stats=True)
    assert out == want["tokens"] and stats.accepted == want["accepted"] and stats.steps == want["steps"]
    assert pool.num_free_blocks == free


def test_penalised_guided_speculative_replay_equals_the_eager_loop():
    """penalties first, then the mask: a planted choice guide on the penalised sampled sequence, none on the greedy one with its ban"""
    K, names = 4, ("planted4", None)
    sampling = _sampling(None, K)
    _, banned = _unpenalised(None, K)
    want = _eager(None, K, NEW, lambda b, h, n: [WRONG] * K, sampling, names=names)
    print(f"guided: steps {want['steps']}, accepted {want['accepted']}")
    assert want["bits"] == 0 and _in_language(_auto("planted4"), want["tokens"][0]) and banned not in want["tokens"][1]
    got, sg = _replay(None, K, NEW, ConstDrafter(), sampling, names=names)
    assert got["tokens"] == want["tokens"] and got["bits"] == 0
    assert got["accepted"] == want["accepted"] and got["steps"] == want["steps"] and got["lens"] == want["lens"]
    assert np.array_equal(got["state"], want["state"]) and np.array_equal(got["state"], _host_state(_prompts(BATCH), got["tokens"]))


# ------------------------------------------------------------------------------------------------ 2. generate
def test_penalised_without_penalty_fields_is_the_unpenalised_run(monkeypatch):
    from atom_amd import ops
    from atom_amd.e2e import SpeculativeParams, generate
    gen = importlib.import_module("atom_amd.e2e.generate")
    made, graphs = [], []

    class Penalties(gen.LogitPenalties):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    class Graph(gen.SpecDecodeGraph):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            graphs.append(self)

    def refuse(*a, **kw):
        raise AssertionError("a penalty op was launched without a penalty field")

    monkeypatch.setattr(gen, "LogitPenalties", Penalties)
    monkeypatch.setattr(gen, "SpecDecodeGraph", Graph)
    for name in ("penalize", "penalize_rows"):
        monkeypatch.setattr(ops, name, refuse)
    K = 4
    plain, _ = _unpenalised(None, K)
    model, prompts = _get_model(None), _prompts(BATCH)
    pool = _spec_pool(prompts, 4, NEW, K)
    try:
        got = generate(model, prompts, NEW, pool, sampling=_plain_sampling(), speculative=SpeculativeParams(num_draft_tokens=K, penalised=True))
        assert not made and graphs[-1].penalties is None and graphs[-1].penalised is None
    finally:
        graphs.clear()                                       # see test_speculative_without_a_guide_launches_no_guide_op
    assert got == plain


@pytest.mark.parametrize("K", [1, 4])
def test_budgets_are_kept_and_the_pool_is_restored(K):
    from atom_amd.e2e import SamplingParams, SpeculativeParams, generate
    model, prompts = _get_model(None), _prompts(BATCH)
    pool = _spec_pool(prompts, 4, K + 2, K)
    free = pool.num_free_blocks
    sampling = SamplingParams(temperature=0.7, seed=3, frequency_penalty=0.5)
    longest = None
    for new in sorted({1, 2, K, K + 2}, reverse=True):
        got, stats = generate(model, prompts, new, pool, sampling=sampling, speculative=SpeculativeParams(num_draft_tokens=K, penalised=True),
                              return_spec_stats=True)
        assert [len(row) for row in got] == [new] * BATCH
        assert [1 + a + s for a, s in zip(stats.accepted, stats.steps)] == [new] * BATCH
        assert pool.num_free_blocks == free
        longest = got if longest is None else longest
        assert [row[:1] for row in got] == [row[:1] for row in longest]


def test_default_speculative_params_still_refuse_penalties():
    from atom_amd.e2e import SamplingParams, SpeculativeParams, generate
    model, prompts = _get_model(None), _prompts(1)
    pool = _spec_pool(prompts, 4, 8, 4)
    free = pool.num_free_blocks
    for name, kw in (("repetition_penalty", dict(repetition_penalty=1.3)), ("presence_penalty", dict(presence_penalty=0.5)),
                     ("frequency_penalty", dict(frequency_penalty=0.5)), ("logit_bias", dict(logit_bias={3: 1.0}))):
        with pytest.raises(ValueError, match=name):
            generate(model, prompts, 4, pool, speculative=SpeculativeParams(), sampling=SamplingParams(**kw))
    for kw in (dict(logprobs=0), dict(return_logits=True), dict(num_beams=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            generate(model, prompts, 4, pool, speculative=SpeculativeParams(penalised=True), sampling=SamplingParams(frequency_penalty=0.5), **kw)
    assert pool.num_free_blocks == free


def test_spec_decode_graph_penalties_need_a_sampler():
    from atom_amd.e2e import LogitPenalties, SamplingParams, SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    model, prompts = _get_model(None), _prompts(BATCH)
    pool = _spec_pool(prompts, 4, 8, 2)
    seqs, _, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=8 + 2)
    try:
        with pytest.raises(ValueError, match="sampler"):
            SpecDecodeGraph(model, skv, 8, params=SpeculativeParams(num_draft_tokens=2, penalised=True),
                            penalties=LogitPenalties(BATCH, VOCAB, DEV, SamplingParams(frequency_penalty=0.5)))
    finally:
        skv.close()
        for c in seqs:
            c.release()


# ------------------------------------------------------------------------------------------------ 3. no hidden synchronisation
def test_penalised_speculative_step_does_not_synchronise():
    from atom_amd.e2e import LogitPenalties, SpecDecodeGraph, SpeculativeParams
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
    K, new = 4, 21
    sampling = _sampling(2, K)
    model, prompts = _get_model(2), _prompts(BATCH)
    pool = _spec_pool(prompts, 2, new, K)
    seqs, _, first_logits = _prefill(model, prompts, pool)
    pen = LogitPenalties(BATCH, VOCAB, DEV, sampling)
    pen.reset(prompts)
    first = _Choose(sampling, BATCH).first(pen.apply(first_logits.contiguous()))
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K, penalised=True), sampler=sampling, penalties=pen)
    sg.start(prompts, first)
    sg.step()
    sg.step()                                                # eager warm-up and the capture are allowed to synchronise
    torch.cuda.set_sync_debug_mode("error")
    try:
        while sg.steps_done < sg.max_steps:
            sg.step()
        sg.commit()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    skv.close()
    assert sg.n_out.tolist() == [new] * BATCH and int(sg.done[0]) == 1
    assert np.array_equal(_state_of(pen), _host_state(prompts, [row[:new] for row in sg.tokens.tolist()]))
    for c in seqs:
        c.release()
