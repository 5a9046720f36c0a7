"""GPU tests of generation with logit penalties: generate(..., sampling=) with the penalty fields of SamplingParams and
DecodeGraph(..., penalties=) on the tiny models, prompts and pools of tests/test_gpu_generate.py, 41 new tokens.  Every comparison is
EXACT: the replayed step runs the eager step's kernels on the eager step's inputs, the penalised row is a function of the raw logits'
bits, the state words and the parameters (tests/penalty_ref.py), and the token a function of that row (tests/sample_ref.py)."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import penalty_ref, sample_ref
from tests.test_gpu_generate import NEW, SEED, VOCAB, _kv_heads, _model, _pages, _pool, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
PENALTY_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")


def _plain(params):
    """the same draws without any penalty"""
    from atom_amd.e2e import SamplingParams
    d = SamplingParams()
    return [dataclasses.replace(q, **{f: getattr(d, f) for f in PENALTY_FIELDS}) for q in params]


def _base_params(batch):
    """greedy + repetition; sampled + presence / frequency; sampled, to get a ban; all default; everything at once"""
    from atom_amd.e2e import SamplingParams
    return [SamplingParams(0.0, 0, 1.0, 5, repetition_penalty=1.3),
            SamplingParams(0.8, 50, 0.9, 2 ** 40 + 3, presence_penalty=0.5, frequency_penalty=0.3),
            SamplingParams(0.3, 0, 1.0, 11),
            SamplingParams(),
            SamplingParams(1.0, 0, 0.95, 2 ** 63 + 1, repetition_penalty=1.2, presence_penalty=-0.25, frequency_penalty=0.2,
                           logit_bias={3: 1.5, 500: -2.0, VOCAB - 1: 4.0})][:batch]


def _cap(prompts, new=NEW):
    return max(-(-(len(p) + new - 1) // 16) for p in prompts)


def _generate(model, prompts, heads, sampling, **kw):
    from atom_amd.e2e import generate
    pool = _pool(2, heads, _pages([len(p) for p in prompts], 16, NEW) + 2, 16)
    return generate(model, prompts, NEW, pool, return_logits=True, sampling=sampling, **kw)


def _with_ban(params, plain_tokens):
    """sequence 2 (where there is one) gets the most frequent token of its unpenalised run banned"""
    if len(params) < 3:
        return params, None
    row = plain_tokens[2]
    banned = max(sorted(set(row)), key=row.count)
    return params[:2] + [dataclasses.replace(params[2], logit_bias={banned: float("-inf")})] + params[3:], banned


def _tables(params):
    width = max(len(q.logit_bias or ()) for q in params)
    ids = np.full((len(params), width), -1, dtype=np.int32)
    vals = np.zeros((len(params), width), dtype=np.float32)
    for b, q in enumerate(params):
        for j, (t, v) in enumerate(sorted((q.logit_bias or {}).items())):
            ids[b, j], vals[b, j] = t, v
    return ids, vals


def _eager_penalised(model, prompts, pool, params, new, cap):
    """the loop a user writes: eager prefill, then per token one forward, ops.penalize (counting the token just fed in) and ops.sample
    with the token's number as the step: (tokens [new, batch], raw logits [new, batch, vocab])"""
    from atom_amd import ops
    from atom_amd.e2e import Sampler
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    s = Sampler(len(prompts), DEV, params)
    state = torch.zeros((len(prompts), VOCAB), dtype=torch.int16, device=DEV)
    for b, p in enumerate(prompts):
        state[b, torch.tensor(p, device=DEV)] = -32768
    f32 = lambda f: torch.tensor([float(getattr(q, f)) for q in params], dtype=torch.float32, device=DEV)
    rep, pres, freq = f32("repetition_penalty"), f32("presence_penalty"), f32("frequency_penalty")
    ids_np, vals_np = _tables(params)
    bias = (None, None) if ids_np.shape[1] == 0 else (torch.from_numpy(ids_np).to(DEV), torch.from_numpy(vals_np).to(DEV))
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    logits, _ = model(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    logits = logits[torch.tensor(lens).cumsum(0) - 1]
    toks, logs = [], []
    for i in range(new):
        if i > 0:
            for c in seqs:
                c.acquire_one()
            kv = BatchedKvCacheInt4(seqs)
            kv.max_pages = cap
            logits, _ = model(ids, BatchLenInfo([], len(seqs), DEV), None, kv)
        pen = ops.penalize(logits, state, ids if i > 0 else None, rep, pres, freq, *bias)
        ids = ops.sample(pen, s.temperature, s.top_k, s.top_p, s.seeds, step_offset=i)
        toks.append(ids)
        logs.append(logits)
    return torch.stack(toks), torch.stack(logs)


def _reference_tokens(logits, prompts, params):
    """penalty_ref on the kept raw logits [new, batch, vocab] and the token history, then sample_ref: one list per sequence"""
    raw = penalty_ref.bits_of(logits)
    ids, vals = _tables(params)
    out = []
    for b, q in enumerate(params):
        words = np.zeros(VOCAB, dtype=np.uint16)
        words[prompts[b]] = 0x8000
        row = []
        for i in range(raw.shape[0]):
            if i > 0:
                words[row[-1]] = penalty_ref.count_up(words[row[-1]])
            pen, _ = penalty_ref.penalize_row(raw[i, b], words, None, q.repetition_penalty, q.presence_penalty, q.frequency_penalty, ids[b], vals[b])
            row.append(sample_ref.sample_row(pen, q.temperature, q.top_k, q.top_p, q.seed, i))
        out.append(row)
    return out


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kv_heads):
        if kv_heads not in cache:
            cache[kv_heads] = _model(kv_heads, SEED[kv_heads])
        return cache[kv_heads]
    return get


@pytest.fixture(scope="module")
def runs(models):
    """(plain tokens, params with the ban, banned token, penalised tokens, raw logits of the penalised run) per (kv_heads, batch)"""
    cache = {}

    def get(kv_heads, batch):
        if (kv_heads, batch) not in cache:
            model, prompts = models(kv_heads), _prompts(batch)
            plain, _ = _generate(model, prompts, _kv_heads(kv_heads), _plain(_base_params(batch)))
            params, banned = _with_ban(_base_params(batch), plain)
            tokens, logits = _generate(model, prompts, _kv_heads(kv_heads), params)
            cache[(kv_heads, batch)] = (plain, params, banned, tokens, logits)
        return cache[(kv_heads, batch)]
    return get


@pytest.mark.parametrize("kv_heads,batch", [(None, 1), (None, 5), (2, 5)])
def test_penalised_generate_equals_the_eager_loop_and_the_reference(models, runs, kv_heads, batch):
    model, prompts = models(kv_heads), _prompts(batch)
    plain, params, banned, tokens, logits = runs(kv_heads, batch)
    capacity = _pages([len(p) for p in prompts], 16, NEW) + 2
    toks, logs = _eager_penalised(model, prompts, _pool(2, _kv_heads(kv_heads), capacity, 16), params, NEW, _cap(prompts))
    assert tokens == toks.t().tolist()
    assert logits.shape == logs.shape and torch.equal(logits.view(torch.int16), logs.view(torch.int16))
    assert tokens == _reference_tokens(logits, prompts, params)
    print("sequences that differ from their unpenalised run:", [a != b for a, b in zip(tokens, plain)], "banned:", banned)


def test_penalties_change_what_they_should_and_nothing_else(runs):
    """Batch 5, MHA.  The parameters of _base_params: sequence 0 greedy with repetition 1.3; 1 sampled (T 0.8, k 50, p 0.9) with
    presence 0.5 and frequency 0.3; 2 sampled at T 0.3 with the most frequent token of its unpenalised run banned; 3 all default; 4
    repetition 1.2, presence -0.25, frequency 0.2 and three bias entries.  The banned token occurs in sequence 2's unpenalised run by
    construction, so that sequence differs from it whatever the model does.  Measured on the GPU with these parameters: sequences 0, 1,
    2 and 4 all differ from their unpenalised runs (MHA; with the GQA model 1, 2 and 4 do, and the greedy sequence 0 does not)."""
    plain, params, banned, tokens, _ = runs(None, 5)
    assert not params[3].penalises and tokens[3] == plain[3]          # the all-default sequence beside penalised ones
    assert banned in plain[2] and banned not in tokens[2]
    differ = [b for b in (0, 1, 2, 4) if tokens[b] != plain[b]]
    print("penalised sequences that differ from their unpenalised run:", differ)
    assert differ


def test_logprobs_describe_the_raw_logits(models, runs):
    from atom_amd import ops
    model, prompts = models(None), _prompts(5)
    plain, params, _, tokens, logits = runs(None, 5)
    got_tokens, got_logits, lp = _generate(model, prompts, 4, params, logprobs=2)
    assert got_tokens == tokens and torch.equal(got_logits.view(torch.int16), logits.view(torch.int16))
    chosen = torch.tensor(tokens, dtype=torch.int64, device=DEV).t().contiguous()
    for i in (0, 1, NEW - 1):                                        # the model's distribution: ops.logprob on the RAW row
        want = ops.logprob(logits[i], chosen[i], 2)
        for a, b in zip((lp.token_logprobs[i], lp.token_ranks[i], lp.top_ids[i], lp.top_logprobs[i]), want):
            assert torch.equal(a, b), i
    _, _, lp_plain = _generate(model, prompts, 4, _plain(params), logprobs=2)
    assert tokens[3] == plain[3]                                     # the tokens agree: so do the values, bit for bit
    assert torch.equal(lp.token_logprobs[:, 3], lp_plain.token_logprobs[:, 3]) and torch.equal(lp.token_ranks[:, 3], lp_plain.token_ranks[:, 3])
    assert torch.equal(lp.top_ids[:, 3], lp_plain.top_ids[:, 3]) and torch.equal(lp.top_logprobs[:, 3], lp_plain.top_logprobs[:, 3])


def test_default_sampling_allocates_no_state(models, monkeypatch):
    """with every penalty field at its default generate() builds no LogitPenalties and its DecodeGraph has none; with one field set
    it builds one, of the batch's size, and hands it to the graph"""
    import importlib
    from atom_amd.e2e import SamplingParams
    gen = importlib.import_module("atom_amd.e2e.generate")     # the module: the package's attribute of that name is the function
    made, graphs = [], []

    class Penalties(gen.LogitPenalties):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    class Graph(gen.DecodeGraph):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            graphs.append(self)

    monkeypatch.setattr(gen, "LogitPenalties", Penalties)
    monkeypatch.setattr(gen, "DecodeGraph", Graph)
    model, prompts = models(2), _prompts(2)
    for sampling in (None, SamplingParams(0.9, 0, 1.0, 3), [SamplingParams(repetition_penalty=1.0, logit_bias={}), SamplingParams(repetition_penalty=0.0)]):
        _generate(model, prompts, 2, sampling)
        assert not made and graphs[-1].penalties is None and graphs[-1].penalised is None
    _generate(model, prompts, 2, [SamplingParams(), SamplingParams(frequency_penalty=0.5)])
    assert len(made) == 1 and graphs[-1].penalties is made[0] and made[0].batch == 2 and made[0].max_bias == 0
    assert made[0].state.shape == (2, VOCAB) and graphs[-1].penalised.shape == (2, VOCAB)
    counts = (made[0].state & 0x7FFF).sum(dim=1).tolist()
    assert counts == [NEW - 1, NEW - 1]                              # every token fed back in was counted, the last one never was


def test_decode_graph_with_penalties_needs_a_sampler_and_replays_without_synchronising(models):
    from atom_amd.e2e import DecodeGraph, LogitPenalties, SamplingParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    from tests.test_gpu_generate import _prefill
    model, prompts, steps = models(2), _prompts(2), 12
    params = [SamplingParams(0.0, 0, 1.0, 4, repetition_penalty=1.5), SamplingParams(0.7, 0, 1.0, 9, presence_penalty=1.0, logit_bias={7: -float("inf")})]
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    pen = LogitPenalties(2, VOCAB, DEV, params)
    pen.reset(prompts)
    with pytest.raises(ValueError):
        DecodeGraph(model, skv, steps, penalties=pen)
    dg = DecodeGraph(model, skv, steps, keep_logits=True, sampler=params, penalties=pen)
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
    ids, vals = _tables(params)
    history = [first.tolist()] + dg.tokens.tolist()          # row i: the tokens step i consumes
    raw = penalty_ref.bits_of(dg.logits)
    for b, q in enumerate(params):
        words = np.zeros(VOCAB, dtype=np.uint16)
        words[prompts[b]] = 0x8000
        for i in range(steps):                               # step i counts the token it is fed, then draws number i + 1
            words[history[i][b]] = penalty_ref.count_up(words[history[i][b]])
            row, _ = penalty_ref.penalize_row(raw[i, b], words, None, q.repetition_penalty, q.presence_penalty, q.frequency_penalty, ids[b], vals[b])
            assert history[i + 1][b] == sample_ref.sample_row(row, q.temperature, q.top_k, q.top_p, q.seed, i + 1), (b, i)
        assert np.array_equal(penalty_ref.bits_of(pen.state)[b, :VOCAB], words)
