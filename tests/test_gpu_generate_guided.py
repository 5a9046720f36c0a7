"""GPU tests of guided generation: generate(..., guide=) and DecodeGraph(..., guide=) on the tiny models, prompts and pools of
tests/test_gpu_generate.py, 41 new tokens.  Every comparison is EXACT: the masked row is a function of the raw logits' bits, the
automaton's state and its mask (tests/guide_ref.py), the state a function of the tokens, and the token a function of the masked row
(argmax, or tests/penalty_ref.py and tests/sample_ref.py) -- so the tokens are reproduced from the returned raw logits alone."""
import re

import numpy as np
import pytest
import torch

from tests import guide_ref, penalty_ref, sample_ref
from tests.test_gpu_generate import NEW, SEED, VOCAB, _kv_heads, _model, _pages, _pool, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EOS = VOCAB - 1
INTEGER = r"-?(0|[1-9][0-9]*)"
INTEGER_PREFIX = r"-?(0|[1-9][0-9]*)?"        # what a prefix of a match looks like
CHOICES = [[17], [250, 3], [250, 700, 41], [5, 6, 7, 8]]


def _strings():
    """a synthetic token-string table for the 1000-token vocabulary: digits, punctuation, letters and multi-character pieces (numbers
    of two and three digits, signed digits, words, letter pairs); the last token is EOS and has no string"""
    s = [str(d) for d in range(10)] + list("-.,:;!? _+") + [chr(c) for c in range(ord("a"), ord("z") + 1)]
    s += [chr(c) for c in range(ord("A"), ord("Z") + 1)] + [f"{n}" for n in range(10, 100)] + [f"-{d}" for d in range(1, 10)]
    s += ["true", "false", "null", "00", "007", "-0", "1.5", "--"] + [f"{n}" for n in range(100, 1000, 7)]
    a = 0
    while len(s) < VOCAB - 1:
        s.append(chr(ord("a") + a // 26 % 26) + chr(ord("a") + a % 26) + ("" if a < 676 else "x"))
        a += 1
    assert len(s) == VOCAB - 1 and len(set(s)) == len(s)
    return s + [None]


@pytest.fixture(scope="module")
def automata():
    from atom_amd.e2e import TokenAutomaton
    strings = _strings()
    integer = TokenAutomaton.from_regex(INTEGER, strings, EOS)
    choice = TokenAutomaton.from_sequences(CHOICES, EOS, VOCAB)
    words = TokenAutomaton.from_regex(r"(true|false|null)( [a-z]+){1,3}[.!?]", strings, EOS)
    return strings, integer, choice, words


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kv_heads):
        if kv_heads not in cache:
            cache[kv_heads] = _model(kv_heads, SEED[kv_heads])
        return cache[kv_heads]
    return get


def _guides(automata, batch):
    _, integer, choice, words = automata
    return [integer, choice, None, integer, words][:batch]


def _params(mode, batch):
    from atom_amd.e2e import SamplingParams
    if mode == "greedy":
        return None
    plain = [SamplingParams(0.9, 0, 1.0, 5), SamplingParams(0.0, 0, 1.0, 2), SamplingParams(0.7, 40, 0.9, 2 ** 40 + 3), SamplingParams(1.3, 0, 0.8, 11),
             SamplingParams(1.0, 3, 1.0, 2 ** 63 + 1)]
    if mode == "sampled":
        return plain[:batch]
    import dataclasses
    extra = [dict(repetition_penalty=1.3), dict(presence_penalty=0.5, frequency_penalty=0.3), dict(), dict(frequency_penalty=1.5, logit_bias={1: 4.0, EOS: -1.0}),
             dict(repetition_penalty=1.2, presence_penalty=-0.25, logit_bias={3: 1.5, 500: -2.0})]
    return [dataclasses.replace(q, **kw) for q, kw in zip(plain, extra)][:batch]


def _generate(model, prompts, heads, **kw):
    from atom_amd.e2e import generate
    pool = _pool(2, heads, _pages([len(p) for p in prompts], 16, NEW) + 2, 16)
    return generate(model, prompts, NEW, pool, **kw)


def _bias_tables(params):
    width = max(len(q.logit_bias or ()) for q in params)
    ids, vals = np.full((len(params), width), -1, dtype=np.int32), np.zeros((len(params), width), dtype=np.float32)
    for b, q in enumerate(params):
        for j, (t, v) in enumerate(sorted((q.logit_bias or {}).items())):
            ids[b, j], vals[b, j] = t, v
    return ids, vals


def _reference_tokens(logits, prompts, params, guides):
    """the tokens from the kept raw logits [new, batch, vocab]: per sequence penalty_ref (if any field is set anywhere), guide_ref's mask
    at the state guide_ref's walk has reached, then the first argmax or sample_ref's draw number i; also the states after every token"""
    raw = guide_ref.bits_of(logits)
    penalised = params is not None and any(q.penalises for q in params)
    ids, vals = _bias_tables(params) if penalised else (None, None)
    out, states = [], []
    for b, auto in enumerate(guides):
        words = np.zeros(VOCAB, dtype=np.uint16)
        words[prompts[b]] = 0x8000
        mask = None if auto is None else guide_ref.mask_from_csr(auto.indptr, auto.edge_tok, -(-VOCAB // 32))
        s, row, walk = (guide_ref.FREE if auto is None else auto.start), [], []
        for i in range(raw.shape[0]):
            bits = raw[i, b]
            if i > 0 and auto is not None:
                s, st = guide_ref.advance_one(s, row[-1], auto.indptr, auto.edge_tok, auto.edge_next, auto.num_states, auto.num_edges)
                assert st == 0
            if penalised:
                q = params[b]
                if i > 0:
                    words[row[-1]] = penalty_ref.count_up(words[row[-1]])
                bits, _ = penalty_ref.penalize_row(bits, words, None, q.repetition_penalty, q.presence_penalty, q.frequency_penalty, ids[b], vals[b])
            if auto is not None:
                bits, st = guide_ref.mask_row(bits, s, mask, auto.num_states)
                assert st == 0 and (bits != guide_ref.NEG_INF).sum() <= len(auto.allowed(s))
            if params is None:
                row.append(int(np.argmax(bits.view(np.float16).astype(np.float32))))
            else:
                q = params[b]
                row.append(sample_ref.sample_row(bits, q.temperature, q.top_k, q.top_p, q.seed, i))
            walk.append(s)
        out.append(row)
        states.append(walk)
    return out, states


@pytest.mark.parametrize("mode", ["greedy", "sampled", "penalised"])
@pytest.mark.parametrize("kv_heads,batch", [(None, 1), (None, 5), (2, 5)])
def test_guided_generate_is_reproduced_from_its_raw_logits(models, automata, kv_heads, batch, mode):
    model, prompts = models(kv_heads), _prompts(batch)
    guides, params = _guides(automata, batch), _params(mode, batch)
    tokens, logits = _generate(model, prompts, _kv_heads(kv_heads), guide=guides, sampling=params, return_logits=True)
    assert logits.shape == (NEW, batch, VOCAB) and all(len(row) == NEW for row in tokens)
    assert not torch.isnan(logits).any()
    want, _ = _reference_tokens(logits, prompts, params, guides)
    assert tokens == want
    for row, auto in zip(tokens, guides):                      # and every guided row walks its automaton to the end
        assert auto is None or guide_ref.DEAD not in guide_ref.walk(auto.start, row, auto.indptr, auto.edge_tok, auto.edge_next)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_choices_come_out_as_one_of_the_choices_followed_by_eos(models, automata, mode):
    _, _, choice, _ = automata
    out = _generate(models(None), _prompts(5), 4, guide=choice, sampling=_params(mode, 5), eos_token_id=EOS)
    print("choices:", out)
    for row in out:
        assert row[-1] == EOS and row[:-1] in CHOICES, row


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_regex_output_is_a_prefix_of_a_match_and_a_match_where_eos_appears(models, automata, mode):
    strings, integer, _, words = automata
    model, prompts = models(2), _prompts(5)
    for auto, full, prefix in ((integer, INTEGER, INTEGER_PREFIX), (words, r"(true|false|null)( [a-z]+){1,3}[.!?]", None)):
        out = _generate(model, prompts, 2, guide=auto, sampling=_params(mode, 5), eos_token_id=EOS)
        ended = 0
        for row in out:
            text = "".join(strings[t] for t in row if t != EOS)
            assert EOS not in row[:-1]
            if row[-1] == EOS:
                ended += 1
                assert re.fullmatch(full, text), text
            else:
                assert len(row) == NEW
                if prefix is not None:
                    assert re.fullmatch(prefix, text), text
            assert auto.accepts(row) == (row[-1] == EOS)
        print(f"{full} ({mode}): {ended} of {len(out)} rows reached EOS:", ["".join(strings[t] for t in row if t != EOS) for row in out])


def test_a_guide_on_some_rows_leaves_the_others_alone(models, automata):
    _, integer, choice, _ = automata
    model, prompts = models(None), _prompts(5)
    plain = _generate(model, prompts, 4)
    guided = _generate(model, prompts, 4, guide=[None, integer, None, choice, None])
    for b in (0, 2, 4):
        assert guided[b] == plain[b], b
    for b in (1, 3):
        assert guided[b] != plain[b], b


def _graph(model, prompts, steps, guide, **kw):
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    from tests.test_gpu_generate import _prefill
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    return DecodeGraph(model, skv, steps, guide=guide, **kw), skv, first


def test_a_token_outside_the_language_sets_rejected_and_frees_the_row(models, automata):
    from atom_amd import ops
    from atom_amd.e2e import LogitGuide
    _, integer, choice, _ = automata
    model, prompts, steps = models(2), _prompts(2), 10
    guide = LogitGuide(2, VOCAB, DEV, [choice, integer])
    dg, skv, _ = _graph(model, prompts, steps, guide, keep_logits=True)
    first = [999 - 1, 1]                                          # row 0: no choice starts with it; row 1: "1", inside the language
    assert choice.step(choice.start, first[0]) is None and integer.step(integer.start, first[1]) is not None
    tokens = dg.run(torch.tensor(first, dtype=torch.int64, device=DEV)).t().tolist()      # no exception comes from the device
    skv.close()
    assert guide.status_bits() == ops.GUIDE_REJECTED
    assert guide.state.tolist()[0] == ops.GUIDE_DEAD and guide.state.tolist()[1] >= 0
    raw = guide_ref.bits_of(dg.logits)
    assert tokens[0] == [int(np.argmax(raw[i, 0].view(np.float16).astype(np.float32))) for i in range(steps)]   # unconstrained from then on
    mask = guide_ref.mask_from_csr(integer.indptr, integer.edge_tok, -(-VOCAB // 32))
    s, fed = integer.start, first[1]
    for i in range(steps):
        s, st = guide_ref.advance_one(s, fed, integer.indptr, integer.edge_tok, integer.edge_next, integer.num_states, integer.num_edges)
        row, _ = guide_ref.mask_row(raw[i, 1], s, mask, integer.num_states)
        fed = int(np.argmax(row.view(np.float16).astype(np.float32)))
        assert st == 0 and tokens[1][i] == fed, i
    assert guide.state.tolist()[1] - guide.offsets[1] == guide_ref.walk(integer.start, [first[1]] + tokens[1][:-1], integer.indptr,
                                                                        integer.edge_tok, integer.edge_next)[-1]


def test_generate_raises_on_a_status_bit(models, automata, monkeypatch):
    """a state pushed outside the tables behind generate's back: BAD_STATE is read once after the loop and raised"""
    import importlib
    gen = importlib.import_module("atom_amd.e2e.generate")
    _, integer, _, _ = automata

    class Broken(gen.LogitGuide):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.start[0] = self.num_states + 5
            self.state.copy_(self.start)

    monkeypatch.setattr(gen, "LogitGuide", Broken)
    with pytest.raises(RuntimeError, match="BAD_STATE"):
        _generate(models(2), _prompts(2), 2, guide=integer)


def test_no_guide_allocates_nothing_and_launches_nothing(models, monkeypatch):
    import importlib
    from atom_amd import ops
    from atom_amd.e2e import SamplingParams
    gen = importlib.import_module("atom_amd.e2e.generate")
    made, graphs = [], []

    class Guide(gen.LogitGuide):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    class Graph(gen.DecodeGraph):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            graphs.append(self)

    def refuse(*a, **kw):
        raise AssertionError("a guide op was launched without a guide")

    monkeypatch.setattr(gen, "LogitGuide", Guide)
    monkeypatch.setattr(gen, "DecodeGraph", Graph)
    monkeypatch.setattr(ops, "guide_mask", refuse)
    monkeypatch.setattr(ops, "guide_advance", refuse)
    model, prompts = models(2), _prompts(2)
    for kw in (dict(), dict(sampling=SamplingParams(0.9, 0, 1.0, 3)), dict(sampling=SamplingParams(frequency_penalty=0.5)), dict(guide=None),
               dict(guide=[None, None])):
        _generate(model, prompts, 2, **kw)
        assert not made and graphs[-1].guide is None and graphs[-1].guided is None


def test_guide_is_refused_with_beams_and_with_speculative(models, automata):
    from atom_amd.e2e import SpeculativeParams
    _, integer, _, _ = automata
    model, prompts = models(2), _prompts(2)
    with pytest.raises(ValueError, match="guide"):
        _generate(model, prompts, 2, guide=integer, num_beams=2)
    with pytest.raises(ValueError, match="guide"):
        _generate(model, prompts, 2, guide=integer, speculative=SpeculativeParams())
    with pytest.raises(ValueError, match="guide"):
        _generate(model, prompts, 2, guide=[integer])              # one automaton per prompt


def test_guided_replay_does_not_synchronise(models, automata):
    from atom_amd.e2e import LogitGuide, SamplingParams
    _, integer, choice, _ = automata
    model, prompts, steps = models(2), _prompts(2), 12
    for kw in (dict(), dict(sampler=[SamplingParams(0.8, 0, 1.0, 4), SamplingParams(0.0, 0, 1.0, 9)])):
        guide = LogitGuide(2, VOCAB, DEV, [integer, choice])
        dg, skv, _ = _graph(model, prompts, steps, guide, **kw)
        dg.input_ids.copy_(torch.tensor([1, 250], dtype=torch.int64, device=DEV))
        dg.step()
        dg.step()                                                  # eager warm-up and the capture are allowed to synchronise
        torch.cuda.set_sync_debug_mode("error")
        try:
            while dg.steps_done < steps:
                dg.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        skv.close()
        assert guide.status_bits() == 0
        rows = dg.tokens.t().tolist()
        assert integer.accepts([1] + rows[0]) == (rows[0][-1] == EOS) and choice.accepts([250] + rows[1])
