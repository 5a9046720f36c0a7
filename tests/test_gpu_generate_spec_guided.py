"""GPU tests of guided speculative decoding: SpecDecodeGraph(guide=) / generate(guide=, speculative=
SpeculativeParams(guided=True)) on the tiny models, prompts and pools of tests/test_gpu_generate.py, 41 new tokens on pages of 16.
Every comparison is EXACT.  The eager side is the loop a user writes without this feature: host-built BatchedKvCacheInt4 over
un-reserved sequences, the verify forward as a chunked prefill of Q = K + 1 tokens per sequence, the walk by tests/guide_walk_ref.py,
the mask by tests/guide_ref.py on the forward's own bits, accept and emit by tests/spec_ref.py, and each row's token by argmax or a
one-row ops.sample.

The choice guide of ``_planted_choices(K)`` plants every accept count itself: a two-way branch (never forced), then a run of r tokens
that are the only ones allowed, for r = 0, 1, .., K and 2 K + 1, then EOS.  Under a drafter that is always wrong (a token no state
allows) a step accepts exactly the forced drafts: r of them behind branch r, K inside the long run and in the EOS tail."""
import importlib

import numpy as np
import pytest
import torch

from tests import guide_ref, guide_walk_ref, spec_ref
from tests.test_gpu_generate import NEW, VOCAB, _kv_heads, _prefill, _prompts
from tests.test_gpu_generate_guided import EOS, INTEGER, _params, _strings
from tests.test_gpu_generate_spec import _Choose, _cap, _get_model, _spec_pool

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
WRONG = VOCAB - 3                                              # no automaton below has an edge over it, and it is not EOS
_AUTO, _EAGER, _MASKS = {}, {}, {}
EMPTY = (np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))    # the table a None row walks: FREE stays


def _planted_choices(K):
    seqs, tok = [[]], 200
    for d, run in enumerate(list(range(K + 1)) + [2 * K + 1]):
        tail = list(range(tok, tok + run))
        tok += run
        seqs = [s + [100 + 2 * d + o] + tail for s in seqs for o in (0, 1)]
    return seqs


def _auto(name):
    from atom_amd.e2e import TokenAutomaton
    if name not in _AUTO:
        if name == "integer":
            _AUTO[name] = TokenAutomaton.from_regex(INTEGER, _strings(), EOS)
        elif name.startswith("planted"):
            _AUTO[name] = TokenAutomaton.from_sequences(_planted_choices(int(name[7:])), EOS, VOCAB)
        else:                                                  # "singleL": one choice of L tokens
            _AUTO[name] = TokenAutomaton.from_sequences([list(range(300, 300 + int(name[6:])))], EOS, VOCAB)
    return _AUTO[name]


def _guides(names):
    return [None if n is None else _auto(n) for n in names]


def _mask_of(auto):
    if id(auto) not in _MASKS:
        _MASKS[id(auto)] = guide_ref.mask_from_csr(auto.indptr, auto.edge_tok, -(-VOCAB // 32))
    return _MASKS[id(auto)]


def _masked(logits, states, autos):
    """``logits`` [rows, vocab] masked on the host, row r in (local) state ``states[r]`` of ``autos[r]``; a device tensor again"""
    bits = guide_ref.bits_of(logits)
    out = bits.copy()
    for r, (s, auto) in enumerate(zip(states, autos)):
        if auto is not None:
            out[r], st = guide_ref.mask_row(bits[r], s, _mask_of(auto), auto.num_states)
            assert st == 0
    return torch.from_numpy(out.view(np.int16)).to(DEV).view(torch.float16)


def _tables(auto):
    return EMPTY if auto is None else (auto.indptr, auto.edge_tok, auto.edge_next)


class ConstDrafter:
    """every draft is WRONG: a fill, capturable"""

    def propose(self, hist, hist_len, n_out, out):
        out.fill_(WRONG)


def _propose(kind, K):
    if kind == "wrong":
        return (lambda b, h, n: [WRONG] * K), ConstDrafter()
    return (lambda b, h, n: spec_ref.draft_rule(h, len(h), K, 3, 1)), None           # None: generate's own NgramDrafter(3, 1)


def _eager(kv_heads, names, K, new, kind, sampled, force):
    """the eager loop (computed once per case): dict of tokens, accepted, steps, accept counts per step, final lengths, final committed
    states (local to each automaton) and status bits"""
    key = (kv_heads, tuple(names), K, new, kind, sampled, force)
    if key in _EAGER:
        return _EAGER[key]
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    batch, autos = len(names), _guides(names)
    sampling = _params("sampled", batch) if sampled else None
    propose, _ = _propose(kind, K)
    model, prompts = _get_model(kv_heads), _prompts(batch)
    Q, cap = K + 1, _cap(prompts, new, K)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    seqs, _, first_logits = _prefill(model, prompts, pool)
    choose = _Choose(sampling, batch)
    state = [guide_ref.FREE if a is None else a.start for a in autos]
    first = choose.first(_masked(first_logits, state, autos)).tolist()
    hist = [list(p) + [t] for p, t in zip(prompts, first)]
    n_out, accepted, steps, counts, bits = [1] * batch, [0] * batch, [0] * batch, [], 0
    adds, prev = [0] * batch, [[0] * Q for _ in range(batch)]
    blen = BatchLenInfo([Q] * batch, 0, DEV)
    while min(n_out) < new:
        ids = []
        for b, a in enumerate(autos):
            drafts = [int(t) for t in propose(b, hist[b], n_out[b])]
            indptr, tok, nxt = _tables(a)
            state[b], prev[b], row, st = guide_walk_ref.walk(state[b], adds[b], prev[b], [hist[b][-1]] + drafts, indptr, tok, nxt,
                                                             indptr.size - 1, tok.size, force)
            bits |= st
            ids.append(row)
        for c in seqs:
            c.acquire(Q)
        kv = BatchedKvCacheInt4(seqs)
        kv.max_pages = cap
        logits, _ = model(torch.tensor([t for row in ids for t in row], dtype=torch.int64, device=DEV), blen, kv, None)
        masked = _masked(logits, [s for b in range(batch) for s in prev[b]], [a for a in autos for _ in range(Q)])
        targets = choose.rows(masked, n_out, Q)
        acc = [spec_ref.accept_count(ids[b][1:], targets[b], K) for b in range(batch)]
        for b, c in enumerate(seqs):
            e = spec_ref.emit_count(acc[b], new, n_out[b])
            hist[b] += targets[b][:e]
            c._seqlen -= Q - e                               # the rejected slots are dropped: the sequence keeps its e verified tokens
            c.trim()
            adds[b] = e
            if e:
                n_out[b], accepted[b], steps[b] = n_out[b] + e, accepted[b] + e - 1, steps[b] + 1
        counts.append(acc)
    for b in range(batch):                                    # the commit after the last step
        state[b], st = guide_walk_ref.commit(state[b], adds[b], prev[b], Q)
        bits |= st
    lens = [c.seqlen for c in seqs]
    for c in seqs:
        c.release()
    _EAGER[key] = dict(tokens=[h[len(p):] for h, p in zip(hist, prompts)], accepted=accepted, steps=steps, counts=counts, lens=lens,
                       states=state, bits=bits)
    return _EAGER[key]


def _local_states(guide, autos):
    out = []
    for s, a in zip(guide.state.tolist(), autos):
        k = None if a is None else [i for i, x in enumerate(guide.automata) if x is a][0]
        out.append(s if (a is None or s < 0) else s - int(guide.offsets[k]))
    return out


def _replay(kv_heads, names, K, new, kind, sampled, force, first=None):
    """SpecDecodeGraph(guide=) over a static cache: the same dict as ``_eager`` (without the counts), and the graph"""
    from atom_amd.e2e import LogitGuide, SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    batch, autos = len(names), _guides(names)
    sampling = _params("sampled", batch) if sampled else None
    model, prompts = _get_model(kv_heads), _prompts(batch)
    pool = _spec_pool(prompts, _kv_heads(kv_heads), new, K)
    free = pool.num_free_blocks
    seqs, _, first_logits = _prefill(model, prompts, pool)
    guide = LogitGuide(batch, VOCAB, DEV, autos)
    if first is None:
        first = _Choose(sampling, batch).first(guide.mask(first_logits.contiguous()))
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K, guided=True, force_drafts=force),
                         drafter=_propose(kind, K)[1], sampler=sampling, guide=guide)
    assert sg.guided.shape == (batch * (K + 1), VOCAB) and guide.row_state.shape == (batch, K + 1)
    sg.start(prompts, first)
    toks, n_out = sg.run().tolist(), sg.n_out.tolist()
    skv.close()                                              # raises if the overflow bit was ever set
    lens = [c.seqlen for c in seqs]
    for c in seqs:
        c.release()
    assert pool.num_free_blocks == free
    return dict(tokens=[row[:n] for row, n in zip(toks, n_out)], accepted=sg.accepted.tolist(), steps=sg.steps.tolist(), lens=lens,
                states=_local_states(guide, autos), bits=guide.status_bits()), sg


def _in_language(auto, row):
    s = auto.start
    for t in row:
        s = auto.step(s, t)
        if s is None:
            return False
    return True


# kv_heads, guides per sequence, K, drafter, sampled, force_drafts
CASES = [
    (None, ("planted4", None), 4, "wrong", False, True),
    (2, ("planted2", None), 2, "wrong", True, True),
    (None, ("integer", "planted2", None, "integer", "planted2"), 2, "wrong", False, True),
    (2, ("integer", "planted4", None, "integer", "single13"), 4, "ngram", True, True),
    (2, ("planted4", None), 4, "ngram", False, False),
    (None, ("integer", "planted2", None, "integer", "single13"), 2, "ngram", True, False),
]


# ------------------------------------------------------------------------------------------------ 1. replay equals the eager loop
@pytest.mark.parametrize("kv_heads,names,K,kind,sampled,force", CASES)
def test_guided_speculative_replay_equals_the_eager_loop(kv_heads, names, K, kind, sampled, force):
    want = _eager(kv_heads, names, K, NEW, kind, sampled, force)
    autos, prompts = _guides(names), _prompts(len(names))
    print(f"kv_heads={kv_heads} guides={names} K={K} drafter={kind} sampled={sampled} force={force}: steps {want['steps']}, accepted "
          f"{want['accepted']}, accept counts per sequence {[sorted({step[b] for step in want['counts']}) for b in range(len(names))]}")
    assert want["bits"] == 0 and all(len(row) == NEW for row in want["tokens"])
    assert [1 + a + s for a, s in zip(want["accepted"], want["steps"])] == [NEW] * len(names)
    for b, (name, auto) in enumerate(zip(names, autos)):
        if auto is not None:                                  # the language: the EAGER output never leaves its automaton
            assert _in_language(auto, want["tokens"][b]), b
        if name is not None and name.startswith("planted") and kind == "wrong" and force:
            seen = {step[b] for step in want["counts"]}
            assert seen == set(range(K + 1)), "the automaton did not plant every accept count 0 .. K in the EAGER loop"
    got, _ = _replay(kv_heads, names, K, NEW, kind, sampled, force)
    assert got["tokens"] == want["tokens"]
    assert got["accepted"] == want["accepted"] and got["steps"] == want["steps"]
    assert got["lens"] == want["lens"] == [len(p) + NEW - 1 for p in prompts]
    assert got["states"] == want["states"] and got["bits"] == 0
    for b, auto in enumerate(autos):                          # the committed state is the host walk of all tokens but the last
        if auto is not None:
            assert got["states"][b] == guide_ref.walk(auto.start, got["tokens"][b][:-1], auto.indptr, auto.edge_tok, auto.edge_next)[-1]


@pytest.mark.parametrize("case", [0, 3, 5])
def test_generate_takes_guide_and_speculative_together(case):
    from atom_amd.e2e import SpeculativeParams, generate
    kv_heads, names, K, kind, sampled, force = CASES[case]
    want = _eager(kv_heads, names, K, NEW, kind, sampled, force)
    model, autos, prompts = _get_model(kv_heads), _guides(names), _prompts(len(names))
    pool = _spec_pool(prompts, _kv_heads(kv_heads), NEW, K)
    free = pool.num_free_blocks
    spec = SpeculativeParams(num_draft_tokens=K, guided=True, force_drafts=force)
    sampling = _params("sampled", len(names)) if sampled else None
    got, stats = generate(model, prompts, NEW, pool, guide=autos, sampling=sampling, speculative=spec,
                          drafter=_propose(kind, K)[1], return_spec_stats=True)
    assert got == want["tokens"] and stats.accepted == want["accepted"] and stats.steps == want["steps"]
    assert pool.num_free_blocks == free
    cut = generate(model, prompts, NEW, pool, guide=autos, sampling=sampling, speculative=spec, drafter=_propose(kind, K)[1], eos_token_id=EOS)
    for name, auto, row, full in zip(names, autos, cut, want["tokens"]):
        assert row == (full[:full.index(EOS) + 1] if EOS in full else full)
        if auto is not None:
            assert _in_language(auto, row)
        if name is not None and name.startswith("planted"):   # a choice guide's output: one of its choices, then EOS
            assert row[-1] == EOS and row[:-1] in _planted_choices(int(name[7:]))


# ------------------------------------------------------------------------------------------------ 2. forced runs pay
@pytest.mark.parametrize("K", [2, 4])
def test_a_single_choice_is_emitted_at_full_acceptance(K):
    from atom_amd.e2e import SpeculativeParams, generate
    L = 2 * K + 5
    auto, choice = _auto(f"single{L}"), list(range(300, 300 + L))
    model, prompts = _get_model(2), _prompts(2)
    pool = _spec_pool(prompts, 2, NEW, K)
    kw = dict(guide=auto, drafter=ConstDrafter(), return_spec_stats=True)
    got, stats = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K, guided=True), **kw)
    assert got == [choice + [EOS] * (NEW - L)] * 2
    n_out, steps = 1, 0
    while n_out < NEW:                                        # what the rules give when every draft is accepted
        n_out, steps = n_out + spec_ref.emit_count(K, NEW, n_out), steps + 1
    assert stats.steps == [steps] * 2 and stats.accepted == [NEW - 1 - steps] * 2 and steps < (NEW - 1) / K
    cut = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K, guided=True), eos_token_id=EOS,
                   guide=auto, drafter=ConstDrafter())
    assert cut == [choice + [EOS]] * 2
    slow, slow_stats = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K, guided=True, force_drafts=False), **kw)
    assert slow == got and slow_stats.steps == [NEW - 1] * 2 and slow_stats.accepted == [0, 0]      # one step per token


# ------------------------------------------------------------------------------------------------ 3. unconstrained rows
def test_the_unconstrained_row_equals_its_row_under_speculative_alone():
    from atom_amd.e2e import SpeculativeParams, generate
    K = 4
    model, prompts = _get_model(None), _prompts(2)
    pool = _spec_pool(prompts, 4, NEW, K)
    alone, s0 = generate(model, prompts, NEW, pool, speculative=SpeculativeParams(num_draft_tokens=K), return_spec_stats=True)
    mixed, s1 = generate(model, prompts, NEW, pool, guide=[_auto("planted4"), None], speculative=SpeculativeParams(num_draft_tokens=K, guided=True),
                         return_spec_stats=True)
    assert mixed[1] == alone[1] and (s1.accepted[1], s1.steps[1]) == (s0.accepted[1], s0.steps[1])
    assert mixed[0] != alone[0] and _in_language(_auto("planted4"), mixed[0])


# ------------------------------------------------------------------------------------------------ 4. the status word
def test_a_first_token_without_an_edge_finishes_and_leaves_rejected():
    from atom_amd import ops
    names, K = ("planted2", "integer"), 2
    first = torch.tensor([WRONG, 1], dtype=torch.int64, device=DEV)       # row 0: no choice starts with it; row 1: "1"
    assert _auto("planted2").step(0, WRONG) is None and _auto("integer").step(0, 1) is not None
    got, sg = _replay(2, names, K, 12, "wrong", False, True, first=first)   # no exception comes from the device
    assert got["bits"] == ops.GUIDE_REJECTED
    assert got["states"][0] == ops.GUIDE_DEAD and got["states"][1] >= 0
    assert all(len(row) == 12 for row in got["tokens"]) and _in_language(_auto("integer"), got["tokens"][1])
    assert int(sg.done[0]) == 1


def test_generate_raises_on_rejected(monkeypatch):
    """the first token drawn WITHOUT its mask behind generate's back: it has no edge, and the commit behind it sets REJECTED.  Two new
    tokens: one eager step and the commit-only walk, so the frames the exception keeps alive hold no captured graph"""
    from atom_amd.e2e import SpeculativeParams, generate
    gen = importlib.import_module("atom_amd.e2e.generate")
    model, prompts = _get_model(2), _prompts(2)
    pool = _spec_pool(prompts, 2, 2, 2)
    plain = generate(model, prompts, 1, pool)
    auto = _auto("single13")
    assert all(auto.step(auto.start, row[0]) is None for row in plain)

    class Unmasked(gen.LogitGuide):
        def mask(self, logits, out=None):
            return logits

    monkeypatch.setattr(gen, "LogitGuide", Unmasked)
    free = pool.num_free_blocks
    with pytest.raises(RuntimeError, match="REJECTED"):
        generate(model, prompts, 2, pool, guide=auto, speculative=SpeculativeParams(num_draft_tokens=2, guided=True))
    assert pool.num_free_blocks == free


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_stay():
    from atom_amd.e2e import SamplingParams, SpeculativeParams, generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _get_model(None), _prompts(1)
    pool = _spec_pool(prompts, 4, 8, 4)
    free = pool.num_free_blocks
    auto = _auto("integer")
    with pytest.raises(ValueError, match=r"guide does not combine with speculative.*SpeculativeParams\(guided=True\)"):
        generate(model, prompts, 4, pool, guide=auto, speculative=SpeculativeParams())
    spec = SpeculativeParams(guided=True)
    for name, kw in [("logprobs", dict(logprobs=0)), ("return_logits", dict(return_logits=True)), ("caches", dict(caches=[KvCacheInt4(pool, 0)])),
                     ("repetition_penalty", dict(sampling=SamplingParams(repetition_penalty=1.3))),
                     ("presence_penalty", dict(sampling=SamplingParams(presence_penalty=0.5))),
                     ("frequency_penalty", dict(sampling=[SamplingParams(frequency_penalty=0.5)])),
                     ("logit_bias", dict(sampling=SamplingParams(logit_bias={3: 1.0})))]:
        with pytest.raises(ValueError, match=name):
            generate(model, prompts, 4, pool, guide=auto, speculative=spec, **kw)
    with pytest.raises(ValueError, match="num_beams"):
        generate(model, prompts, 4, pool, guide=auto, speculative=spec, num_beams=2)
    assert pool.num_free_blocks == free


# ------------------------------------------------------------------------------------------------ 6. launch parity
def test_speculative_without_a_guide_launches_no_guide_op(monkeypatch):
    from atom_amd import ops
    from atom_amd.e2e import SpeculativeParams, generate
    gen = importlib.import_module("atom_amd.e2e.generate")
    made, graphs = [], []

    class Guide(gen.LogitGuide):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    class Graph(gen.SpecDecodeGraph):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            graphs.append(self)

    def refuse(*a, **kw):
        raise AssertionError("a guide op was launched without a guide")

    monkeypatch.setattr(gen, "LogitGuide", Guide)
    monkeypatch.setattr(gen, "SpecDecodeGraph", Graph)
    for name in ("guide_mask", "guide_advance", "guide_walk_rows"):
        monkeypatch.setattr(ops, name, refuse)
    model, prompts = _get_model(2), _prompts(2)
    pool = _spec_pool(prompts, 2, 6, 2)
    outs = []
    try:
        for kw in (dict(speculative=SpeculativeParams(num_draft_tokens=2)), dict(speculative=SpeculativeParams(num_draft_tokens=2, guided=True)),
                   dict(speculative=SpeculativeParams(num_draft_tokens=2, guided=True), guide=[None, None])):
            outs.append(generate(model, prompts, 6, pool, **kw))
            assert not made and graphs[-1].guide is None and graphs[-1].guided is None
    finally:
        # instance -> Graph -> __init__ -> its closure -> this list -> instance is a cycle: left alone, the captured graphs inside would
        # be destroyed whenever the cyclic collector runs next, which may be in the middle of another test's capture
        graphs.clear()
    assert outs[0] == outs[1] == outs[2]


def test_guided_speculative_replay_does_not_synchronise():
    from atom_amd.e2e import LogitGuide, SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    K, new = 2, 16
    model, prompts = _get_model(2), _prompts(2)
    autos = [_auto("integer"), _auto("planted2")]
    for sampling in (None, _params("sampled", 2)):
        pool = _spec_pool(prompts, 2, new, K)
        seqs, _, first_logits = _prefill(model, prompts, pool)
        guide = LogitGuide(2, VOCAB, DEV, autos)
        first = guide.mask(first_logits.contiguous()).argmax(-1)
        skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
        sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K, guided=True), sampler=sampling, guide=guide)
        sg.start(prompts, first)
        sg.step()
        sg.step()                                                  # eager warm-up and the capture are allowed to synchronise
        torch.cuda.set_sync_debug_mode("error")
        try:
            while sg.steps_done < sg.max_steps:
                sg.step()
            sg.commit()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        skv.close()
        assert guide.status_bits() == 0 and sg.n_out.tolist() == [new] * 2
        for auto, row in zip(autos, sg.tokens.tolist()):
            assert _in_language(auto, row[:new])
        for c in seqs:
            c.release()
