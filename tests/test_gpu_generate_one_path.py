"""GPU tests of what the three graph classes and generate() share (atom_amd/e2e/generate.py): the step after ``max_steps`` raises
``RuntimeError`` naming the class it was called on, and generate() with sampling, penalties, a guide and log-probabilities at once --
the one path where the token choice runs with every stage on, eagerly for the first token and inside the replayed step.  The model is
the tiny two-layer one of tests/test_gpu_generate.py; the all-features run uses a vocabulary of 1003, no multiple of 8: the logits'
rows are not 16-byte aligned, the kernels' scalar tails run and the static buffers are views of padded ones.  Every comparison is exact
(tests/penalty_ref.py, guide_ref.py, sample_ref.py), the log-probabilities as tests/logprob_ref.py allows."""
import numpy as np
import pytest
import torch

from tests import guide_ref, logprob_ref, penalty_ref, sample_ref
from tests.test_gpu_generate import SEED, _cfg, _model, _pages, _pool, _prefill, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def model():
    return _model(2, SEED[2])


# ------------------------------------------------------------------------------------------------ the step after the last
def test_decode_graph_names_itself_after_its_last_step(model):
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    prompts, steps = _prompts(2), 3
    seqs, first, _ = _prefill(model, prompts, _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16))
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    dg = DecodeGraph(model, skv, steps)
    dg.run(first)                                              # eager, captured and replayed, replayed
    assert dg.steps_done == steps
    with pytest.raises(RuntimeError, match=r"^DecodeGraph: all 3 steps are taken$"):
        dg.step()
    skv.close()
    assert dg.steps_done == steps


def test_spec_decode_graph_names_itself_after_its_last_step(model):
    from atom_amd.e2e import SpecDecodeGraph, SpeculativeParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    prompts, new, K = _prompts(2), 3, 2
    seqs, first, _ = _prefill(model, prompts, _pool(2, 2, _pages([len(p) for p in prompts], 16, new + K) + 2, 16))
    skv = StaticBatchedKvCacheInt4(seqs, reserve=new + K)
    sg = SpecDecodeGraph(model, skv, new, params=SpeculativeParams(num_draft_tokens=K))
    sg.start(prompts, first)
    assert sg.max_steps == new - 1
    sg.step()
    sg.step()
    with pytest.raises(RuntimeError, match=r"^SpecDecodeGraph: all 2 steps are taken$"):
        sg.step()
    sg.commit()
    skv.close()
    assert sg.n_out.tolist() == [new, new] and sg.steps_done == 2


def test_beam_decode_graph_names_itself_after_its_last_step(model):
    from atom_amd import ops
    from atom_amd.e2e import BeamDecodeGraph
    from atom_amd.utils import StaticBeamKvCacheInt4
    prompts, steps, W = _prompts(2), 2, 2
    pool = _pool(2, 2, (W + 1) * _pages([len(p) for p in prompts], 16, steps + 1) + len(prompts) * W + 2, 16)
    seqs, _, first = _prefill(model, prompts, pool)
    _, _, ids, lp = ops.logprob(first.contiguous(), None, W)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    _, token, cum, fin, length = ops.beam_select(ids, lp, torch.zeros(2, dtype=torch.float32, device=DEV), z, z, None, W, w_in=1)
    skv = StaticBeamKvCacheInt4(seqs, W, steps)
    bg = BeamDecodeGraph(model, skv, steps)
    bg.run(token, cum, fin, length)
    with pytest.raises(RuntimeError, match=r"^BeamDecodeGraph: all 2 steps are taken$"):
        bg.step()
    skv.close()
    assert bg.steps_done == steps


# ------------------------------------------------------------------------------------------------ every stage at once
VOCAB, NEW, TOP = 1003, 4, 3
EOS = VOCAB - 1


def _odd_model():
    from atom_amd.e2e import LlamaForCausalLM
    cfg = _cfg(2)
    cfg.vocab_size = VOCAB
    torch.manual_seed(3)
    model = LlamaForCausalLM(cfg).cuda()
    g = torch.Generator().manual_seed(103)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    return model


def _reference(raw, prompts, params, guides):
    """the tokens from the raw logits' bits [new, batch, vocab]: per sequence the occurrence words (prompt flags, every token fed back
    counted), penalty_ref, guide_ref's mask at the state the earlier new tokens led to, sample_ref's draw number i"""
    width = max(len(q.logit_bias or ()) for q in params)
    out = []
    for b, (q, auto) in enumerate(zip(params, guides)):
        ids, vals = np.full(width, -1, dtype=np.int32), np.zeros(width, dtype=np.float32)
        for j, (t, v) in enumerate(sorted((q.logit_bias or {}).items())):
            ids[j], vals[j] = t, v
        words = np.zeros(VOCAB, dtype=np.uint16)
        words[prompts[b]] = 0x8000
        mask = guide_ref.mask_from_csr(auto.indptr, auto.edge_tok, -(-VOCAB // 32))
        s, row = auto.start, []
        for i in range(raw.shape[0]):
            if i > 0:
                s, st = guide_ref.advance_one(s, row[-1], auto.indptr, auto.edge_tok, auto.edge_next, auto.num_states, auto.num_edges)
                assert st == 0
                words[row[-1]] = penalty_ref.count_up(words[row[-1]])
            bits, _ = penalty_ref.penalize_row(raw[i, b], words, None, q.repetition_penalty, q.presence_penalty, q.frequency_penalty, ids, vals)
            bits, st = guide_ref.mask_row(bits, s, mask, auto.num_states)
            assert st == 0
            row.append(sample_ref.sample_row(bits, q.temperature, q.top_k, q.top_p, q.seed, i))
        out.append(row)
    return out


def test_sampling_penalties_guide_and_logprobs_at_once():
    from atom_amd.e2e import SamplingParams, TokenAutomaton, generate
    model, prompts = _odd_model(), _prompts(2)
    # row 0: one state that allows every third token and the row's last three (the tail past 1000); row 1: a choice, then EOS for ever
    thirds = TokenAutomaton(1, [(0, t, 0) for t in sorted(set(range(0, VOCAB, 3)) | {1000, 1001, 1002})], 0, VOCAB)
    guides = [thirds, TokenAutomaton.from_sequences([[250, 3], [1001, 700, 41]], EOS, VOCAB)]
    params = [SamplingParams(0.9, 0, 1.0, 5, repetition_penalty=1.3, frequency_penalty=0.4, logit_bias={1001: 4.0, 3: -1.5}),
              SamplingParams(0.7, 40, 0.9, 11, presence_penalty=0.5, logit_bias={250: 1.0})]
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, NEW) + 2, 16)
    tokens, logits, lp = generate(model, prompts, NEW, pool, sampling=params, guide=guides, logprobs=TOP, return_logits=True)
    assert logits.shape == (NEW, 2, VOCAB) and not torch.isnan(logits).any() and all(len(row) == NEW for row in tokens)
    want = _reference(guide_ref.bits_of(logits), prompts, params, guides)
    print("tokens:", tokens, "reference:", want)
    assert [row[0] for row in tokens] == [row[0] for row in want]          # the first token: the eager call in generate()
    assert tokens == want                                                    # ... the eager, the captured and the replayed step
    for row, auto in zip(tokens, guides):                                   # and both rows stay inside their automata
        assert guide_ref.DEAD not in guide_ref.walk(auto.start, row, auto.indptr, auto.edge_tok, auto.edge_next)
    # the log-probabilities describe the RAW rows, whatever was drawn from them
    chosen = torch.tensor(tokens, dtype=torch.int64).t().contiguous()
    flat = lambda x: x.reshape((NEW * 2,) + tuple(x.shape[2:]))
    logprob_ref.assert_matches((flat(lp.token_logprobs), flat(lp.token_ranks), flat(lp.top_ids), flat(lp.top_logprobs)),
                               flat(logits), flat(chosen), TOP)
