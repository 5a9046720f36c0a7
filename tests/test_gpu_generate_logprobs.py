"""GPU tests of generate(..., logprobs=), DecodeGraph(..., logprobs=), score() and perplexity() on the tiny models, prompts and pools of
tests/test_gpu_generate.py, 41 new tokens: the eager first step, the captured step and the replays.  Log-probabilities, ranks and
top-n are compared with tests/logprob_ref.py on the returned logits (rank and ids exactly, log-probabilities bitwise up to the
contract's one-step allowance on lz); the tokens must be bit-identical to a run without log-probabilities."""
import math

import pytest
import torch

from tests import logprob_ref
from tests.test_gpu_generate import NEW, SEED, _model, _pages, _pool, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def model():
    return _model(2, SEED[2])


def _generate(model, prompts, **kw):
    from atom_amd.e2e import generate
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, NEW) + 2, 16)
    return generate(model, prompts, NEW, pool, return_logits=True, **kw)


def _check_against_the_reference(tokens, logits, lp, n):
    """every step's row of ``lp`` against the reference on that step's logits with the chosen tokens as targets"""
    batch = len(tokens)
    assert lp.token_logprobs.shape == (NEW, batch) and lp.token_logprobs.dtype == torch.float32 and lp.token_logprobs.is_cuda
    assert lp.token_ranks.shape == (NEW, batch) and lp.token_ranks.dtype == torch.int32
    assert lp.top_ids.shape == (NEW, batch, n) and lp.top_ids.dtype == torch.int64 and lp.top_logprobs.shape == (NEW, batch, n)
    chosen = torch.tensor(tokens, dtype=torch.int64).t().contiguous()           # [NEW, batch]
    flat = lambda x: x.reshape((NEW * batch,) + tuple(x.shape[2:]))
    moved = logprob_ref.assert_matches((flat(lp.token_logprobs), flat(lp.token_ranks), flat(lp.top_ids), flat(lp.top_logprobs)),
                                       flat(logits), flat(chosen), n)
    print(f"{NEW * batch} rows, {moved} on a neighbour of lz")
    return chosen


def test_greedy_generate_with_logprobs(model):
    prompts = _prompts(2)
    plain_tokens, plain_logits = _generate(model, prompts)
    tokens, logits, lp = _generate(model, prompts, logprobs=5)
    assert tokens == plain_tokens and torch.equal(logits.view(torch.int16), plain_logits.view(torch.int16))
    chosen = _check_against_the_reference(tokens, logits, lp, 5)
    assert int(lp.token_ranks.abs().max()) == 0
    assert torch.equal(lp.top_ids[..., 0].cpu(), chosen)
    assert torch.equal(lp.top_logprobs[..., 0].view(torch.int32), lp.token_logprobs.view(torch.int32))
    assert bool((lp.top_logprobs[..., :-1] >= lp.top_logprobs[..., 1:]).all()) and float(lp.token_logprobs.max()) <= 0


def test_sampled_generate_with_logprobs(model):
    from atom_amd.e2e import SamplingParams
    prompts = _prompts(2)
    params = [SamplingParams(0.0, 0, 1.0, 3), SamplingParams(1.3, 2, 1.0, 9)]
    plain_tokens, plain_logits = _generate(model, prompts, sampling=params)
    tokens, logits, lp = _generate(model, prompts, sampling=params, logprobs=5)
    assert tokens == plain_tokens and torch.equal(logits.view(torch.int16), plain_logits.view(torch.int16))
    _check_against_the_reference(tokens, logits, lp, 5)
    ranks = lp.token_ranks.cpu()
    assert int(ranks[:, 0].abs().max()) == 0                  # T = 0: ops.sample takes the first token of the order
    assert int(ranks[:, 1].min()) >= 0 and int(ranks[:, 1].max()) < 2
    print("rank-1 draws on the top-2 row:", int(ranks[:, 1].sum()), "of", NEW)
    assert int(ranks[:, 1].sum()) > 0                         # T = 1.3 over 41 steps: not the greedy run


def test_logprobs_zero_and_no_logits(model):
    from atom_amd.e2e import generate
    prompts = _prompts(2)
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, NEW) + 2, 16)
    tokens, lp = generate(model, prompts, NEW, pool, logprobs=0)
    _, _, full = _generate(model, prompts, logprobs=5)
    assert lp.top_ids is None and lp.top_logprobs is None
    assert torch.equal(lp.token_ranks, full.token_ranks) and torch.equal(lp.token_logprobs.view(torch.int32), full.token_logprobs.view(torch.int32))
    one_tokens, one = generate(model, prompts, 1, pool, logprobs=3)             # no decode graph at all: row 0 alone
    assert [t[:1] for t in tokens] == one_tokens and one.top_ids.shape == (1, 2, 3)
    assert torch.equal(one.top_ids, full.top_ids[:1, :, :3])


def test_score_and_perplexity(model):
    from atom_amd.e2e import perplexity, score
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    sequences = [_prompts(2)[1], [17]]                        # 19 tokens and one token
    lens = [len(s) for s in sequences]
    pool = _pool(2, 2, _pages(lens, 16) + 2, 16)
    free = pool.num_free_blocks
    seqs = [KvCacheInt4(pool, n) for n in lens]
    ids = torch.tensor([t for s in sequences for t in s], dtype=torch.int64, device=DEV)
    logits, _ = model(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    for c in seqs:
        c.release()
    assert logits.shape[0] == 20
    got = score(model, sequences, pool, top_n=4)
    assert pool.num_free_blocks == free
    assert [tuple(d["logprob"].shape) for d in got] == [(18,), (0,)] and [tuple(d["top_ids"].shape) for d in got] == [(18, 4), (0, 4)]
    assert got[0]["rank"].dtype == torch.int32 and got[1]["rank"].numel() == 0 and got[1]["top_logprobs"].shape == (0, 4)
    d = got[0]
    targets = torch.tensor(sequences[0][1:], dtype=torch.int64)
    logprob_ref.assert_matches((d["logprob"], d["rank"], d["top_ids"], d["top_logprobs"]), logits[:18], targets, 4)
    # the ignored last rows, through the op itself on the same logits
    from atom_amd import ops
    all_targets = torch.tensor(sequences[0][1:] + [-1, -1], dtype=torch.int64, device=DEV)
    lp, rk, _, _ = ops.logprob(logits, all_targets)
    assert lp[18:].tolist() == [0.0, 0.0] and rk[18:].tolist() == [-1, -1]
    assert torch.equal(lp[:18].view(torch.int32), d["logprob"].view(torch.int32))
    plain = score(model, sequences, pool)
    assert sorted(plain[0]) == ["logprob", "rank"] and torch.equal(plain[0]["logprob"].view(torch.int32), d["logprob"].view(torch.int32))
    want = math.exp(-float(d["logprob"].cpu().double().sum()) / 18)
    ppl = perplexity(model, sequences, pool)
    print("perplexity", ppl)
    assert ppl == want and 1.0 < ppl < float("inf")


def test_decode_graph_without_logprobs_allocates_none_of_the_buffers(model):
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    from tests.test_gpu_generate import _prefill
    prompts = _prompts(2)
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, 4) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=4)
    try:
        dg = DecodeGraph(model, skv, 4)
        assert dg.logprobs is None
        assert dg.token_logprobs is None and dg.token_ranks is None and dg.top_ids is None and dg.top_logprobs is None
        with_lp = DecodeGraph(model, skv, 4, logprobs=0)
        assert with_lp.token_logprobs.shape == (4, 2) and with_lp.token_ranks.dtype == torch.int32 and with_lp.top_ids is None
        assert DecodeGraph(model, skv, 4, logprobs=7).top_logprobs.shape == (4, 2, 7)
    finally:
        skv.close()
