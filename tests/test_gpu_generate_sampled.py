"""GPU tests of sampled generation: generate(..., sampling=) and DecodeGraph(..., sampler=) on the tiny models, prompts and pools of
tests/test_gpu_generate.py (and one Mixtral and one LoRA model of their own test files), 41 new tokens.  Every comparison is EXACT:
the replayed step runs the eager step's kernels on the eager step's inputs, and the sampler's token is a function of the logits'
bits, the parameters, the seed and the step (tests/sample_ref.py).  The eager side sets ``max_pages`` as that file does."""
import pytest
import torch

from tests import sample_ref
from tests.test_gpu_generate import NEW, SEED, _kv_heads, _model, _pages, _pool, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _params(batch):
    from atom_amd.e2e import SamplingParams
    return [SamplingParams(1.0, 0, 1.0, 11), SamplingParams(0.8, 50, 0.9, 2 ** 40 + 3), SamplingParams(0.0, 0, 1.0, 5),
            SamplingParams(1.5, 0, 0.5, 7), SamplingParams(0.3, 2, 1.0, 2 ** 63 + 1)][:batch]


def _eager_sampled(model, prompts, pool, params, new, cap):
    """the loop a user writes: eager prefill, ops.sample with step 0 on the prompts' last rows, then per token acquire_one, a new
    BatchedKvCacheInt4, one forward, ops.sample with the token's number as the step: (sequences, tokens [new, batch], logits)"""
    from atom_amd import ops
    from atom_amd.e2e import Sampler
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    s = Sampler(len(prompts), DEV, params)
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
        ids = ops.sample(logits, s.temperature, s.top_k, s.top_p, s.seeds, step_offset=i)
        toks.append(ids)
        logs.append(logits)
    return seqs, torch.stack(toks), torch.stack(logs)


def _reference_tokens(logits, params):
    """sample_ref on kept logits [new, batch, vocab]: one list of tokens per sequence"""
    T, K, P, S = ([getattr(q, f) for q in params] for f in ("temperature", "top_k", "top_p", "seed"))
    rows = [sample_ref.sample(logits[i], T, K, P, S, step=i) for i in range(logits.size(0))]
    return [list(r) for r in zip(*rows)]


def _cap(prompts, new=NEW):
    return max(-(-(len(p) + new - 1) // 16) for p in prompts)


def _generate(model, prompts, heads, sampling, new=NEW, **kw):
    from atom_amd.e2e import generate
    pool = _pool(2, heads, _pages([len(p) for p in prompts], 16, new) + 2, 16)
    return generate(model, prompts, new, pool, return_logits=True, sampling=sampling, **kw)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kv_heads):
        if kv_heads not in cache:
            cache[kv_heads] = _model(kv_heads, SEED[kv_heads])
        return cache[kv_heads]
    return get


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("kv_heads", [None, 2])
def test_sampled_generate_equals_the_eager_loop_and_the_reference(models, kv_heads, batch):
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    model, prompts, params = models(kv_heads), _prompts(batch), _params(batch)
    capacity = _pages([len(p) for p in prompts], 16, NEW) + 2
    pe = _pool(2, _kv_heads(kv_heads), capacity, 16)
    se, toks, logs = _eager_sampled(model, prompts, pe, params, NEW, _cap(prompts))
    pg = _pool(2, _kv_heads(kv_heads), capacity, 16)
    free = pg.num_free_blocks
    caches = [KvCacheInt4(pg, 0) for _ in prompts]
    got_tokens, got_logits = generate(model, prompts, NEW, pg, caches=caches, return_logits=True, sampling=params)
    assert got_tokens == toks.t().tolist()
    assert got_logits.shape == logs.shape and torch.equal(got_logits.view(torch.int16), logs.view(torch.int16))
    assert got_tokens == _reference_tokens(got_logits, params)
    assert [c.seqlen for c in caches] == [len(p) + NEW - 1 for p in prompts] == [c.seqlen for c in se]
    for c in caches:
        c.release()
    assert pg.num_free_blocks == free
    print("distinct tokens per sequence:", [len(set(row)) for row in got_tokens])


def test_temperature_zero_is_greedy_where_the_maximum_is_unique(models):
    from atom_amd.e2e import SamplingParams
    model, prompts = models(None), _prompts(5)
    greedy, greedy_logits = _generate(model, prompts, 4, None)
    cold, cold_logits = _generate(model, prompts, 4, SamplingParams(temperature=0.0, seed=3))
    checked = 0
    for b in range(len(prompts)):
        for i in range(NEW):                                 # a sequence is compared until a tied maximum lets the two rules part
            assert torch.equal(cold_logits[i, b], greedy_logits[i, b])
            row = greedy_logits[i, b].float()
            if int((row == row.max()).sum()) != 1:
                break
            assert cold[b][i] == greedy[b][i]
            checked += 1
    print("tokens compared:", checked, "of", NEW * len(prompts))
    assert checked >= NEW


def test_seeds_separate_the_sequences_and_repeat(models):
    """sequence 1's seed does not reach sequence 0; equal seeds give equal runs; T = 1 over 41 steps is not the greedy run"""
    from atom_amd.e2e import SamplingParams
    model, prompts = models(2), _prompts(2)
    a = [SamplingParams(1.0, 0, 1.0, 21), SamplingParams(1.0, 0, 1.0, 22)]
    b = [a[0], SamplingParams(1.0, 0, 1.0, 23)]
    ta, la = _generate(model, prompts, 2, a)
    tb, _ = _generate(model, prompts, 2, b)
    ta2, la2 = _generate(model, prompts, 2, a)
    greedy, _ = _generate(model, prompts, 2, None)
    assert ta[0] == tb[0] and ta[1] != tb[1]
    assert ta == ta2 and torch.equal(la.view(torch.int16), la2.view(torch.int16))
    assert ta[0] != greedy[0] and ta[1] != greedy[1]
    one, _ = _generate(model, prompts, 2, SamplingParams(1.0, 0, 1.0, 21))      # one SamplingParams serves every prompt
    assert one[0] == ta[0]


def test_replay_loop_with_a_sampler_does_not_synchronise(models):
    from atom_amd.e2e import DecodeGraph, SamplingParams
    from atom_amd.utils import StaticBatchedKvCacheInt4
    from tests.test_gpu_generate import _prefill
    model, prompts, steps = models(2), _prompts(2), 20
    params = [SamplingParams(1.0, 40, 0.95, 4), SamplingParams(0.7, 0, 1.0, 2 ** 33)]
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    dg = DecodeGraph(model, skv, steps, keep_logits=True, sampler=params)
    dg.input_ids.copy_(first)
    dg.step()
    dg.step()                                                # eager warm-up and the capture are allowed to synchronise
    for upto, swap in ((steps - 5, False), (steps, True)):
        if swap:
            dg.sampler.set(params[::-1])                     # between replays: copies from the host into the fixed buffers
        torch.cuda.set_sync_debug_mode("error")
        try:
            while dg.steps_done < upto:
                dg.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    skv.close()
    assert skv.seqlens == [len(p) + steps for p in prompts]
    T, K, P, S = ([getattr(q, f) for q in params] for f in ("temperature", "top_k", "top_p", "seed"))
    for i in range(steps):                                   # step i of the graph is draw i + 1; the last five with the parameters swapped
        sw = slice(None, None, -1) if i >= steps - 5 else slice(None)
        assert dg.tokens[i].tolist() == sample_ref.sample(dg.logits[i], T[sw], K[sw], P[sw], S[sw], step=i + 1), i


def test_mixtral_generates_with_sampling():
    from tests import test_gpu_moe as moe
    from atom_amd.e2e import SamplingParams
    from atom_amd.utils import KvCacheInt4
    model, prompts, new = moe._model(), moe._prompts(2), moe.NEW
    params = [SamplingParams(1.0, 0, 0.9, 8), SamplingParams(0.6, 20, 1.0, 9)]
    capacity = _pages([len(p) for p in prompts], 16, new) + 2
    _, toks, logs = _eager_sampled(model, prompts, _pool(2, 2, capacity, 16), params, new, _cap(prompts, new))
    got_tokens, got_logits = _generate(model, prompts, 2, params, new=new)
    assert got_tokens == toks.t().tolist() == _reference_tokens(got_logits, params)
    assert torch.equal(got_logits.view(torch.int16), logs.view(torch.int16))


def test_lora_model_generates_with_sampling():
    from tests import test_gpu_lora_model as lm
    from atom_amd.e2e import SamplingParams, generate
    _, lora = lm._models(None)
    mgr = lm._manager(None)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, lm.VOCAB, (n,), generator=g).tolist() for n in lm.PROMPT_LENS]
    params = [SamplingParams(1.0, 0, 1.0, 31), SamplingParams(2.0, 10, 0.8, 32)]
    lora.set_adapters((1, -1), mgr)
    try:
        _, toks, logs = _eager_sampled(lora, prompts, lm._pool(None), params, lm.NEW, _cap(prompts, lm.NEW))
        got_tokens, got_logits = generate(lora, prompts, lm.NEW, lm._pool(None), return_logits=True, sampling=params)
        assert got_tokens == toks.t().tolist() == _reference_tokens(got_logits, params)
        assert torch.equal(got_logits.view(torch.int16), logs.view(torch.int16))
    finally:
        lora.set_adapters(None)
