"""GPU tests of beam search by graph replay: beam_search / generate(num_beams=) / BeamDecodeGraph on the tiny models, prompts and pools
of tests/test_gpu_generate.py, 41 new tokens on pages of 16.  Every comparison is EXACT: the eager side keeps every beam as an
independent sequence of a second pool and re-materialises each child after every step by copying ALL of its parent's pages, so
nothing is shared; it runs the same forward and ops.logprob and selects with tests/beam_ref.py.  Its host-built cache takes the
static cache's row width as ``max_pages``, so the KV-split count is the same on both sides."""
import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.test_gpu_generate import NEW, SEED, _kv_heads, _model, _pages, _pool, _prefill, _prompts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_EAGER = {}


def _cap(prompts, new=NEW):
    return max(-(-(len(p) + new - 1) // 16) for p in prompts)


def _beam_pool(prompts, heads, W, new=NEW):
    return _pool(2, heads, (W + 1) * _pages([len(p) for p in prompts], 16, new) + len(prompts) * W + 2, 16)


def _eager_beam(kv_heads, batch, W, eos, new=NEW):
    """the loop a user writes without this feature (computed once per case): (parents [new][rows], tokens [new][rows], cum float32 [rows])"""
    key = (kv_heads, batch, W, eos, new)
    if key in _EAGER:
        return _EAGER[key]
    from atom_amd import ops
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    model, prompts = _model(kv_heads, SEED[kv_heads]), _prompts(batch)
    pool, G = _beam_pool(prompts, _kv_heads(kv_heads), W, new), len(prompts)
    seqs, _, first = _prefill(model, prompts, pool)
    _, _, ids, lp = ops.logprob(first.contiguous(), None, W)
    z = np.zeros(G, np.int32)
    parent, token, cum, fin, length = beam_ref.select(ids.cpu().numpy(), lp.cpu().numpy(), np.zeros(G, np.float32), z, z, eos, 1, W)
    parents, tokens = [parent.tolist()], [token.tolist()]
    beams = []
    for c in seqs:
        for _ in range(W):
            s = KvCacheInt4(pool, c.seqlen)
            pool.buf[torch.tensor(s.indicies, device=DEV)] = pool.buf[torch.tensor(c.indicies, device=DEV)]
            pool.param[torch.tensor(s.indicies, device=DEV)] = pool.param[torch.tensor(c.indicies, device=DEV)]
            beams.append(s)
    for _ in range(new - 1):
        for s in beams:
            s.acquire_one()
        kv = BatchedKvCacheInt4(beams)
        kv.max_pages = _cap(prompts, new)
        logits, _ = model(torch.from_numpy(token).to(DEV), BatchLenInfo([], G * W, DEV), None, kv)
        _, _, ids, lp = ops.logprob(logits, None, W)
        parent, token, cum, fin, length = beam_ref.select(ids.cpu().numpy(), lp.cpu().numpy(), cum, fin, length, eos, W, W)
        src = torch.tensor([i for r in range(G * W) for i in beams[r - r % W + int(parent[r])].indicies], device=DEV)
        dst = torch.tensor([i for r in range(G * W) for i in beams[r].indicies], device=DEV)
        pool.buf[dst] = pool.buf[src]                        # the gather is evaluated first: every child is a full copy of its parent
        pool.param[dst] = pool.param[src]
        parents.append(parent.tolist())
        tokens.append(token.tolist())
    _EAGER[key] = (parents, tokens, cum)
    return _EAGER[key]


def _hyps(h):
    return [[(x.tokens, x.sum_logprob, x.score) for x in per_prompt] for per_prompt in h]


def _search(kv_heads, batch, W, eos, new=NEW, **kw):
    from atom_amd.e2e import beam_search
    model, prompts = _model(kv_heads, SEED[kv_heads]), _prompts(batch)
    pool = _beam_pool(prompts, _kv_heads(kv_heads), W, new)
    free = pool.num_free_blocks
    got = beam_search(model, prompts, new, pool, W, eos_token_id=eos, **kw)
    assert pool.num_free_blocks == free                      # the pool's free count is restored
    return got


@pytest.mark.parametrize("kv_heads,W,batch", [(None, 2, 1), (None, 2, 2), (None, 4, 1), (None, 4, 2), (2, 2, 1), (2, 4, 2)])
def test_beam_search_equals_the_eager_loop(kv_heads, W, batch):
    parents, tokens, cum = _eager_beam(kv_heads, batch, W, None)
    distinct = len({t for row in tokens for t in row})
    print("distinct tokens:", distinct, "parent changes:", sum(p != list(range(W)) * batch for p in parents))
    assert distinct >= 8, "the tiny model collapsed: pick another seed for the EAGER loop"
    assert any(p != list(range(W)) * batch for p in parents[1:]), "no beam ever changed its parent in the EAGER loop"
    hyps, (gp, gt, gc) = _search(kv_heads, batch, W, None, num_return=W, return_trace=True)
    assert gt.tolist() == tokens and gp.tolist() == parents
    assert np.array_equal(gc.cpu().numpy().view(np.uint32), cum.view(np.uint32))
    assert _hyps(hyps) == beam_ref.backtrack(parents, tokens, cum, W)


def test_generate_with_one_beam_is_greedy_and_with_more_the_best_hypothesis():
    from atom_amd.e2e import generate
    model, prompts = _model(None, SEED[None]), _prompts(2)
    pool = _beam_pool(prompts, 4, 4)
    free = pool.num_free_blocks
    greedy = generate(model, prompts, NEW, pool)
    assert generate(model, prompts, NEW, pool, num_beams=1) == greedy
    parents, tokens, cum = _eager_beam(None, 2, 4, None)
    assert generate(model, prompts, NEW, pool, num_beams=4) == [h[0][0] for h in beam_ref.backtrack(parents, tokens, cum, 4)]
    assert generate(model, prompts, 1, pool, num_beams=4) == [row[:1] for row in greedy]       # no decode step at all
    assert pool.num_free_blocks == free


def test_an_early_eos_freezes_its_hypothesis_and_the_length_penalty_ranks():
    W, batch = 4, 2
    _, tokens, cum = _eager_beam(None, batch, W, None)
    best = beam_ref.backtrack(_eager_beam(None, batch, W, None)[0], tokens, cum, W)[0][0][0]
    eos = best[5]                                            # a token of the W = 4 run itself: some beam produces it by step 5
    parents, tokens, cum = _eager_beam(None, batch, W, eos)
    want = {lp: beam_ref.backtrack(parents, tokens, cum, W, eos, lp) for lp in (0.0, 1.0, 2.0)}
    lengths = [len(h[0]) for per_prompt in want[1.0] for h in per_prompt]
    print("eos", eos, "hypothesis lengths:", lengths, "distinct tokens:", len({t for row in tokens for t in row}))
    assert min(lengths) < NEW, "no hypothesis finished early in the EAGER loop: pick another eos"
    assert len({t for row in tokens for t in row}) >= 8, "the tiny model collapsed: pick another seed for the EAGER loop"
    for per_prompt in want[1.0]:                             # frozen: a finished hypothesis ends with its eos and holds no token after it
        for toks, _, _ in per_prompt:
            assert eos not in toks[:-1]
    for lp in (0.0, 1.0, 2.0):
        hyps, (gp, gt, gc) = _search(None, batch, W, eos, length_penalty=lp, num_return=W, return_trace=True)
        assert gt.tolist() == tokens and gp.tolist() == parents
        assert np.array_equal(gc.cpu().numpy().view(np.uint32), cum.view(np.uint32))
        assert _hyps(hyps) == want[lp]
    assert _hyps(_search(None, batch, W, eos)) == [per_prompt[:1] for per_prompt in want[1.0]]  # num_return defaults to the best


def test_beam_replay_loop_does_not_synchronise():
    from atom_amd import ops
    from atom_amd.e2e import BeamDecodeGraph
    from atom_amd.utils import StaticBeamKvCacheInt4
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
    W, steps = 4, 20
    model, prompts = _model(2, SEED[2]), _prompts(2)
    pool = _beam_pool(prompts, 2, W, steps + 1)
    seqs, _, first = _prefill(model, prompts, pool)
    _, _, ids, lp = ops.logprob(first.contiguous(), None, W)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    _, token, cum, fin, length = ops.beam_select(ids, lp, torch.zeros(2, dtype=torch.float32, device=DEV), z, z, None, W, w_in=1)
    skv = StaticBeamKvCacheInt4(seqs, W, steps)
    bg = BeamDecodeGraph(model, skv, steps)
    bg.input_ids.copy_(token)
    bg.cum.copy_(cum)
    bg.length.copy_(length)
    bg.step()
    bg.step()                                                # eager warm-up and the capture are allowed to synchronise
    torch.cuda.set_sync_debug_mode("error")
    try:
        while bg.steps_done < steps:
            bg.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    skv.close()
    assert skv.seqlens == [len(p) + steps for p in prompts for _ in range(W)]
    parents, tokens, want_cum = _eager_beam(2, 2, W, None, steps + 1)
    assert bg.tokens.tolist() == tokens[1:] and bg.parents.tolist() == parents[1:]
    assert np.array_equal(bg.cum.cpu().numpy().view(np.uint32), want_cum.view(np.uint32))


def test_generate_refuses_what_beam_search_does_not_cover():
    from atom_amd.e2e import SamplingParams, beam_search, generate
    from atom_amd.utils import KvCacheInt4
    model, prompts = _model(None, SEED[None]), _prompts(1)
    pool = _beam_pool(prompts, 4, 2)
    free = pool.num_free_blocks
    for kw in (dict(sampling=SamplingParams()), dict(logprobs=0), dict(return_logits=True), dict(caches=[KvCacheInt4(pool, 0)])):
        with pytest.raises(ValueError, match="num_beams"):
            generate(model, prompts, 4, pool, num_beams=2, **kw)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            beam_search(model, prompts, 4, pool, bad)
    with pytest.raises(ValueError):
        beam_search(model, prompts, 4, pool, 2, num_return=3)
    assert pool.num_free_blocks == free
