"""Greedy token generation by graph replay: ``DecodeGraph`` captures ONE decode step of a ``LlamaForCausalLM`` over a
``StaticBatchedKvCacheInt4`` -- page tables stepped on the device (ops.kv_step_i4), the model's forward, argmax, the token written
back as the next input -- and replays it for every following token; ``generate`` is the loop around it: eager prefill, then replays.
Nothing between two steps touches the host: no page-table upload, no ``.item()``.
"""
from __future__ import annotations

from typing import Sequence

import torch

from ..utils import BatchedKvCacheInt4, BatchLenInfo, KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4


class DecodeGraph:
    """One greedy decode step over ``static_kv``, run up to ``max_steps`` times.

    Static buffers: ``input_ids`` int64 [batch] (the tokens the next step consumes), ``tokens`` int64 [max_steps, batch] (row i: the
    tokens step i produced) and, with ``keep_logits=True``, ``logits`` fp16 [max_steps, batch, vocab]; a device counter indexes the rows.
    A step is ``static_kv.step()`` (every sequence gains a slot, its page tables are rebuilt on the device), the model's forward for
    one token per sequence, ``argmax``.  The first ``step()`` runs eagerly: it builds what a capture cannot -- the fused weight
    operands, the weight-scale pair tags, the workspace.  The second is captured on torch's capture stream (one stream: a single
    chain of launches) and replayed; every later one is a replay.  ``steps_done`` counts on the host; the capacity check is the
    cache's status word (``static_kv.sync_host()``), read after the loop."""

    def __init__(self, model, static_kv: StaticBatchedKvCacheInt4, max_steps: int, *, keep_logits: bool = False):
        assert max_steps >= 1
        self.model, self.kv, self.max_steps = model, static_kv, int(max_steps)
        device = static_kv.data.device
        self.batch = batch = static_kv.last_page_offset.numel()
        self.input_ids = torch.zeros(batch, dtype=torch.int64, device=device)
        self.tokens = torch.zeros((self.max_steps, batch), dtype=torch.int64, device=device)
        self.logits = (torch.zeros((self.max_steps, batch, model.config.vocab_size), dtype=torch.float16, device=device)
                       if keep_logits else None)
        self._counter = torch.zeros(1, dtype=torch.int64, device=device)
        self._blen = BatchLenInfo([], batch, device)
        self._graph = None
        self.steps_done = 0

    @torch.no_grad()
    def _step(self):
        self.kv.step()
        logits, _ = self.model(self.input_ids, self._blen, None, self.kv)
        nxt = logits.argmax(dim=-1)
        self.tokens.index_copy_(0, self._counter, nxt.unsqueeze(0))
        if self.logits is not None:
            self.logits.index_copy_(0, self._counter, logits.unsqueeze(0))
        self.input_ids.copy_(nxt)
        self._counter.add_(1)

    def step(self):
        """The next step: eager the first time, captured and replayed the second, replayed afterwards.  Asynchronous."""
        if self.steps_done >= self.max_steps:
            raise RuntimeError(f"DecodeGraph: all {self.max_steps} steps are taken")
        if self.steps_done == 0:
            self._step()
        else:
            if self._graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):              # a capture records the launches and runs none of them
                    self._step()
                self._graph = graph
            self._graph.replay()
        self.steps_done += 1

    def run(self, first_tokens: torch.Tensor) -> torch.Tensor:
        """Feed ``first_tokens`` [batch] and take every step that is left; returns ``tokens`` [max_steps, batch]."""
        self.input_ids.copy_(first_tokens.reshape(self.batch))
        while self.steps_done < self.max_steps:
            self.step()
        return self.tokens


@torch.no_grad()
def generate(model, prompts: Sequence[Sequence[int]], max_new_tokens: int, pool: KvPoolInt4, *, eos_token_id: int = None,
             caches: Sequence[KvCacheInt4] = None, return_logits: bool = False):
    """Greedy generation for a batch of prompts (lists of token ids): returns one list of new tokens per prompt, cut after its first
    ``eos_token_id``.  The prompts are prefilled eagerly in one forward; the first new token is the argmax of each prompt's last row;
    the other ``max_new_tokens - 1`` come from a ``DecodeGraph`` over a ``StaticBatchedKvCacheInt4`` with that many tokens reserved
    from ``pool``.  All sequences run all steps (stopping is a host-side cut afterwards).
    ``caches``: one ``KvCacheInt4`` of ``pool`` per prompt to generate into (tokens they already hold are a cached prefix of the
    prompt); they are left consistent -- ``seqlen`` counts the prompt and every token that was fed back, no spare pages.  Default:
    fresh caches, released at the end.  ``return_logits``: also return every step's logits, fp16 [max_new_tokens, batch, vocab]."""
    assert max_new_tokens >= 1 and len(prompts) > 0 and all(len(p) > 0 for p in prompts)
    device = pool.buf.device
    seqs = [KvCacheInt4(pool, 0) for _ in prompts] if caches is None else list(caches)
    assert len(seqs) == len(prompts)
    lens = [len(p) for p in prompts]
    for c, n in zip(seqs, lens):
        c.acquire(n)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=device)
    logits, _ = model(ids, BatchLenInfo(lens, 0, device), BatchedKvCacheInt4(seqs), None)
    last = torch.tensor(lens, dtype=torch.int64).cumsum(0).sub_(1).to(device)
    all_logits = logits.index_select(0, last).unsqueeze(0)
    new = all_logits.argmax(dim=-1)                            # [1, batch]
    if max_new_tokens > 1:
        static = StaticBatchedKvCacheInt4(seqs, reserve=max_new_tokens - 1)
        try:
            dg = DecodeGraph(model, static, max_new_tokens - 1, keep_logits=return_logits)
            new = torch.cat([new, dg.run(new[0])])
            if return_logits:
                all_logits = torch.cat([all_logits, dg.logits])
        finally:
            static.close()
    out = []
    for row in new.t().tolist():
        if eos_token_id is not None and eos_token_id in row:
            row = row[:row.index(eos_token_id) + 1]
        out.append(row)
    if caches is None:
        for c in seqs:
            c.release()
    return (out, all_logits) if return_logits else out
