"""Token generation by graph replay: ``DecodeGraph`` captures ONE decode step of a ``LlamaForCausalLM`` over a
``StaticBatchedKvCacheInt4`` -- page tables stepped on the device (ops.kv_step_i4), the model's forward, argmax (or, with a
``Sampler``, ops.sample: temperature / top-k / top-p, one launch), the token written back as the next input -- and replays it for
every following token; ``generate`` is the loop around it: eager prefill, then replays.
Nothing between two steps touches the host: no page-table upload, no ``.item()``, no logits on the host.
With ``logprobs=`` a step also records the chosen token's log-probability, its rank and the top-n alternatives (ops.logprob, one more
launch on the same logits); ``score`` / ``perplexity`` run given sequences through one prefill and one ops.logprob.
``beam_search`` / ``BeamDecodeGraph`` are the beam-search form of the same loop: ops.logprob's top-n, ops.beam_select and the device-side
fork of a ``StaticBeamKvCacheInt4`` inside the replayed step.
``SpecDecodeGraph`` / ``generate(speculative=)`` spend a step's nearly free rows on speculative decoding: n-gram drafts, one verify forward
over K + 1 positions per sequence, accept and commit on the device (ops.spec_draft_ngram, ops.spec_accept, ops.kv_step_rows_i4;
DESIGN.md 4.17).
``DecodeGraph(guide=)`` / ``generate(guide=)`` restrict every sequence's next token to what a token automaton (``e2e/guide.py``) allows in
the state its own output has led to: ops.guide_advance and ops.guide_mask, two more launches of the replayed step.
``SpecDecodeGraph(guide=)`` / ``generate(guide=, speculative=SpeculativeParams(guided=True))`` do both at once: ops.guide_walk_rows gives
every verify row a state of its own and writes the drafts a state forces, ops.guide_mask masks the batch * (K + 1) rows.
``SpecDecodeGraph(penalties=)`` / ``generate(sampling=, speculative=SpeculativeParams(penalised=True))`` penalise every verify row as if
the drafts in front of it had been emitted and count what a step emitted on the device: ops.penalize_rows, one launch.
``generate(rolling_kv=True)`` runs a sliding-window model over a ``RollingKvCacheInt4``: a ring of pages per sequence, advanced inside the
replayed step (ops.kv_step_ring_i4), so the pages a sequence holds do not grow with the tokens it generates.
"""
from __future__ import annotations

import dataclasses
from typing import Mapping, Sequence, Union

import torch

from .. import ops
from ..utils import (BatchedKvCacheInt4, BatchLenInfo, KvCacheInt4, KvPoolInt4, RollingKvCacheInt4, StaticBatchedKvCacheInt4,
                     StaticBeamKvCacheInt4)
from .guide import LogitGuide, TokenAutomaton


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """How one sequence draws its tokens (ops.sample): ``temperature`` <= 0 is greedy, ``top_k`` outside 1 .. vocab - 1 and
    ``top_p`` >= 1 are off, ``seed`` is any 64-bit integer.  Token i of a sequence is draw number i of its seed: the stream is a
    function of the seed and the logits alone, whatever the batch around it.
    What the sequence is drawn FROM (ops.penalize, in front of ops.sample): ``repetition_penalty`` divides the positive and multiplies
    the other logits of every token of the prompt or generated so far (<= 0 and 1 are off), ``presence_penalty`` is subtracted once
    from, ``frequency_penalty`` once per occurrence of, every token generated so far (the prompt does not count), ``logit_bias`` maps
    token ids to a float added last (``-inf`` bans a token); at most 512 entries."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Mapping[int, float] = None

    @property
    def penalises(self) -> bool:
        """False when the four penalty fields change no logit (the neutral row of ops.penalize)"""
        rep = float(self.repetition_penalty)
        return not ((not rep > 0 or rep == 1.0) and float(self.presence_penalty) == 0 and float(self.frequency_penalty) == 0
                    and not self.logit_bias)


@dataclasses.dataclass
class TokenLogprobs:
    """What ``generate(..., logprobs=n)`` records per new token, device tensors with one row per token: ``token_logprobs`` float32
    [tokens, batch] and ``token_ranks`` int32 [tokens, batch] of the chosen token (rank 0: the greedy token) and, for n >= 1,
    ``top_ids`` int64 / ``top_logprobs`` float32 [tokens, batch, n], the n most probable tokens in order (else None)."""
    token_logprobs: torch.Tensor
    token_ranks: torch.Tensor
    top_ids: torch.Tensor = None
    top_logprobs: torch.Tensor = None


def _check_logprobs(logprobs):
    if logprobs is not None and not 0 <= int(logprobs) <= ops.LOGPROB_MAX_TOP:
        raise ValueError(f"logprobs must be None or 0 .. {ops.LOGPROB_MAX_TOP}, got {logprobs}")
    return None if logprobs is None else int(logprobs)


def _params_list(params, batch: int = None) -> list:
    """One ``SamplingParams`` or one per sequence, as a list; with ``batch``: one entry per sequence, checked."""
    ps = [params] * (1 if batch is None else batch) if isinstance(params, SamplingParams) else list(params)
    if batch is not None and (len(ps) != batch or not all(isinstance(q, SamplingParams) for q in ps)):
        raise ValueError(f"sampling: one SamplingParams, or one per sequence ({batch})")
    return ps


def _static_rows(rows: int, vocab: int, device) -> torch.Tensor:
    """A static fp16 [rows, vocab] buffer whose rows start on 16 bytes: a view of vocab rounded up to 8 columns"""
    return torch.zeros((rows, -(-vocab // 8) * 8), dtype=torch.float16, device=device)[:, :vocab]


class Sampler:
    """The per-sequence sampling parameters as four ``[batch]`` device buffers at FIXED addresses (``temperature`` float32, ``top_k``
    int32, ``top_p`` float32, ``seeds`` int64), so a captured ``ops.sample`` follows ``set``."""

    def __init__(self, batch: int, device, params: Union[SamplingParams, Sequence[SamplingParams]] = SamplingParams()):
        self.batch = int(batch)
        self.temperature = torch.empty(self.batch, dtype=torch.float32, device=device)
        self.top_k = torch.empty(self.batch, dtype=torch.int32, device=device)
        self.top_p = torch.empty(self.batch, dtype=torch.float32, device=device)
        self.seeds = torch.empty(self.batch, dtype=torch.int64, device=device)
        self.set(params)

    def set(self, params: Union[SamplingParams, Sequence[SamplingParams]]):
        """One ``SamplingParams`` for all sequences or one per sequence, copied into the buffers in place."""
        ps = _params_list(params, self.batch)
        seeds = [int(q.seed) & (2 ** 64 - 1) for q in ps]
        self.temperature.copy_(torch.tensor([float(q.temperature) for q in ps], dtype=torch.float32))
        self.top_k.copy_(torch.tensor([max(min(int(q.top_k), 2 ** 31 - 1), -1) for q in ps], dtype=torch.int32))
        self.top_p.copy_(torch.tensor([float(q.top_p) for q in ps], dtype=torch.float32))
        self.seeds.copy_(torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64))   # the same 64 bits

    def sample(self, logits: torch.Tensor, step: torch.Tensor = None, step_offset: int = 0) -> torch.Tensor:
        """Draw number ``step[0] + step_offset`` of every sequence from ``logits`` fp16 [batch, vocab]; int64 [batch]."""
        return ops.sample(logits, self.temperature, self.top_k, self.top_p, self.seeds, step=step, step_offset=step_offset)


class LogitPenalties:
    """The penalty side of ``SamplingParams`` as device buffers at FIXED addresses, so a captured ``ops.penalize`` follows ``set`` and
    the state it advances itself: ``state`` int16 [batch, vocab rounded up to 8] (per token: the sign bit says it occurs in the
    prompt, the low 15 bits count how often it was generated), ``repetition`` / ``presence`` / ``frequency`` float32 [batch] and the
    bias table ``bias_ids`` int32 / ``bias_vals`` float32 [batch, max_bias], padded with -1 / 0.  ``max_bias`` defaults to the longest
    ``logit_bias`` of ``params``; a later ``set`` must fit it."""

    def __init__(self, batch: int, vocab: int, device, params: Union[SamplingParams, Sequence[SamplingParams]] = SamplingParams(),
                 max_bias: int = None):
        self.batch, self.vocab = int(batch), int(vocab)
        if max_bias is None:
            max_bias = max([len(q.logit_bias or ()) for q in _params_list(params) if isinstance(q, SamplingParams)] or [0])
        if not 0 <= int(max_bias) <= ops.PENALTY_MAX_BIAS:
            raise ValueError(f"logit_bias: at most {ops.PENALTY_MAX_BIAS} entries per sequence, got {max_bias}")
        self.max_bias = int(max_bias)
        self.state = torch.zeros((self.batch, -(-self.vocab // 8) * 8), dtype=torch.int16, device=device)
        self.repetition = torch.empty(self.batch, dtype=torch.float32, device=device)
        self.presence = torch.empty(self.batch, dtype=torch.float32, device=device)
        self.frequency = torch.empty(self.batch, dtype=torch.float32, device=device)
        self.bias_ids = torch.empty((self.batch, self.max_bias), dtype=torch.int32, device=device)
        self.bias_vals = torch.empty((self.batch, self.max_bias), dtype=torch.float32, device=device)
        self.set(params)

    def set(self, params: Union[SamplingParams, Sequence[SamplingParams]]):
        """One ``SamplingParams`` for all sequences or one per sequence, copied into the buffers in place; the state is not touched."""
        ps = _params_list(params, self.batch)
        ids = torch.full((self.batch, self.max_bias), -1, dtype=torch.int32)
        vals = torch.zeros((self.batch, self.max_bias), dtype=torch.float32)
        for b, q in enumerate(ps):
            bias = sorted((int(t), float(v)) for t, v in (q.logit_bias or {}).items())
            if len(bias) > self.max_bias:
                raise ValueError(f"logit_bias: {len(bias)} entries, this LogitPenalties holds {self.max_bias} per sequence")
            if any(not 0 <= t < 2 ** 31 for t, _ in bias):
                raise ValueError("logit_bias: token ids must be 0 .. 2^31 - 1")
            if bias:
                ids[b, :len(bias)] = torch.tensor([t for t, _ in bias], dtype=torch.int32)
                vals[b, :len(bias)] = torch.tensor([v for _, v in bias], dtype=torch.float32)
        self.repetition.copy_(torch.tensor([float(q.repetition_penalty) for q in ps], dtype=torch.float32))
        self.presence.copy_(torch.tensor([float(q.presence_penalty) for q in ps], dtype=torch.float32))
        self.frequency.copy_(torch.tensor([float(q.frequency_penalty) for q in ps], dtype=torch.float32))
        self.bias_ids.copy_(ids)
        self.bias_vals.copy_(vals)

    def reset(self, prompts: Sequence[Sequence[int]]):
        """Every count to zero, the prompt flag on the tokens of ``prompts`` (one list of ids per sequence; ids outside the
        vocabulary are skipped).  Eager torch indexing: it runs once per generation."""
        assert len(prompts) == self.batch
        self.state.zero_()
        rows = [b for b, p in enumerate(prompts) for t in p if 0 <= int(t) < self.vocab]
        cols = [int(t) for p in prompts for t in p if 0 <= int(t) < self.vocab]
        if rows:
            dev = self.state.device
            self.state[torch.tensor(rows, dtype=torch.int64, device=dev), torch.tensor(cols, dtype=torch.int64, device=dev)] = -32768

    def apply(self, logits: torch.Tensor, fed: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
        """``logits`` fp16 [batch, vocab] penalised (ops.penalize, one launch); ``fed`` int64 [batch]: the tokens to count first."""
        has_bias = self.max_bias > 0
        return ops.penalize(logits, self.state, fed, self.repetition, self.presence, self.frequency,
                            self.bias_ids if has_bias else None, self.bias_vals if has_bias else None, out=out)

    def apply_rows(self, logits: torch.Tensor, input_ids: torch.Tensor, commit_tokens: torch.Tensor, commit_counts: torch.Tensor,
                   out: torch.Tensor = None) -> torch.Tensor:
        """The verify rows ``logits`` fp16 [batch * Q, vocab] of a speculative step penalised (ops.penalize_rows, one launch): the
        first ``commit_counts[b]`` of ``commit_tokens[b]`` are counted into ``state`` first, row j of a sequence then sees the drafts
        ``input_ids[b, 1 .. j]`` counted as well; the drafts leave ``state`` as it is."""
        has_bias = self.max_bias > 0
        return ops.penalize_rows(logits, self.state, input_ids, commit_tokens, commit_counts, self.repetition, self.presence,
                                 self.frequency, self.bias_ids if has_bias else None, self.bias_vals if has_bias else None, out=out)

    def commit(self, tokens: torch.Tensor, counts: torch.Tensor):
        """Counts the first ``counts[b]`` (int32 [batch]) of ``tokens[b]`` (int64 [batch, n]) into ``state`` and does nothing else
        (ops.penalize_rows without logits, one launch)."""
        ops.penalize_rows(None, self.state[:, :self.vocab], None, tokens, counts)


def _as_sampler(sampler, batch: int, device):
    """None, a ``Sampler`` of ``batch`` rows, or one built from ``SamplingParams`` (one, or one per sequence)"""
    sampler = sampler if sampler is None or isinstance(sampler, Sampler) else Sampler(batch, device, sampler)
    assert sampler is None or sampler.batch == batch
    return sampler


def _choose_tokens(logits: torch.Tensor, sampler: Sampler, penalties: LogitPenalties, guide: LogitGuide, *, fed: torch.Tensor = None,
                   penalised: torch.Tensor = None, guided: torch.Tensor = None, step: torch.Tensor = None, step_offset: int = 0):
    """The next token of every row of the raw ``logits`` fp16 [batch, vocab], int64 [batch]: penalised (``penalties``: ``fed`` is counted
    first, into the static buffer ``penalised`` if given), then masked (``guide``: in place in the penalised row, else into ``guided``
    if given), then the argmax or, with ``sampler``, draw number ``step[0] + step_offset``.  A stage that is None adds no launch;
    ``logits`` is left as it is (log-probabilities and returned logits describe it)."""
    row = logits
    if penalties is not None:                              # the token fed in is counted, then the row is penalised: one launch
        row = penalties.apply(logits, fed=fed, out=penalised)
    if guide is not None:                                  # what the state does not allow becomes -inf: one launch
        row = guide.mask(row, out=guided if penalties is None else row)
    if sampler is None:
        return row.argmax(dim=-1)
    return sampler.sample(row, step=step, step_offset=step_offset)


class _StepReplay:
    """A step of device work, ``_step()``, run up to ``max_steps`` times by graph replay.  The first ``step()`` runs eagerly: it builds
    what a capture cannot -- the fused weight operands, the weight-scale pair tags, the workspace.  The second is captured on torch's
    capture stream (one stream: a single chain of launches) and replayed; every later one is a replay.  ``steps_done`` counts on the
    host; nothing reaches the host between two steps."""

    def __init__(self, max_steps: int):
        self.max_steps = int(max_steps)
        self._graph = None
        self.steps_done = 0

    def step(self):
        """The next step: eager the first time, captured and replayed the second, replayed afterwards.  Asynchronous."""
        if self.steps_done >= self.max_steps:
            raise RuntimeError(f"{type(self).__name__}: all {self.max_steps} steps are taken")
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


class DecodeGraph(_StepReplay):
    """One decode step over ``static_kv``, run up to ``max_steps`` times: greedy, or sampled with ``sampler`` (a ``Sampler``, or
    ``SamplingParams`` -- one, or one per sequence -- to build ``self.sampler`` from).  Step i (from 0) takes draw number i + 1 of
    every sequence; draw 0 belongs to the token the caller feeds in.  ``self.sampler.set(...)`` between steps changes the parameters
    of the steps that follow, replayed ones included.

    Static buffers: ``input_ids`` int64 [batch] (the tokens the next step consumes), ``tokens`` int64 [max_steps, batch] (row i: the
    tokens step i produced) and, with ``keep_logits=True``, ``logits`` fp16 [max_steps, batch, vocab]; a device counter indexes the rows.
    A step is ``static_kv.step()`` (every sequence gains a slot, its page tables are rebuilt on the device), the model's forward for
    one token per sequence, ``argmax`` (``sampler=None``) or ``ops.sample`` reading the device counter as its step.  ``step()`` runs it
    eagerly, captures it and replays it as ``_StepReplay`` says; the capacity check is the cache's status word
    (``static_kv.sync_host()``), read after the loop.

    ``logprobs``: None is the step above.  0 adds one ops.logprob after the argmax / ops.sample, on the same logits with the chosen
    tokens as targets, and records ``token_logprobs`` float32 / ``token_ranks`` int32 [max_steps, batch]; 1 .. 32 also records the
    top-n, ``top_ids`` int64 / ``top_logprobs`` float32 [max_steps, batch, n].  The values are the model's distribution at T = 1
    without truncation, whatever the sampler's parameters.

    ``penalties`` (a ``LogitPenalties``; needs a sampler): None is the step above, launch for launch.  Otherwise the step counts the
    tokens of ``input_ids`` in ``penalties.state`` and penalises the logits into the static buffer ``penalised`` (ops.penalize, one
    more launch), and ops.sample draws from that.  ``logits`` and the log-probabilities stay those of the raw logits.

    ``guide`` (a ``LogitGuide``): None is the step above, launch for launch.  Otherwise the step first advances every sequence's
    automaton state over ``input_ids`` (ops.guide_advance), and after the forward -- and the penalties, if any -- masks the row with the
    state's allowed set (ops.guide_mask) into the static buffer ``guided``, or in place into ``penalised``; ops.sample or the argmax
    reads the masked row.  ``logits`` and the log-probabilities stay those of the raw logits here too."""

    def __init__(self, model, static_kv: StaticBatchedKvCacheInt4, max_steps: int, *, keep_logits: bool = False, sampler=None,
                 logprobs: int = None, penalties: LogitPenalties = None, guide: LogitGuide = None):
        assert max_steps >= 1
        super().__init__(max_steps)
        self.model, self.kv = model, static_kv
        device = static_kv.data.device
        self.batch = batch = static_kv.last_page_offset.numel()
        self.input_ids = torch.zeros(batch, dtype=torch.int64, device=device)
        self.tokens = torch.zeros((self.max_steps, batch), dtype=torch.int64, device=device)
        self.logits = (torch.zeros((self.max_steps, batch, model.config.vocab_size), dtype=torch.float16, device=device)
                       if keep_logits else None)
        self._counter = torch.zeros(1, dtype=torch.int64, device=device)
        self._blen = BatchLenInfo([], batch, device)
        self.sampler = _as_sampler(sampler, batch, device)
        self.penalties, self.penalised = penalties, None
        if penalties is not None:
            if self.sampler is None:
                raise ValueError("DecodeGraph: penalties need a sampler (temperature = 0 is greedy over the penalised row)")
            assert penalties.batch == batch and penalties.vocab == model.config.vocab_size
            self.penalised = _static_rows(batch, penalties.vocab, device)
        self.guide, self.guided = guide, None
        if guide is not None:
            assert guide.batch == batch and guide.vocab == model.config.vocab_size
            if penalties is None:
                self.guided = _static_rows(batch, guide.vocab, device)
        self.logprobs = n = _check_logprobs(logprobs)
        self.token_logprobs = self.token_ranks = self.top_ids = self.top_logprobs = None
        if n is not None:
            self.token_logprobs = torch.zeros((self.max_steps, batch), dtype=torch.float32, device=device)
            self.token_ranks = torch.zeros((self.max_steps, batch), dtype=torch.int32, device=device)
            if n > 0:
                self.top_ids = torch.zeros((self.max_steps, batch, n), dtype=torch.int64, device=device)
                self.top_logprobs = torch.zeros((self.max_steps, batch, n), dtype=torch.float32, device=device)

    @torch.no_grad()
    def _step(self):
        if self.guide is not None:                         # the token fed in moves every sequence's automaton: one launch
            self.guide.advance(self.input_ids)
        self.kv.step()
        logits, _ = self.model(self.input_ids, self._blen, None, self.kv)
        nxt = _choose_tokens(logits, self.sampler, self.penalties, self.guide, fed=self.input_ids, penalised=self.penalised,
                             guided=self.guided, step=self._counter, step_offset=1)
        self.tokens.index_copy_(0, self._counter, nxt.unsqueeze(0))
        if self.logprobs is not None:
            got = ops.logprob(logits, nxt, self.logprobs)
            for buf, x in zip((self.token_logprobs, self.token_ranks, self.top_ids, self.top_logprobs), got):
                if buf is not None:
                    buf.index_copy_(0, self._counter, x.unsqueeze(0))
        if self.logits is not None:
            self.logits.index_copy_(0, self._counter, logits.unsqueeze(0))
        self.input_ids.copy_(nxt)
        self._counter.add_(1)

    def run(self, first_tokens: torch.Tensor) -> torch.Tensor:
        """Feed ``first_tokens`` [batch] and take every step that is left; returns ``tokens`` [max_steps, batch]."""
        self.input_ids.copy_(first_tokens.reshape(self.batch))
        while self.steps_done < self.max_steps:
            self.step()
        return self.tokens


@dataclasses.dataclass(frozen=True)
class SpeculativeParams:
    """Speculative decoding: every step feeds each sequence its last token and ``num_draft_tokens`` (K, 1 .. 8)
    guessed ones, scores the K + 1 positions in one forward and keeps the longest prefix of guesses the model agrees with, so a step
    emits 1 .. K + 1 tokens.  The shipped drafter looks the sequence's last ``ngram_max`` .. ``ngram_min`` tokens (1 .. 8) up in its own
    history.  ``poll_every``: the loop reads its 4-byte ``done`` word every so many steps -- its only synchronisation.
    ``guided=True`` lets ``generate`` take ``speculative`` together with ``guide`` (without a guide it changes nothing);
    ``force_drafts`` then overwrites a draft that follows an automaton state with a single allowed token by that token.
    ``penalised=True`` lets ``generate`` take ``speculative`` together with the penalty fields of ``SamplingParams`` (DESIGN.md 4.20;
    without such a field it changes nothing): every verify row is penalised as if the drafts in front of it had been emitted.
    ``penalised`` is the last argument of the constructor and an attribute that ``==``, ``hash`` and ``repr`` include, but an init-only
    one: the six fields above, their order and ``dataclasses.astuple`` are what callers of earlier versions unpack, and stay as they
    were (``dataclasses.replace`` therefore wants ``penalised=`` passed again)."""
    num_draft_tokens: int = 4
    ngram_max: int = 3
    ngram_min: int = 1
    poll_every: int = 8
    guided: bool = False
    force_drafts: bool = True
    penalised: dataclasses.InitVar[bool] = False

    def __post_init__(self, penalised=False):
        object.__setattr__(self, "penalised", bool(penalised))                # frozen: the one attribute that is not a field
        if not 1 <= int(self.num_draft_tokens) <= ops.SPEC_MAX_DRAFT:
            raise ValueError(f"num_draft_tokens must be 1 .. {ops.SPEC_MAX_DRAFT}, got {self.num_draft_tokens}")
        if not 1 <= int(self.ngram_min) <= int(self.ngram_max) <= ops.SPEC_MAX_NGRAM:
            raise ValueError(f"n-gram sizes must satisfy 1 <= ngram_min <= ngram_max <= {ops.SPEC_MAX_NGRAM}, "
                             f"got {self.ngram_min} .. {self.ngram_max}")
        if int(self.poll_every) < 1:
            raise ValueError(f"poll_every must be positive, got {self.poll_every}")

    def _key(self):
        return dataclasses.astuple(self) + (self.penalised,)

    def __eq__(self, other):
        return self._key() == other._key() if other.__class__ is self.__class__ else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"{self.__class__.__name__}({', '.join(f'{f.name}={getattr(self, f.name)!r}' for f in dataclasses.fields(self))}, penalised={self.penalised!r})"


@dataclasses.dataclass(frozen=True)
class SpecStats:
    """What ``generate(..., return_spec_stats=True)`` adds: per sequence the drafts accepted and the steps that emitted a token
    (tokens = 1 + accepted + steps; the first token comes from the prefill)."""
    accepted: list
    steps: list


class NgramDrafter:
    """The shipped drafter: ``ops.spec_draft_ngram`` over the sequence's own history (prompt-lookup decoding).  A drafter is any object
    with ``propose(hist, hist_len, n_out, out)`` that writes K drafts per row into ``out`` (int64 [batch, K], a strided view of the
    step's ``input_ids``) with capturable device work only: ``hist`` int32 [batch, hist_cap] / ``hist_len`` int32 [batch] hold the
    prompt and every emitted token, ``n_out`` int32 [batch] counts the emitted ones."""

    def __init__(self, ngram_max: int = 3, ngram_min: int = 1):
        self.ngram_max, self.ngram_min = int(ngram_max), int(ngram_min)

    def propose(self, hist, hist_len, n_out, out):
        ops.spec_draft_ngram(hist, hist_len, out, ngram_max=self.ngram_max, ngram_min=self.ngram_min)


class SpecDecodeGraph(_StepReplay):
    """One speculative step over ``static_kv``, run until every sequence holds ``max_new`` tokens (its budget), as ``DecodeGraph`` runs
    a decode step (``_StepReplay``: eager, captured, replayed).  With Q = K + 1 a step is
      1. ``static_kv.step_rows(adds, lookahead=Q)``: the tokens the last step accepted are committed, Q tentative slots follow them;
      2. ``drafter.propose``: K drafts into columns 1 .. K of ``input_ids`` (column 0 is the last emitted token);
      3. the model's forward over the ``batch * Q`` rows as Q-token prefill requests on the static cache (the verify forward);
      4. ``argmax`` per row, or with ``sampler`` ``ops.sample(..., step=draw, rows_per_seq=Q)``: row j of a sequence takes draw number
         ``n_out + j``, the draw non-speculative sampling takes for that token, so accepting is comparing;
      5. ``ops.spec_accept``: the agreed prefix and the model's own next token go to ``tokens`` and ``hist``, every counter moves.
    Static buffers: ``input_ids`` int64 [batch, Q], ``tokens`` int64 [batch, max_new], ``hist`` int32 [batch, hist_cap] / ``hist_len``,
    ``n_out`` / ``budget`` / ``adds`` int32 [batch], ``draw`` int64 [batch], ``accepted`` / ``steps`` int32 [batch], ``done`` int32 [1].
    ``start`` fills them from the prompts and the first token; ``step()`` never synchronises; ``run()`` replays until ``done``.
    The cache must hold ``max_new + K`` reserved tokens per sequence (see ``generate``).  ``sampler``: a ``Sampler`` (or
    ``SamplingParams``) of ``batch`` rows; its four buffers are expanded Q-fold ONCE here, so a later ``sampler.set`` is not followed.
    ``guide`` (a ``LogitGuide`` whose ``state`` holds the states BEFORE the first tokens): None is the step above,
    launch for launch, with nothing allocated.  Otherwise ``guide.walk_rows`` runs between 2 and 3 -- the last step's ``adds`` committed
    into ``guide.state``, the automaton state behind every row, and with ``params.force_drafts`` the drafts a state forces written over
    the drafter's -- and ``guide.mask_rows`` between 3 and 4 masks the ``batch * Q`` rows, each with its own state, into the static
    buffer ``guided``, which the argmax or ops.sample reads; ``commit()`` also commits the last step's states.
    ``penalties`` (a ``LogitPenalties`` whose ``state`` holds the prompt flags alone; needs a sampler): None is the step
    above, launch for launch, with nothing allocated.  Otherwise ``start`` counts the first tokens, and ``penalties.apply_rows`` runs
    between 3 and 4 (ops.penalize_rows, one launch): the tokens the last step emitted -- the first ``adds`` of its ``_targets`` -- are
    counted into ``penalties.state``, then row j is penalised with drafts 1 .. j counted on top, into the static buffer ``penalised``;
    the guide's mask, if any, then runs in place there (no ``guided`` buffer), and ops.sample reads it.  ``commit()`` also counts the
    last step's tokens."""

    def __init__(self, model, static_kv: StaticBatchedKvCacheInt4, max_new: int, *, params: SpeculativeParams = SpeculativeParams(),
                 drafter=None, sampler=None, guide: LogitGuide = None, penalties: LogitPenalties = None):
        assert max_new >= 2
        super().__init__(int(max_new) - 1)                     # every step emits a token for every unfinished row: the all-rejected bound
        self.model, self.kv, self.max_new, self.params = model, static_kv, int(max_new), params
        device = static_kv.data.device
        self.batch = batch = static_kv.last_page_offset.numel()
        self.K = K = int(params.num_draft_tokens)
        self.Q = Q = K + 1
        self.drafter = NgramDrafter(params.ngram_max, params.ngram_min) if drafter is None else drafter
        self.hist_cap = max(static_kv.seqlens) + self.max_new   # the longest prompt (the cache's lengths at construction) + every new token
        i32 = dict(dtype=torch.int32, device=device)
        self.input_ids = torch.zeros((batch, Q), dtype=torch.int64, device=device)
        self.tokens = torch.zeros((batch, self.max_new), dtype=torch.int64, device=device)
        self.hist = torch.zeros((batch, self.hist_cap), **i32)
        self.hist_len, self.n_out, self.budget, self.adds = (torch.zeros(batch, **i32) for _ in range(4))
        self.accepted, self.steps = torch.zeros(batch, **i32), torch.zeros(batch, **i32)
        self.draw = torch.zeros(batch, dtype=torch.int64, device=device)
        self.done = torch.zeros(1, **i32)
        self._targets = torch.zeros(batch * Q, dtype=torch.int64, device=device)
        self._blen = BatchLenInfo([Q] * batch, 0, device)
        self.sampler = _as_sampler(sampler, batch, device)
        self._sample_rows = None
        if self.sampler is not None:
            s = self.sampler
            self._sample_rows = tuple(t.repeat_interleave(Q) for t in (s.temperature, s.top_k, s.top_p, s.seeds))
        self.penalties, self.penalised = penalties, None
        if penalties is not None:
            if self.sampler is None:
                raise ValueError("SpecDecodeGraph: penalties need a sampler (temperature = 0 is greedy over the penalised row)")
            assert penalties.batch == batch and penalties.vocab == model.config.vocab_size
            self.penalised = _static_rows(batch * Q, penalties.vocab, device)
        self.guide, self.guided = guide, None
        if guide is not None:
            assert guide.batch == batch and guide.vocab == model.config.vocab_size
            guide.rows(Q)
            if penalties is None:
                self.guided = _static_rows(batch * Q, guide.vocab, device)

    def start(self, prompts: Sequence[Sequence[int]], first_tokens: torch.Tensor, budget: Sequence[int] = None):
        """The state after the prefill: ``hist`` = each prompt and its first new token (draw 0), one token emitted.  ``budget``: new
        tokens per sequence, the first included (default ``max_new`` each; at most that)."""
        assert len(prompts) == self.batch and max(len(p) for p in prompts) + self.max_new <= self.hist_cap
        budget = [self.max_new] * self.batch if budget is None else [int(x) for x in budget]
        assert len(budget) == self.batch and all(1 <= x <= self.max_new for x in budget)
        device = self.hist.device
        first = first_tokens.reshape(self.batch).to(torch.int64)
        rows = torch.zeros((self.batch, self.hist_cap), dtype=torch.int32)
        for b, p in enumerate(prompts):
            rows[b, :len(p)] = torch.tensor(list(p), dtype=torch.int32)
        lens = torch.tensor([len(p) for p in prompts], dtype=torch.int64, device=device)
        self.hist.copy_(rows)
        self.hist.scatter_(1, lens.unsqueeze(1), first.to(torch.int32).unsqueeze(1))
        self.hist_len.copy_((lens + 1).to(torch.int32))
        self.tokens.zero_()
        self.tokens[:, 0] = first
        self.input_ids.zero_()
        self.input_ids[:, 0] = first
        self.n_out.fill_(1)
        self.draw.fill_(1)
        self.budget.copy_(torch.tensor(budget, dtype=torch.int32))
        for t in (self.adds, self.accepted, self.steps, self.done):
            t.zero_()
        if self.penalties is not None:                     # the first tokens are counted here; the first step commits nothing more
            self.penalties.commit(first.unsqueeze(1), torch.ones_like(self.adds))
            self._targets.zero_()

    @torch.no_grad()
    def _step(self):
        Q = self.Q
        self.kv.step_rows(self.adds, lookahead=Q)
        self.drafter.propose(self.hist, self.hist_len, self.n_out, self.input_ids[:, 1:])
        if self.guide is not None:                         # last step's commit, every row's state, the forced drafts: one launch
            self.guide.walk_rows(self.adds, self.input_ids, force=bool(self.params.force_drafts))
        logits, _ = self.model(self.input_ids.view(-1), self._blen, self.kv, None)
        if self.penalties is not None:                     # the last step's tokens counted, every row under its own drafts: one launch
            logits = self.penalties.apply_rows(logits, self.input_ids, self._targets.view(self.batch, Q), self.adds, out=self.penalised)
        if self.guide is not None:                         # every row masked with its own state: one launch
            logits = self.guide.mask_rows(logits, out=self.guided if self.penalties is None else logits)
        if self.sampler is None:
            targets = logits.argmax(dim=-1)
        else:
            targets = ops.sample(logits, *self._sample_rows, step=self.draw, rows_per_seq=Q, out=self._targets)
        ops.spec_accept(targets.view(self.batch, Q), self.input_ids, self.n_out, self.budget, self.tokens, self.hist, self.hist_len,
                        self.adds, self.draw, self.accepted, self.steps, self.done)

    def commit(self):
        """After the last step: its accepted tokens become part of the sequences (``step_rows`` without look-ahead; the count is
        zeroed so that a second call commits nothing).  ``static_kv.sync_host()`` / ``close()`` then read prompt + tokens fed back."""
        self.kv.step_rows(self.adds, lookahead=0)
        if self.guide is not None:                         # the last step's accepted tokens move the committed automaton states
            self.guide.walk_rows(self.adds, None)
        if self.penalties is not None:                     # and the counts of the penalty state
            self.penalties.commit(self._targets.view(self.batch, self.Q), self.adds)
        self.adds.zero_()

    def run(self) -> torch.Tensor:
        """Steps until every sequence has its budget -- the ``done`` word is read every ``params.poll_every`` steps, the only
        synchronisation -- and at most ``max_new - 1`` of them, then ``commit()``; returns ``tokens`` [batch, max_new] (row b holds
        ``n_out[b]`` tokens)."""
        poll = int(self.params.poll_every)
        while self.steps_done < self.max_steps:
            self.step()
            if self.steps_done % poll == 0 and self.steps_done < self.max_steps and int(self.done.item()):
                break
        self.commit()
        return self.tokens


# What the features of ``generate`` refuse, in the order the checks fire and a message names them.  "penalties": the penalty fields of
# ``SamplingParams`` that are set, in the order the prompts set them (none of them under ``SpeculativeParams(penalised=True)``).  Of the
# two that ``guide`` refuses a message names the first.
_UNGUIDED = "speculative unless it is SpeculativeParams(guided=True)"
_UNPENALISED = "penalties unless it is SpeculativeParams(penalised=True)"     # a message lists the fields themselves, as "penalties" does
_REFUSES = (("guide", ("num_beams", _UNGUIDED)),
            ("speculative", ("num_beams", "logprobs", "return_logits", "caches", _UNPENALISED)),
            ("num_beams", ("sampling", "logprobs", "return_logits", "caches")),
            ("rolling_kv", ("caches", "num_beams", "speculative")))


def _check_combination(caches, return_logits, sampling, logprobs, num_beams, speculative, drafter, return_spec_stats, guide,
                       rolling_kv=False):
    """Raises ``ValueError`` for the first entry of ``_REFUSES`` that applies (and for a drafter or statistics without ``speculative``)."""
    named = {"guide": guide is not None, "speculative": speculative is not None, "num_beams": num_beams is not None,
             "sampling": sampling is not None, "logprobs": logprobs is not None, "return_logits": bool(return_logits),
             "caches": caches is not None, _UNGUIDED: speculative is not None and not speculative.guided,
             "rolling_kv": bool(rolling_kv)}
    named = {name: [name] * given for name, given in named.items()}          # what a message lists for each name: itself, if given
    used, neutral = named.setdefault("penalties", []), SamplingParams()
    for q in ([] if sampling is None else _params_list(sampling)):
        for field in ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"):
            if isinstance(q, SamplingParams) and q.penalises and getattr(q, field) != getattr(neutral, field) and field not in used:
                used.append(field)
    named[_UNPENALISED] = [] if speculative is not None and speculative.penalised else used
    for feature, others in _REFUSES:
        refused = [name for other in others for name in named[other]] if named[feature] else []
        if refused:
            raise ValueError(f"generate: {feature} does not combine with {', '.join(refused[:1] if feature == 'guide' else refused)}")
        if feature == "speculative" and not named[feature] and (drafter is not None or return_spec_stats):
            raise ValueError("generate: drafter and return_spec_stats need speculative")


def _rolling_window(model) -> int:
    """The one sliding window that every attention layer of ``model`` carries -- what ``generate(rolling_kv=True)`` sizes the rings
    by.  A layer without a window would read a history the rolling cache has released, and layers of different windows would need
    rings of their own: both are a ``ValueError`` that names the layer."""
    layers = [m for m in model.modules() if hasattr(m, "window") and hasattr(m, "layer_idx") and hasattr(m, "rope_kw")]
    if not layers:
        raise ValueError("generate: rolling_kv needs a model with attention layers that carry a sliding window, found none")
    for m in layers:
        if m.window is None:
            raise ValueError(f"generate: rolling_kv needs a sliding window on every attention layer; layer {m.layer_idx} has none "
                             f"(config.sliding_window unset, use_sliding_window False, or a layer_types entry that is not "
                             f"'sliding_attention')")
        if m.window != layers[0].window:
            raise ValueError(f"generate: rolling_kv needs one window for all layers; layer {m.layer_idx} has {m.window}, layer "
                             f"{layers[0].layer_idx} has {layers[0].window}")
    return layers[0].window


def _prefill(model, prompts: Sequence[Sequence[int]], seqs: Sequence[KvCacheInt4], device):
    """The eager prefill of ``prompts`` into ``seqs`` (one cache each, acquired here; releasing them stays with the caller): one forward
    over all of them.  Returns the logits fp16 [tokens, vocab] and the row of each prompt's last token (int64 [batch], on the host)."""
    lens = [len(p) for p in prompts]
    for c, n in zip(seqs, lens):
        c.acquire(n)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=device)
    logits, _ = model(ids, BatchLenInfo(lens, 0, device), BatchedKvCacheInt4(seqs), None)
    return logits, torch.tensor(lens, dtype=torch.int64).cumsum(0).sub_(1)


@torch.no_grad()
def generate(model, prompts: Sequence[Sequence[int]], max_new_tokens: int, pool: KvPoolInt4, *, eos_token_id: int = None,
             caches: Sequence[KvCacheInt4] = None, return_logits: bool = False,
             sampling: Union[SamplingParams, Sequence[SamplingParams]] = None, logprobs: int = None, num_beams: int = None,
             speculative: SpeculativeParams = None, drafter=None, return_spec_stats: bool = False,
             guide: Union[TokenAutomaton, Sequence[TokenAutomaton]] = None, rolling_kv: bool = False):
    """Generation for a batch of prompts (lists of token ids): returns one list of new tokens per prompt, cut after its first
    ``eos_token_id``.  Greedy by default; ``sampling`` -- one ``SamplingParams`` or one per prompt -- draws every token with
    ops.sample instead, on the device: new token i of prompt b is draw number i of its seed, so a prompt's tokens do not depend
    on the prompts beside it (as far as its logits do not).  The penalty fields of ``SamplingParams`` (repetition, presence,
    frequency, ``logit_bias``) change the logits a token is drawn from, on the device (ops.penalize): the prompt's tokens are flagged,
    every new token is counted as it is fed back in.  With all of them at their defaults no state is allocated and no launch added;
    ``return_logits`` and ``logprobs`` always describe the raw logits.
    The prompts are prefilled eagerly in one forward; the first new token is the argmax of each prompt's last row (or draw 0);
    the other ``max_new_tokens - 1`` come from a ``DecodeGraph`` over a ``StaticBatchedKvCacheInt4`` with that many tokens reserved
    from ``pool``.  All sequences run all steps (stopping is a host-side cut afterwards).
    ``caches``: one ``KvCacheInt4`` of ``pool`` per prompt to generate into (tokens they already hold are a cached prefix of the
    prompt); they are left consistent -- ``seqlen`` counts the prompt and every token that was fed back, no spare pages.  Default:
    fresh caches, released at the end.  ``return_logits``: also return every step's logits, fp16 [max_new_tokens, batch, vocab].
    ``logprobs`` (None, or 0 .. 32): a ``TokenLogprobs`` is appended to what is returned -- ``(out, lp)`` or ``(out, all_logits, lp)`` --
    with ``max_new_tokens`` rows of device tensors, row 0 from the prompts' last prefill rows: every new token's log-probability and
    rank and, for n >= 1, the n most probable tokens of its step.  The values describe the model's distribution at T = 1 without
    truncation, whatever ``sampling`` is (a token drawn at another temperature or inside a top-k still gets the probability the
    untempered, untruncated model gives it).  Rows after a prompt's EOS are computed like its tokens: cutting them is the caller's job.
    ``num_beams`` (1 .. 16): beam search instead -- the tokens of ``beam_search``'s best hypothesis per prompt (``length_penalty`` 1), in
    the same shape.  Out of scope with it, refused with ``ValueError``: ``sampling``, ``logprobs``, ``return_logits`` and ``caches``.
    ``num_beams=None`` is the code above, launch for launch.
    ``speculative`` (a ``SpeculativeParams``): prefill and the first token as above (draw 0); the rest comes from a ``SpecDecodeGraph``,
    1 .. K + 1 tokens per replayed step, drafted by ``drafter`` (default: ``NgramDrafter`` with the parameters' n-gram sizes).  The
    tokens are those of the verify forward: greedy rows are its argmax, sampled rows the draws non-speculative sampling would take from
    the same logits.  (A verify row and a one-token step run different kernels, so near-ties of the logits may resolve differently from
    ``speculative=None``.)  The reserve is ``max_new_tokens + K`` tokens per sequence: a sequence commits at most its prompt and the
    ``max_new_tokens - 1`` tokens fed back, and every step -- those a finished sequence idles through included -- addresses K + 1
    tentative slots behind the committed ones, so ``prompt + max_new_tokens - 1 + K + 1`` is the furthest slot and the cache's overflow
    bit is never set by a correct run.  ``return_spec_stats=True`` appends a ``SpecStats`` (per sequence: drafts accepted, steps).
    Out of scope with it, refused with ``ValueError``: ``num_beams``, ``logprobs``, ``return_logits``, ``caches`` and, unless it is
    ``SpeculativeParams(penalised=True)``, the penalty fields of ``SamplingParams``; stopping at EOS stays a host-side cut.  With
    ``penalised=True`` every verify row is penalised as if the drafts in front of it had been emitted (ops.penalize_rows, one launch per
    step, which also counts the tokens the step before emitted): row j sees the state non-speculative decoding has at
    that position, rejected drafts leave no trace.  It combines with ``guided=True``: penalties first, then the mask.
    ``speculative=None`` is the code above, launch for launch.
    ``guide`` (one ``TokenAutomaton`` for every prompt, or a list with one automaton or None per prompt): guided decoding -- every new
    token of a guided prompt is one its automaton allows in the state its earlier new tokens led to (the prompt is not walked).  The
    first token is drawn from the prefill's last rows masked at the start states; the graph's first step then advances over it
    (ops.guide_advance, ops.guide_mask: two launches per step, nothing on the host).  Automata built by ``from_sequences`` /
    ``from_regex`` end in a state that allows only EOS, so after its EOS a guided row emits EOS until the cut.  The status word is read
    once after the loop: a state outside the tables, or a token without an edge (neither occurs in a correct run), raises
    ``RuntimeError``.  Combines with ``caches``, ``sampling`` (penalties first, then the mask), ``logprobs`` and ``return_logits`` (both
    keep describing the raw logits); ``num_beams`` (beam rows change parents) is refused with ``ValueError``, and so is ``speculative``
    unless it is ``SpeculativeParams(guided=True)``: then every verify row is masked with a state of its own (ops.guide_walk_rows, and
    ops.guide_mask over the ``batch * (K + 1)`` rows: two launches per step), a draft that follows a state with a
    single allowed token is replaced by that token (``force_drafts``), and what ``speculative`` refuses stays refused.
    ``guide=None`` is the code above, launch for launch, with nothing allocated.
    ``rolling_kv=True`` (a sliding-window model: every attention layer must carry the same window W, else ``ValueError`` naming the
    layer): the decode loop runs over a ``RollingKvCacheInt4`` in place of the static cache -- ``ceil(W / page) + 1`` pages per sequence
    however many tokens are generated, the ring advanced on the device inside the replayed step (ops.kv_step_ring_i4).
    The prompt is still prefilled into ordinary pages (peak ``ceil(prompt / page)`` pages per sequence); those behind the window go back
    to the pool before the first replayed step.  Same tokens and logits as the default wherever both caches give the attention op the
    same KV split.  Combines with ``sampling``, the penalties, ``logprobs``, ``return_logits`` and ``guide``; refused with
    ``ValueError``: ``caches`` (a cache without its head is no ``KvCacheInt4``), ``num_beams`` and ``speculative``.
    ``rolling_kv=False`` is the code above, launch for launch."""
    _check_combination(caches, return_logits, sampling, logprobs, num_beams, speculative, drafter, return_spec_stats, guide, rolling_kv)
    window = _rolling_window(model) if rolling_kv else None
    if num_beams is not None:
        return [hyps[0].tokens for hyps in beam_search(model, prompts, max_new_tokens, pool, num_beams, eos_token_id=eos_token_id)]
    n_lp = _check_logprobs(logprobs)
    assert max_new_tokens >= 1 and len(prompts) > 0 and all(len(p) > 0 for p in prompts)
    device = pool.buf.device
    seqs = [KvCacheInt4(pool, 0) for _ in prompts] if caches is None else list(caches)
    assert len(seqs) == len(prompts)
    logits, last = _prefill(model, prompts, seqs, device)
    all_logits = logits.index_select(0, last.to(device)).unsqueeze(0)
    sampler = None if sampling is None else Sampler(len(prompts), device, sampling)
    penalties = None
    if sampler is not None and any(q.penalises for q in _params_list(sampling)):
        penalties = LogitPenalties(len(prompts), logits.size(-1), device, sampling)
        penalties.reset(prompts)
    guides = None
    if guide is not None and (isinstance(guide, TokenAutomaton) or any(g is not None for g in guide)):
        guides = LogitGuide(len(prompts), logits.size(-1), device, guide)
    # draw 0; nothing is generated yet: the penalties see the prompt flags alone, the guide's mask is that of the start states
    new = _choose_tokens(all_logits[0], sampler, penalties, guides).unsqueeze(0)     # [1, batch]
    lp = None if n_lp is None else [x if x is None else x.unsqueeze(0) for x in ops.logprob(all_logits[0], new[0], n_lp)]
    stats = None
    if speculative is not None:
        rows, stats = new.t().tolist(), SpecStats([0] * len(prompts), [0] * len(prompts))
        if max_new_tokens > 1:
            static = StaticBatchedKvCacheInt4(seqs, reserve=max_new_tokens + int(speculative.num_draft_tokens))
            try:
                sg = SpecDecodeGraph(model, static, max_new_tokens, params=speculative, drafter=drafter, sampler=sampler,
                                     guide=guides, penalties=penalties if speculative.penalised else None)
                sg.start(prompts, new[0])
                toks, counts = sg.run().tolist(), sg.n_out.tolist()
                rows = [row[:n] for row, n in zip(toks, counts)]
                stats = SpecStats(sg.accepted.tolist(), sg.steps.tolist())
            finally:
                static.close()
        new = None
    elif max_new_tokens > 1:
        static = RollingKvCacheInt4(seqs, window) if rolling_kv else StaticBatchedKvCacheInt4(seqs, reserve=max_new_tokens - 1)
        try:
            dg = DecodeGraph(model, static, max_new_tokens - 1, keep_logits=return_logits, sampler=sampler, logprobs=n_lp,
                             penalties=penalties, guide=guides)
            new = torch.cat([new, dg.run(new[0])])
            if lp is not None:
                rest = (dg.token_logprobs, dg.token_ranks, dg.top_ids, dg.top_logprobs)
                lp = [a if a is None else torch.cat([a, b]) for a, b in zip(lp, rest)]
            if return_logits:
                all_logits = torch.cat([all_logits, dg.logits])
        finally:
            static.close()
    bits = 0 if guides is None else guides.status_bits()       # the one read of the guide's status word
    out = []
    for row in (rows if speculative is not None else new.t().tolist()):
        if eos_token_id is not None and eos_token_id in row:
            row = row[:row.index(eos_token_id) + 1]
        out.append(row)
    if caches is None:
        for c in seqs:
            c.release()
    if bits:
        raise RuntimeError("generate: the guide's status word is " + " | ".join(
            name for name, bit in (("REJECTED", ops.GUIDE_REJECTED), ("BAD_STATE", ops.GUIDE_BAD_STATE)) if bits & bit)
            + ": a token without an edge was emitted, or a state left the tables")
    res = (out, all_logits) if return_logits else (out,)
    if lp is not None:
        res = res + (TokenLogprobs(*lp),)
    if return_spec_stats:
        res = res + (stats,)
    return res if len(res) > 1 else out


@dataclasses.dataclass(frozen=True)
class BeamHypothesis:
    """One result of ``beam_search``: the new ``tokens`` (cut after the first EOS), ``sum_logprob`` -- the FP32 sum of their
    log-probabilities, accumulated on the device -- and ``score`` = sum_logprob / len(tokens) ** length_penalty in float64."""
    tokens: list
    sum_logprob: float
    score: float


def backtrack_beams(parents, tokens, cum, num_beams: int, eos_token_id=None, length_penalty: float = 1.0):
    """The host side of beam search.  ``parents`` / ``tokens``: one list of groups * num_beams entries per step (a parent is the row
    inside its group), ``cum``: the final rows' summed log-probabilities.  Follows every final row back to step 0, cuts the tokens
    after the first ``eos_token_id`` and ranks each group by score descending, then beam index: a list of ``BeamHypothesis`` per group."""
    W, steps = int(num_beams), len(tokens)
    out = []
    for g in range(len(cum) // W):
        hyps = []
        for b in range(W):
            row, toks = b, []
            for t in range(steps - 1, -1, -1):
                toks.append(int(tokens[t][g * W + row]))
                row = int(parents[t][g * W + row])
            toks.reverse()
            if eos_token_id is not None and eos_token_id in toks:
                toks = toks[:toks.index(eos_token_id) + 1]
            s = float(cum[g * W + b])
            hyps.append((BeamHypothesis(toks, s, s / float(len(toks)) ** float(length_penalty)), b))
        out.append([h for h, _ in sorted(hyps, key=lambda hb: (-hb[0].score, hb[1]))])
    return out


class BeamDecodeGraph(_StepReplay):
    """One beam-search step over a ``StaticBeamKvCacheInt4``, run up to ``max_steps`` times, as ``DecodeGraph`` runs a decode step
    (``_StepReplay``: eager, captured, replayed; nothing reaches the host in between).  A step is ``kv.step()``, the
    model's forward on groups * num_beams rows, ``ops.logprob(top_n=num_beams)``, ``ops.beam_select`` (the beams' state ``cum`` float32 /
    ``finished`` int32 / ``length`` int32 [rows] is updated in place), the winners' ``parents`` int32 / ``tokens`` int64 recorded in row
    i of [max_steps, rows] at the device counter, ``kv.fork(parent)`` and the tokens written back as the next input.  The caller sets
    ``input_ids`` and the state from the step after the prefill (``run``)."""

    def __init__(self, model, beam_kv: StaticBeamKvCacheInt4, max_steps: int, *, eos_token_id: int = None):
        assert max_steps >= 1
        super().__init__(max_steps)
        self.model, self.kv = model, beam_kv
        self.eos = -1 if eos_token_id is None else int(eos_token_id)
        device = beam_kv.data.device
        self.num_beams = W = beam_kv.num_beams
        self.batch = batch = beam_kv.groups * W
        if W > model.config.vocab_size:
            raise ValueError(f"{W} beams over a vocabulary of {model.config.vocab_size}")
        self.input_ids = torch.zeros(batch, dtype=torch.int64, device=device)
        self.tokens = torch.zeros((self.max_steps, batch), dtype=torch.int64, device=device)
        self.parents = torch.zeros((self.max_steps, batch), dtype=torch.int32, device=device)
        self.cum = torch.zeros(batch, dtype=torch.float32, device=device)
        self.finished = torch.zeros(batch, dtype=torch.int32, device=device)
        self.length = torch.zeros(batch, dtype=torch.int32, device=device)
        self._parent = torch.zeros(batch, dtype=torch.int32, device=device)
        self._token = torch.zeros(batch, dtype=torch.int64, device=device)
        self._top = (None, None, torch.zeros((batch, W), dtype=torch.int64, device=device),
                     torch.zeros((batch, W), dtype=torch.float32, device=device))
        self._counter = torch.zeros(1, dtype=torch.int64, device=device)
        self._blen = BatchLenInfo([], batch, device)

    @torch.no_grad()
    def _step(self):
        self.kv.step()
        logits, _ = self.model(self.input_ids, self._blen, None, self.kv)
        _, _, top_ids, top_lp = ops.logprob(logits, None, self.num_beams, out=self._top)
        ops.beam_select(top_ids, top_lp, self.cum, self.finished, self.length, self.eos, self.num_beams,
                        out=(self._parent, self._token, self.cum, self.finished, self.length))
        self.parents.index_copy_(0, self._counter, self._parent.unsqueeze(0))
        self.tokens.index_copy_(0, self._counter, self._token.unsqueeze(0))
        self.kv.fork(self._parent)
        self.input_ids.copy_(self._token)
        self._counter.add_(1)

    def run(self, first_tokens: torch.Tensor, cum: torch.Tensor, finished: torch.Tensor, length: torch.Tensor):
        """Feed the winners of the step after the prefill ([rows] each) and take every step that is left; returns ``(parents, tokens)``."""
        self.input_ids.copy_(first_tokens.reshape(self.batch))
        self.cum.copy_(cum)
        self.finished.copy_(finished)
        self.length.copy_(length)
        while self.steps_done < self.max_steps:
            self.step()
        return self.parents, self.tokens


@torch.no_grad()
def beam_search(model, prompts: Sequence[Sequence[int]], max_new_tokens: int, pool: KvPoolInt4, num_beams: int, *,
                eos_token_id: int = None, length_penalty: float = 1.0, num_return: int = 1, return_trace: bool = False):
    """Beam search for a batch of prompts (lists of token ids) with ``num_beams`` (1 .. 16) beams each: per prompt a list of the
    ``num_return`` best ``BeamHypothesis``, best first.  The prompts are prefilled eagerly in one forward, as ``generate`` does; the
    first beams are the ``num_beams`` most probable first tokens (ops.logprob on the prompts' last rows, ops.beam_select with one row
    per group); the other ``max_new_tokens - 1`` steps come from a ``BeamDecodeGraph`` over a ``StaticBeamKvCacheInt4`` reserved from
    ``pool`` (per prompt about num_beams x the pages of the new tokens, plus one spare per beam).  All beams run all steps: a beam that
    produced ``eos_token_id`` is frozen -- it keeps its summed log-probability and competes with it, un-normalised, against the live
    beams.  After the loop one read of the cache's status word, then the host follows ``parents`` / ``tokens`` back,
    cuts every hypothesis after its first EOS and ranks by ``sum_logprob / length ** length_penalty`` (float64), ties by beam index.
    ``return_trace``: also return the search's record ``(parents int32, tokens int64 [max_new_tokens, rows], sum_logprob float32
    [rows])``, rows = prompts x num_beams, as device tensors -- what the host followed back.
    Out of scope: sampling, penalties, log-probability records, returned logits, caller-owned caches, early stopping."""
    W = int(num_beams)
    if not 1 <= W <= ops.BEAM_MAX_BEAMS:
        raise ValueError(f"num_beams must be 1 .. {ops.BEAM_MAX_BEAMS}, got {num_beams}")
    if not 1 <= int(num_return) <= W:
        raise ValueError(f"num_return must be 1 .. num_beams, got {num_return}")
    assert max_new_tokens >= 1 and len(prompts) > 0 and all(len(p) > 0 for p in prompts)
    device, G = pool.buf.device, len(prompts)
    seqs = [KvCacheInt4(pool, 0) for _ in prompts]
    try:
        logits, last = _prefill(model, prompts, seqs, device)
        if W > logits.size(-1):
            raise ValueError(f"{W} beams over a vocabulary of {logits.size(-1)}")
        _, _, top_ids, top_lp = ops.logprob(logits.index_select(0, last.to(device)), None, W)
        zi = torch.zeros(G, dtype=torch.int32, device=device)
        parent, token, cum, finished, length = ops.beam_select(top_ids, top_lp, torch.zeros(G, dtype=torch.float32, device=device), zi, zi,
                                                               eos_token_id, W, w_in=1)
        parents, tokens = parent.unsqueeze(0), token.unsqueeze(0)
        if max_new_tokens > 1:
            kv = StaticBeamKvCacheInt4(seqs, W, reserve=max_new_tokens - 1)
            try:
                bg = BeamDecodeGraph(model, kv, max_new_tokens - 1, eos_token_id=eos_token_id)
                more = bg.run(token, cum, finished, length)
                parents, tokens, cum = torch.cat([parents, more[0]]), torch.cat([tokens, more[1]]), bg.cum
            finally:
                kv.close()                                     # the one sync_host()
        hyps = backtrack_beams(parents.tolist(), tokens.tolist(), cum.tolist(), W, eos_token_id, length_penalty)
    finally:
        for c in seqs:
            c.release()
    hyps = [h[:int(num_return)] for h in hyps]
    return (hyps, (parents, tokens, cum)) if return_trace else hyps


@torch.no_grad()
def score(model, sequences: Sequence[Sequence[int]], pool: KvPoolInt4, *, top_n: int = 0):
    """Teacher-forced log-probabilities of given ``sequences`` (lists of token ids) through the real kernels: one eager prefill of all
    of them into fresh caches of ``pool`` (released afterwards), then one ops.logprob over all rows, the targets being each sequence
    shifted by one (-1, ignored, on its last row).  Returns one dict per sequence: ``logprob`` float32 [len - 1] (of token i + 1 given
    tokens 0 .. i), ``rank`` int32 [len - 1] and, for ``top_n`` >= 1, ``top_ids`` int64 / ``top_logprobs`` float32 [len - 1, top_n];
    device tensors, empty for a sequence of one token.  Out of scope: sequences scored in chunks over a cached prefix -- a sequence
    and its logits ([tokens, vocab] fp16) must fit one prefill."""
    assert len(sequences) > 0 and all(len(s) > 0 for s in sequences)
    device = pool.buf.device
    lens = [len(s) for s in sequences]
    seqs = [KvCacheInt4(pool, 0) for _ in sequences]
    try:
        logits, _ = _prefill(model, sequences, seqs, device)
        targets = torch.tensor([t for s in sequences for t in list(s[1:]) + [-1]], dtype=torch.int64, device=device)
        got = ops.logprob(logits, targets, top_n)
    finally:
        for c in seqs:
            c.release()
    out, at = [], 0
    for n in lens:
        rows = slice(at, at + n - 1)
        d = dict(logprob=got[0][rows], rank=got[1][rows])
        if top_n > 0:
            d.update(top_ids=got[2][rows], top_logprobs=got[3][rows])
        out.append(d)
        at += n
    return out


def perplexity(model, sequences: Sequence[Sequence[int]], pool: KvPoolInt4) -> float:
    """exp(-SUM logprob / SUM (len - 1)) over ``score(model, sequences, pool)``, summed in float64 on the host; at least one sequence
    must have two tokens."""
    import math
    lps = torch.cat([d["logprob"] for d in score(model, sequences, pool)]).cpu().double()
    assert lps.numel() > 0, "perplexity needs a sequence of at least two tokens"
    return math.exp(-float(lps.sum()) / lps.numel())
