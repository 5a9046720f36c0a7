"""INT4 paged KV-cache bookkeeping with the API of the reference's ``punica/utils/kvcache.py`` (KvPoolInt4 :6-55,
KvCacheInt4 :58-98, BatchedKvCacheInt4 :101-128): same class / property / method names and the same tensor layouts, so
code written against the reference's objects runs on these.  Host-side only; the device work is in atom_amd.ops
(init_kv_i4 / append_kv_i4 / batch_decode_i4 -> csrc/kv_i4.hip, batch_prefill_i4 -> csrc/prefill_i4.hip).
``StaticBatchedKvCacheInt4`` (not in the reference) keeps the page tables at fixed device addresses and advances them on the device
(ops.kv_step_i4 -> csrc/kv_step.hip), for decode steps replayed from a captured graph.  ``StaticBeamKvCacheInt4`` is its beam-search
form: several rows per prompt that share full pages and are reordered on the device (ops.kv_beam_fork_i4 -> csrc/beam.hip).
``RollingKvCacheInt4`` is the static cache of a sliding-window model: a ring of pages per sequence, the pages behind the window
released (ops.kv_step_ring_i4 -> csrc/kv_step.hip; the attention ops' ``_ring`` entry points -> csrc/prefill_i4.hip).

Pool layout (reference kvcache.py:17-26, page.cuh:78-110):
    buf    uint8 [capacity, num_layers, 2, num_heads, block_len, head_dim // 2]   packed u4, K at [.., 0, ..], V at [.., 1, ..]
    param  fp16  [capacity, num_layers, 2, num_heads, block_len, 2]              (scale, zero) per token and head
num_heads is the model's K/V head count: num_key_value_heads for a grouped-query model (its query heads share them, ops.batch_decode_i4).
"""
from __future__ import annotations

from typing import Sequence

import torch


class KvPoolInt4:
    def __init__(self, num_layers: int, num_heads: int, head_dim: int, capacity: int, block_len: int,
                 device: torch.device):
        shape = (capacity, num_layers, 2, num_heads, block_len)
        self._buf = torch.empty(shape + (head_dim // 2,), dtype=torch.uint8, device=device)
        self._param = torch.empty(shape + (2,), dtype=torch.float16, device=device)
        self._free = set(range(capacity))

    buf = property(lambda self: self._buf)
    param = property(lambda self: self._param)
    num_layers = property(lambda self: self._buf.shape[1])
    block_len = property(lambda self: self._buf.shape[4])
    num_free_blocks = property(lambda self: len(self._free))

    def alloc_block(self) -> int:
        return self._free.pop()

    def free_block(self, idx: int):
        if not 0 <= idx < self._buf.size(0) or idx in self._free:
            raise AssertionError(f"block {idx} is not an allocated block of this pool")
        self._free.add(idx)


class KvCacheInt4:
    """Pages of ONE sequence."""

    def __init__(self, pool: KvPoolInt4, init_len: int):
        if init_len < 0:
            raise ValueError("init_len must be non-negative")
        self._pool = pool
        self._seqlen = init_len
        self._indicies = [pool.alloc_block() for _ in range(-(-init_len // pool.block_len))]

    pool = property(lambda self: self._pool)
    seqlen = property(lambda self: self._seqlen)
    indicies = property(lambda self: self._indicies)          # (sic) the reference's spelling

    def acquire_one(self):
        """Make room for one more token (a new page when the last one is full)."""
        if self._seqlen % self._pool.block_len == 0 and len(self._indicies) * self._pool.block_len == self._seqlen:
            self._indicies.append(self._pool.alloc_block())
        self._seqlen += 1

    def acquire(self, n: int):
        """Make room for ``n`` more tokens (a chunk of a prefill: n x acquire_one)."""
        if n < 0:
            raise ValueError("n must be non-negative")
        for _ in range(n):
            self.acquire_one()

    def reserve(self, n: int):
        """Allocate the pages that ``n`` more tokens will need, without adding a token: ``acquire_one`` then allocates nothing until
        they are used up.  A sequence holding spare pages must be ``trim()``med before it is handed to ``BatchedKvCacheInt4``, which
        counts every page of the list as part of the sequence."""
        if n < 0:
            raise ValueError("n must be non-negative")
        while len(self._indicies) * self._pool.block_len < self._seqlen + n:
            self._indicies.append(self._pool.alloc_block())

    def trim(self):
        """Return the spare pages (those beyond ceil(seqlen / block_len)) to the pool."""
        keep = -(-self._seqlen // self._pool.block_len)
        for idx in self._indicies[keep:]:
            self._pool.free_block(idx)
        del self._indicies[keep:]

    def release(self):
        for idx in self._indicies:
            self._pool.free_block(idx)
        self._indicies.clear()
        self._seqlen = 0


class BatchedKvCacheInt4:
    """Device-side page tables of a batch of sequences: what the kernels take."""

    def __init__(self, kv: Sequence[KvCacheInt4]):
        assert len(kv) > 0
        pool = kv[0].pool
        assert all(c.pool is pool for c in kv)
        device = pool.buf.device
        counts = [len(c.indicies) for c in kv]
        self.data = pool.buf
        self.param = pool.param
        self.indptr = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=device)
        self.indicies = torch.tensor([i for c in kv for i in c.indicies], dtype=torch.int32, device=device)
        self.last_page_offset = torch.tensor([(c.seqlen - 1) % pool.block_len + 1 for c in kv], dtype=torch.int32,
                                             device=device)
        self.max_pages = max(counts)            # host-side hint for the decode kernel's KV split (not in the reference)
        self.seqlens = [c.seqlen for c in kv]   # host-side lengths: the prefill attention's cached prefixes (not in the reference)

    @property
    def page_size(self):
        return self.data.size(-2)


class StaticBatchedKvCacheInt4:
    """Page tables of a batch at FIXED device addresses, advanced on the device: takes the place of a ``BatchedKvCacheInt4`` in every
    op and module, for a decode loop that replays one captured step.  The pages for ``reserve`` more tokens per sequence are taken
    from the pool up front (``KvCacheInt4.reserve``); ``step()`` is one launch (ops.kv_step_i4) that adds a token to every sequence and
    rebuilds ``indptr`` / ``indicies`` / ``last_page_offset`` in place.  The host does not follow along: ``seqlens`` and the
    sequences' ``seqlen`` are those of construction or of the last ``sync_host()``.  ``max_pages`` is the static row width ``cap`` of
    the page table, so the attention ops size their KV split by the reserve, not by the current lengths.
    While this object is open the sequences hold spare pages: build no ``BatchedKvCacheInt4`` from them before ``close()``."""

    device_lengths = True      # the lengths live on the device: ``seqlens`` is stale between sync_host() calls (read by LlamaAttention)

    def __init__(self, kv: Sequence[KvCacheInt4], reserve: int):
        assert len(kv) > 0
        pool = kv[0].pool
        assert all(c.pool is pool for c in kv)
        assert len({id(c) for c in kv}) == len(kv)
        device = pool.buf.device
        for c in kv:
            c.reserve(reserve)
        self._kv = list(kv)
        batch, cap = len(kv), max(1, max(len(c.indicies) for c in kv))
        self.data = pool.buf
        self.param = pool.param
        self.max_pages = cap
        self.seqlens = [c.seqlen for c in kv]
        # rows padded with the sequence's last page (the device never copies the padding: row_pages bounds every row)
        rows = [list(c.indicies) + [c.indicies[-1] if c.indicies else 0] * (cap - len(c.indicies)) for c in kv]
        self.page_table = torch.tensor(rows, dtype=torch.int32, device=device)
        self.row_pages = torch.tensor([len(c.indicies) for c in kv], dtype=torch.int32, device=device)
        # lengths [2, batch] (double-buffered, atom_kv_step_i4) and the state words in ONE buffer: sync_host() is one copy
        self._dev = torch.tensor(self.seqlens + [0] * batch + [0, 0, 0, 0], dtype=torch.int32, device=device)
        self.lengths = self._dev[:2 * batch]
        self.state = self._dev[2 * batch:]
        self.indptr = torch.zeros(batch + 1, dtype=torch.int32, device=device)
        self.indicies = torch.zeros(batch * cap, dtype=torch.int32, device=device)
        self.last_page_offset = torch.zeros(batch, dtype=torch.int32, device=device)
        self.step(0)

    @property
    def page_size(self):
        return self.data.size(-2)

    def step(self, add: int = 1):
        """One launch on the current stream: every sequence gains ``add`` tokens (0: rebuild the tables only).  Capturable."""
        from .. import ops
        ops.kv_step_i4(self, add)

    def step_rows(self, adds: torch.Tensor, lookahead: int = 0):
        """One launch on the current stream (ops.kv_step_rows_i4): sequence b gains ``adds[b]`` tokens (int32 [batch] on the device)
        and the tables cover ``lookahead`` tentative slots behind that -- the K + 1 tokens a verify step of speculative decoding
        writes, of which the next ``step_rows`` commits the accepted ones.  ``sync_host()`` reads the committed lengths.  Capturable."""
        from .. import ops
        ops.kv_step_rows_i4(self, adds, lookahead)

    def sync_host(self):
        """Read the lengths and the status word back (one copy, the only synchronisation) and bring ``seqlens`` and the sequences'
        ``seqlen`` up to date.  Raises if a sequence ran out of reserved pages (it kept its last legal length) or a stored length was
        out of range; the status word is cleared."""
        batch = len(self._kv)
        host = self._dev.tolist()
        status, parity = host[2 * batch], host[2 * batch + 1] & 1
        self.seqlens = host[parity * batch:(parity + 1) * batch]
        for c, n in zip(self._kv, self.seqlens):
            c._seqlen = n
        if status:
            self.state[0].zero_()
            raise RuntimeError(f"StaticBatchedKvCacheInt4: status {status} (1: a sequence needed more than its reserved pages and was not "
                               f"advanced, 2: a stored length was out of range); lengths now {self.seqlens}")

    def close(self):
        """``sync_host()``, then every sequence returns its spare pages: they are ordinary ``KvCacheInt4`` again."""
        try:
            self.sync_host()
        finally:
            for c in self._kv:
                c.trim()


class RollingKvCacheInt4:
    """The static cache of a sliding-window model: the attributes of ``StaticBatchedKvCacheInt4`` -- every windowed attention op and
    module takes it in its place -- but each sequence holds a RING of ``R = ceil((window - 1 + max_add) / page_size) + 1`` pages however
    long it grows: logical page g (tokens g * page_size ...) lives in slot ``g % R`` of its ``page_table`` row, and ``step(add)``
    (ops.kv_step_ring_i4, one launch) lists the pages the step's new rows still see, in logical order, and writes the position of each
    list's first token to ``kv_start``.  The presence of ``kv_start`` is what sends the attention ops to their ``_ring`` entry points;
    they refuse a call without a window or with one wider than ``window`` (the history behind it is gone).

    ``kv``: prefilled ``KvCacheInt4`` sequences without spare pages.  The constructor returns every page that lies wholly behind the
    window of the current length to the pool, takes fresh ones up to ``R`` per sequence (``RuntimeError`` before anything changes if
    the pool cannot give them), and lays each row out so that logical page g sits in slot g % R.  From then on the sequences' page
    lists are the rings, which no ``KvCacheInt4`` method understands: use the sequences again only after ``close()``.
    ``max_add``: the most tokens one ``step`` may add (1: decode steps; q for chunks of q tokens); ``max_pages = R``."""

    device_lengths = True      # the lengths live on the device: ``seqlens`` is stale between sync_host() calls (read by LlamaAttention)

    def __init__(self, kv: Sequence[KvCacheInt4], window: int, max_add: int = 1):
        assert len(kv) > 0
        pool = kv[0].pool
        assert all(c.pool is pool for c in kv)
        assert len({id(c) for c in kv}) == len(kv)
        if isinstance(window, bool) or int(window) != window or window < 1 or int(max_add) != max_add or max_add < 1:
            raise ValueError(f"window and max_add must be integers >= 1, got {window!r} and {max_add!r}")
        P, device = pool.block_len, pool.buf.device
        assert all(len(c.indicies) == -(-c.seqlen // P) for c in kv), "the sequences must hold no spare pages"
        self.window, self.max_add = int(window), int(max_add)
        R = -(-(self.window - 1 + self.max_add) // P) + 1
        first = [max(0, c.seqlen - self.window) // P for c in kv]           # the first page a step to the current length lists
        need = sum(R - (len(c.indicies) - f) for c, f in zip(kv, first))
        if need > pool.num_free_blocks + sum(first):
            raise RuntimeError(f"RollingKvCacheInt4: {need} more pages needed ({len(kv)} rings of {R}), {pool.num_free_blocks} free in "
                               f"the pool and {sum(first)} behind the window")
        for c, f in zip(kv, first):                                         # every sequence first: the pool may need these pages back
            for idx in c.indicies[:f]:
                pool.free_block(idx)
        rows = []
        for c, f in zip(kv, first):
            live = {g % R: idx for g, idx in enumerate(c.indicies[f:], start=f)}
            rows.append([live[s] if s in live else pool.alloc_block() for s in range(R)])
            c._indicies[:] = rows[-1]                                       # what close() releases
        self._kv = list(kv)
        batch = len(kv)
        self.data = pool.buf
        self.param = pool.param
        self.max_pages = R
        self.seqlens = [c.seqlen for c in kv]
        self.page_table = torch.tensor(rows, dtype=torch.int32, device=device)
        self.row_pages = torch.full((batch,), R, dtype=torch.int32, device=device)
        self._dev = torch.tensor(self.seqlens + [0] * batch + [0, 0, 0, 0], dtype=torch.int32, device=device)
        self.lengths = self._dev[:2 * batch]
        self.state = self._dev[2 * batch:]
        self.indptr = torch.zeros(batch + 1, dtype=torch.int32, device=device)
        self.indicies = torch.zeros(batch * R, dtype=torch.int32, device=device)
        self.last_page_offset = torch.zeros(batch, dtype=torch.int32, device=device)
        self.kv_start = torch.zeros(batch, dtype=torch.int32, device=device)
        self.step(0)

    @property
    def page_size(self):
        return self.data.size(-2)

    def step(self, add: int = 1):
        """One launch on the current stream: every sequence gains ``add`` tokens (0: rebuild the tables only), at most ``max_add``.
        Capturable."""
        if int(add) > self.max_add:
            raise ValueError(f"RollingKvCacheInt4: a step of {add} tokens on rings sized for max_add={self.max_add}")
        from .. import ops
        ops.kv_step_ring_i4(self, add)

    def sync_host(self):
        """Read the lengths and the status word back (one copy, the only synchronisation) and bring ``seqlens`` and the sequences'
        ``seqlen`` up to date.  Raises if a sequence's live pages outgrew its ring (it kept its last legal length) or a stored length
        was out of range; the status word is cleared."""
        batch = len(self._kv)
        host = self._dev.tolist()
        status, parity = host[2 * batch], host[2 * batch + 1] & 1
        self.seqlens = host[parity * batch:(parity + 1) * batch]
        for c, n in zip(self._kv, self.seqlens):
            c._seqlen = n
        if status:
            self.state[0].zero_()
            raise RuntimeError(f"RollingKvCacheInt4: status {status} (1: a sequence needed more live pages than its ring holds and was "
                               f"not advanced, 2: a stored length was out of range); lengths now {self.seqlens}")

    def close(self):
        """``sync_host()``, then every sequence is RELEASED: its history has lost its head, which no ``KvCacheInt4`` can describe."""
        try:
            self.sync_host()
        finally:
            for c in self._kv:
                c.release()


class StaticBeamKvCacheInt4:
    """The static cache of a beam search: ``num_beams`` rows per prompt (row g * W + b is beam b of prompt g, ``groups`` prompts), with
    the attributes of ``StaticBatchedKvCacheInt4`` -- every attention op and ``ops.kv_step_i4`` take it unchanged -- plus ``fork(parent)``
    (ops.kv_beam_fork_i4): row r continues the history of row ``parent[r]`` of its group, on the device.  Full pages are shared between
    rows by reference; only the one partial page is ever copied, into the row's ``spare`` page.

    ``prompt_seqs`` hold the prefilled prompts (no spare pages).  Per row the constructor takes from the pool the pages from the
    prompt's partial-page position to the end of ``reserve`` more tokens (beam 0 starts in the prompt's own last page, so one fewer
    where that page is partial) and one spare; if the pool cannot give them all it raises before keeping any.  Every row is pointed at
    its prompt's pages, then one ``fork`` with every parent 0: beam 0 keeps appending into the prompt's own last page, the other beams
    get copies.  From then on pages change rows on the device; the host tracks only the SET it allocated, and ``close()`` returns
    exactly that set.  The prompt sequences keep their page lists and lengths, but the contents of a prompt's partial last page are
    consumed by the search: release the prompt sequences after ``close()``, not before.

    ``page_table`` / ``spare`` are views of one buffer ``tables`` and ``table_out`` / ``spare_out`` of ``tables_out``: a fork gathers
    from the first into the second and copies back in one device-to-device copy."""

    def __init__(self, prompt_seqs: Sequence[KvCacheInt4], num_beams: int, reserve: int):
        assert len(prompt_seqs) > 0 and 1 <= int(num_beams) <= 16 and reserve >= 0
        pool = prompt_seqs[0].pool
        assert all(c.pool is pool for c in prompt_seqs)
        assert len({id(c) for c in prompt_seqs}) == len(prompt_seqs)
        P, W, device = pool.block_len, int(num_beams), pool.buf.device
        assert all(len(c.indicies) == -(-c.seqlen // P) for c in prompt_seqs), "prompt sequences must hold no spare pages"
        self.groups, self.num_beams = len(prompt_seqs), W
        row_pages = [max(1, -(-(c.seqlen + reserve) // P)) for c in prompt_seqs]
        # pages a row needs of its own: from the prompt's partial-page position on (beam 0: from behind the prompt's pages), one spare
        need = [[n - (len(c.indicies) if b == 0 else c.seqlen // P) + 1 for b in range(W)] for c, n in zip(prompt_seqs, row_pages)]
        total = sum(sum(x) for x in need)
        if total > pool.num_free_blocks:
            raise RuntimeError(f"StaticBeamKvCacheInt4: {total} pages needed ({self.groups} prompts x {W} beams, reserve {reserve}), "
                               f"{pool.num_free_blocks} free in the pool")
        self._pool = pool
        self._pages = [pool.alloc_block() for _ in range(total)]     # the set close() returns
        fresh = iter(self._pages)
        batch, cap = self.groups * W, max(row_pages)
        rows, spare = [], []
        for c, n, per_beam in zip(prompt_seqs, row_pages, need):
            for b in range(W):
                own = [next(fresh) for _ in range(per_beam[b])]
                spare.append(own.pop())
                row = list(c.indicies[:n - len(own)]) + own
                rows.append(row + [row[-1]] * (cap - n))              # padding: never read (row_pages bounds every row)
        self.data = pool.buf
        self.param = pool.param
        self.max_pages = cap
        self.seqlens = [c.seqlen for c in prompt_seqs for _ in range(W)]
        self.tables = torch.tensor([i for r in rows for i in r] + spare, dtype=torch.int32, device=device)
        self.tables_out = torch.zeros_like(self.tables)
        self.page_table, self.spare = self.tables[:batch * cap].view(batch, cap), self.tables[batch * cap:]
        self.table_out, self.spare_out = self.tables_out[:batch * cap].view(batch, cap), self.tables_out[batch * cap:]
        self.row_pages = torch.tensor([n for n in row_pages for _ in range(W)], dtype=torch.int32, device=device)
        self._dev = torch.tensor(self.seqlens + [0] * batch + [0, 0, 0, 0], dtype=torch.int32, device=device)
        self.lengths = self._dev[:2 * batch]
        self.state = self._dev[2 * batch:]
        self.indptr = torch.zeros(batch + 1, dtype=torch.int32, device=device)
        self.indicies = torch.zeros(batch * cap, dtype=torch.int32, device=device)
        self.last_page_offset = torch.zeros(batch, dtype=torch.int32, device=device)
        self.fork(torch.zeros(batch, dtype=torch.int32, device=device))
        self.step(0)

    @property
    def page_size(self):
        return self.data.size(-2)

    def step(self, add: int = 1):
        """One launch on the current stream: every row gains ``add`` tokens (0: rebuild the tables only).  Capturable."""
        from .. import ops
        ops.kv_step_i4(self, add)

    def fork(self, parent: torch.Tensor):
        """Row r continues row ``parent[r]`` (int32 [groups * num_beams] on the device, the row inside the group) of its group:
        ops.kv_beam_fork_i4.  The next ``step()`` rebuilds the tables the attention ops read.  Capturable."""
        from .. import ops
        ops.kv_beam_fork_i4(self, parent)

    def sync_host(self):
        """Read the lengths and the status word back (one copy, the only synchronisation) into ``seqlens``.  Raises if a row ran out of
        reserved pages, a stored length was out of range, or a fork met a parent outside its group or a page outside the pool (the
        row was kept as it was); the status word is cleared."""
        batch = self.groups * self.num_beams
        host = self._dev.tolist()
        status, parity = host[2 * batch], host[2 * batch + 1] & 1
        self.seqlens = host[parity * batch:(parity + 1) * batch]
        if status:
            self.state[0].zero_()
            raise RuntimeError(f"StaticBeamKvCacheInt4: status {status} (1: a row needed more than its reserved pages and was not "
                               f"advanced, 2: a stored length was out of range, 4: a fork's parent was outside its group, 8: a fork met "
                               f"a page id outside the pool); lengths now {self.seqlens}")

    def close(self):
        """``sync_host()``, then every page the constructor took goes back to the pool."""
        try:
            self.sync_host()
        finally:
            for idx in self._pages:
                self._pool.free_block(idx)
            self._pages = []
