"""Host restatement of beam search (include/atom_hip.h), in numpy and plain Python: ``select`` is atom_beam_select with
the same key and the same order, ``RefBeamCache`` the page bookkeeping of atom_kv_beam_fork_i4 + atom_kv_step_i4 with the tables and
``spare`` as Python lists and the pool's buffers as arrays, ``backtrack`` the host side of ``beam_search``.  Shared by the CPU tests
(which check it against brute force and hand-written orders) and the GPU tests (which check the kernels against it, bit for bit)."""
import numpy as np

BAD_LENGTH, BAD_PARENT, BAD_PAGE = 2, 4, 8


def score_key(s):
    """order-preserving uint32 key of float32 scores: -0 -> +0, NaN -> -inf, then sign-magnitude to unsigned"""
    u = np.asarray(s, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFF800000)
    u[u == np.uint32(0x80000000)] = np.uint32(0)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select(top_ids, top_lp, cum, finished, length, eos, w_in, w_out):
    """(parent int32, token int64, cum float32, finished int32, length int32), [groups * w_out] each"""
    top_ids, top_lp = np.asarray(top_ids, dtype=np.int64), np.asarray(top_lp, dtype=np.float32)
    cum, finished, length = np.asarray(cum, dtype=np.float32), np.asarray(finished, dtype=np.int32), np.asarray(length, dtype=np.int32)
    rows, C = top_ids.shape
    assert rows % w_in == 0 and w_in in (1, w_out) and w_out <= C
    eos = -1 if eos is None else int(eos)
    frozen = max(eos, 0)
    out = ([], [], [], [], [])
    for g in range(rows // w_in):
        cands = []                                            # (key, parent, c): the order is key descending, parent, c ascending
        for b in range(w_in):
            r = g * w_in + b
            if finished[r]:
                cands.append((int(score_key(cum[r])[0]), b, 0))
            else:
                scores = (cum[r] + top_lp[r]).astype(np.float32)          # one FP32 addition each
                cands += [(int(k), b, c) for c, k in enumerate(score_key(scores))]
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        for i in range(w_out):
            if i >= len(cands):
                vals = (0, frozen, np.float32(-np.inf), 1, length[g * w_in])
            else:
                _, b, c = cands[i]
                r = g * w_in + b
                if finished[r]:
                    vals = (b, frozen, cum[r], 1, length[r])
                else:
                    t = int(top_ids[r, c])
                    vals = (b, t, np.float32(cum[r] + top_lp[r, c]), int(eos >= 0 and t == eos), length[r] + 1)
            for o, v in zip(out, vals):
                o.append(v)
    dtypes = (np.int32, np.int64, np.float32, np.int32, np.int32)
    return tuple(np.array(o, dtype=d) for o, d in zip(out, dtypes))


class RefBeamCache:
    """``tables[r]`` (lists of page ids), ``spare[r]``, ``row_pages[r]``, ``lens[r]`` and the pool's buffers ``arrays`` (each
    [capacity, ...]: a page is ``a[id]``).  ``step`` is atom_kv_step_i4's length rule, ``fork`` atom_kv_beam_fork_i4."""

    def __init__(self, tables, spare, row_pages, lens, page_size, num_beams, arrays=()):
        self.tables, self.spare = [list(t) for t in tables], list(spare)
        self.row_pages, self.lens = list(row_pages), list(lens)
        self.P, self.W, self.arrays = int(page_size), int(num_beams), list(arrays)
        self.cap = len(self.tables[0])
        self.status = 0

    def step(self, add=1):
        for r, n in enumerate(self.lens):
            if add > min(self.row_pages[r], self.cap) * self.P - n:
                self.status |= 1
            else:
                self.lens[r] = n + add

    def fork(self, parent):
        old_t, old_s = [list(t) for t in self.tables], list(self.spare)
        capacity = self.arrays[0].shape[0] if self.arrays else 2 ** 31 - 1
        copies = []
        for r in range(len(old_t)):
            maxlen = min(max(self.row_pages[r], 0), self.cap) * self.P
            n = self.lens[r]
            if not 0 <= n <= maxlen:
                n, self.status = min(max(n, 0), maxlen), self.status | BAD_LENGTH
            full, off = divmod(n, self.P)
            p = r
            if not 0 <= int(parent[r]) < self.W:
                self.status |= BAD_PARENT
            else:
                p = r - r % self.W + int(parent[r])
            copy = off > 0 and p != r
            if copy:
                src, dst = old_t[p][full], old_s[r]
                if not (0 <= src < capacity and 0 <= dst < capacity) or src == dst:
                    copy, p, self.status = False, r, self.status | BAD_PAGE
            row = old_t[p][:full] + old_t[r][full:]
            if copy:
                row[full], self.spare[r] = dst, old_t[r][full]
                copies.append((src, dst))
            self.tables[r] = row
        for a in self.arrays:                                 # sources are table pages, destinations spares: no copy reads another's target
            for src, dst in copies:
                a[dst] = a[src]

    def slot(self, r, pos):
        """(page id, offset) of token ``pos`` of row ``r``"""
        return self.tables[r][pos // self.P], pos % self.P

    def writable(self):
        """per row: the pages it may write -- its partial page, its reserve and its spare.  A fork permutes nothing between rows: each
        row's set is the same before and after (it only swaps its partial page with its spare)."""
        return [set(row[self.lens[r] // self.P:self.row_pages[r]]) | {self.spare[r]} for r, row in enumerate(self.tables)]

    def check_ownership(self, all_pages):
        """the invariant: no partial or reserve page in two rows, spares distinct and in no table, no page from outside ``all_pages``"""
        later = [i for r, row in enumerate(self.tables) for i in row[self.lens[r] // self.P:self.row_pages[r]]]
        assert len(later) == len(set(later)), "a partial or reserve page is referenced by two rows"
        in_tables = {i for r, row in enumerate(self.tables) for i in row[:self.row_pages[r]]}
        assert len(set(self.spare)) == len(self.spare) and not in_tables & set(self.spare), "a spare page is in a table"
        assert in_tables | set(self.spare) <= set(all_pages), "a page from outside the allocated set"


def backtrack(parents, tokens, cum, num_beams, eos=None, length_penalty=1.0):
    """per group the list of (tokens, sum_logprob, score) ranked by score descending, then beam index: every final row followed back
    through ``parents`` / ``tokens`` (one list of groups * num_beams entries per step), cut after the first eos, score in float64"""
    W, out = int(num_beams), []
    for g in range(len(cum) // W):
        hyps = []
        for b in range(W):
            row, toks = g * W + b, []
            for t in reversed(range(len(tokens))):
                toks.insert(0, int(tokens[t][row]))
                row = g * W + int(parents[t][row])
            if eos is not None and eos in toks:
                toks = toks[:toks.index(eos) + 1]
            s = float(cum[g * W + b])
            hyps.append((-(s / float(len(toks)) ** float(length_penalty)), b, toks, s))
        out.append([(toks, s, -neg) for neg, b, toks, s in sorted(hyps, key=lambda h: (h[0], h[1]))])
    return out
