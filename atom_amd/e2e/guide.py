"""Guided decoding: ``TokenAutomaton`` -- a deterministic automaton over token ids, built from explicit edges, from a list of token
sequences (a "choice") or from a regular expression over the tokens' strings -- and ``LogitGuide``, the automata of a batch stacked
into device tables at fixed addresses with one state per sequence, masked and stepped by ops.guide_mask / ops.guide_advance inside the
replayed decode step, and by ops.guide_walk_rows with one state per verify row inside the replayed speculative step
(DESIGN.md 4.19).  Building an automaton is host work done once, offline; nothing here reads a token back from
the device while generating."""
from __future__ import annotations

from typing import Iterable, Sequence, Union

import numpy as np
import torch

from .. import ops

MAX_CODE_POINT = 0x10FFFF


class TokenAutomaton:
    """A deterministic automaton over token ids: ``num_states`` states, ``edges`` an iterable of ``(state, token, next)``, ``start`` the
    start state, ``vocab_size`` the number of tokens (default: the largest edge token + 1).  Raises ``ValueError`` for a duplicate
    ``(state, token)``, a ``next`` or ``start`` outside 0 .. num_states - 1, a token outside 0 .. vocab_size - 1 and for ANY state
    without an outgoing edge: so every state allows at least one token and a masked row of logits is never all -inf.
    ``final`` (a set of states, default all) is what ``accepts`` takes for the end of a sequence; the device tables ignore it.
    The edges are kept as CSR numpy arrays, sorted by (state, token): ``indptr`` int32 [num_states + 1], ``edge_tok`` and ``edge_next``
    int32 [num_edges]."""

    def __init__(self, num_states: int, edges: Iterable, start: int = 0, vocab_size: int = None, final=None):
        self.num_states, self.start = int(num_states), int(start)
        if self.num_states < 1:
            raise ValueError("TokenAutomaton: at least one state")
        if not 0 <= self.start < self.num_states:
            raise ValueError(f"TokenAutomaton: start {start} outside 0 .. {self.num_states - 1}")
        e = np.array(sorted((int(s), int(t), int(n)) for s, t, n in edges), dtype=np.int64).reshape(-1, 3)
        src, tok, nxt = e[:, 0], e[:, 1], e[:, 2]
        self.vocab_size = int(vocab_size) if vocab_size is not None else (int(tok.max()) + 1 if tok.size else 1)
        if tok.size and (src.min() < 0 or src.max() >= self.num_states):
            raise ValueError(f"TokenAutomaton: an edge leaves a state outside 0 .. {self.num_states - 1}")
        if tok.size and (nxt.min() < 0 or nxt.max() >= self.num_states):
            raise ValueError(f"TokenAutomaton: an edge's next state lies outside 0 .. {self.num_states - 1}")
        if tok.size and (tok.min() < 0 or tok.max() >= self.vocab_size):
            raise ValueError(f"TokenAutomaton: an edge's token lies outside 0 .. {self.vocab_size - 1}")
        if tok.size > 1 and bool(((src[1:] == src[:-1]) & (tok[1:] == tok[:-1])).any()):
            raise ValueError("TokenAutomaton: duplicate (state, token): the automaton must be deterministic")
        counts = np.bincount(src, minlength=self.num_states)
        if bool((counts == 0).any()):
            raise ValueError(f"TokenAutomaton: state {int(np.flatnonzero(counts == 0)[0])} has no outgoing edge")
        self.indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.edge_tok, self.edge_next = tok.astype(np.int32), nxt.astype(np.int32)
        self.final = None if final is None else frozenset(int(s) for s in final)
        if self.final is not None and any(not 0 <= s < self.num_states for s in self.final):
            raise ValueError("TokenAutomaton: a final state lies outside the automaton")

    @property
    def num_edges(self) -> int:
        return int(self.edge_tok.size)

    def step(self, state: int, token: int):
        """the state after ``token`` in ``state``, or None where the state has no such edge (the host walk)"""
        lo, hi = int(self.indptr[state]), int(self.indptr[state + 1])
        e = lo + int(np.searchsorted(self.edge_tok[lo:hi], token))
        return int(self.edge_next[e]) if e < hi and int(self.edge_tok[e]) == int(token) else None

    def allowed(self, state: int):
        """the tokens with an edge out of ``state``, ascending"""
        return self.edge_tok[int(self.indptr[state]):int(self.indptr[state + 1])].tolist()

    def accepts(self, tokens: Sequence[int]) -> bool:
        """True iff the automaton can read all of ``tokens`` from its start state and ends in a final state"""
        s = self.start
        for t in tokens:
            s = self.step(s, t)
            if s is None:
                return False
        return self.final is None or s in self.final

    @classmethod
    def from_sequences(cls, seqs: Iterable[Sequence[int]], eos_token_id: int, vocab_size: int) -> "TokenAutomaton":
        """The trie of the token sequences ``seqs`` (a "choice"): each complete sequence allows ``eos_token_id``, which leads to an END
        state whose only edge is EOS -> END.  ``accepts`` holds exactly for a given sequence followed by one or more EOS."""
        eos = int(eos_token_id)
        children, complete = [{}], set()
        for seq in seqs:
            node = 0
            for t in seq:
                t = int(t)
                if t == eos:
                    raise ValueError("from_sequences: a sequence contains eos_token_id")
                if t not in children[node]:
                    children.append({})
                    children[node][t] = len(children) - 1
                node = children[node][t]
            complete.add(node)
        if not complete:
            raise ValueError("from_sequences: no sequence given")
        end = len(children)
        edges = [(s, t, n) for s, ch in enumerate(children) for t, n in ch.items()]
        edges += [(s, eos, end) for s in sorted(complete)] + [(end, eos, end)]
        return cls(end + 1, edges, 0, vocab_size, final=[end])

    @classmethod
    def from_regex(cls, pattern: str, vocab: Sequence[str], eos_token_id: int, max_states: int = 4096) -> "TokenAutomaton":
        """The token sequences whose strings, joined, match ``pattern`` in full, each followed by ``eos_token_id``.  ``vocab[i]`` is
        token i's string; None or "" means the token is never allowed (the EOS token's own string is not used either).
        Supported, with full-match semantics over code points: literals, ``\\``-escapes of non-alphanumeric characters, ``\\n \\t \\r``,
        ``\\d \\w \\s`` (ASCII: [0-9], [A-Za-z0-9_], [ \\t\\n\\r\\f\\v]), ``.`` (any code point but a newline), classes ``[a-z0-9_]`` and
        ``[^...]``, groups ``( )``, ``|``, ``* + ?``, ``{m}``, ``{m,}``, ``{m,n}``.  Anything else -- anchors, backreferences, ``(?...)``
        groups and lookaround, lazy or possessive quantifiers, flags, other escapes -- raises ``ValueError`` naming the construct.
        The pipeline: parse; Thompson NFA over alphabet classes cut at the pattern's own code points plus "any other"; subset
        construction (more than ``max_states`` DFA states: ``ValueError``); states that cannot reach acceptance dropped; for DFA state q
        and token string w an edge iff delta*(q, w) exists (numpy, one gather per character position for all tokens at once);
        accepting states gain EOS -> END, END has EOS -> END.  Only states that are reachable from the start AND can reach END through
        token edges are kept, so every state allows a token.  ``ValueError`` too when no token sequence can match.
        This runs offline, once per pattern and vocabulary, and is NOT tuned: its cost is roughly states x tokens x the longest token."""
        eos, vocab = int(eos_token_id), list(vocab)
        if not 0 <= eos < len(vocab):
            raise ValueError(f"from_regex: eos_token_id {eos} outside the vocabulary of {len(vocab)}")
        ast = _Parser(pattern).parse()
        bounds, class_of_set = _alphabet(ast)
        table, accepting = _dfa(ast, class_of_set, len(bounds), int(max_states))          # [Q + 1, classes], row Q: the sink
        Q = table.shape[0] - 1
        # the token strings as class ids [V, longest], -1 padded; unusable tokens have length 0
        words = [w if (i != eos and w) else "" for i, w in enumerate(vocab)]
        lens = np.array([len(w) for w in words], dtype=np.int64)
        longest = int(lens.max()) if lens.size else 0
        cp = np.zeros((len(words), max(longest, 1)), dtype=np.int64)
        for i, w in enumerate(words):
            if w:
                cp[i, :len(w)] = [ord(c) for c in w]
        cid = np.searchsorted(bounds, cp, side="right") - 1                                # the class of every code point
        usable = np.flatnonzero(lens > 0)
        edges, chunk = [], max(1, (1 << 22) // max(len(usable), 1))
        for q0 in range(0, Q, chunk):
            qs = np.arange(q0, min(q0 + chunk, Q), dtype=np.int64)
            cur = np.repeat(qs[:, None], len(usable), axis=1)                              # [states, tokens]
            for pos in range(longest):
                nxt = table[cur, cid[usable, pos][None, :]]
                cur = np.where((lens[usable] > pos)[None, :], nxt, cur)
            si, ti = np.nonzero(cur != Q)
            edges.append(np.stack([qs[si], usable[ti], cur[si, ti]], axis=1))
        edges = np.concatenate(edges) if edges else np.zeros((0, 3), dtype=np.int64)
        end = Q
        extra = [(int(q), eos, end) for q in np.flatnonzero(accepting)] + [(end, eos, end)]
        edges = np.concatenate([edges, np.array(extra, dtype=np.int64).reshape(-1, 3)])
        # token level: keep what reaches END, then what the start reaches
        alive = _reach(end, edges[:, 2], edges[:, 0], Q + 1)
        edges = edges[alive[edges[:, 0]] & alive[edges[:, 2]]]
        if not alive[0]:
            raise ValueError(f"from_regex: no sequence of this vocabulary's tokens matches {pattern!r}")
        seen = _reach(0, edges[:, 0], edges[:, 2], Q + 1)
        edges = edges[seen[edges[:, 0]]]
        new_id = np.full(Q + 1, -1, dtype=np.int64)
        new_id[np.flatnonzero(seen)] = np.arange(int(seen.sum()))                          # the start stays 0, END stays last
        edges = np.stack([new_id[edges[:, 0]], edges[:, 1], new_id[edges[:, 2]]], axis=1)
        return cls(int(seen.sum()), edges.tolist(), 0, len(vocab), final=[int(new_id[end])])


def _reach(root: int, src, dst, n: int):
    """the states reachable from ``root`` along src -> dst, as a boolean array"""
    order = np.argsort(src, kind="stable")
    src, dst = np.asarray(src)[order], np.asarray(dst)[order]
    first = np.searchsorted(src, np.arange(n + 1))
    seen = np.zeros(n, dtype=bool)
    seen[root] = True
    todo = [root]
    while todo:
        s = todo.pop()
        for d in np.unique(dst[first[s]:first[s + 1]]).tolist():
            if not seen[d]:
                seen[d] = True
                todo.append(d)
    return seen


# ------------------------------------------------------------------------------------------------ the regular-expression front end
_DIGIT = [(48, 57)]
_WORD = [(48, 57), (65, 90), (95, 95), (97, 122)]
_SPACE = [(9, 13), (32, 32)]
_CONTROL = {"n": 10, "t": 9, "r": 13}
_MAX_REPEAT = 1000


def _normalise(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return tuple(out)


def _negate(ranges):
    out, at = [], 0
    for lo, hi in _normalise(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CODE_POINT:
        out.append((at, MAX_CODE_POINT))
    return tuple(out)


class _Parser:
    """pattern -> ('set', ranges) | ('cat', [nodes]) | ('alt', [nodes]) | ('rep', node, m, n or None)"""

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("from_regex: the pattern must be a str")
        self.p, self.i = pattern, 0

    def fail(self, what):
        raise ValueError(f"from_regex: unsupported or malformed construct {what} at position {self.i} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        c = self.peek()
        if c is None or c not in "*+?{":
            return node
        if c == "{":
            m, n = self.braces()
        else:
            self.i += 1
            m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
        c = self.peek()
        if c == "?":
            self.fail("lazy quantifier")
        if c == "+":
            self.fail("possessive quantifier")
        if c is not None and c in "*{":
            self.fail("multiple repeat")
        return ("rep", node, m, n)

    def braces(self):
        close = self.p.find("}", self.i)
        body = self.p[self.i + 1:close] if close > 0 else None
        parts = None if body is None else body.split(",")
        if parts is None or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
            self.fail("'{' that is not {m}, {m,} or {m,n}")
        m = int(parts[0])
        n = m if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if (n is not None and n < m) or max(m, n or 0) > _MAX_REPEAT:
            self.fail(f"repeat count (min > max, or above {_MAX_REPEAT})")
        self.i = close + 1
        return m, n

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                self.fail("'(?...)' group (non-capturing, named, lookaround or flags)")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            return ("set", _negate([(10, 10)]))
        if c == "\\":
            return ("set", _normalise(self.escape()))
        if c in "^$":
            self.i -= 1
            self.fail(f"anchor {c!r}")
        if c in "*+?{":
            self.i -= 1
            self.fail(f"quantifier {c!r} with nothing to repeat")
        return ("set", ((ord(c), ord(c)),))

    def escape(self):
        """after a backslash: the ranges it stands for"""
        c = self.peek()
        if c is None:
            self.fail("trailing backslash")
        self.i += 1
        if c in "dws":
            return {"d": _DIGIT, "w": _WORD, "s": _SPACE}[c]
        if c in _CONTROL:
            return [(_CONTROL[c], _CONTROL[c])]
        if c.isalnum() or ord(c) > 127:
            self.i -= 2
            self.fail("backreference" if c.isdigit() else f"escape '\\{c}'")
        return [(ord(c), ord(c))]

    def char_class(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        ranges, first = [], True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unterminated '['")
            self.i += 1
            if c == "]" and not first:
                break
            first = False
            if c == "[" and self.peek() == ":":
                self.fail("POSIX class '[:'")
            lo = self.escape() if c == "\\" else [(ord(c), ord(c))]
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                self.i += 1
                d = self.peek()
                self.i += 1
                hi = self.escape() if d == "\\" else [(ord(d), ord(d))]
                if len(lo) != 1 or lo[0][0] != lo[0][1] or len(hi) != 1 or hi[0][0] != hi[0][1] or hi[0][0] < lo[0][0]:
                    self.fail("bad character range")
                ranges.append((lo[0][0], hi[0][0]))
            else:
                ranges.extend(lo)
        return _negate(ranges) if negate else _normalise(ranges)


def _sets(node, out):
    if node[0] == "set":
        out.add(node[1])
    elif node[0] == "rep":
        _sets(node[1], out)
    else:
        for child in node[1]:
            _sets(child, out)


def _alphabet(ast):
    """The code points cut at every boundary of the pattern's sets: ``bounds`` (ascending int64; piece j is bounds[j] ..
    bounds[j + 1] - 1, so ``searchsorted(bounds, cp, 'right') - 1`` is a code point's piece) and, per set, the pieces inside it.  The
    pieces outside every set are the "any other" class: they have no transition anywhere."""
    sets = set()
    _sets(ast, sets)
    cuts = {0}
    for ranges in sets:
        for lo, hi in ranges:
            cuts.add(lo)
            if hi + 1 <= MAX_CODE_POINT:
                cuts.add(hi + 1)
    bounds = np.array(sorted(cuts), dtype=np.int64)
    pieces = {}
    for ranges in sets:
        ids = []
        for lo, hi in ranges:
            a, b = int(np.searchsorted(bounds, lo, side="right")) - 1, int(np.searchsorted(bounds, hi, side="right")) - 1
            ids.extend(range(a, b + 1))
        pieces[ranges] = ids
    return bounds, pieces


def _dfa(ast, class_of_set, num_classes: int, max_states: int):
    """Thompson NFA, subset construction, dead states dropped: (table int64 [Q + 1, classes] with row and value Q as the sink, accepting
    bool [Q]); state 0 is the start"""
    eps, moves = [], []                                       # per NFA state: epsilon targets, (set, target) moves

    def new():
        eps.append([])
        moves.append([])
        return len(eps) - 1

    def build(node, a, b):                                    # a fragment from state a to state b
        kind = node[0]
        if kind == "set":
            moves[a].append((node[1], b))
        elif kind == "cat":
            at = a
            for i, child in enumerate(node[1]):
                to = b if i == len(node[1]) - 1 else new()
                build(child, at, to)
                at = to
            if not node[1]:
                eps[a].append(b)
        elif kind == "alt":
            for child in node[1]:
                s, e = new(), new()
                eps[a].append(s)
                build(child, s, e)
                eps[e].append(b)
        else:
            _, child, m, n = node
            at = a
            for _ in range(m):
                to = new()
                build(child, at, to)
                at = to
            if n is None:                                     # a loop state: zero or more further copies
                loop, e = new(), new()
                eps[at].append(loop)
                build(child, loop, e)
                eps[e].append(loop)
                eps[loop].append(b)
            else:
                for _ in range(n - m):
                    to = new()
                    eps[at].append(b)
                    build(child, at, to)
                    at = to
                eps[at].append(b)

    start, accept = new(), new()
    build(ast, start, accept)

    def closure(states):
        seen, todo = set(states), list(states)
        while todo:
            for t in eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    first = closure([start])
    ids, order, rows = {first: 0}, [first], []
    at = 0
    while at < len(order):
        by_class = {}
        for s in order[at]:
            for ranges, t in moves[s]:
                for c in class_of_set[ranges]:
                    by_class.setdefault(c, set()).add(t)
        row = {}
        for c, targets in by_class.items():
            nxt = closure(targets)
            if nxt not in ids:
                if len(order) >= max_states:
                    raise ValueError(f"from_regex: the pattern needs more than max_states = {max_states} DFA states")
                ids[nxt] = len(order)
                order.append(nxt)
            row[c] = ids[nxt]
        rows.append(row)
        at += 1
    n = len(order)
    accepting = np.array([accept in s for s in order], dtype=bool)
    src = np.array([q for q, row in enumerate(rows) for _ in row], dtype=np.int64)
    dst = np.array([t for row in rows for t in row.values()], dtype=np.int64)
    alive = np.zeros(n, dtype=bool)
    for q in np.flatnonzero(accepting).tolist():              # what reaches an accepting state
        if not alive[q]:
            alive |= _reach(q, dst, src, n)
    if not alive[0]:
        raise ValueError("from_regex: the pattern matches nothing")
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[np.flatnonzero(alive)] = np.arange(int(alive.sum()))
    Q = int(alive.sum())
    table = np.full((Q + 1, num_classes), Q, dtype=np.int64)
    for q, row in enumerate(rows):
        if alive[q]:
            for c, t in row.items():
                if alive[t]:
                    table[new_id[q], c] = new_id[t]
    return table, accepting[alive]


# ------------------------------------------------------------------------------------------------ the device side
class LogitGuide:
    """The automata of a batch as device tables at FIXED addresses, so captured ``ops.guide_mask`` / ``ops.guide_advance`` launches
    follow ``reset`` and the states they advance themselves.  ``guides``: one ``TokenAutomaton`` or None per sequence, or one automaton
    for all sequences.  The distinct automata (by identity) are stacked in the order they first appear: automaton k's state s is the
    global state ``offsets[k] + s``.  ``indptr`` int32 [S + 1], ``edge_tok`` / ``edge_next`` int32 [E] (targets global), ``mask_bits``
    int32 [S, mask_ld] (the 32-bit words of the allowed sets, built from the same edges; mask_ld is ceil(vocab / 32) rounded up to 4),
    ``start`` / ``state`` int32 [batch] (``ops.GUIDE_FREE`` for None) and ``status`` int32 [1]."""

    def __init__(self, batch: int, vocab: int, device, guides: Union[TokenAutomaton, Sequence[TokenAutomaton]]):
        self.batch, self.vocab = int(batch), int(vocab)
        gs = [guides] * self.batch if isinstance(guides, TokenAutomaton) else list(guides)
        if len(gs) != self.batch or not all(g is None or isinstance(g, TokenAutomaton) for g in gs):
            raise ValueError(f"guide: one TokenAutomaton, or one (or None) per sequence ({self.batch})")
        self.automata, index = [], {}
        for g in gs:
            if g is not None and id(g) not in index:
                if g.vocab_size > self.vocab:
                    raise ValueError(f"guide: an automaton over {g.vocab_size} tokens for logits of {self.vocab}")
                index[id(g)] = len(self.automata)
                self.automata.append(g)
        if not self.automata:
            raise ValueError("guide: no automaton given (every sequence unconstrained needs no LogitGuide)")
        self.offsets = np.concatenate([[0], np.cumsum([g.num_states for g in self.automata])]).astype(np.int64)
        edge_base = np.concatenate([[0], np.cumsum([g.num_edges for g in self.automata])]).astype(np.int64)
        self.num_states, self.num_edges = int(self.offsets[-1]), int(edge_base[-1])
        self.mask_ld = -(-(-(-self.vocab // 32)) // 4) * 4
        if self.num_states * self.mask_ld >= 2 ** 31 or self.num_edges >= 2 ** 31:
            raise ValueError(f"guide: {self.num_states} states x {self.mask_ld} mask words (or {self.num_edges} edges) exceed int32")
        indptr = np.concatenate([g.indptr[:-1].astype(np.int64) + edge_base[k] for k, g in enumerate(self.automata)] + [edge_base[-1:]])
        edge_tok = np.concatenate([g.edge_tok for g in self.automata])
        edge_next = np.concatenate([g.edge_next.astype(np.int64) + self.offsets[k] for k, g in enumerate(self.automata)])
        bits = np.zeros((self.num_states, self.mask_ld), dtype=np.uint32)
        owner = np.repeat(np.arange(self.num_states), np.diff(indptr))
        np.bitwise_or.at(bits, (owner, edge_tok >> 5), np.uint32(1) << (edge_tok & 31).astype(np.uint32))
        starts = [ops.GUIDE_FREE if g is None else int(self.offsets[index[id(g)]]) + g.start for g in gs]
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        self.indptr, self.edge_tok, self.edge_next = to(indptr), to(edge_tok), to(edge_next)
        self.mask_bits = torch.from_numpy(bits.view(np.int32)).to(device)
        self.start = to(np.array(starts, dtype=np.int32))
        self.state = self.start.clone()
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.row_state = None                                  # int32 [batch, Q] once rows(Q) is called: the verify rows' states

    def reset(self):
        """every sequence back to its start state (FREE for None), the status word cleared; device copies, nothing synchronises"""
        self.state.copy_(self.start)
        self.status.zero_()

    def mask(self, logits: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """``logits`` fp16 [batch, vocab] with every token the sequence's state does not allow at -inf (ops.guide_mask, one launch)"""
        return ops.guide_mask(logits, self.state, self.mask_bits, out=out, status=self.status)

    def advance(self, tokens: torch.Tensor) -> torch.Tensor:
        """every sequence's state stepped over ``tokens`` int64 [batch], in place (ops.guide_advance, one launch)"""
        return ops.guide_advance(self.state, tokens, self.indptr, self.edge_tok, self.edge_next, status=self.status)

    def rows(self, Q: int) -> torch.Tensor:
        """``row_state`` int32 [batch, Q]: one state per verify row of a speculative step, allocated once at a fixed
        address; a later call must ask for the same Q"""
        Q = int(Q)
        if not 1 <= Q <= ops.GUIDE_MAX_ROWS:
            raise ValueError(f"guide: rows per sequence must be 1 .. {ops.GUIDE_MAX_ROWS}, got {Q}")
        if self.row_state is None:
            self.row_state = torch.zeros((self.batch, Q), dtype=torch.int32, device=self.state.device)
        if self.row_state.size(1) != Q:
            raise ValueError(f"guide: row states were allocated for {self.row_state.size(1)} rows per sequence, not {Q}")
        return self.row_state

    def walk_rows(self, adds: torch.Tensor, input_ids: torch.Tensor, force: bool = True) -> torch.Tensor:
        """the last step's ``adds`` committed into ``state``, then ``row_state`` walked over ``input_ids`` int64 [batch, Q] with forced
        drafts written into it (ops.guide_walk_rows, one launch); ``input_ids=None``: the commit alone.  Needs ``rows(Q)`` first."""
        if self.row_state is None:
            raise RuntimeError("guide: walk_rows needs rows(Q) first")
        return ops.guide_walk_rows(self.state, adds, self.row_state, input_ids, self.indptr, self.edge_tok, self.edge_next, force=force,
                                   status=self.status)

    def mask_rows(self, logits: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """``logits`` fp16 [batch * Q, vocab], every row masked with its own ``row_state`` (ops.guide_mask over all rows, one launch)"""
        if self.row_state is None:
            raise RuntimeError("guide: mask_rows needs rows(Q) first")
        return ops.guide_mask(logits, self.row_state.view(-1), self.mask_bits, out=out, status=self.status)

    def status_bits(self) -> int:
        """the status word (``ops.GUIDE_REJECTED`` | ``ops.GUIDE_BAD_STATE``): the one call here that synchronises"""
        return int(self.status.item())
