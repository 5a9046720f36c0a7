"""Planted and random inputs of atom_guide_walk_rows, shared by tests/test_guide_walk_cpu.py (host build of guide_math.h's ``walk``) and
tests/test_gpu_guide_walk.py (the kernel).

Tables: ``planted_table()`` -- a fan-out state, a chain of twelve single-edge states (longer than any Q), a single-edge state whose
target lies outside the table, a state with two bad targets, a state whose indptr DEcreases and one whose indptr ends beyond num_edges
-- and ``random_table(seed, S)``: a sane automaton of S states, half of them with exactly one edge, with a single-edge chain in front.
Cases (``cases``): for every ``add`` in -1 .. Q + 1 and every variant -- a right path, a wrong draft at each position 1 .. Q - 1, an
``ids[0]`` without an edge, a token that is an edge token plus 2^32, random tokens -- one sequence whose committed state and last row
states come from valid states, FREE, DEAD and values outside the table."""
import numpy as np

from tests import guide_ref, guide_walk_ref

QS = [1, 2, 5, 9]
CHAIN = 12
BAD_SINGLE, BAD_NEXT, DECREASING, BEYOND = 14, 15, 16, 17
NO_EDGE = 900                                                  # no table below has an edge over it


def planted_table():
    """(indptr int32 [19], edge_tok, edge_next); 18 states"""
    S = 18
    edges = {0: [(3, 1), (5, 2), (7, 0)]}
    for s in range(1, 1 + CHAIN):                             # 1 -> 2 -> .. -> 13: one edge each
        edges[s] = [(10 + s, s + 1)]
    edges[13] = [(3, 1), (6, BAD_SINGLE), (8, 0), (9, BAD_NEXT)]
    edges[BAD_SINGLE] = [(8, 99)]                             # forced, and its target is outside the table
    edges[BAD_NEXT] = [(10, S), (20, 4), (30, -1)]
    indptr, tok, nxt = [0], [], []
    for s in range(BAD_NEXT + 1):
        tok += [t for t, _ in edges[s]]
        nxt += [n for _, n in edges[s]]
        indptr.append(len(tok))
    E = len(tok)
    indptr += [E - 2, E + 1000]                               # DECREASING: E .. E - 2, empty after the clamp; BEYOND: E - 2 .. E
    return np.array(indptr, dtype=np.int32), np.array(tok, dtype=np.int32), np.array(nxt, dtype=np.int32)


def random_table(seed, S):
    """a sane automaton: states 0 .. min(S - 1, CHAIN) - 1 a single-edge chain, the others one edge (half of them) or 2 .. 6"""
    rng = np.random.default_rng(4000 + 100 * seed + S)
    indptr, tok, nxt = [0], [], []
    chain = min(S - 1, CHAIN)
    for s in range(S):
        if s < chain:
            ts, ns = [int(rng.integers(0, 50))], [s + 1]
        else:
            n = 1 if rng.random() < 0.5 else int(rng.integers(2, 7))
            ts = sorted(rng.choice(50, size=n, replace=False).tolist())
            ns = rng.integers(0, S, size=n).tolist()
        tok += ts
        nxt += ns
        indptr.append(len(tok))
    return np.array(indptr, dtype=np.int32), np.array(tok, dtype=np.int32), np.array(nxt, dtype=np.int32)


def tables():
    """(name, (indptr, edge_tok, edge_next)) of every table the tests walk"""
    out = [("planted", planted_table())]
    for i, S in enumerate([2, 3, 7, 13, 40]):
        out.append((f"random{S}", random_table(i, S)))
    return out


def _range(s, indptr, E):
    lo = min(max(int(indptr[s]), 0), E)
    return lo, max(min(max(int(indptr[s + 1]), 0), E), lo)


def cases(table, Q, seed=0):
    """(states int32 [N], adds int32 [N], prev int32 [N, Q], ids int64 [N, Q]): see the module docstring"""
    indptr, tok, nxt = table
    S, E = indptr.size - 1, tok.size
    rng = np.random.default_rng(77 * Q + seed + S)
    odd = [guide_ref.FREE, guide_ref.DEAD, -3, S, 2 ** 31 - 1, -(2 ** 31)]

    def some_state():
        return int(rng.integers(0, S)) if rng.random() < 0.7 else odd[int(rng.integers(0, len(odd)))]

    variants = ["right"] + [("wrong", p) for p in range(1, Q)] + ["first", "big", "random"]
    states, adds, prevs, idss = [], [], [], []
    for add in range(-1, Q + 2):
        for v in variants:
            state, prev = some_state(), [some_state() for _ in range(Q)]
            if v == "right" and 1 <= add <= Q:
                prev[add - 1] = int(rng.integers(0, S))        # the right path starts inside the table at least here
            elif v == "right":
                state = int(rng.integers(0, S))
            s, _ = guide_walk_ref.commit(state, add, prev, Q)
            r, ids = s, []
            for j in range(Q):                                 # a path of edges as far as the table has one
                lo, hi = _range(r, indptr, E) if 0 <= r < S else (0, 0)
                t = int(tok[int(rng.integers(lo, hi))]) if hi > lo else int(rng.integers(0, 50))
                ids.append(t)
                r, _ = guide_walk_ref.step_one(r, t, indptr, tok, nxt, S, E)
            if v == "first":
                ids[0] = NO_EDGE
            elif v == "big":
                ids[int(rng.integers(0, Q))] += 2 ** 32
            elif v == "random":
                ids = rng.integers(0, 50, size=Q).tolist()
            elif v != "right":
                ids[v[1]] = NO_EDGE + v[1]
            states.append(state)
            adds.append(add)
            prevs.append(prev)
            idss.append(ids)
    return (np.array(states, dtype=np.int32), np.array(adds, dtype=np.int32), np.array(prevs, dtype=np.int32).reshape(-1, Q),
            np.array(idss, dtype=np.int64).reshape(-1, Q))
