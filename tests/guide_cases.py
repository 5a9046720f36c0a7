"""Planted inputs of the guided-decoding ops, shared by tests/test_guide_cpu.py (host build of guide_math.h) and tests/test_gpu_guide.py.

Advance: ONE table whose states have 0, 1, 2, 3, 4, 5, 1023, 1024 and 1025 edges (tokens 3, 5, 7, ...: odd, so every even token lies
between two edges), then a state with two targets out of range, a state whose indptr DEcreases (clamped to an empty range) and a state
whose indptr ends beyond num_edges (clamped to it); and the (state, token) pairs that reach every branch of the contract.
Mask: a table of eight mask rows per vocabulary (all zero, all ones, one bit at 0 / vocab - 1 / 2047 / 2048, two random) with every
padding word and every bit >= vocab set to 1, states that mix those rows with FREE, DEAD, -3 and num_states, and logits that are random
16-bit patterns (NaN payloads, -0, infinities, subnormals all occur) with the special ones planted in front."""
import numpy as np

from tests import guide_ref

ADV_VOCAB = 4096
ADV_LENGTHS = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025]
BAD_NEXT_STATE, DECREASING_STATE, BEYOND_STATE = 9, 10, 11
SPECIAL_BITS = [0x8000, 0x0000, 0x7C00, 0xFC00, 0x7E01, 0xFFFF, 0x7DFF, 0x0001, 0x8001, 0x03FF, 0x3C00]


def advance_table():
    """(indptr int32 [13], edge_tok int32 [E], edge_next int32 [E]); 12 states"""
    num_states = len(ADV_LENGTHS) + 3
    indptr, tok, nxt = [0], [], []
    for s, n in enumerate(ADV_LENGTHS):
        tok += [3 + 2 * i for i in range(n)]
        nxt += [(7 * s + i) % num_states for i in range(n)]
        indptr.append(len(tok))
    tok += [10, 20, 30]                                       # state 9: the edges over 10 and 30 lead outside the table
    nxt += [num_states, 4, -1]
    indptr.append(len(tok))                                   # = E: where state 10 starts
    E = len(tok)
    indptr += [E - 2, E + 1000]                               # state 10: E .. E - 2 (empty after the clamp); state 11: E - 2 .. E
    return np.array(indptr, dtype=np.int32), np.array(tok, dtype=np.int32), np.array(nxt, dtype=np.int32)


def advance_pairs():
    """(states, tokens) as Python lists: every branch, every row length, every kind of token"""
    pairs = []
    for s, n in enumerate(ADV_LENGTHS):
        if n == 0:
            pairs += [(s, 3), (s, 0)]
            continue
        first, last, mid = 3, 3 + 2 * (n - 1), 3 + 2 * (n // 2)
        pairs += [(s, first), (s, last), (s, mid), (s, first - 1), (s, 0), (s, last + 1), (s, last + 2), (s, mid + 1),
                  (s, -1), (s, ADV_VOCAB), (s, 2 ** 32 + mid), (s, 2 ** 63 - 1), (s, -(2 ** 63)), (s, mid - 2 ** 32)]
        if n >= 1023:                                         # every depth of the search: a run of neighbours at both ends
            pairs += [(s, 3 + 2 * i) for i in (1, 2, 3, n - 4, n - 3, n - 2, 511, 512, 513)]
    pairs += [(BAD_NEXT_STATE, 10), (BAD_NEXT_STATE, 20), (BAD_NEXT_STATE, 30), (BAD_NEXT_STATE, 25)]
    pairs += [(DECREASING_STATE, 20), (DECREASING_STATE, 30), (BEYOND_STATE, 20), (BEYOND_STATE, 30), (BEYOND_STATE, 10)]
    pairs += [(guide_ref.FREE, 3), (guide_ref.DEAD, 3), (-3, 3), (12, 3), (2 ** 31 - 1, 3), (-(2 ** 31), 3)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def mask_table(vocab, seed=0):
    """(mask uint32 [8, mask_ld], num_states 8): mask_ld is three words larger than needed, padding and bits >= vocab all ones"""
    rng = np.random.default_rng(1000 + vocab + seed)
    words = -(-vocab // 32)
    allow = np.zeros((8, vocab), dtype=bool)
    allow[1] = True
    allow[2, 0] = True
    allow[3, vocab - 1] = True
    if vocab > 2047:
        allow[4, 2047] = True
    if vocab > 2048:
        allow[5, 2048] = True
    allow[6] = rng.random(vocab) < 0.5
    allow[7] = rng.random(vocab) < 0.05
    padded = np.ones((8, (words + 3) * 32), dtype=bool)
    padded[:, :vocab] = allow
    mask = np.packbits(padded.reshape(8, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(8, words + 3)
    return np.ascontiguousarray(mask), 8


STATE_CYCLE = [6, guide_ref.FREE, 0, 8, 1, guide_ref.DEAD, 2, -3, 3, 6, 4, 5, 7]     # 8 = num_states; 6 twice: two rows share a state


def mask_states(batch, shift=0):
    return np.array([STATE_CYCLE[(i + shift) % len(STATE_CYCLE)] for i in range(batch)], dtype=np.int32)


def mask_logits(batch, vocab, seed=0):
    """uint16 [batch, vocab]: random patterns, the special ones in front of every row"""
    rng = np.random.default_rng(7 * vocab + batch + seed)
    bits = rng.integers(0, 65536, (batch, vocab), dtype=np.uint32).astype(np.uint16)
    n = min(vocab, len(SPECIAL_BITS))
    bits[:, :n] = np.array(SPECIAL_BITS[:n], dtype=np.uint16)
    return bits
