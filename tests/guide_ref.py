"""Host restatement of the guided-decoding ops from the text of include/atom_hip.h, not from the kernels: the mask of
one row and of a batch, one step of one sequence and of a batch (a linear scan where the kernel searches), and the host walk of a CSR
automaton.  numpy and Python integers only."""
import numpy as np

FREE, DEAD = -1, -2
REJECTED, BAD_STATE = 1, 2
NEG_INF = 0xFC00


def bits_of(t):
    """a torch fp16 / int16 tensor (any device) as numpy uint16"""
    import torch
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def allowed_row(mask_row, vocab):
    """bool [vocab] from the 32-bit words of one mask row: token v is allowed iff (word[v >> 5] >> (v & 31)) & 1"""
    words = np.asarray(mask_row).view(np.uint32).astype(np.uint64)
    v = np.arange(vocab, dtype=np.uint64)
    return ((words[(v >> np.uint64(5)).astype(np.int64)] >> (v & np.uint64(31))) & np.uint64(1)).astype(bool)


def mask_row(bits, state, mask, num_states):
    """(out uint16 [vocab], status bits) of one row ``bits`` (uint16 [vocab]) in ``state``; ``mask`` [>= num_states, mask_ld] words"""
    bits = np.asarray(bits, dtype=np.uint16)
    s = int(state)
    if 0 <= s < num_states:
        return np.where(allowed_row(mask[s], bits.size), bits, np.uint16(NEG_INF)).astype(np.uint16), 0
    return bits.copy(), (0 if s in (FREE, DEAD) else BAD_STATE)


def mask_batch(bits, states, mask, num_states):
    """(out uint16 [batch, vocab], status bits)"""
    out, status = np.empty_like(np.asarray(bits, dtype=np.uint16)), 0
    for b in range(out.shape[0]):
        out[b], st = mask_row(bits[b], states[b], mask, num_states)
        status |= st
    return out, status


def advance_one(s, t, indptr, edge_tok, edge_next, num_states, num_edges):
    """(new state, status bits) of one sequence in state ``s`` over token ``t`` (any Python integer)"""
    s, t = int(s), int(t)
    if s in (FREE, DEAD):
        return s, 0
    if not 0 <= s < num_states:
        return DEAD, BAD_STATE
    lo = min(max(int(indptr[s]), 0), num_edges)
    hi = max(min(max(int(indptr[s + 1]), 0), num_edges), lo)
    for e in range(lo, hi):
        if int(edge_tok[e]) == t:
            nxt = int(edge_next[e])
            return (nxt, 0) if 0 <= nxt < num_states else (DEAD, BAD_STATE)
    return DEAD, REJECTED


def advance_batch(states, tokens, indptr, edge_tok, edge_next, num_states=None, num_edges=None):
    """(new states int32 [batch], status bits)"""
    num_states = len(indptr) - 1 if num_states is None else num_states
    num_edges = len(edge_tok) if num_edges is None else num_edges
    out, status = np.empty(len(states), dtype=np.int32), 0
    for b, (s, t) in enumerate(zip(states, tokens)):
        out[b], st = advance_one(s, t, indptr, edge_tok, edge_next, num_states, num_edges)
        status |= st
    return out, status


def mask_from_csr(indptr, edge_tok, mask_ld):
    """uint32 [num_states, mask_ld] with exactly the bits of the edges"""
    S = len(indptr) - 1
    mask = np.zeros((S, mask_ld), dtype=np.uint32)
    for s in range(S):
        for t in edge_tok[indptr[s]:indptr[s + 1]]:
            mask[s, int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
    return mask


def walk(start, tokens, indptr, edge_tok, edge_next):
    """the host walk: the states after each token from ``start`` (DEAD from the first token without an edge on)"""
    S, E = len(indptr) - 1, len(edge_tok)
    s, out = int(start), []
    for t in tokens:
        s, _ = advance_one(s, t, indptr, edge_tok, edge_next, S, E)
        out.append(s)
    return out
