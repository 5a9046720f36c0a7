"""Host restatement of atom_guide_walk_rows from the text of include/atom_hip.h, line by line over
tests/guide_ref.py's ``advance_one``: the commit of the last speculative step, the state behind every verify row, the forced drafts.
Plain Python integers and lists; nothing here looks at the kernel."""
from tests import guide_ref
from tests.guide_ref import BAD_STATE, DEAD, REJECTED

MAX_ROWS = 9


def step_one(s, t, indptr, edge_tok, edge_next, num_states, num_edges):
    """``advance_one`` except that a token without an edge gives DEAD without a status bit"""
    s1, st = guide_ref.advance_one(s, t, indptr, edge_tok, edge_next, num_states, num_edges)
    return s1, st & BAD_STATE


def forced_token(s, indptr, edge_tok, num_states, num_edges):
    """the single token state ``s`` allows, or None: s inside the table and exactly one edge in its clamped range"""
    s = int(s)
    if not 0 <= s < num_states:
        return None
    lo = min(max(int(indptr[s]), 0), num_edges)
    hi = max(min(max(int(indptr[s + 1]), 0), num_edges), lo)
    return int(edge_tok[lo]) if hi - lo == 1 else None


def commit(state, add, prev, Q):
    """(committed state, status bits): rule 1"""
    state, add, bits = int(state), int(add), 0
    if 1 <= add <= Q:
        s = int(prev[add - 1])
    else:
        s = state
        if add != 0:
            bits |= BAD_STATE
    if state != DEAD and s == DEAD:
        bits |= REJECTED
    return s, bits


def walk(state, add, prev, ids, indptr, edge_tok, edge_next, num_states, num_edges, force, commit_only=False):
    """one sequence: (committed state, row states [Q] -- ``prev`` unchanged when ``commit_only`` --, ids [Q] with the forced drafts
    written in, status bits)"""
    Q = len(prev)
    s, bits = commit(state, add, prev, Q)
    ids = [int(t) for t in ids]
    if commit_only:
        return s, [int(x) for x in prev], ids, bits
    r, rows = s, []
    for j in range(Q):
        if force and j >= 1:
            only = forced_token(r, indptr, edge_tok, num_states, num_edges)
            if only is not None:
                ids[j] = only
        r, st = step_one(r, ids[j], indptr, edge_tok, edge_next, num_states, num_edges)
        bits |= st
        rows.append(r)
    return s, rows, ids, bits


def walk_batch(states, adds, row_state, input_ids, indptr, edge_tok, edge_next, num_states=None, num_edges=None, force=True,
               commit_only=False):
    """a batch: (states [batch], row_state [batch][Q], input_ids [batch][Q], status bits) as Python lists"""
    num_states = len(indptr) - 1 if num_states is None else num_states
    num_edges = len(edge_tok) if num_edges is None else num_edges
    out_s, out_r, out_i, bits = [], [], [], 0
    for b in range(len(states)):
        s, rows, ids, st = walk(states[b], adds[b], list(row_state[b]), list(input_ids[b]), indptr, edge_tok, edge_next, num_states,
                                num_edges, force, commit_only)
        out_s.append(s)
        out_r.append(rows)
        out_i.append(ids)
        bits |= st
    return out_s, out_r, out_i, bits
