"""The checker's restatement of atom_penalize_rows_f16 (include/atom_hip.h) on the host, built on
tests/penalty_ref.py: per sequence the commit of the pending tokens, then per verify row the word bumps of the drafts in front of it,
then ``penalty_ref.penalize_row`` under those words.  ``wrong=`` swaps ONE rule for the obvious wrong one, for the tests that show a
planted case tells the two apart."""
import numpy as np

from tests import penalty_ref

MAX_ROWS = 9
WRONG = ("col0_counted", "drafts_written", "sees_later_drafts", "commit_after", "dup_once")


def clamp_count(count, width):
    """how many pending tokens are read: the count clamped to 0 .. min(width, 9)"""
    return min(max(int(count), 0), min(int(width), MAX_ROWS))


def _bump(words, token):
    token = int(token)
    if 0 <= token < words.size:                                # compared with the range before it is an index
        words[token] = penalty_ref.count_up(words[token])


def penalize_rows_seq(bits, words, ids, pending=(), count=0, rep=1.0, pres=0.0, freq=0.0, bias_ids=(), bias_vals=(), wrong=None):
    """one sequence: ``bits`` uint16 [rows, vocab] (None: the commit alone), ``words`` uint16 [vocab], ``ids`` [rows] (column 0 the
    last emitted token, then the drafts), ``pending`` the tokens to commit of which ``count`` (clamped) are read.
    Returns (out uint16 [rows, vocab] or None, the state words after the call)."""
    assert wrong is None or wrong in WRONG
    words = np.array(words, dtype=np.uint16)
    take = [int(t) for t in list(pending)[:clamp_count(count, len(pending))]]
    if wrong == "dup_once":
        take = list(dict.fromkeys(take))
    committed = words.copy()
    for t in take:
        _bump(committed, t)
    if bits is None:
        return None, committed
    bits = np.asarray(bits, dtype=np.uint16)
    rows = bits.shape[0]
    assert 1 <= rows <= MAX_ROWS and len(ids) == rows
    w = words.copy() if wrong == "commit_after" else committed.copy()
    if wrong == "sees_later_drafts":
        for j in range(1, rows):
            _bump(w, ids[j])
    out = []
    for j in range(rows):
        if wrong != "sees_later_drafts" and (j >= 1 or wrong == "col0_counted"):
            _bump(w, ids[j])
        out.append(penalty_ref.penalize_row(bits[j], w, None, rep, pres, freq, bias_ids, bias_vals)[0])
    after = w if wrong == "drafts_written" else committed
    return np.stack(out), after


def penalize_rows(logits, state, input_ids, commit_tokens=None, commit_counts=None, rep=None, pres=None, freq=None, bias_ids=None,
                  bias_vals=None, wrong=None):
    """every sequence: ``logits`` [batch * rows, vocab] (None: the commit alone, the vocabulary is the state's width), ``state``
    [batch, >= vocab], ``input_ids`` [batch, rows].  Returns (out uint16 [batch * rows, vocab] or None, state uint16 [batch, vocab])."""
    state = penalty_ref.bits_of(state)
    batch = state.shape[0]
    to_list = lambda x: x.detach().cpu().tolist() if hasattr(x, "detach") else [list(r) if hasattr(r, "__len__") else r for r in x]
    bits = ids = None
    vocab = state.shape[1]
    if logits is not None:
        bits = penalty_ref.bits_of(logits)
        vocab = bits.shape[1]
        ids = to_list(input_ids)
        rows = len(ids[0])
        assert bits.shape[0] == batch * rows
        bits = bits.reshape(batch, rows, vocab)
    words = state[:, :vocab]
    pend = [()] * batch if commit_tokens is None else to_list(commit_tokens)
    cnt = [0] * batch if commit_counts is None else to_list(commit_counts)
    R, P, F = (penalty_ref._per_row(x, batch, d) for x, d in ((rep, 1.0), (pres, 0.0), (freq, 0.0)))
    I = [()] * batch if bias_ids is None else to_list(bias_ids)
    V = [()] * batch if bias_vals is None else to_list(bias_vals)
    res = [penalize_rows_seq(None if bits is None else bits[b], words[b], None if ids is None else ids[b], pend[b], cnt[b], R[b], P[b], F[b],
                             I[b], V[b], wrong=wrong) for b in range(batch)]
    out = None if bits is None else np.concatenate([r[0] for r in res])
    return out, np.stack([r[1] for r in res])


def sequential(bits, words, ids, pending=(), count=0, rep=1.0, pres=0.0, freq=0.0, bias_ids=(), bias_vals=()):
    """the same sequence the way non-speculative decoding reaches it: per row a scratch copy of the state, the pending tokens and then
    drafts 1 .. j fed one at a time through ``penalty_ref.penalize_row(fed=)``; the row is what the last call writes.
    Returns (out uint16 [rows, vocab], the state after the pending tokens alone)."""
    bits = np.asarray(bits, dtype=np.uint16)
    take = [int(t) for t in list(pending)[:clamp_count(count, len(pending))]]
    out, after = [], None
    for j in range(bits.shape[0]):
        scratch = np.array(words, dtype=np.uint16)
        row = None
        for n, t in enumerate(take + [int(t) for t in ids[1:j + 1]]):
            row, scratch = penalty_ref.penalize_row(bits[j], scratch, t, rep, pres, freq, bias_ids, bias_vals)
            if j == 0 and n == len(take) - 1:
                after = scratch.copy()
        if row is None:
            row, scratch = penalty_ref.penalize_row(bits[j], scratch, None, rep, pres, freq, bias_ids, bias_vals)
        out.append(row)
    if after is None:
        after = np.array(words, dtype=np.uint16)
    return np.stack(out), after
