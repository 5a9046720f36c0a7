"""GPU tests of ops.guide_walk_rows: the kernel bit for bit against tests/guide_walk_ref.py on the planted and random
cases of tests/guide_walk_cases.py -- batches on both sides of the 64-thread workgroup, ``input_ids`` contiguous and as columns of a
wider buffer, both ``force`` values, the commit-only form, the status word -- the op captured and replayed over buffers changed in
place, and LogitGuide.mask_rows over batch * Q rows against tests/guide_ref.py's mask row by row."""
import numpy as np
import pytest
import torch

from tests import guide_cases, guide_ref, guide_walk_cases as C, guide_walk_ref as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SENTINEL = -(0x5A5A5A5A5A5A5A5A)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pick(table, Q, batch, start):
    """``batch`` of the cases of (table, Q), cycled from ``start`` (None: every case once)"""
    states, adds, prev, ids = C.cases(table, Q)
    pick = np.arange(len(states)) if batch is None else (start + np.arange(batch)) % len(states)
    return states[pick], adds[pick], prev[pick], ids[pick]


def _run(table, states, adds, prev, ids, force, wide=0, commit_only=False, before=0):
    """the op on fresh device buffers: (states, row states, the WHOLE ids buffer [batch, Q + wide], status) as numpy / int"""
    from atom_amd import ops
    batch, Q = prev.shape
    d_state, d_adds, d_rows = _dev(states), _dev(adds), _dev(prev)
    whole = torch.full((batch, Q + wide), SENTINEL, dtype=torch.int64, device=DEV)
    view = whole[:, wide // 2:wide // 2 + Q]
    view.copy_(_dev(ids))
    status = torch.full((1,), before, dtype=torch.int32, device=DEV)
    got = ops.guide_walk_rows(d_state, d_adds, d_rows, None if commit_only else view, *(_dev(t) for t in table), force=force, status=status)
    assert got is d_rows
    assert d_adds.cpu().numpy().tolist() == adds.tolist()                      # only read
    return d_state.cpu().numpy(), d_rows.cpu().numpy(), whole.cpu().numpy(), int(status.item())


def _check(table, Q, batch, start, force, wide=0, commit_only=False, before=0):
    states, adds, prev, ids = _pick(table, Q, batch, start)
    indptr, tok, nxt = table
    want_s, want_r, want_i, want_bits = W.walk_batch(states, adds, prev.tolist(), ids.tolist(), indptr, tok, nxt, force=force,
                                                     commit_only=commit_only)
    got_s, got_r, whole, got_bits = _run(table, states, adds, prev, ids, force, wide, commit_only, before)
    assert got_s.tolist() == want_s and got_r.tolist() == want_r
    lo = wide // 2
    assert whole[:, lo:lo + Q].tolist() == want_i                              # forced drafts written, every other draft as it was
    assert (whole[:, :lo] == SENTINEL).all() and (whole[:, lo + Q:] == SENTINEL).all()     # the columns beside the view: untouched
    assert got_bits == before | want_bits                                      # the status word only gains bits
    if commit_only:
        assert want_r == prev.tolist() and want_i == ids.tolist()
    if not force:
        assert want_i == ids.tolist()
    return want_bits, int((np.array(want_i, dtype=np.int64) != ids).sum())


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("batch", [1, 3, 65, None])
@pytest.mark.parametrize("Q", C.QS)
def test_walk_rows_equals_the_restatement(Q, batch, force):
    """every table; batch None holds every case once (more than 64 sequences for every Q > 1)"""
    bits, written = 0, 0
    for k, (name, table) in enumerate(C.tables()):
        st, n = _check(table, Q, batch, 7 * k, force)
        bits, written = bits | st, written + n
    if batch is None:
        assert bits == guide_ref.REJECTED | guide_ref.BAD_STATE
        assert (written > 0) == (force and Q > 1)


@pytest.mark.parametrize("Q,wide", [(1, 1), (2, 3), (5, 4), (9, 7)])
def test_walk_rows_on_columns_of_a_wider_buffer(Q, wide):
    """ids_ld > Q, the view starting ``wide // 2`` columns in (an odd number of them too: 8-byte, not 16-byte, aligned rows)"""
    for name, table in C.tables()[:3]:
        for batch in (1, 3, 65):
            _check(table, Q, batch, 11, True, wide=wide)
            _check(table, Q, batch, 5, False, wide=wide)


@pytest.mark.parametrize("Q", C.QS)
def test_commit_only_leaves_rows_and_ids_alone_and_status_only_gains_bits(Q):
    for name, table in C.tables()[:2]:
        for batch in (3, 65, None):
            _check(table, Q, batch, 3, True, commit_only=True, before=4)
            _check(table, Q, batch, 3, True, before=4 | guide_ref.REJECTED)


def test_a_first_token_without_an_edge_is_rejected_at_the_next_commit():
    """two calls on the same buffers, as two steps make them: all rows DEAD and no bit, then REJECTED with the commit"""
    from atom_amd import ops
    table = C.planted_table()
    tabs = [_dev(t) for t in table]
    state, adds = _dev(np.array([0, 0], dtype=np.int32)), torch.zeros(2, dtype=torch.int32, device=DEV)
    rows, status = torch.zeros((2, 3), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = _dev(np.array([[C.NO_EDGE, 11, 12], [3, 77, 78]], dtype=np.int64))
    ops.guide_walk_rows(state, adds, rows, ids, *tabs, status=status)
    assert rows.tolist() == [[guide_ref.DEAD] * 3, [1, 2, 3]] and ids.tolist() == [[C.NO_EDGE, 11, 12], [3, 11, 12]]
    assert state.tolist() == [0, 0] and int(status.item()) == 0
    adds.copy_(_dev(np.array([1, 3], dtype=np.int32)))
    ops.guide_walk_rows(state, adds, rows, None, *tabs, status=status)
    assert state.tolist() == [guide_ref.DEAD, 3] and int(status.item()) == guide_ref.REJECTED


def test_walk_rows_captured_and_replayed_follows_its_buffers():
    from atom_amd import ops
    Q, batch, wide = 5, 65, 2
    table = C.planted_table()
    indptr, tok, nxt = table
    tabs = [_dev(t) for t in table]
    state, adds = torch.zeros(batch, dtype=torch.int32, device=DEV), torch.zeros(batch, dtype=torch.int32, device=DEV)
    rows = torch.zeros((batch, Q), dtype=torch.int32, device=DEV)
    whole = torch.zeros((batch, Q + wide), dtype=torch.int64, device=DEV)
    view, status = whole[:, 1:1 + Q], torch.zeros(1, dtype=torch.int32, device=DEV)

    def step():
        ops.guide_walk_rows(state, adds, rows, view, *tabs, force=True, status=status)

    step()                                                                      # eager warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    rounds = [_pick(table, Q, batch, start) for start in (0, 23, 41)]
    staged = [tuple(_dev(a) for a in r) for r in rounds]
    kept = []
    status.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s, a, p, i in staged:                                               # every buffer changes in place between replays
            state.copy_(s)
            adds.copy_(a)
            rows.copy_(p)
            view.copy_(i)
            graph.replay()
            kept.append((state.clone(), rows.clone(), view.clone(), status.clone()))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    seen = 0
    for n, ((s, a, p, i), got) in enumerate(zip(rounds, kept)):
        want_s, want_r, want_i, bits = W.walk_batch(s, a, p.tolist(), i.tolist(), indptr, tok, nxt, force=True)
        seen |= bits
        assert got[0].tolist() == want_s and got[1].tolist() == want_r and got[2].tolist() == want_i, n
        assert int(got[3].item()) == seen, n
    assert seen == guide_ref.REJECTED | guide_ref.BAD_STATE


@pytest.mark.parametrize("vocab", [1003, 2049])
def test_mask_rows_masks_every_row_with_its_own_state(vocab):
    """LogitGuide.mask_rows over batch * Q rows: one vocabulary off the 8-element vector width, one across the 2048-element tile"""
    from atom_amd.e2e import LogitGuide, TokenAutomaton
    batch, Q = 3, 5
    choice = TokenAutomaton.from_sequences([[17, 31], [250, 3], [250, 700, 41], [5, 6, 7, 8], [min(2047, vocab - 3), vocab - 2, 9]], vocab - 1, vocab)
    guide = LogitGuide(batch, vocab, DEV, [choice, None, choice])
    rows = guide.rows(Q)
    S = guide.num_states
    states = np.array([[0, 1, choice.num_states - 1, guide_ref.DEAD, 3], [guide_ref.FREE] * Q, [2, 4, S, 5, 0]], dtype=np.int32)
    rows.copy_(_dev(states))
    bits = guide_cases.mask_logits(batch * Q, vocab)
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16)
    out = torch.zeros((batch * Q, -(-vocab // 8) * 8), dtype=torch.float16, device=DEV)[:, :vocab]
    got = guide.mask_rows(logits, out=out)
    assert got is out
    mask = guide.mask_bits.cpu().numpy().view(np.uint32)
    res = guide_ref.bits_of(out)
    status = 0
    for r, s in enumerate(states.reshape(-1)):
        want, st = guide_ref.mask_row(bits[r], s, mask, S)
        status |= st
        assert np.array_equal(res[r], want), r
        if 0 <= s < S:
            assert (want != guide_ref.NEG_INF).sum() <= len(choice.allowed(int(s)))
    assert guide.status_bits() == status == guide_ref.BAD_STATE
    assert np.array_equal(guide_ref.bits_of(logits), bits)                     # the input is only read
