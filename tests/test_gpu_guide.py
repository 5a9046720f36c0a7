"""GPU tests of the guided-decoding ops: ops.guide_mask and ops.guide_advance bit for bit against tests/guide_ref.py on the planted
inputs of tests/guide_cases.py -- every row length around the 8-element vector and the 2048-element tile, both access paths, every
kind of state and token -- and both ops captured in one graph and replayed over buffers changed in place."""
import numpy as np
import pytest
import torch

from tests import guide_cases, guide_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SENTINEL = 0x5A5A
VOCABS = [1, 7, 8, 9, 31, 32, 33, 2047, 2048, 2049, 4104, 32000]


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.float16)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).to(DEV)
    return torch.from_numpy(a).to(DEV)


def _rows(bits, ld, offset=0, fill=None):
    """a device fp16 buffer [batch, ld] (``offset`` elements behind a 16-byte boundary) holding ``bits`` in its first columns; returns
    (the [batch, vocab] view, the whole [batch, ld] view)"""
    batch, vocab = bits.shape
    host = np.full((batch, ld), SENTINEL if fill is None else fill, dtype=np.uint16)
    host[:, :vocab] = bits
    flat = torch.zeros(batch * ld + 8 + offset, dtype=torch.float16, device=DEV)
    assert flat.data_ptr() % 16 == 0
    whole = flat[offset:offset + batch * ld].view(batch, ld)
    whole.copy_(_dev(host))
    return whole[:, :vocab], whole


def _ld(kind, vocab):
    return {"tight": vocab, "by8": -(-vocab // 8) * 8, "plus3": vocab + 3}[kind]


def _check_mask(vocab, batch, ld, out_ld, offset=0, out_offset=0, in_place=False, shift=0):
    from atom_amd import ops
    mask, S = guide_cases.mask_table(vocab)
    states = guide_cases.mask_states(batch, shift)
    bits = guide_cases.mask_logits(batch, vocab)
    want, want_status = guide_ref.mask_batch(bits, states, mask, S)
    logits, whole_in = _rows(bits, ld, offset)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    if in_place:
        out, whole_out = logits, whole_in
    else:
        out, whole_out = _rows(np.full((batch, vocab), SENTINEL, dtype=np.uint16), out_ld, out_offset)
    got = ops.guide_mask(logits, _dev(states), _dev(mask), out=out, status=status)
    assert got is out
    res = guide_ref.bits_of(whole_out)
    assert np.array_equal(res[:, :vocab], want), (vocab, batch, ld, out_ld)
    assert (res[:, vocab:] == SENTINEL).all()                               # columns vocab .. out_ld - 1 are never written
    if not in_place:
        assert np.array_equal(guide_ref.bits_of(whole_in)[:, :vocab], bits)  # the input is only read
    assert int(status.item()) == want_status
    assert want_status == (guide_ref.BAD_STATE if any(int(s) in (-3, S) for s in states) else 0)
    return want, states


@pytest.mark.parametrize("kind", ["tight", "by8", "plus3"])
@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("vocab", VOCABS)
def test_mask_equals_the_reference(vocab, batch, kind):
    """ld = vocab, vocab rounded up to 8 (the 16-byte path whenever vocab >= 8) and vocab + 3 (the element path); mask_ld three words
    larger than needed with every padding word and every bit >= vocab set; the states of guide_cases.STATE_CYCLE from a start that
    moves with the vocabulary"""
    ld = _ld(kind, vocab)
    want, states = _check_mask(vocab, batch, ld, ld, shift=VOCABS.index(vocab))
    if batch == 65:                                                         # every kind of row occurred, and two rows share state 6
        assert {int(s) for s in states} == set(guide_cases.STATE_CYCLE) and (states == 6).sum() >= 2
        assert (want[states == 0] == guide_ref.NEG_INF).all()               # the all-zero mask row: nothing but -inf ...
        bits = guide_cases.mask_logits(batch, vocab)
        assert np.array_equal(want[states == 1], bits[states == 1])         # ... the all-ones row: nothing changed
        assert ((want[states == 3] != guide_ref.NEG_INF).sum(axis=1) <= 1).all()


@pytest.mark.parametrize("vocab", [9, 2049, 4104])
def test_mask_with_offset_bases_and_unequal_leading_dimensions(vocab):
    by8 = _ld("by8", vocab)
    _check_mask(vocab, 3, by8, by8, offset=1)                               # the input one element off 16 bytes: the element path
    _check_mask(vocab, 3, by8, by8, out_offset=1)
    _check_mask(vocab, 13, by8 + 8, by8, shift=2)                           # both on the 16-byte path, different leading dimensions
    _check_mask(vocab, 13, vocab, by8 + 16, shift=5)


@pytest.mark.parametrize("vocab,kind", [(7, "tight"), (2049, "by8"), (2049, "plus3"), (32000, "tight")])
def test_mask_in_place(vocab, kind):
    _check_mask(vocab, 13, _ld(kind, vocab), None, in_place=True)


def test_mask_does_not_depend_on_the_batch_around_a_row():
    from atom_amd import ops
    vocab = 4104
    mask, S = guide_cases.mask_table(vocab)
    bits = guide_cases.mask_logits(13, vocab)
    states = guide_cases.mask_states(13)
    full = guide_ref.bits_of(ops.guide_mask(_dev(bits), _dev(states), _dev(mask)))
    for b in (0, 6, 12):
        alone = guide_ref.bits_of(ops.guide_mask(_dev(bits[b:b + 1]), _dev(states[b:b + 1]), _dev(mask)))
        assert np.array_equal(alone[0], full[b])


def _advance_inputs(batch, start=0):
    states, tokens = guide_cases.advance_pairs()
    pick = [(start + i) % len(states) for i in range(batch)]
    return [states[i] for i in pick], [tokens[i] for i in pick]


@pytest.mark.parametrize("batch,start", [(1, 0), (1, 61), (64, 0), (65, 30), (300, 0), (None, 0)])
def test_advance_equals_the_reference(batch, start):
    """the planted (state, token) pairs, cycled to the batch (None: each pair once); 300 holds every pair"""
    from atom_amd import ops
    indptr, tok, nxt = guide_cases.advance_table()
    states, tokens = _advance_inputs(batch or len(guide_cases.advance_pairs()[0]), start)
    want, want_status = guide_ref.advance_batch(states, tokens, indptr, tok, nxt)
    state = _dev(np.array(states, dtype=np.int32))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.guide_advance(state, _dev(np.array(tokens, dtype=np.int64)), _dev(indptr), _dev(tok), _dev(nxt), status=status)
    assert got is state and state.cpu().numpy().tolist() == want.tolist()
    assert int(status.item()) == want_status
    if batch in (300, None):
        assert want_status == guide_ref.REJECTED | guide_ref.BAD_STATE
        assert set(zip(states, tokens)) == set(zip(*guide_cases.advance_pairs()))


@pytest.mark.parametrize("pairs,bits", [([(8, 3), (8, 2051), (1, 3), (-1, 5), (-2, 5)], 0), ([(8, 3), (8, 4)], 1), ([(0, 3)], 1),
                                         ([(10, 20)], 1), ([(9, 10)], 2), ([(12, 3), (1, 3)], 2), ([(9, 30), (8, 2 ** 32 + 5)], 3)])
def test_advance_sets_exactly_the_reference_status_bits(pairs, bits):
    """only a token without an edge sets REJECTED, only a state or target outside the table sets BAD_STATE; bits already set stay"""
    from atom_amd import ops
    indptr, tok, nxt = guide_cases.advance_table()
    states, tokens = [p[0] for p in pairs], [p[1] for p in pairs]
    want, want_status = guide_ref.advance_batch(states, tokens, indptr, tok, nxt)
    assert want_status == bits
    for before in (0, 4):
        state, status = _dev(np.array(states, dtype=np.int32)), torch.full((1,), before, dtype=torch.int32, device=DEV)
        ops.guide_advance(state, _dev(np.array(tokens, dtype=np.int64)), _dev(indptr), _dev(tok), _dev(nxt), status=status)
        assert state.cpu().tolist() == want.tolist() and int(status.item()) == before | bits


def test_both_ops_captured_and_replayed_follow_their_buffers():
    from atom_amd import ops
    vocab, batch = 2049, 5
    indptr, tok, nxt = guide_cases.advance_table()
    S = indptr.size - 1
    mask = np.zeros((S, -(-vocab // 32) + 1), dtype=np.uint32)
    mask[:, :] = guide_ref.mask_from_csr(np.minimum(np.maximum.accumulate(indptr), tok.size), tok, mask.shape[1])
    bits = guide_cases.mask_logits(batch, vocab)
    d_indptr, d_tok, d_nxt, d_mask = _dev(indptr), _dev(tok), _dev(nxt), _dev(mask)
    state = torch.zeros(batch, dtype=torch.int32, device=DEV)
    tokens = torch.zeros(batch, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    logits, out = _dev(bits), torch.zeros((batch, vocab), dtype=torch.float16, device=DEV)

    def step():
        ops.guide_advance(state, tokens, d_indptr, d_tok, d_nxt, status=status)
        ops.guide_mask(logits, state, d_mask, out=out, status=status)

    rounds = [([8, 7, 1, -1, 3], [5, 3, 3, 9, 7]), ([6, 8, 8, -2, 5], [2047, 2051, 4, 3, 11]), ([2, 9, 12, 4, 7], [5, 10, 3, 9, 2049])]
    state.copy_(_dev(np.array(rounds[0][0], dtype=np.int32)))
    tokens.copy_(_dev(np.array(rounds[0][1], dtype=np.int64)))
    step()                                                                  # eager warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    staged = [(_dev(np.array(s, dtype=np.int32)), _dev(np.array(t, dtype=np.int64)), _dev(guide_cases.mask_logits(batch, vocab, seed=i + 1)))
              for i, (s, t) in enumerate(rounds)]
    kept = []
    status.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s, t, l in staged:                                              # state, tokens and logits change in place between replays
            state.copy_(s)
            tokens.copy_(t)
            logits.copy_(l)
            graph.replay()
            kept.append((state.clone(), out.clone(), status.clone()))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    seen = 0
    for i, ((s, t), (got_state, got_out, got_status)) in enumerate(zip(rounds, kept)):
        want_state, st1 = guide_ref.advance_batch(s, t, indptr, tok, nxt)
        want_out, st2 = guide_ref.mask_batch(guide_cases.mask_logits(batch, vocab, seed=i + 1), want_state, mask, S)
        seen |= st1 | st2
        assert got_state.cpu().tolist() == want_state.tolist(), i
        assert np.array_equal(guide_ref.bits_of(got_out), want_out), i
        assert int(got_status.item()) == seen, i
    assert seen == guide_ref.REJECTED | guide_ref.BAD_STATE
