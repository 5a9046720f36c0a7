"""GPU tests of ops.penalize (atom_penalize_f16): every comparison is bit for bit against tests/penalty_ref.py, on the output AND on
the state -- the result is specified line by line as a function of the logits' bits, the state words and the parameters, so there is
no tolerance.  The kernel works in tiles of ops.PENALTY_TILE elements, eight per thread, with a 16-byte and a 2-byte access path and a
build with and one without the bias stage: the sizes below are the smallest that reach each."""
import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import penalty_cases, penalty_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TILE = ops.PENALTY_TILE
VOCABS = [1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
SENTINEL_H, SENTINEL_S = 0x5555, 0x2AAA            # padding between rows: must come back untouched


def _f32(x):
    return torch.tensor(x, dtype=torch.float32, device=DEV)


def _rows(batch, vocab, seed, seen=0.3):
    """(logits bits, state words) uint16 [batch, vocab]: planted specials among N(0, 3^2) logits; `seen` of the tokens with a count,
    a prompt flag or both, the extremes 32767 and 0xFFFF among them"""
    rng = np.random.default_rng(seed)
    bits = np.stack([penalty_cases.background(rng, vocab) for _ in range(batch)])
    words = np.where(rng.random((batch, vocab)) < seen, rng.integers(0, 6, (batch, vocab)), 0).astype(np.uint16)
    words |= np.where(rng.random((batch, vocab)) < seen / 3, 0x8000, 0).astype(np.uint16)
    words[:, ::41] = np.where(rng.random(words[:, ::41].shape) < 0.5, 32767, 0xFFFF)
    return bits, words


def _buffer(words, ld, offset, sentinel, dtype):
    """a [batch, ld] buffer `offset` elements off a 16-byte boundary, filled with `sentinel`, holding `words` in its first columns"""
    batch, vocab = words.shape
    flat = torch.full((batch * ld + 16,), sentinel, dtype=torch.int16, device=DEV)
    assert flat.data_ptr() % 16 == 0
    full = flat[offset:offset + batch * ld].view(batch, ld)
    full[:, :vocab] = torch.from_numpy(words.view(np.int16)).to(DEV)
    return flat, full.view(dtype)[:, :vocab] if dtype == torch.float16 else full


def _check_padding(flat, batch, vocab, ld, offset, sentinel):
    got = flat.cpu().numpy().view(np.uint16)
    body = np.zeros(got.size, dtype=bool)
    for b in range(batch):
        body[offset + b * ld:offset + b * ld + vocab] = True
    assert (got[~body] == sentinel).all()


def _bias(batch, vocab, width, seed):
    """bias table [batch, width]: distinct ids per row, -1 padding, ids >= vocab among them"""
    rng = np.random.default_rng(seed)
    ids = np.full((batch, width), -1, dtype=np.int32)
    vals = rng.normal(0.0, 2.0, (batch, width)).astype(np.float32)
    for b in range(batch):
        n = min(width, vocab + 2, 1 + b + width // 2)
        pick = rng.choice(vocab + 2, n, replace=False)          # vocab and vocab + 1: ignored
        ids[b, rng.choice(width, n, replace=False)] = pick
    return ids, vals


def _run_and_check(bits, words, ld, out_ld, state_ld, offset, fed, rep, pres, freq, bias=None, in_place=False):
    batch, vocab = bits.shape
    lflat, logits = _buffer(bits, ld, offset, SENTINEL_H, torch.float16)
    sflat, state = _buffer(words, state_ld, offset, SENTINEL_S, torch.int16)
    if in_place:
        oflat, out, out_ld = lflat, logits, ld
    else:
        oflat, out = _buffer(np.zeros_like(bits), out_ld, offset, SENTINEL_H, torch.float16)
    ids, vals = (None, None) if bias is None else (torch.from_numpy(bias[0]).to(DEV), torch.from_numpy(bias[1]).to(DEV))
    fed_t = None if fed is None else torch.tensor(fed, dtype=torch.int64, device=DEV)
    got = ops.penalize(logits, state, fed_t, _f32(rep), _f32(pres), _f32(freq), ids, vals, out=out)
    assert got is out
    want_out, want_state = penalty_ref.penalize(bits, words, fed, rep, pres, freq, None if bias is None else bias[0], None if bias is None else bias[1])
    got_out, got_state = penalty_ref.bits_of(out), penalty_ref.bits_of(state)[:, :vocab]
    bad = np.argwhere(got_out != want_out)
    assert bad.size == 0, [(int(b), int(i), hex(int(bits[b, i])), hex(int(words[b, i])), hex(int(got_out[b, i])), hex(int(want_out[b, i]))) for b, i in bad[:6]]
    assert np.array_equal(got_state, want_state), np.argwhere(got_state != want_state)[:6].tolist()
    _check_padding(oflat, batch, vocab, out_ld, offset, SENTINEL_H)
    _check_padding(sflat, batch, vocab, state_ld, offset, SENTINEL_S)
    if not in_place:
        assert np.array_equal(penalty_ref.bits_of(logits), bits)
        _check_padding(lflat, batch, vocab, ld, offset, SENTINEL_H)
    return got_out, got_state


def _params(batch, shift=0):
    rep = [(1.3, 1.0, 0.8, 1.0)[(b + shift) % 4] for b in range(batch)]
    pres = [(0.0, 0.5, -0.25, 0.0)[(b + shift) % 4] for b in range(batch)]
    freq = [(0.0, 0.25, 0.1, 0.0)[(b + shift) % 4] for b in range(batch)]
    return rep, pres, freq


def _pad8(n, extra=0):
    return -(-n // 8) * 8 + extra


# ------------------------------------------------------------------------------------------------ 1. shapes and layouts
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", [1, 3])
def test_shapes_on_both_access_paths(vocab, batch):
    """aligned bases with leading dimensions that are multiples of 8 (the 16-byte path, a row tail that is no whole access) and an
    odd leading dimension or a base 2 bytes off (the 2-byte path); ld, out_ld and state_ld differ and exceed vocab"""
    bits, words = _rows(batch, vocab, seed=vocab + batch)
    fed = [(17 * b + vocab // 2) % vocab for b in range(batch)]
    for n, (ld, out_ld, state_ld, offset) in enumerate(((_pad8(vocab), _pad8(vocab, 8), _pad8(vocab, 16), 0), (vocab + 1, vocab + 3, vocab + 2, 0),
                                                       (_pad8(vocab, 8), _pad8(vocab, 8), _pad8(vocab, 8), 1))):
        rep, pres, freq = _params(batch, n)
        _run_and_check(bits, words, ld, out_ld, state_ld, offset, fed, rep, pres, freq)                       # the build without bias
        _run_and_check(bits, words, ld, out_ld, state_ld, offset, fed, rep, pres, freq, bias=_bias(batch, vocab, 16, vocab + n))


@pytest.mark.parametrize("vocab", [9, TILE + 1, 3 * TILE + 5])
def test_in_place_equals_out_of_place(vocab):
    batch = 3
    bits, words = _rows(batch, vocab, seed=vocab)
    rep, pres, freq = _params(batch, 2)
    fed = [0, vocab - 1, vocab // 2]
    for ld, offset in ((_pad8(vocab, 8), 0), (vocab + 1, 1)):
        for bias in (None, _bias(batch, vocab, 8, vocab)):
            a = _run_and_check(bits, words, ld, ld + 8, ld, offset, fed, rep, pres, freq, bias=bias)
            b = _run_and_check(bits, words, ld, ld, ld, offset, fed, rep, pres, freq, bias=bias, in_place=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_null_arguments_are_neutral():
    bits, words = _rows(2, 1000, seed=5)
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16)
    out = ops.penalize(logits)                                       # no state, no parameters: a copy
    assert out.data_ptr() != logits.data_ptr() and np.array_equal(penalty_ref.bits_of(out), bits)
    state = torch.from_numpy(words.view(np.int16)).to(DEV)
    out = ops.penalize(logits, state, presence=_f32([0.5, 0.0]))     # rep and freq null; row 1 neutral
    assert np.array_equal(penalty_ref.bits_of(out), penalty_ref.penalize(bits, words, pres=[0.5, 0.0])[0])
    assert np.array_equal(penalty_ref.bits_of(state), words)
    ids = torch.tensor([[3, -1], [-1, -1]], dtype=torch.int32, device=DEV)
    vals = torch.tensor([[1.5, 9.0], [9.0, 9.0]], dtype=torch.float32, device=DEV)
    out = ops.penalize(logits, bias_ids=ids, bias_vals=vals)         # a bias without any state
    assert np.array_equal(penalty_ref.bits_of(out), penalty_ref.penalize(bits, bias_ids=ids, bias_vals=vals)[0])
    with pytest.raises(ValueError):
        ops.penalize(logits, fed=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.penalize(logits, state.to(torch.int32))
    with pytest.raises(ValueError):
        ops.penalize(logits, bias_ids=torch.zeros((2, 513), dtype=torch.int32, device=DEV), bias_vals=torch.zeros((2, 513), device=DEV))


# ------------------------------------------------------------------------------------------------ 2. neutral rows
@pytest.mark.parametrize("with_bias", [False, True])
def test_neutral_row_beside_a_penalised_one(with_bias):
    """rows 0 and 2 neutral (rep 1 and rep off), row 1 penalised: the neutral rows' bits pass through, NaN payloads included, although
    their state is full of seen tokens -- and their fed tokens are still counted"""
    vocab, batch = TILE + 9, 3
    bits, words = _rows(batch, vocab, seed=77, seen=0.6)
    nan_at = np.flatnonzero((bits[0] & 0x7FFF) > 0x7C00)
    assert nan_at.size > 3 and len({int(x) for x in bits[0, nan_at]}) > 2
    words[0, nan_at] = 3                                             # seen NaNs in a neutral row
    fed = [int(nan_at[0]), 5, TILE]
    bias = None
    if with_bias:                                                    # row 1 has entries; rows 0 and 2 only padding
        ids, vals = np.full((batch, 4), -1, dtype=np.int32), np.ones((batch, 4), dtype=np.float32)
        ids[1] = [0, TILE, vocab - 1, vocab]
        bias = (ids, vals)
    got_out, got_state = _run_and_check(bits, words, _pad8(vocab), _pad8(vocab), _pad8(vocab), 0, fed, [1.0, 1.5, -3.0], [0.0, 0.5, 0.0], [0.0] * 3, bias=bias)
    assert np.array_equal(got_out[0], bits[0]) and np.array_equal(got_out[2], bits[2]) and not np.array_equal(got_out[1], bits[1])
    for b in (0, 2):
        assert got_state[b, fed[b]] == penalty_ref.count_up(words[b, fed[b]]) != words[b, fed[b]]


def test_a_bias_entry_alone_makes_a_row_non_neutral():
    """the same row twice, parameters neutral; row 1 has one bias entry with id >= vocab, which changes no element but ends the
    row's neutrality: its seen NaNs are recomputed (0x7E00), row 0's are copied"""
    vocab = 100
    bits, words = _rows(1, vocab, seed=3)
    bits, words = np.repeat(bits, 2, 0), np.repeat(words, 2, 0)
    bits[:, 10], words[:, 10] = 0x7C01, 2
    ids = np.array([[-1], [vocab]], dtype=np.int32)
    got_out, _ = _run_and_check(bits, words, 104, 104, 104, 0, None, [1.0] * 2, [0.0] * 2, [0.0] * 2, bias=(ids, np.ones((2, 1), dtype=np.float32)))
    assert got_out[0, 10] == 0x7C01 and got_out[1, 10] == 0x7E00


# ------------------------------------------------------------------------------------------------ 3. fed positions
@pytest.mark.parametrize("neutral", [False, True])
def test_fed_positions(neutral):
    """element 0, vocab - 1, both sides of a tile edge and of a thread's eight; -1, vocab and far values count nothing"""
    vocab = 2 * TILE + 3
    spots = [0, vocab - 1, TILE - 1, TILE, 7, 8, -1, vocab, vocab + 1, -2 ** 40, 2 ** 40, 2 ** 31, 2 ** 32 + 5]
    batch = len(spots)
    bits, words = _rows(batch, vocab, seed=9)
    rep, pres, freq = ([1.0] * batch, [0.0] * batch, [0.0] * batch) if neutral else ([1.2] * batch, [0.5] * batch, [0.25] * batch)
    _, got_state = _run_and_check(bits, words, _pad8(vocab), _pad8(vocab), _pad8(vocab, 8), 0, spots, rep, pres, freq)
    for b, s in enumerate(spots):
        changed = np.flatnonzero(got_state[b] != words[b]).tolist()
        assert changed == ([s] if 0 <= s < vocab and (words[b, s] & 0x7FFF) != 0x7FFF else []), (b, s, changed)
    assert (got_state[:6] != words[:6]).sum() >= 4 and np.array_equal(got_state[6:], words[6:])


# ------------------------------------------------------------------------------------------------ 4. planted rows
@pytest.mark.parametrize("case", penalty_cases.planted(), ids=lambda c: c.name)
def test_planted_rows(case):
    bits, words = case.bits[None, :], case.words[None, :]
    bias = None
    if case.bias_ids:
        bias = (np.array([case.bias_ids], dtype=np.int32), np.array([case.bias_vals], dtype=np.float32))
    ld = _pad8(bits.shape[1])
    got_out, got_state = _run_and_check(bits, words, ld, ld, ld, 0, None if case.fed is None else [case.fed], [case.rep], [case.pres], [case.freq], bias=bias)
    want_out, want_state = penalty_cases.expected(case)
    assert np.array_equal(got_out[0], want_out) and np.array_equal(got_state[0], want_state)
    if case.tells is not None:                                       # ... and the kernel is not the wrong rule
        assert not np.array_equal(got_out[0], penalty_cases.expected(case, wrong=case.tells)[0])


# ------------------------------------------------------------------------------------------------ 5. bias lists
def test_bias_edge_cases():
    """ids at tile edges and at a thread's edges, a -inf bias, ids of -1 and >= vocab (ignored), an empty list, a full 512-entry list"""
    vocab, batch = 2 * TILE + 11, 4
    bits, words = _rows(batch, vocab, seed=31)
    width = ops.PENALTY_MAX_BIAS
    rng = np.random.default_rng(2)
    ids = np.full((batch, width), -1, dtype=np.int32)
    vals = rng.normal(0.0, 3.0, (batch, width)).astype(np.float32)
    edges = [0, 7, 8, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, vocab - 1]
    ids[0, :len(edges)] = edges
    ids[0, len(edges):len(edges) + 4] = [vocab, vocab + 1, 2 ** 31 - 1, -5]
    vals[0, [1, 4]] = -np.inf
    vals[0, 2] = np.inf
    ids[1] = rng.choice(vocab, width, replace=False)                 # a full list, ids in no order
    ids[2, 300] = TILE                                               # one entry deep inside the padding; row 3: an empty list
    rep, pres, freq = [1.0, 1.3, 1.0, 1.0], [0.0, 0.5, 0.0, 0.0], [0.0, 0.25, 0.0, 0.0]
    got_out, _ = _run_and_check(bits, words, _pad8(vocab), _pad8(vocab), _pad8(vocab), 0, [1, 2, 3, 4], rep, pres, freq, bias=(ids, vals))
    assert got_out[0, 7] == 0xFC00 or (bits[0, 7] & 0x7FFF) > 0x7C00 or bits[0, 7] == 0x7C00
    assert np.array_equal(got_out[3], bits[3])                       # neutral: nothing but padding in its list
    one = _run_and_check(bits[:1], words[:1], _pad8(vocab), _pad8(vocab), _pad8(vocab), 0, None, [1.0], [0.0], [0.0],
                         bias=(np.array([[6]], dtype=np.int32), np.array([[-np.inf]], dtype=np.float32)))[0]
    assert one[0, 6] == 0xFC00                                       # a one-entry list bans its token


# ------------------------------------------------------------------------------------------------ 6. capture
def test_captured_call_advances_its_state():
    """the same call captured once and replayed three times with fed and the logits changed in place: the counts advance by three, and
    each output is the reference's for the state that replay found"""
    vocab, batch = TILE + 100, 3
    bits, words = _rows(batch, vocab, seed=13)
    words[:, 50] = 0
    ld = _pad8(vocab)
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16)
    state = torch.zeros((batch, ld), dtype=torch.int16, device=DEV)
    state[:, :vocab] = torch.from_numpy(words.view(np.int16)).to(DEV)
    rep, pres, freq = [1.3, 1.0, 1.0], [0.0, 0.0, 0.5], [0.25, 0.0, 0.1]
    ids, vals = _bias(batch, vocab, 8, 4)
    args = (_f32(rep), _f32(pres), _f32(freq), torch.from_numpy(ids).to(DEV), torch.from_numpy(vals).to(DEV))
    fed = torch.tensor([50, 50, TILE], dtype=torch.int64, device=DEV)
    out = torch.zeros((batch, vocab), dtype=torch.float16, device=DEV)
    ops.penalize(logits, state, fed, *args, out=out)                 # eager once
    want_out, want_state = penalty_ref.penalize(bits, words, fed, rep, pres, freq, ids, vals)
    assert np.array_equal(penalty_ref.bits_of(out), want_out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.penalize(logits, state, fed, *args, out=out)
    assert np.array_equal(penalty_ref.bits_of(state)[:, :vocab], want_state)   # a capture runs nothing
    for i in range(3):
        if i == 2:
            fed.copy_(torch.tensor([50, 7, vocab - 1], dtype=torch.int64))
            bits = _rows(batch, vocab, seed=14)[0]
            logits.copy_(torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16))
        out.zero_()
        graph.replay()
        want_out, want_state = penalty_ref.penalize(bits, want_state, fed, rep, pres, freq, ids, vals)
        assert np.array_equal(penalty_ref.bits_of(out), want_out), i
        assert np.array_equal(penalty_ref.bits_of(state)[:, :vocab], want_state), i
    assert (want_state[0, 50] & 0x7FFF) == 4 and (want_state[1, 50] & 0x7FFF) == 3 and (want_state[2, TILE] & 0x7FFF) >= 3
