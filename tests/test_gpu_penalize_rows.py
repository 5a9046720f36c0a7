"""GPU tests of ops.penalize_rows (atom_penalize_rows_f16): every comparison is bit for bit, on the output AND on the
whole state.  Two yardsticks: the kernel that is there already -- per (sequence, row) a clone of the state row with the pending tokens
and drafts 1 .. j fed one at a time through ``ops.penalize(fed=)`` on a one-row view -- and the host reference
tests/penalty_rows_ref.py.  The kernel works per (tile of ops.PENALTY_TILE elements, sequence), eight elements per thread, with a
16-byte and a 2-byte access path and a build with and one without the bias stage: the sizes below are the smallest that reach each."""
import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import penalty_ref, penalty_rows_cases, penalty_rows_ref
from tests.test_gpu_penalize import SENTINEL_H, SENTINEL_S, _bias, _buffer, _check_padding, _f32, _pad8, _rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TILE = ops.PENALTY_TILE
VOCABS = [1, 8, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
REP, PRES, FREQ = (1.3, 1.0, 0.8), (0.0, 0.5, -0.25), (0.0, 0.25, 0.1)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _tokens(rng, shape, vocab):
    """few distinct values, so that drafts repeat and meet pending tokens; the edges of the vocabulary and values outside it"""
    pool = np.array([0, vocab - 1, vocab // 2, min(7, vocab - 1), min(8, vocab - 1), (TILE - 1) % vocab, TILE % vocab, -1, vocab, vocab + 3,
                     2 ** 40], dtype=np.int64)
    return pool[rng.integers(0, pool.size, shape)]


def _yardstick(bits, words, ids, pend, counts, rep, pres, freq, bias=None):
    """the existing kernel, token by token: (out uint16 [batch * rows, vocab], state uint16 [batch, vocab] after the pending tokens)"""
    batch, vocab = words.shape
    rows = bits.shape[0] // batch
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16)
    state = torch.from_numpy(words.view(np.int16)).to(DEV)
    R, P, F = _f32(rep), _f32(pres), _f32(freq)
    bi, bv = (None, None) if bias is None else (torch.from_numpy(bias[0]).to(DEV), torch.from_numpy(bias[1]).to(DEV))
    out, after = np.zeros_like(bits), words.copy()
    for b in range(batch):
        take = [] if pend is None else [int(t) for t in pend[b][:penalty_rows_ref.clamp_count(counts[b], len(pend[b]))]]
        kw = dict(repetition=R[b:b + 1], presence=P[b:b + 1], frequency=F[b:b + 1], bias_ids=None if bi is None else bi[b:b + 1],
                  bias_vals=None if bv is None else bv[b:b + 1])
        for j in range(rows):
            scratch, row = state[b:b + 1].clone(), logits[b * rows + j:b * rows + j + 1]
            got = None
            for n, t in enumerate(take + [int(t) for t in ids[b][1:j + 1]]):
                got = ops.penalize(row, scratch, _i64([t]), **kw)
                if j == 0 and n == len(take) - 1:
                    after[b] = penalty_ref.bits_of(scratch)[0]
            if got is None:
                got = ops.penalize(row, scratch, None, **kw)
            out[b * rows + j] = penalty_ref.bits_of(got)[0]
    return out, after


def _run(bits, words, ids, pend, counts, rep, pres, freq, bias=None, lds=None, offsets=(0, 0, 0), in_place=False, yardstick=True):
    """runs ops.penalize_rows on buffers of the leading dimensions ``lds`` (logits, out, state), each ``offsets`` elements off 16 bytes,
    and compares the output, the whole state and every padding word"""
    batch, vocab = words.shape
    total = bits.shape[0]
    ld, out_ld, state_ld = lds or (_pad8(vocab), _pad8(vocab, 8), _pad8(vocab, 16))
    lflat, logits = _buffer(bits, ld, offsets[0], SENTINEL_H, torch.float16)
    sflat, state = _buffer(words, state_ld, offsets[2], SENTINEL_S, torch.int16)
    if in_place:
        oflat, out, out_ld, o_off = lflat, logits, ld, offsets[0]
    else:
        (oflat, out), o_off = _buffer(np.zeros_like(bits), out_ld, offsets[1], SENTINEL_H, torch.float16), offsets[1]
    bi, bv = (None, None) if bias is None else (torch.from_numpy(bias[0]).to(DEV), torch.from_numpy(bias[1]).to(DEV))
    ct, cc = (None, None) if pend is None else (_i64(np.asarray(pend, dtype=np.int64)), _i32(counts))
    got = ops.penalize_rows(logits, state, _i64(np.asarray(ids, dtype=np.int64)), ct, cc, _f32(rep), _f32(pres), _f32(freq), bi, bv, out=out)
    assert got is out
    want_out, want_state = penalty_rows_ref.penalize_rows(bits, words, ids, pend, counts, rep, pres, freq, None if bias is None else bias[0],
                                                          None if bias is None else bias[1])
    got_out, got_state = penalty_ref.bits_of(out), penalty_ref.bits_of(state)[:, :vocab]
    bad = np.argwhere(got_out != want_out)
    assert bad.size == 0, [(int(r), int(i), hex(int(bits[r, i])), hex(int(got_out[r, i])), hex(int(want_out[r, i]))) for r, i in bad[:6]]
    assert np.array_equal(got_state, want_state), np.argwhere(got_state != want_state)[:6].tolist()
    if yardstick:
        y_out, y_state = _yardstick(bits, words, ids, pend, counts, rep, pres, freq, bias)
        bad = np.argwhere(got_out != y_out)
        assert bad.size == 0, [(int(r), int(i), hex(int(got_out[r, i])), hex(int(y_out[r, i]))) for r, i in bad[:6]]
        assert np.array_equal(got_state, y_state)              # the WHOLE state: drafts have left nothing behind
    _check_padding(oflat, total, vocab, out_ld, o_off, SENTINEL_H)
    _check_padding(sflat, batch, vocab, state_ld, offsets[2], SENTINEL_S)
    if not in_place:
        assert np.array_equal(penalty_ref.bits_of(logits), bits)
        _check_padding(lflat, total, vocab, ld, offsets[0], SENTINEL_H)
    return got_out, got_state


def _random(batch, rows, vocab, seed, width=None):
    rng = np.random.default_rng(seed)
    bits, _ = _rows(batch * rows, vocab, seed=seed)
    _, words = _rows(batch, vocab, seed=seed + 1)
    ids = _tokens(rng, (batch, rows), vocab)
    pend = _tokens(rng, (batch, rows if width is None else width), vocab)
    counts = [(0, rows, 1, rows - 1)[(b + seed) % 4] for b in range(batch)]
    par = [[x[(b + seed) % 3] for b in range(batch)] for x in (REP, PRES, FREQ)]
    return bits, words, ids.tolist(), pend.tolist(), counts, par


# ------------------------------------------------------------------------------------------------ 1. shapes and layouts
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rows", [1, 2, 5, 9])
@pytest.mark.parametrize("batch", [1, 3])
def test_shapes_on_both_access_paths(vocab, rows, batch):
    """the 16-byte path (aligned bases, leading dimensions that are multiples of 8 and differ), then the 2-byte path: an odd leading
    dimension, and each of logits / out / state two bytes off in turn"""
    bits, words, ids, pend, counts, par = _random(batch, rows, vocab, seed=7 * vocab + rows + batch)
    p8 = _pad8(vocab, 8)
    layouts = ((None, (0, 0, 0)), ((vocab + 1, vocab + 3, vocab + 2), (0, 0, 0)), ((p8, p8, p8), (1, 0, 0)), ((p8, p8, p8), (0, 1, 0)),
               ((p8, p8, p8), (0, 0, 1)))
    for n, (lds, offsets) in enumerate(layouts):
        _run(bits, words, ids, pend, counts, *par, lds=lds, offsets=offsets, yardstick=n < 2)          # the build without bias
        _run(bits, words, ids, pend, counts, *par, bias=_bias(batch, vocab, 16, vocab + n), lds=lds, offsets=offsets, yardstick=n < 2)


def test_a_real_vocabulary():
    bits, words, ids, pend, counts, par = _random(2, 5, 32000, seed=3)
    _run(bits, words, ids, pend, counts, *par)
    _run(bits, words, ids, pend, counts, *par, bias=_bias(2, 32000, 40, 9), yardstick=False)


@pytest.mark.parametrize("vocab", [9, TILE + 1, 2 * TILE + 5])
def test_in_place_equals_out_of_place(vocab):
    bits, words, ids, pend, counts, par = _random(3, 5, vocab, seed=vocab)
    for bias in (None, _bias(3, vocab, 8, 2)):
        for lds, offsets in ((None, (0, 0, 0)), ((vocab + 1,) * 3, (0, 0, 0)), ((_pad8(vocab),) * 3, (1, 1, 0))):
            a = _run(bits, words, ids, pend, counts, *par, bias=bias, lds=lds, offsets=offsets, yardstick=False)
            b = _run(bits, words, ids, pend, counts, *par, bias=bias, lds=lds, offsets=offsets, in_place=True, yardstick=False)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 2. planted drafts and commits
CASES = penalty_rows_cases.planted()


def _batch_of(cases):
    width = max(max(len(c.pending) for c in cases), 1)
    nb = max(len(c.bias_ids) for c in cases)
    bias = None
    if nb:
        bias = (np.full((len(cases), nb), -1, dtype=np.int32), np.zeros((len(cases), nb), dtype=np.float32))
        for b, c in enumerate(cases):
            bias[0][b, :len(c.bias_ids)] = c.bias_ids
            bias[1][b, :len(c.bias_vals)] = c.bias_vals
    pend = [(c.pending + [-1] * width)[:width] for c in cases]
    counts = [min(c.count, len(c.pending)) if c.count > 0 else c.count for c in cases]     # a row is padded: the count stays inside it
    return (np.concatenate([c.bits for c in cases]), np.stack([c.words for c in cases]), [c.ids for c in cases], pend, counts,
            [c.rep for c in cases], [c.pres for c in cases], [c.freq for c in cases], bias)


def _check_cases(cases, got_out, got_state):
    R = penalty_rows_cases.ROWS
    for b, c in enumerate(cases):
        want_out, want_state = penalty_rows_cases.expected(c)
        assert np.array_equal(got_out[b * R:(b + 1) * R], want_out) and np.array_equal(got_state[b], want_state), c.name


@pytest.mark.parametrize("layout", ["vec", "scalar"])
def test_planted_sequences_in_one_launch(layout):
    """every planted sequence as one batch; VOCAB + 3 lies inside the padding of the leading dimensions, which comes back untouched"""
    *args, bias = _batch_of(CASES)
    V = penalty_rows_cases.VOCAB
    lds = (_pad8(V, 8),) * 3 if layout == "vec" else (V + 5, V + 7, V + 9)
    got_out, got_state = _run(*args, bias=bias, lds=lds)
    _check_cases(CASES, got_out, got_state)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_planted_sequence_alone(case):
    """batch 1, with the bias stage only where the case has a bias, and the count as the case gives it (-3, 40)"""
    *args, bias = _batch_of([case])
    args[4] = [case.count]
    V = penalty_rows_cases.VOCAB
    got_out, got_state = _run(*args, bias=bias, lds=(_pad8(V, 8),) * 3)
    _check_cases([case], got_out, got_state)


def test_neutral_sequence_between_two_penalised_ones():
    """its rows are copied bit for bit -- NaN payloads, -0 -- although its state is full of seen tokens, and its state is committed"""
    by_name = {c.name: c for c in CASES}
    cases = [by_name["all_equal"], by_name["neutral"], by_name["two_tiles_and_tail"]]
    for with_bias in (False, True):
        *args, _ = _batch_of(cases)
        bias = None
        if with_bias:                                          # the neutral sequence has padding alone: it stays neutral
            bias = (np.array([[3, -1], [-1, -1], [TILE, 9]], dtype=np.int32), np.array([[1.0, 5.0], [7.0, 7.0], [-2.0, 0.5]], dtype=np.float32))
        got_out, got_state = _run(*args, bias=bias)
        R = penalty_rows_cases.ROWS
        assert np.array_equal(got_out[R:2 * R], cases[1].bits)
        assert np.isin([0x7C01, 0xFE00, 0x8000, 0xFFFF], got_out[R:2 * R]).all()
        assert got_state[1, 1] == 4 and got_state[1, TILE] == 0x8001 and got_state[1, penalty_rows_cases.VOCAB - 1] == 1


def test_commit_counts_and_forms():
    """counts 0, 1, rows, -3 and 40 against rows of 12 and of 3 pending tokens (the clamp is min(width, 9)), no commit arrays at all,
    and the commit alone: the state moves as with logits, nothing else is touched"""
    batch, rows, vocab = 5, 5, TILE + 9
    for width in (12, 3):
        bits, words, ids, pend, _, _ = _random(batch, rows, vocab, seed=width, width=width)
        pend[3] = [8, 8, vocab, 8, -1, 8, 2 ** 40, TILE, TILE, 8, 8, 8][:width]            # duplicates and values out of range
        pend[4] = [8, vocab, 8, -1, 8, 2 ** 40, TILE, 8, TILE, 8, 8, 8][:width]
        words[3:, 8] = words[3:, TILE] = 0x8000
        counts = [0, 1, rows, -3, 40]
        par = ([1.3] * batch, [0.5] * batch, [0.25] * batch)
        _, with_logits = _run(bits, words, ids, pend, counts, *par)
        assert with_logits[3, 8] == 0x8000 and with_logits[3, TILE] == 0x8000              # -3 commits nothing, drafts leave nothing
        assert (with_logits[4, 8], with_logits[4, TILE]) == ((0x8004, 0x8002) if width == 12 else (0x8002, 0x8000))
        sflat, state = _buffer(words, _pad8(vocab, 8), 0, SENTINEL_S, torch.int16)
        assert ops.penalize_rows(None, state[:, :vocab], None, _i64(pend), _i32(counts)) is None
        assert np.array_equal(penalty_ref.bits_of(state)[:, :vocab], with_logits)
        assert np.array_equal(with_logits, penalty_rows_ref.penalize_rows(None, words, None, pend, counts)[1])
        _check_padding(sflat, batch, vocab, _pad8(vocab, 8), 0, SENTINEL_S)
    _, untouched = _run(bits, words, ids, None, None, *par)
    assert np.array_equal(untouched, words)


# ------------------------------------------------------------------------------------------------ 3. bias
@pytest.mark.parametrize("max_bias", [0, 3, 512])
def test_bias_widths(max_bias):
    batch, rows, vocab = 3, 5, 2 * TILE + 11
    bits, words, ids, pend, counts, par = _random(batch, rows, vocab, seed=max_bias)
    bias = None
    if max_bias:
        bias = _bias(batch, vocab, max_bias, 5)
        bias[0][0, 0], bias[1][0, 0] = -1, 3.0
        free = [t for t in (TILE, 8, vocab - 1) if t not in bias[0][1].tolist()]
        ids[1][1] = ids[1][2] = free[0]                        # an id equal to a draft, with a -inf bias
        bias[0][1, 0], bias[1][1, 0] = free[0], -np.inf
        bits[rows:2 * rows, free[0]] = 0x4200                  # 3.0 in every row of sequence 1
    got_out, _ = _run(bits, words, ids, pend, counts, *par, bias=bias)
    if max_bias:
        assert (got_out[rows:2 * rows, ids[1][1]] == 0xFC00).all()


def test_a_bias_entry_alone_makes_a_sequence_non_neutral():
    """the same sequence twice with neutral parameters; sequence 1 has one bias entry with id >= vocab, which changes no element but
    ends its neutrality: the NaNs of its seen and drafted tokens are recomputed (0x7E00), sequence 0's are copied"""
    vocab, rows = 100, 3
    rng = np.random.default_rng(2)
    one = np.stack([penalty_ref.bits_of(np.float16(rng.normal(0, 3, vocab))) for _ in range(rows)])
    one[:, 5], one[:, 6], one[:, 7] = 0x7C01, 0xFE00, 0x7DFF
    bits = np.concatenate([one, one])
    words = np.zeros((2, vocab), dtype=np.uint16)
    words[:, 5] = 1                                           # 5 is seen, 6 is drafted at row 1, 7 is neither
    ids = [[0, 6, 9]] * 2
    bias = (np.array([[-1], [vocab]], dtype=np.int32), np.array([[1.0], [1.0]], dtype=np.float32))
    got_out, _ = _run(bits, words, ids, None, None, [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], bias=bias)
    assert np.array_equal(got_out[:rows], one)
    assert (got_out[rows:, 5] == 0x7E00).all() and got_out[rows:, 6].tolist() == [0xFE00, 0x7E00, 0x7E00] and (got_out[rows:, 7] == 0x7DFF).all()


# ------------------------------------------------------------------------------------------------ 4. capture
def test_captured_call_follows_its_buffers_and_advances_its_state():
    """one call captured, replayed twice with input_ids, commit_counts and rep changed in place between the replays"""
    batch, rows, vocab = 3, 5, TILE + 100
    bits, words, ids, pend, counts, (rep, pres, freq) = _random(batch, rows, vocab, seed=13)
    pend = [[50, 50, TILE, 7, 50]] * batch
    counts = [2, 0, 5]
    ld = _pad8(vocab)
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.float16)
    state = torch.zeros((batch, ld), dtype=torch.int16, device=DEV)
    state[:, :vocab] = torch.from_numpy(words.view(np.int16)).to(DEV)
    b_ids, b_vals = _bias(batch, vocab, 8, 4)
    t_ids, t_pend, t_counts, t_rep = _i64(ids), _i64(pend), _i32(counts), _f32(rep)
    args = (t_rep, _f32(pres), _f32(freq), torch.from_numpy(b_ids).to(DEV), torch.from_numpy(b_vals).to(DEV))
    out = torch.zeros((batch * rows, vocab), dtype=torch.float16, device=DEV)
    ops.penalize_rows(logits, state, t_ids, t_pend, t_counts, *args, out=out)                 # eager once
    want_out, want_state = penalty_rows_ref.penalize_rows(bits, words, ids, pend, counts, rep, pres, freq, b_ids, b_vals)
    assert np.array_equal(penalty_ref.bits_of(out), want_out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.penalize_rows(logits, state, t_ids, t_pend, t_counts, *args, out=out)
    assert np.array_equal(penalty_ref.bits_of(state)[:, :vocab], want_state)                  # a capture runs nothing
    for i in range(2):
        if i == 1:
            ids, counts, rep = [[1, 50, 50, TILE, vocab - 1]] * batch, [5, 1, 0], [1.0, 2.0, 0.5]
            t_ids.copy_(_i64(ids)), t_counts.copy_(_i32(counts)), t_rep.copy_(_f32(rep))
        out.zero_()
        graph.replay()
        want_out, want_state = penalty_rows_ref.penalize_rows(bits, want_state, ids, pend, counts, rep, pres, freq, b_ids, b_vals)
        assert np.array_equal(penalty_ref.bits_of(out), want_out), i
        assert np.array_equal(penalty_ref.bits_of(state)[:, :vocab], want_state), i
    assert (want_state[0, 50] & 0x7FFF) == min((int(words[0, 50]) & 0x7FFF) + 7, 32767)
