"""GPU tests of ops.logprob (atom_logprob_f16) against tests/logprob_ref.py: rank and top_ids EXACTLY, logprob and top_logprobs
bitwise the reference's value with lz or one of its two float32 neighbours, one choice per row (the last bit of a double-precision
log is the contract's only allowance).  Shapes are the smallest at which each path of csrc/logprob.hip can go wrong: one slab of
8192 tokens and its edges, 32,768 / 32,769 (the register-resident form and the one that reads the row again), 2^17 + 1 and 2^18."""
import numpy as np
import pytest
import torch

from tests import logprob_cases, logprob_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _logits(rows, vocab, seed, sigma=3.0, layout="plain"):
    """fp16 [rows, vocab] on the GPU, N(0, sigma^2) (ties are common from a few thousand tokens on); ``pad3``: ld = vocab + 3;
    ``off1``: a view ``[:, 1:]`` of a wider tensor, every row base off 16 bytes"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((rows, vocab), generator=g) * sigma).half()
    if layout == "plain":
        return x.to(DEV)
    wide = torch.full((rows, vocab + (3 if layout == "pad3" else 1)), 7.0, dtype=torch.float16)      # the padding would win every maximum
    if layout == "pad3":
        wide[:, :vocab] = x
        return wide.to(DEV)[:, :vocab]
    wide[:, 1:] = x
    return wide.to(DEV)[:, 1:]


def _targets(logits, seed):
    """random targets, the row maximum's first index on row 0, an ignored target on the last row of three or more"""
    rows, vocab = logits.shape
    g = torch.Generator().manual_seed(seed + 1)
    t = torch.randint(0, vocab, (rows,), generator=g)
    t[0] = int(logits[0].float().argmax())
    if rows >= 3:
        t[-1] = -1
    return t.to(DEV)


def _check(logits, targets, top_n):
    from atom_amd import ops
    got = ops.logprob(logits, targets, top_n)
    moved = logprob_ref.assert_matches(got, logits, targets, top_n)
    print(f"{tuple(logits.shape)} ld {logits.stride(0)} top_n {top_n}: {moved} of {logits.size(0)} rows on a neighbour of lz")
    return got


@pytest.mark.parametrize("vocab", [1, 7, 8, 1000, 8191, 8192, 8193, 32000, 32768, 32769, 131073, 262144])
def test_every_row_length_matches_the_reference(vocab):
    logits = _logits(3, vocab, seed=vocab)
    _check(logits, _targets(logits, vocab), 32 if vocab in (8193, 32769) else 5)


@pytest.mark.parametrize("rows", [1, 130])
def test_row_counts(rows):
    logits = _logits(rows, 1000, seed=rows, sigma=1.0)
    lp, rk, ti, tl = _check(logits, _targets(logits, rows), 20)
    assert int(rk[0]) == 0 and int(ti[0, 0]) == int(logits[0].float().argmax())


@pytest.mark.parametrize("layout", ["pad3", "off1"])
@pytest.mark.parametrize("vocab", [1000, 8193, 32769])
def test_rows_off_16_bytes_take_the_2_byte_loads(vocab, layout):
    logits = _logits(3, vocab, seed=vocab + 5, layout=layout)
    assert logits.stride(0) % 8 != 0 or logits.data_ptr() % 16 != 0
    _check(logits, _targets(logits, vocab), 5)


def test_aligned_rows_with_a_padded_stride_take_the_16_byte_loads():
    wide = torch.full((3, 8200 + 8), 9.0, dtype=torch.float16)
    wide[:, :8197] = _logits(3, 8197, seed=3).cpu()
    logits = wide.to(DEV)[:, :8197]                             # ld % 8 == 0, vocab % 8 != 0: a vector body and a 2-byte tail
    _check(logits, _targets(logits, 3), 5)


def test_planted_families():
    for c in logprob_cases.planted():
        logits = torch.from_numpy(c.bits.view(np.int16).copy()).view(torch.float16).to(DEV)
        targets = torch.tensor(c.targets, dtype=torch.int64, device=DEV)
        _check(logits, targets, c.top_n)


def test_known_answers():
    from atom_amd import ops
    equal = torch.ones((1, 1 << 18), dtype=torch.float16, device=DEV)
    lp, rk, ti, tl = ops.logprob(equal, torch.tensor([200000], device=DEV), 32)
    assert rk.tolist() == [200000] and ti.tolist() == [list(range(32))]
    want = np.float32(-18.0 * np.log(2.0))
    near = {float(np.nextafter(want, np.float32(s), dtype=np.float32)) for s in (-np.inf, np.inf)} | {float(want)}
    assert float(lp[0]) in near and tl.unique().numel() == 1 and float(tl[0, 0]) == float(lp[0])
    hot = torch.full((1, 100), -65504.0, dtype=torch.float16, device=DEV)
    hot[0, 37] = 65504.0
    lp, rk, ti, tl = ops.logprob(hot, torch.tensor([5], device=DEV), 2)
    assert lp.tolist() == [-131008.0] and rk.tolist() == [6] and ti.tolist() == [[37, 0]] and float(tl[0, 1]) == -131008.0
    # Z = 2^40: lz is the difference of two doubles near 27.7 (ulp 2^-48), so a last-bit difference of the log leaves 2^-48, not 0
    assert abs(float(tl[0, 0])) <= 2.0 ** -47


def test_top_n_only_and_targets_only():
    from atom_amd import _lib as L
    from atom_amd import ops
    logits = _logits(3, 8193, seed=21)
    targets = _targets(logits, 21)
    full = ops.logprob(logits, targets, 5)
    lp, rk, ti, tl = ops.logprob(logits, None, 5)
    assert lp is None and rk is None and torch.equal(ti, full[2]) and torch.equal(tl.view(torch.int32), full[3].view(torch.int32))
    logprob_ref.assert_matches((None, None, ti, tl), logits, None, 5)
    lp, rk, ti, tl = ops.logprob(logits, targets)
    assert ti is None and tl is None and torch.equal(rk, full[1]) and torch.equal(lp.view(torch.int32), full[0].view(torch.int32))
    # the entry point with one of the two outputs: rank only (no weight sum), log-probability only (no counts)
    rank = torch.full((3,), 77, dtype=torch.int32, device=DEV)
    only = torch.full((3,), 77.0, dtype=torch.float32, device=DEV)
    call = L.lib().atom_logprob_f16
    stream = L.current_stream(DEV)
    L.check(call(logits.data_ptr(), logits.stride(0), 3, 8193, targets.data_ptr(), None, rank.data_ptr(), 0, None, None, stream), "rank")
    L.check(call(logits.data_ptr(), logits.stride(0), 3, 8193, targets.data_ptr(), only.data_ptr(), None, 0, None, None, stream), "logprob")
    assert torch.equal(rank, full[1]) and torch.equal(only.view(torch.int32), full[0].view(torch.int32))


def test_out_buffers_and_refusals():
    from atom_amd import ops
    logits = _logits(2, 1000, seed=8)
    targets = _targets(logits, 8)
    out = (torch.empty(2, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV),
           torch.empty((2, 4), dtype=torch.int64, device=DEV), torch.empty((2, 4), device=DEV))
    got = ops.logprob(logits, targets, 4, out=out)
    assert all(a is b for a, b in zip(got, out))
    logprob_ref.assert_matches(got, logits, targets, 4)
    with pytest.raises(TypeError):
        ops.logprob(logits, targets.int(), 4)
    with pytest.raises(TypeError):
        ops.logprob(logits, targets, 3, out=out)
    with pytest.raises(ValueError):
        ops.logprob(logits, targets, 33)
    with pytest.raises(ValueError):
        ops.logprob(logits, None, 0)
    with pytest.raises(ValueError):
        ops.logprob(logits.t(), None, 2)


def test_captured_op_follows_targets_changed_in_place():
    from atom_amd import ops
    logits = _logits(4, 32000, seed=12)
    first, second = _targets(logits, 12), _targets(logits, 13)
    assert not torch.equal(first, second)
    eager = [ops.logprob(logits, t, 5) for t in (first, second)]
    targets = first.clone()
    out = tuple(torch.zeros_like(x) for x in eager[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.logprob(logits, targets, 5, out=out)
    for t, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        targets.copy_(t)
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    logprob_ref.assert_matches(eager[1], logits, second, 5)
