"""GPU tests of ops.sample (atom_sample_f16): every comparison is EXACT against tests/sample_ref.py -- the token is specified op by
op as a function of the row's fp16 bits, its parameters, the seed and the step, so there is no tolerance and no excluded case.
The kernel has three forms by row length (registers up to 32,768 tokens; registers + LDS up to 131,072; re-read beyond) and two load
paths (16-byte loads where the base and the row stride allow, 2-byte loads otherwise): the sizes below are the smallest that reach each."""
import numpy as np
import pytest
import torch

from tests import sample_cases, sample_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
T_VALUES = [0.0, 0.3, 1.0, 4.0, 1e-6, 1e6]
P_VALUES = [1.0, 0.9, 0.5, 1e-4, 0.0]


def _k_values(vocab):
    return [0, 1, 2, 50, vocab, vocab + 1, -1]


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype, device=DEV)


def _seed_tensor(seeds):
    return _dev([s - 2 ** 64 if s >= 2 ** 63 else s for s in (int(x) & (2 ** 64 - 1) for x in seeds)], torch.int64)


def _logits(batch, vocab, seed):
    """N(0, 3^2) rows; every third row on a grid of 1/4 (many ties), every fifth with NaN, -inf and +inf planted"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, vocab), generator=g) * 3.0
    x[::3] = (x[::3] * 4).round() / 4
    x = x.half()
    for b in range(0, batch, 5):
        for j, v in enumerate((float("nan"), float("-inf"), float("inf"))):
            x[b, (7 * b + 3 * j) % vocab] = v
    return x


def _mixed_params(batch, vocab, shift=0):
    ks = _k_values(vocab)
    T = [T_VALUES[(b + shift) % len(T_VALUES)] for b in range(batch)]
    K = [ks[(b // 2 + shift) % len(ks)] for b in range(batch)]
    Pp = [P_VALUES[(b // 3 + shift) % len(P_VALUES)] for b in range(batch)]
    seeds = [(b * 0x9E3779B97F4A7C15 + shift) & (2 ** 64 - 1) for b in range(batch)]
    return T, K, Pp, seeds


def _run(logits, T, K, Pp, seeds, step=0, step_offset=0):
    from atom_amd import ops
    st = None if step is None else _dev([step], torch.int64)
    return ops.sample(logits, _dev(T, torch.float32), _dev(K, torch.int32), _dev(Pp, torch.float32), _seed_tensor(seeds), step=st,
                      step_offset=step_offset)


def _check(logits_dev, T, K, Pp, seeds, step=0, step_offset=0):
    got = _run(logits_dev, T, K, Pp, seeds, step, step_offset)
    want = sample_ref.sample(logits_dev, T, K, Pp, seeds, step=(step or 0) + step_offset)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.tensor(want, dtype=torch.int64)), (got.tolist(), want)
    return got


# ------------------------------------------------------------------------------------------------ 1. vocab x batch, mixed parameters
@pytest.mark.parametrize("vocab", [1, 2, 63, 64, 65, 1000, 1023, 1025, 32000])
def test_mixed_parameters_per_row(vocab):
    """greedy rows among sampled ones, every k, p and T of the lists, in batches of 1, 5 and 70"""
    for batch in (1, 5, 70):
        logits = _logits(batch, vocab, seed=vocab + batch).to(DEV)
        for shift in ((0, 1, 2) if batch < 70 and vocab <= 1025 else (0,)):
            _check(logits, *_mixed_params(batch, vocab, shift), step=shift * 1000)


def test_every_parameter_value_meets_every_other():
    """vocab 65, batch 210 = 6 T x 7 k x 5 p: the full product on one tied row and one random row"""
    vocab = 65
    combos = [(t, k, p) for t in T_VALUES for k in _k_values(vocab) for p in P_VALUES]
    base = _logits(3, vocab, seed=1)
    for r in (0, 1):
        logits = base[r:r + 1].repeat(len(combos), 1).to(DEV)
        T, K, Pp = (list(x) for x in zip(*combos))
        _check(logits, T, K, Pp, list(range(len(combos))), step=9)


def test_null_parameters_are_the_defaults():
    from atom_amd import ops
    logits = _logits(5, 1000, seed=3).to(DEV)
    got = ops.sample(logits)
    assert got.tolist() == sample_ref.sample(logits)                  # T = 1, k and p off, seed 0, step 0
    out = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    assert ops.sample(logits, step_offset=4, out=out) is out and out.tolist() == sample_ref.sample(logits, step=4)
    greedy = ops.sample(logits, temperature=torch.zeros(5, device=DEV))
    assert greedy.tolist() == sample_ref.sample(logits, temperature=0.0)


# ------------------------------------------------------------------------------------------------ 2. layout
@pytest.mark.parametrize("vocab,ld,offset", [(1001, 1008, 0), (1000, 1001, 0), (1000, 1000, 1), (1000, 1008, 1), (65, 72, 0),
                                             (40001, 40008, 0), (40000, 40001, 0), (140001, 140008, 0), (140000, 140001, 0)])
def test_padded_odd_and_offset_rows(vocab, ld, offset):
    """a padded view on the 16-byte path (with a tail that is no whole load), an odd row stride, a base 2 bytes off a 16-byte
    boundary, at a row length of each of the kernel's three forms: the padding holds large logits that must never be read as tokens"""
    batch = 5
    buf = torch.full((batch * ld + 8,), 60000.0, dtype=torch.float16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + batch * ld].view(batch, ld)[:, :vocab]
    view.copy_(_logits(batch, vocab, seed=ld).to(DEV))
    assert view.data_ptr() % 16 == 2 * offset and view.stride(0) == ld
    T, K, Pp, seeds = _mixed_params(batch, vocab, 1)
    got = _run(view, T, K, Pp, seeds, step=2)
    assert got.tolist() == sample_ref.sample(view.contiguous(), T, K, Pp, seeds, step=2)
    assert _run(view, [1.0] * batch, [0] * batch, [1.0] * batch, seeds, step=5).tolist() == sample_ref.sample(view.contiguous(), seeds=seeds, step=5)


# ------------------------------------------------------------------------------------------------ 3. large rows
@pytest.mark.parametrize("vocab,batch", [(128256, 3), (262144, 2)])
def test_large_rows(vocab, batch):
    """128,256: the registers + LDS form; 2^18: the form that reads its slabs again.  Row 0 sampled over the whole row, row 1 with
    top-k and top-p, the last greedy; the second call moves the maximum into the last slab"""
    logits = _logits(batch, vocab, seed=vocab).to(DEV)
    T, K, Pp = [1.0, 0.8, 0.0][:batch], [0, 40, 0][:batch], [1.0, 0.95, 1.0][:batch]
    _check(logits, T, K, Pp, [11, 12, 13][:batch], step=1)
    logits[:, vocab - 3] = 30.0
    logits[-1, vocab - 5] = 30.0
    _check(logits, [1.0, 0.0, 0.0][:batch], [0] * batch, [0.3] * batch, [1, 2, 3][:batch], step=2)


# ------------------------------------------------------------------------------------------------ 4. planted rows
def _case_id(c):
    return c.name


@pytest.mark.parametrize("case", sample_cases.planted(), ids=_case_id)
def test_planted_rows(case):
    b = len(case.seeds)
    logits = torch.from_numpy(case.bits.view(np.int16).copy()).view(torch.float16).unsqueeze(0).repeat(b, 1).to(DEV)
    for step in case.steps:
        want = sample_cases.expected(case, step)
        hi, lo = step >> 20, step & 0xFFFFF                                       # the step split over *step and step_offset
        got = _run(logits, [case.T] * b, [case.k] * b, [case.p] * b, case.seeds, step=hi << 20, step_offset=lo)
        assert got.tolist() == want, (case.name, step)


# ------------------------------------------------------------------------------------------------ 5. randomness plumbing
def test_seed_step_and_offset_plumbing():
    vocab, batch = 1000, 5
    logits = _logits(batch, vocab, seed=8).to(DEV)
    T, K, Pp = [1.0] * batch, [0] * batch, [1.0] * batch
    seeds = [1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 5, 2 ** 64 - 1]                    # high words that matter
    a = _check(logits, T, K, Pp, seeds, step=2 ** 32 + 17)                        # *step above 2^32
    assert a.tolist() != _check(logits, T, K, Pp, seeds, step=17).tolist()
    b = _check(logits, T, K, Pp, seeds, step=2 ** 32, step_offset=17)             # *step + step_offset is one number
    c = _check(logits, T, K, Pp, seeds, step=None, step_offset=2 ** 32 + 17)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a, _run(logits, T, K, Pp, seeds, step=2 ** 32 + 17))       # the same call twice
    low = _check(logits, T, K, Pp, [s & 0xFFFFFFFF for s in seeds], step=2 ** 32 + 17)
    assert low[0] == a[0] and low.tolist()[1:] != a.tolist()[1:]
    for row in range(batch):                                                      # another seed on one row changes only that row
        other = list(seeds)
        other[row] += 1000
        d = _check(logits, T, K, Pp, other, step=2 ** 32 + 17)
        same = [i for i in range(batch) if i != row]
        assert torch.equal(d[same], a[same])
    flat = torch.zeros((batch, 4096), dtype=torch.float16, device=DEV)            # 4096 equal logits: a new seed moves the token
    f0, f1 = _check(flat, T, K, Pp, seeds, step=1), _check(flat, T, K, Pp, [s + 1000 for s in seeds], step=1)
    assert (f0 != f1).all()


def test_a_row_does_not_depend_on_its_batch():
    vocab = 1023
    logits = _logits(70, vocab, seed=4).to(DEV)
    T, K, Pp, seeds = _mixed_params(70, vocab)
    whole = _run(logits, T, K, Pp, seeds, step=6)
    for b in (0, 33, 69):
        alone = _run(logits[b:b + 1], T[b:b + 1], K[b:b + 1], Pp[b:b + 1], seeds[b:b + 1], step=6)
        assert alone[0] == whole[b]


# ------------------------------------------------------------------------------------------------ 6. capture
def test_captured_call_follows_its_buffers():
    from atom_amd import ops
    vocab, batch = 1000, 5
    logits = _logits(batch, vocab, seed=21).to(DEV)
    T, K, Pp, seeds = _mixed_params(batch, vocab)
    bufs = [_dev(T, torch.float32), _dev(K, torch.int32), _dev(Pp, torch.float32), _seed_tensor(seeds)]
    step = _dev([3], torch.int64)
    out = torch.zeros(batch, dtype=torch.int64, device=DEV)
    ops.sample(logits, *bufs, step=step, step_offset=1, out=out)                   # eager once
    assert out.tolist() == sample_ref.sample(logits, T, K, Pp, seeds, step=4)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sample(logits, *bufs, step=step, step_offset=1, out=out)
    for shift, s in ((0, 3), (1, 2 ** 33), (2, 12)):                               # parameters, logits and the counter change in place
        T, K, Pp, seeds = _mixed_params(batch, vocab, shift)
        for buf, new in zip(bufs, (_dev(T, torch.float32), _dev(K, torch.int32), _dev(Pp, torch.float32), _seed_tensor(seeds))):
            buf.copy_(new)
        step.fill_(s)
        logits.copy_(_logits(batch, vocab, seed=30 + shift).to(DEV))
        out.fill_(-1)
        graph.replay()
        assert out.tolist() == sample_ref.sample(logits, T, K, Pp, seeds, step=s + 1), shift
    step.add_(1)                                                                  # a device-side counter, as DecodeGraph's
    graph.replay()
    assert out.tolist() == sample_ref.sample(logits, T, K, Pp, seeds, step=14)
