"""CPU-only: the planted quantiser inputs of tests/quant_planted.py have teeth.  For every (op, mode, clip, eps, hidden size) that
tests/test_gpu_quant_planted.py and the planted u4 tests of tests/test_gpu_kv.py run, every deliberate error that applies to the case
(the ``mutate=`` argument of the references) changes at least one code, scale bit or de-quantised bit of the case's rows -- so a
kernel that made that error could not pass the bit-for-bit comparison with the unmutated oracle.  The counts are printed (-s).  These
are conditions on the INPUTS: where one is missed, the rows change, never the condition."""
import numpy as np
import pytest

from oracle import atom_oracle as O
from tests import quant_planted as P


def _teeth(op, args, mode, clip, what, dequant=True):
    ref = P.run(op, args, mode, clip)
    for k in ("q4", "q8", "s4", "s8", "xq"):
        assert not np.isnan(np.asarray(ref[k], dtype=np.float32)).any(), (what, k)
    counts = {}
    for m in P.MUTANTS:
        if P.applies(m, op, mode, clip, dequant):
            counts[m] = P.moved(ref, P.run(op, args, mode, clip, mutate=m), mode, dequant)
    print(f"{what}: " + ", ".join(f"{m} {n}" for m, n in counts.items()))
    assert counts and all(n > 0 for n in counts.values()), (what, counts)
    return ref


@pytest.mark.parametrize("mode,clip", P.MODE_CLIPS)
def test_the_unmutated_reference_is_the_oracle(mode, clip):
    """mutate=None calls the oracle; and the restatement the mutants are cut into equals the oracle with no mutant active"""
    y = P.tail_rows(mode, clip)
    want = O._quant_row_tail(y if mode == "sim" else y.astype(np.float32), mode, clip)
    got = P._tail(y if mode == "sim" else y.astype(np.float32), mode, clip, None)
    for k in want:
        assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(want[k]).view(np.uint8)), k
    v = np.tile(P.u4_vectors(), (1, 2))
    for a, b in zip(O.quant_o4(v), P.quant_o4(v)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("H", sorted({P.TAIL_H} | {K for op, _, K, _ in P.MULTI_Q_CASES if op == "reorder"}))
@pytest.mark.parametrize("mode,clip", P.MODE_CLIPS)
def test_reorder_rows_have_teeth(mode, clip, H):
    y = P.tail_rows(mode, clip, H)
    assert len(y) == 2 + (2 if mode == "kernel" else 1) + len(P.EDGE_NAMES)
    idx = P.perm(H)
    x = P.scatter(y, idx)
    assert np.array_equal(x[:, idx.astype(np.int64)].view(np.uint16), y.view(np.uint16))
    _teeth("reorder", (y, None), mode, clip, f"reorder {mode} {clip} H={H}")
    a = P.run("reorder", (x, idx), mode, clip)
    b = P.run("reorder", (y, None), mode, clip)
    assert P.moved(a, b, mode) == 0                           # the gathered rows ARE the planted rows
    if clip == 1.0:                                           # the analytic tie rows alone carry the rounding rule, in every group
        t = P.tie_rows(H)
        ref, mut = P.run("reorder", (t, None), mode, clip), P.run("reorder", (t, None), mode, clip, mutate="round_rule")
        G = H // 128 - 1
        assert ((ref["q4"] != mut["q4"]).reshape(2, G, 128).sum(axis=-1) >= 32).all()
        assert ((ref["q8"] != mut["q8"]).sum(axis=-1) >= 32).all()
    if clip < 1.0:                                            # code -8 is there, and only the lower clamp separates it from -7
        ref = P.run("reorder", (y, None), mode, clip)
        assert (ref["q4"] == -8).sum() >= H // 128 - 1


@pytest.mark.parametrize("H", sorted({P.TAIL_H} | {K for op, _, K, _ in P.MULTI_Q_CASES if op == "silu_mul"}))
@pytest.mark.parametrize("mode,clip", P.MODE_CLIPS)
def test_silu_rows_are_exact_and_have_teeth(mode, clip, H):
    """on saturated gates ({0} u [17, 48]) the oracle's silu(a) * b IS a * b: 1 + exp(-a) rounds to 1 in FP32 and the product of two
    halves is exact there -- nothing transcendental is left, and the SiLU op can be compared bit for bit"""
    a, b = P.silu_planted(mode, clip, H)
    assert (((a >= 17) & (a <= 48)) | (a == 0)).all()
    got, want = O.silu_mul(a, b, mode), P.silu_exact(a, b, mode)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.isfinite(want.astype(np.float32)).all()
    ref = _teeth("silu_mul", (a, b), mode, clip, f"silu_mul {mode} {clip} H={H}")
    y = P.tail_rows(mode, clip, H)                            # the rows that are 32 x a half came through unchanged: the planted ties are there
    exact = ((y.astype(np.float32) / np.float32(P.GATE)).astype(np.float16).astype(np.float32) * np.float32(P.GATE) == y.astype(np.float32)).all(axis=1)
    n = len(y) - len(P.EDGE_NAMES)                            # the tie rows and the searched rows
    assert exact[:n].all() and exact.sum() >= n + 5
    t = P.run("reorder", (y, None), mode, clip)
    for k in ("q4", "q8", "s4", "s8"):
        assert np.array_equal(np.asarray(ref[k])[:len(y)][exact], np.asarray(t[k])[exact]), k
    a, b = P.silu_random(7, 1408, seed=1)
    got, want = O.silu_mul(a, b, mode), P.silu_exact(a, b, mode)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and (a == 0).any() and np.isfinite(want.astype(np.float32)).all()


@pytest.mark.parametrize("H", sorted(set(P.NORM_HS) | {K for op, _, K, _ in P.MULTI_Q_CASES if "rmsnorm" in op}))
@pytest.mark.parametrize("eps", P.EPS)
@pytest.mark.parametrize("mode,clip", P.NORM_MODE_CLIPS + [("kernel", 0.9)])
def test_rmsnorm_rows_have_teeth(mode, clip, eps, H):
    x, w, idx = P.norm_rows(H, mode, clip, eps)
    assert len(x) == len(P.NORM_NAMES) + (2 if mode == "kernel" else 0)
    ss = O.sumsq_tree(x[3:4])[0]
    assert 2.0 ** 24 * 0.9 < ss < 2.0 ** 24 * 1.2             # the squares' sum sits at the top of FP32's exact integers
    _teeth("rmsnorm", (x, w, eps, idx), mode, clip, f"rmsnorm {mode} {clip} eps={eps} H={H}")
    xa, res = P.add_split(x)                                  # add-RMSNorm: the same rows as a finite x + residual
    assert np.isfinite(xa.astype(np.float32)).all() and np.isfinite(res.astype(np.float32)).all()
    s = (xa.astype(np.float32) + res.astype(np.float32)).astype(np.float16)
    assert np.array_equal(s.view(np.uint16), x.view(np.uint16)) and (res != 0).mean() > 0.5


def test_u4_vectors_have_teeth():
    v = P.u4_vectors()
    assert len(v) == len(P.U4_NAMES) and np.array_equal(v.astype(np.float16).astype(np.float32), v)      # exact in fp16
    q, sz = P.quant_o4(v)
    assert np.isfinite(sz.astype(np.float32)).all()
    name = dict(zip(P.U4_NAMES, range(len(v))))
    assert (sz[[name["constant"], name["constant_zero"], name["constant_negative"]], 0, 0] == 0).all()
    sub = sz[name["subnormal_scale"], 0, 0]
    assert 0 < float(sub) < 2.0 ** -14                        # a subnormal half
    for m in P.U4_MUTANTS:
        qm, szm = P.quant_o4(v, mutate=m)
        nq = ((q & 0xF) != (qm & 0xF)).sum() + ((q >> 4) != (qm >> 4)).sum()
        ns = (sz.view(np.uint16) != szm.view(np.uint16)).sum()
        rows = ((q != qm).any(axis=1) | (sz.view(np.uint16) != szm.view(np.uint16)).any(axis=(1, 2))).sum()
        print(f"u4 {m}: {nq} codes, {ns} parameter halves, {rows} of {len(v)} vectors")
        assert nq + ns > 0
        if m == "round_rule":
            assert rows >= 5                                  # every tie vector
    for b, h in ((3, 3), (2, 3)):                              # the deals the GPU tests use reach every vector within a few steps
        seen = set()
        for step in range(6):
            m = P.u4_matrix(b, h, seed=step * b * h).reshape(-1, 128)
            seen |= {int(np.flatnonzero((v == r).all(axis=1))[0]) for r in m}
        assert seen == set(range(len(v)))
