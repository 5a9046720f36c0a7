"""GPU tests of sliding-window attention over the paged INT4 cache (ops.batch_decode_i4 / ops.batch_prefill_i4 with ``window=``:
atom_batch_decode_gqa_i4_win, atom_batch_prefill_gqa_i4_win) on the planted inputs of tests/attn_planted.py, against the closed form
and the FP64 reference of tests/attn_window_ref.py.  tests/test_attn_window_cpu.py proves on the CPU, for exactly these cases and
windows, that a lower bound off by one key either way, taken from the chunk's first row or from the sequence's end, or dropped, moves
the closed form by >= 10 x the bound applied here.

Bound: 4e-3 max|ref| + 1e-3 per (query row, head) (attn_planted.bound) for EVERY case, MHA decode included: the windowed op is always
the matrix-core kernel.  Every case runs with the host knowing the longest sequence (the window's tiles split over workgroups where
the plan splits, partial states merged) and with max_pages = 0 (one pass).  The cross product of cases and windows is trimmed: each
case takes three to five windows, every window at least twice per op."""
import types

import numpy as np
import pytest
import torch

from tests import attn_planted as A
from tests import attn_window_ref as W
from tests.helpers import t2n

pytestmark = pytest.mark.gpu

DECODE_WINDOWS = [(1, 64, 300, 600), (2, 63, 65, 300), (16, 100, 128, 600), (1, 63, 64, 100, 300), (2, 16, 65, 128)]
PREFILL_WINDOWS = [(1, 64, 600), (2, 65, 300), (16, 100, 600), (63, 128, 300), (1, 16, 64, 100), (2, 63, 65, 128, 600)]
DECODE = list(zip(W.DECODE_CASES, DECODE_WINDOWS))
PREFILL = list(zip(W.PREFILL_CASES, PREFILL_WINDOWS))
for _runs in (DECODE_WINDOWS, PREFILL_WINDOWS):
    assert all(sum(w in ws for ws in _runs) >= 2 for w in W.WINDOWS)


def _id(cw):
    return A.case_id(cw[0]) + "-w" + "_".join(map(str, cw[1]))


def _kv(c, P):
    """the planted arrays on the device, as the ops take a cache"""
    dev = torch.device("cuda")
    return types.SimpleNamespace(data=torch.from_numpy(c["data"]).to(dev), param=torch.from_numpy(c["param"]).to(dev),
                                 indptr=torch.from_numpy(c["indptr"]).to(dev), indicies=torch.from_numpy(c["indices"]).to(dev),
                                 last_page_offset=torch.from_numpy(c["lpo"]).to(dev), max_pages=max(-(-s // P) for s in c["seqlens"]))


def _run(kv, q, qo_d, max_q, split, window, **rope):
    """the op of the case (qo_d None: decode), the KV range split (where the plan splits) or not"""
    from atom_amd import ops
    full = kv.max_pages
    kv.max_pages = full if split else 0
    try:
        if qo_d is None:
            return t2n(ops.batch_decode_i4(q, kv, A.LAYER, window=window, **rope))
        return t2n(ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, window=window, **rope))
    finally:
        kv.max_pages = full


def _assert_splits(kv, case, prefill, qo, max_q, window):
    """the split run splits where the issue's shapes make the plan split: W >= 300 with the 2100-token sequence (decode), W = 600 with
    the (2000, 8) chunk (prefill); elsewhere the plan's answer is taken as it comes (and checked against the library's query)"""
    from atom_amd import ops
    from atom_amd._lib import lib
    _, P, nkv, G = case
    B = kv.last_page_offset.numel()
    if prefill:
        ws = lib().atom_batch_prefill_gqa_i4_win_workspace_bytes(int(qo[-1]), B, nkv * G, nkv, P, max_q, kv.max_pages, window)
        state = int(qo[-1]) * nkv * G * 130 * 4              # one partial state per (row, query head) and split
        splits = ws // state if ws else 1
        assert ws == (splits * state if splits >= 2 else 0)
        if window == 600:
            assert splits >= 2
        return
    splits = ops.decode_splits(B, kv, nkv * G, window=window)
    assert splits == lib().atom_batch_decode_gqa_i4_win_splits(B, nkv * G, nkv, P, kv.max_pages, window) >= 1
    if window >= 300 and max(case[0]) == 2100:
        assert splits >= 2


def _membership(case, windows, prefill):
    _, P, nkv, G = case
    lens, qo_ref, qo, max_q = W.case_shape(case, prefill)
    qo_d = None if qo is None else torch.from_numpy(qo).cuda()
    q = torch.from_numpy(A.membership_queries(int(qo_ref[-1]), nkv * G, 3)).cuda()
    worst = 0.0
    for w in A.window_starts(max(lens)):
        c = A.build_membership(lens, nkv, P, w, seed=3)
        kv = _kv(c, P)
        for win in windows:
            if w == 0:
                _assert_splits(kv, case, prefill, qo, max_q, win)
            want = W.membership_expected(c, qo_ref, G, win)
            for split in (True, False):
                r = A.error_ratio(_run(kv, q, qo_d, max_q, split, win), want, W.REL)
                worst = max(worst, r.max())
                row, head = np.unravel_index(np.argmax(r), r.shape)
                assert r.max() <= 1.0, (w, win, split, int(row), int(head), r.max())
    print(f"membership {A.case_id(case)} prefill={prefill} windows {windows}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("cw", DECODE, ids=_id)
def test_membership_decode(cw):
    """Uniform softmax over exact-zero keys, one hot dimension per planted token: the row at p holds 15 s / min(p + 1, W) in the
    dimensions of the planted tokens in (p - W, p] and 0 elsewhere, for every planted range (steps of 64)."""
    _membership(*cw, prefill=False)


@pytest.mark.parametrize("cw", PREFILL, ids=_id)
def test_membership_prefill(cw):
    """As the decode test; every row of a chunk must hold the closed form of ITS OWN position's window."""
    _membership(*cw, prefill=True)


def _needle(case, windows, theta, prefill):
    _, P, nkv, G = case
    lens, qo_ref, qo, max_q = W.case_shape(case, prefill)
    qo_d = None if qo is None else torch.from_numpy(qo).cuda()
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 5)
    kv, q, memo = _kv(c, P), torch.from_numpy(qn).cuda(), {}
    for win in windows:
        _assert_splits(kv, case, prefill, qo, max_q, win)
        ref = W.ref_prefill(qn, c, qo_ref, win, G=G, theta=theta, memo=memo)
        for split in (True, False):
            got = _run(kv, q, qo_d, max_q, split, win, rope_theta=theta)
            r = A.error_ratio(got, ref, W.REL)
            row, head = np.unravel_index(np.argmax(r), r.shape)
            print(f"needle {A.case_id(case)} prefill={prefill} theta={theta:g} W={win} split={split}: worst error / bound {r.max():.3f} "
                  f"(row {row}, head {head})")
            assert r.max() <= 1.0, (win, split, int(row), int(head), r.max())


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("cw", DECODE, ids=_id)
def test_needle_decode(cw, theta):
    """Peaked softmax over zero-mean random keys and values: RoPE at every key's own position inside the window"""
    _needle(*cw, theta, prefill=False)


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("cw", PREFILL, ids=_id)
def test_needle_prefill(cw, theta):
    _needle(*cw, theta, prefill=True)


@pytest.mark.parametrize("prefill,case", [(False, W.DECODE_CASES[0]), (False, W.DECODE_CASES[1]), (True, W.PREFILL_CASES[0]),
                                          (True, W.PREFILL_CASES[5])], ids=lambda v: A.case_id(v) if isinstance(v, tuple) else str(v))
def test_window_that_covers_every_sequence_is_plain_causal(prefill, case):
    """W >= every length: the un-windowed op's output within twice the bound (at G = 1 the un-windowed decode op is the FP32 kernel,
    the windowed one the matrix-core kernel), and the FP64 reference of plain causal attention within the bound"""
    from atom_amd import ops
    _, P, nkv, G = case
    lens, qo_ref, qo, max_q = W.case_shape(case, prefill)
    qo_d = None if qo is None else torch.from_numpy(qo).cuda()
    c = A.build_needle(lens, nkv, P, seed=7)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 7)
    kv, q = _kv(c, P), torch.from_numpy(qn).cuda()
    plain = t2n(ops.batch_decode_i4(q, kv, A.LAYER)) if qo_d is None else t2n(ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q))
    ref = A.ref_prefill(qn, c, qo_ref, G=G)
    for win in (max(lens), max(lens) + 1, (1 << 31) - 1):
        for split in (True, False):
            got = _run(kv, q, qo_d, max_q, split, win)
            assert A.error_ratio(got, ref, W.REL).max() <= 1.0, (win, split)
            assert A.error_ratio(got, plain.astype(np.float64), W.REL).max() <= 2.0, (win, split)


@pytest.mark.parametrize("G,nkv,seqlens,win", [(2, 2, [2500], 700), (1, 4, [2500], 1000)])
def test_unmerged_partial_states_merge_inside_o_proj(G, nkv, seqlens, win):
    """merge=False -> dense_layer_gemm_i4_merge_q gives the bits of merge=True + reorder + o_proj (as tests/test_gpu_gqa.py shows for
    the un-windowed op), for a grouped-query and an MHA cache; the splits come from decode_splits(.., window=)"""
    from atom_amd import ops
    from atom_amd.e2e.llama import LinearInt4
    c = A.build_needle(seqlens, nkv, 16, seed=11)
    kv = _kv(c, 16)
    nq, batch = G * nkv, len(seqlens)
    q = torch.from_numpy(A.needle_queries(batch, nq, 11)).cuda()
    o = ops.batch_decode_i4(q, kv, A.LAYER, window=win)
    ref = W.ref_decode(t2n(q), c, win, G=G)
    assert A.error_ratio(t2n(o), ref, W.REL).max() <= 1.0
    splits = ops.decode_splits(batch, kv, nq, window=win)
    assert splits >= 2
    part = ops.batch_decode_i4(q, kv, A.LAYER, merge=False, window=win)
    assert part.shape == (batch, nq, splits, 130)
    hs = nq * 128
    assert ops.merge_q_gemm_fits(batch, hs, 1, hs, splits)
    proj = LinearInt4(hs, hs, "fp16").cuda()
    gw = torch.Generator().manual_seed(2)
    proj.load_fp16_weight((torch.randn(hs, hs, generator=gw) * 0.05).half().cuda())
    ridx = torch.randperm(hs, generator=gw).to(torch.int16).cuda()
    (fused,) = ops.dense_layer_gemm_i4_merge_q(part, splits, proj.single(), reorder_index=ridx)
    (sep,), _ = ops.dense_layer_gemm_i4_multi_q("reorder", o.view(batch, hs), proj.single(), reorder_index=ridx)
    assert torch.equal(fused, sep)


def test_ops_refuse_a_bad_window():
    from atom_amd import ops
    c = A.build_needle([40, 3], 2, 16, seed=1)
    kv = _kv(c, 16)
    q = torch.from_numpy(A.needle_queries(2, 4, 1)).cuda()
    qo = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    for bad in (0, -1, 2.0, "8", True):
        with pytest.raises(ValueError, match="window"):
            ops.batch_decode_i4(q, kv, A.LAYER, window=bad)
        with pytest.raises(ValueError, match="window"):
            ops.batch_prefill_i4(q, qo, kv, A.LAYER, window=bad)
        with pytest.raises(ValueError, match="window"):
            ops.decode_splits(2, kv, 4, window=bad)
    k32 = torch.zeros((2, 2 * 128), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="append_kv"):
        ops.batch_decode_i4(q[:, :2].contiguous(), kv, A.LAYER, append_kv=(k32, k32), window=8)
    # one query per sequence: the prefill entry is the decode entry
    assert torch.equal(ops.batch_prefill_i4(q, qo, kv, A.LAYER, window=8, max_q_len=1), ops.batch_decode_i4(q, kv, A.LAYER, window=8))
