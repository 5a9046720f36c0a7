"""GPU tests of the four paged INT4 attention ops (atom_batch_decode_i4, atom_batch_decode_gqa_i4, atom_batch_prefill_i4,
atom_batch_prefill_gqa_i4) on the planted inputs of tests/attn_planted.py, against its unmutated FP64 references.  On these inputs one
lost or doubled key, a causal edge or a position off by one, a wrong RoPE base / scale / pairing, a wrong page, K/V head or layer and a
read behind a sequence's end each move the reference by >= 10 x the bound applied here (tests/test_attn_planted_cpu.py proves that on
the CPU for exactly these cases), so none of them can hide inside it.

Bounds: the ops' existing ones -- decode 2e-3 max|ref| + 1e-3, prefill and grouped-query 4e-3 max|ref| + 1e-3 -- per (query row, head)
(attn_planted.bound).  Every decode case runs with the host knowing the longest sequence (KV range split over waves / workgroups and
merged) and with max_pages = 0 (no split); every prefill case likewise (partial states + merge / one pass)."""
import types

import numpy as np
import pytest
import torch

from tests import attn_planted as A
from tests.helpers import t2n

pytestmark = pytest.mark.gpu


def _kv(c, P):
    """the planted arrays on the device, as the ops take a cache"""
    dev = torch.device("cuda")
    return types.SimpleNamespace(data=torch.from_numpy(c["data"]).to(dev), param=torch.from_numpy(c["param"]).to(dev),
                                 indptr=torch.from_numpy(c["indptr"]).to(dev), indicies=torch.from_numpy(c["indices"]).to(dev),
                                 last_page_offset=torch.from_numpy(c["lpo"]).to(dev), max_pages=max(-(-s // P) for s in c["seqlens"]))


def _run(kv, q, qo_d, max_q, split, **rope):
    """the op of the case (qo_d None: decode), KV range split or not"""
    from atom_amd import ops
    full = kv.max_pages
    kv.max_pages = full if split else 0
    try:
        if qo_d is None:
            return t2n(ops.batch_decode_i4(q, kv, A.LAYER, **rope))
        return t2n(ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, **rope))
    finally:
        kv.max_pages = full


def _assert_splits(kv, P, nkv, G, qo, max_q):
    """the split runs really split"""
    from atom_amd import ops
    from atom_amd._lib import lib
    B = kv.last_page_offset.numel()
    if qo is None:
        assert ops.decode_splits(B, kv, nkv * G) >= 2
    else:
        assert lib().atom_batch_prefill_gqa_i4_workspace_bytes(int(qo[-1]), B, nkv * G, nkv, P, max_q, kv.max_pages) > 0


def _shape(case, prefill):
    shape, P, nkv, G = case
    if prefill:
        lens, qo = A.prefill_shape(shape)
        return lens, qo, torch.from_numpy(qo).cuda(), max(n for _, n in shape)
    return list(shape), None, None, 1


def _membership(case, prefill):
    shape, P, nkv, G = case
    lens, qo, qo_d, max_q = _shape(case, prefill)
    qo_ref = np.arange(len(lens) + 1) if qo is None else qo
    rel = A.rel_bound(G, prefill)
    q = torch.from_numpy(A.membership_queries(int(qo_ref[-1]), nkv * G, 3)).cuda()
    worst = 0.0
    for w in A.window_starts(max(lens)):
        c = A.build_membership(lens, nkv, P, w, seed=3)
        kv = _kv(c, P)
        if w == 0:
            _assert_splits(kv, P, nkv, G, qo, max_q)
        want = A.membership_expected(c, qo_ref, G)
        for split in (True, False):
            r = A.error_ratio(_run(kv, q, qo_d, max_q, split), want, rel)
            worst = max(worst, r.max())
            row, head = np.unravel_index(np.argmax(r), r.shape)
            assert r.max() <= 1.0, (w, split, int(row), int(head), r.max())
    print(f"membership {A.case_id(case)} prefill={prefill}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_membership_decode(case):
    """Uniform softmax over exact-zero keys; one hot dimension per window token: the output row is 15 s / S in the dimensions of the
    window tokens and 0 elsewhere, for every window position (steps of 64: both sides of every tile, page and KV-split boundary in one
    window), KV range split and not."""
    _membership(case, prefill=False)


@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_membership_prefill(case):
    """As the decode test; row i of a sequence must hold the closed form over exactly the keys <= prefix + i."""
    _membership(case, prefill=True)


def _needle(case, theta, scale, prefill):
    shape, P, nkv, G = case
    lens, qo, qo_d, max_q = _shape(case, prefill)
    qo_ref = np.arange(len(lens) + 1) if qo is None else qo
    rel = A.rel_bound(G, prefill)
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 5)
    kv = _kv(c, P)
    _assert_splits(kv, P, nkv, G, qo, max_q)
    ref = A.ref_prefill(qn, c, qo_ref, G=G, theta=theta, rope_scale=scale)
    q = torch.from_numpy(qn).cuda()
    for split in (True, False):
        got = _run(kv, q, qo_d, max_q, split, rope_theta=theta, rope_scale=scale)
        r = A.error_ratio(got, ref, rel)
        row, head = np.unravel_index(np.argmax(r), r.shape)
        print(f"needle {A.case_id(case)} prefill={prefill} theta={theta:g} scale={scale:g} split={split}: worst error / bound {r.max():.3f} "
              f"(row {row}, head {head}: error {np.abs(got[row, head] - ref[row, head]).max():.3e}, max|ref| {np.abs(ref[row, head]).max():.3f})")
        assert r.max() <= 1.0, (split, int(row), int(head), r.max())


@pytest.mark.parametrize("theta,scale", A.ROPE_PARAMS)
@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_needle_decode(case, theta, scale):
    """Peaked softmax over zero-mean random keys and values, every (rope_theta, rope_scale) pair: relative positions up to 2099, the
    decode kernel's per-tile incremental rotation over 132 tiles."""
    _needle(case, theta, scale, prefill=False)


@pytest.mark.parametrize("theta,scale", A.ROPE_PARAMS)
@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_needle_prefill(case, theta, scale):
    _needle(case, theta, scale, prefill=True)
