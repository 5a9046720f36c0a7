"""CPU-only: the planted attention inputs of tests/attn_planted.py have teeth.  For every shape and parameter set that
tests/test_gpu_attn_planted.py runs, every deliberate error that applies (the ``mutate=`` argument of the FP64 references) leaves
the correct FP64 reference by at least 10 x the bound the GPU test applies -- so a kernel that made that error could not pass --,
and the membership family's closed form equals the FP64 reference to 1e-12.  These are conditions on the INPUTS: where one is
missed, the inputs change (window, scales, NEEDLE_A), never the factor.

Which mutant is checked where, and over which rows ("affected"):
  membership  drop_key / double_key: every key of attn_planted.checked_keys, in a window that holds it: every row that sees the
              key (double_key: and another one), every head.  causal_plus_one (prefill): every row whose next key lies in the
              window, every head.  read_past_end: every row of a sequence whose last page has slots behind its end, every head.
              other_layer: every row and head.
              head_mod (G > 1, more than one K/V head): every head it re-maps, every row that sees >= 15 keys (a one-token
              window holds one scale per head: two draws may lie close).  Position mutants do not apply: zero keys, uniform softmax.
  needle      q_pos_minus_one, key_pos_plus_one, theta, interleaved_pairs, ignore_rope_scale (rope_scale != 1): every sequence of
              >= 2 tokens, its largest (row, head).  other_layer: every row and head.  head_mod: every row, its largest head.
              swap_pages: the longest sequence, the page of its heaviest key against the page half a sequence away.  read_past_end,
              causal_plus_one (calls with a sequence of <= 64 tokens): the call's largest (row, head) -- the short sequences carry
              them; the membership family covers the long ones.  drop_key / double_key do not apply: a random key holds ~1 / S of
              the weight."""
import numpy as np
import pytest

from tests import attn_planted as A

FACTOR = 10.0


def _mut_ratio(ref_fn, ref, rel, mutate, seqs=None):
    return A.error_ratio(ref_fn(mutate=mutate, seqs=seqs), ref, rel)


def _membership(shape, P, nkv, G, prefill):
    if prefill:
        lens, qo = A.prefill_shape(shape)
    else:
        lens, qo = list(shape), np.arange(len(shape) + 1)
    rel, tile = A.rel_bound(G, prefill), A.key_tile(G, prefill)
    q = A.membership_queries(int(qo[-1]), nkv * G, 3)
    want = {(b, j) for b, S in enumerate(lens) for j in A.checked_keys(S, P, tile)}
    seen = set()
    covered = [np.zeros(S, dtype=bool) for S in lens]
    starts = A.window_starts(max(lens))
    memo = {}
    for w in starts:
        c = A.build_membership(lens, nkv, P, w, seed=3)
        for k in [k for k in memo if k[0] == "v"]:           # the window moves in the values alone: the keys (and the page tables, the
            del memo[k]                                      # other layer: same seed) are the same bytes in every window
        fn = lambda **kw: A.ref_prefill(q, c, qo, G=G, memo=memo, **kw)
        ref = fn()
        assert np.abs(ref - A.membership_expected(c, qo, G)).max() <= 1e-12
        for b, S in enumerate(lens):
            r0, r1 = int(qo[b]), int(qo[b + 1])
            pos = np.arange(S - (r1 - r0), S)
            wb = c["win"][b]
            covered[b][wb:wb + A.WINDOW] = True
            for j in A.checked_keys(S, P, tile):
                if not wb <= j < wb + A.WINDOW or (b, j) in seen:
                    continue
                seen.add((b, j))
                for kind in ("drop_key", "double_key"):
                    rows = (pos >= j) & ((pos >= 1) | (kind == "drop_key"))      # (a row's ONLY key counted twice changes nothing)
                    if rows.any():
                        r = _mut_ratio(fn, ref, rel, {kind: j}, seqs=[b])[r0:r1][rows]
                        assert r.min() >= FACTOR, (kind, w, b, j, r.min())
            if prefill:
                rows = (pos + 1 >= wb) & (pos + 1 < min(wb + A.WINDOW, S))
                if rows.any():
                    r = _mut_ratio(fn, ref, rel, {"causal_plus_one": True}, seqs=[b])[r0:r1][rows]
                    assert r.min() >= FACTOR, ("causal_plus_one", w, b, r.min())
        if w in (starts[0], starts[-1]):
            r = _mut_ratio(fn, ref, rel, {"other_layer": True})
            assert r.min() >= FACTOR, ("other_layer", w, r.min())
            r = _mut_ratio(fn, ref, rel, {"read_past_end": True})
            tails = [b for b in range(len(lens)) if c["lpo"][b] < P]
            assert tails
            for b in tails:
                assert r[int(qo[b]):int(qo[b + 1])].min() >= FACTOR, ("read_past_end", w, b)
            if G > 1 and nkv > 1:
                r = _mut_ratio(fn, ref, rel, {"head_mod": True})
                moved = [h for h in range(nkv * G) if h % nkv != h // G]
                for b, S in enumerate(lens):
                    rows = np.arange(S - int(qo[b + 1] - qo[b]), S) >= 14
                    if rows.any():
                        assert r[int(qo[b]):int(qo[b + 1])][rows][:, moved].min() >= FACTOR, ("head_mod", w, b)
    assert seen == want
    assert all(cv.all() for cv in covered)                    # every position of every sequence lay in some window


@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_membership_decode_has_teeth(case):
    _membership(*case, prefill=False)


@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_membership_prefill_has_teeth(case):
    _membership(*case, prefill=True)


def _needle(shape, P, nkv, G, theta, scale, prefill):
    if prefill:
        lens, qo = A.prefill_shape(shape)
    else:
        lens, qo = list(shape), np.arange(len(shape) + 1)
    rel = A.rel_bound(G, prefill)
    c = A.build_needle(lens, nkv, P, seed=5)
    q = A.needle_queries(int(qo[-1]), nkv * G, 5)
    memo = {}
    fn = lambda **kw: A.ref_prefill(q, c, qo, G=G, theta=theta, rope_scale=scale, memo=memo, **kw)
    ref = fn()
    per_seq = lambda r: [r[int(qo[b]):int(qo[b + 1])].max() for b in range(len(lens))]
    positional = [{"q_pos_minus_one": True}, {"key_pos_plus_one": True}, {"theta": A.OTHER_THETA[theta]}, {"interleaved_pairs": True}]
    if scale != 1.0:
        positional.append({"ignore_rope_scale": True})
    for m in positional:
        for b, r in enumerate(per_seq(_mut_ratio(fn, ref, rel, m))):
            if lens[b] >= 2:
                assert r >= FACTOR, (m, b, r)
    assert _mut_ratio(fn, ref, rel, {"other_layer": True}).min() >= FACTOR
    if G > 1 and nkv > 1:
        assert _mut_ratio(fn, ref, rel, {"head_mod": True}).max(axis=1).min() >= FACTOR
    if min(lens) <= 64:
        assert _mut_ratio(fn, ref, rel, {"read_past_end": True}).max() >= FACTOR
    if prefill and min(lens) <= 64:
        assert _mut_ratio(fn, ref, rel, {"causal_plus_one": True}).max() >= FACTOR
    b = int(np.argmax(lens))
    npages = int(c["indptr"][b + 1] - c["indptr"][b])
    pa = A.top_key(q, c, qo, b, 0, G=G, theta=theta, rope_scale=scale) // P
    r = _mut_ratio(fn, ref, rel, {"swap_pages": (pa, (pa + npages // 2) % npages)}, seqs=[b])
    assert per_seq(r)[b] >= FACTOR, ("swap_pages", pa, per_seq(r)[b])


@pytest.mark.parametrize("theta,scale", A.ROPE_PARAMS)
@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_needle_decode_has_teeth(case, theta, scale):
    _needle(*case, theta, scale, prefill=False)


@pytest.mark.parametrize("theta,scale", A.ROPE_PARAMS)
@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_needle_prefill_has_teeth(case, theta, scale):
    _needle(*case, theta, scale, prefill=True)


def test_the_cases_split_their_kv_range():
    """every decode case splits its KV range when the host knows the longest sequence (the GPU test runs it split and unsplit), and
    so does every prefill case (a non-empty workspace = partial states + merge)"""
    from atom_amd._lib import lib
    L = lib()
    for lens, P, nkv, G in A.DECODE_CASES:
        mp = max(-(-s // P) for s in lens)
        assert L.atom_batch_decode_gqa_i4_splits(len(lens), nkv * G, nkv, P, mp) >= 2
        assert L.atom_batch_decode_gqa_i4_splits(len(lens), nkv * G, nkv, P, 0) == 1
    for shape, P, nkv, G in A.PREFILL_CASES:
        lens, qo = A.prefill_shape(shape)
        mp, mq = max(-(-s // P) for s in lens), max(n for _, n in shape)
        assert L.atom_batch_prefill_gqa_i4_workspace_bytes(int(qo[-1]), len(lens), nkv * G, nkv, P, mq, mp) > 0
        assert L.atom_batch_prefill_gqa_i4_workspace_bytes(int(qo[-1]), len(lens), nkv * G, nkv, P, mq, 0) == 0
