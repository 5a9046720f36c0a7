"""GPU tests of attention sinks over the INT4 paged KV cache (StreamingLLM): the _sink attention entries against an
inline FP64 reference, the same entries on a ring list against a list that released nothing (bit for bit), the step with pinned sink
pages (atom_kv_step_sink_i4) against numpy, and ``generate(streaming=)`` against an eager loop on a cache that releases nothing.

The contract: sinks S, window W, per sequence a shift.  The row at position p sees key j iff j <= p and (j < S or j > p - W); the
query rotates by p - shift, a key j < S by j, a key j >= S by j - shift; shift = max(0, p0 - W + 1 - S), p0 the position of the
sequence's first query row.  The bound is the matrix-core ops': 4e-3 max|ref| + 1e-3 per (row, head) (attn_window_ref.REL).

What the two halves of the contract are worth on the 2100-token row of the decode batch (P = 16, 2 K/V heads, G = 4; the FP64 reference
against itself on the CPU, in units of that bound, not asserted): at (S, W) = (64, 16) evaluating with shift = 0 moves every head by
19.7 .. 554 bounds and dropping the ``j < S`` term by 31.3 .. 336; the worst head of the other pairs moves by 129 .. 335 (shift = 0) and
103 .. 399 (no sinks) bounds: (1, 1) 335 / 399, (4, 16) 230 / 154, (16, 63) 294 / 119, (17, 100) 129 / 103."""
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import attn_planted as A
from tests import attn_window_ref as W
from tests.helpers import t2n

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FULL_PAGES = 1 << 15            # max_pages of a list that released nothing: large, so that the window bound governs the plan
SINK_WINDOW = [(1, 1), (4, 16), (16, 63), (17, 100), (64, 16)]
CHUNKS = [(0, 200), (40, 150), (300, 7), (2000, 8)]           # (prefix, q_len); the first two are prompt prefills
RING_CHUNKS, MAX_ADD = [(0, 5), (20, 8), (300, 7), (2000, 8)], 8


def _lens(S, Wn):
    """below the sinks, nothing evicted yet, the first eviction, the tile edges, split boundaries inside the window"""
    return [1, 3, S, S + Wn, S + Wn + 1, 65, 129, 300, 2100]


def _shifts(lens, q_lens, S, Wn):
    return np.asarray([max(0, n - q - Wn + 1 - S) for n, q in zip(lens, q_lens)], dtype=np.int32)


def ref_sinks(qn, c, qo, S, Wn, shifts, G, sinks=True):
    """attn_window_ref.ref_prefill with the ``j < S`` term in ``seen``, the query rotated by pos - shift and the keys by
    where(j < S, j, j - shift).  q f16 [T, nkv * G, 128] -> float64."""
    data, param, indptr, indices = c["data"], c["param"], c["indptr"], c["indices"]
    q64 = np.asarray(qn).astype(np.float64)
    nkv, P = data.shape[3], data.shape[4]
    out = np.zeros(q64.shape)
    for b, n in enumerate(c["seqlens"]):
        r0, r1 = int(qo[b]), int(qo[b + 1])
        pos, j = np.arange(n - (r1 - r0), n), np.arange(n)
        seen = (j[None, :] <= pos[:, None]) & ((j[None, :] > pos[:, None] - Wn) | ((j[None, :] < S) & sinks))
        pages = [int(x) for x in indices[int(indptr[b]):int(indptr[b + 1])]]
        qf = A._rope(q64[r0:r1].transpose(1, 0, 2), pos - shifts[b], 1e4, 1.0)            # [heads, rows, D]
        for hk in range(nkv):
            gather = lambda a, which: a[pages, A.LAYER, which, hk].reshape(len(pages) * P, -1)[:n]
            kf = A._rope(O._dequant_u4_rows(gather(data, 0), gather(param, 0)), np.where(j < S, j, j - shifts[b]), 1e4, 1.0)
            vf = O._dequant_u4_rows(gather(data, 1), gather(param, 1))
            hs, vis = list(range(hk * G, hk * G + G)), np.tile(seen, (G, 1))
            s = np.where(vis, qf[hs].reshape(-1, A.D) @ kf.T / np.sqrt(A.D), -np.inf)
            pr = np.exp(s - s.max(axis=1, keepdims=True))                                  # (every row sees its own key)
            out[r0:r1, hs] = ((pr / pr.sum(axis=1, keepdims=True)) @ vf).reshape(G, r1 - r0, A.D).transpose(1, 0, 2)
    return out


def _dev_kv(c, max_pages, **more):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return types.SimpleNamespace(data=t(c["data"]), param=t(c["param"]), indptr=t(c["indptr"]), indicies=t(c["indices"]),
                                 last_page_offset=t(c["lpo"]), max_pages=max_pages, **{k: t(v) if isinstance(v, np.ndarray) else v
                                                                                      for k, v in more.items()})


def _run(kv, q, qo, max_q, S, Wn, shifts, **rope):
    from atom_amd import ops
    kw = dict(window=Wn, sinks=S, pos_shift=torch.from_numpy(shifts).to(DEV), **rope)
    if qo is None:
        return ops.batch_decode_i4(q, kv, A.LAYER, **kw)
    return ops.batch_prefill_i4(q, torch.from_numpy(qo).to(DEV), kv, A.LAYER, max_q_len=max_q, **kw)


def _problems(S, Wn, chunks):
    """(sequence lengths, qo_indptr for the reference, qo_indptr for the op or None, max_q_len, q_len per sequence): decode, chunks"""
    lens = _lens(S, Wn)
    yield lens, np.arange(len(lens) + 1), None, 1, [1] * len(lens)
    lens, qo = A.prefill_shape(chunks)
    yield lens, qo, qo, max(n for _, n in chunks), [n for _, n in chunks]


@pytest.mark.parametrize("nkv,G", [(2, 1), (2, 4), (4, 7)])
@pytest.mark.parametrize("P", [16, 48, 128])         # 128: the sink pages span more than one key tile
@pytest.mark.parametrize("S,Wn", SINK_WINDOW)
def test_sink_attention_against_fp64(S, Wn, P, nkv, G):
    """decode batch and chunked rows, the theta and the table form, within the matrix-core bound of the FP64 reference"""
    from atom_amd import ops
    table = ops.rope_table(1e4 ** (-np.arange(64) / 64.0), DEV)
    for lens, qo_ref, qo, max_q, q_lens in _problems(S, Wn, CHUNKS):
        c = A.build_needle(lens, nkv, P, seed=S + Wn)
        qn = A.needle_queries(int(qo_ref[-1]), nkv * G, S + Wn)
        shifts = _shifts(lens, q_lens, S, Wn)
        ref = ref_sinks(qn, c, qo_ref, S, Wn, shifts, G)
        kv, q = _dev_kv(c, FULL_PAGES), torch.from_numpy(qn).to(DEV)
        for rope in ({}, dict(rope_table=table)):
            r = A.error_ratio(t2n(_run(kv, q, qo, max_q, S, Wn, shifts, **rope)), ref, W.REL)
            row, head = np.unravel_index(np.argmax(r), r.shape)
            print(f"S={S} W={Wn} P={P} kv={nkv} G={G} chunks={qo is not None} table={bool(rope)}: worst error / bound {r.max():.3f} "
                  f"(row {row}, head {head})")
            assert r.max() <= 1.0, (qo is not None, bool(rope), int(row), int(head), r.max())      # (a NaN fails this too)


def _sink_ring(c, S, Wn, adds, max_add, seed=0):
    """The planted cache ``c`` as atom_kv_step_sink_i4 leaves it after a step of adds[b] tokens: per sequence SP sink slots and a ring
    of R in a scrambled pool where every byte that no correct kernel may read is 0xFF (a NaN scale), as kv_ring_ref.ring_cache"""
    data, param, P, B = c["data"], c["param"], c["data"].shape[4], len(c["seqlens"])
    SP, R = -(-S // P), -(-(Wn - 1 + max_add) // P) + 1
    cap = B * (SP + R) + 3
    table = np.random.default_rng(seed + 17).permutation(cap).astype(np.int32)[:B * (SP + R)].reshape(B, SP + R)
    nd = np.full((cap,) + data.shape[1:], 0xFF, dtype=np.uint8)
    npar = np.full((cap,) + param.shape[1:], 0xFFFF, dtype=np.uint16).view(np.float16)
    cnts, idx, start = [], [], []
    for b, n in enumerate(c["seqlens"]):
        old = c["indices"][int(c["indptr"][b]):int(c["indptr"][b + 1])]
        l, f = (n - 1) // P, max(SP, max(0, n - max(adds[b], 1) - Wn + 1) // P)
        listed = [(g, table[b, g]) for g in range(min(SP, l + 1))] + [(g, table[b, SP + (g - SP) % R]) for g in range(f, l + 1)]
        for g, dst in listed:
            nd[dst], npar[dst] = data[old[g]], param[old[g]]
            if g == l and n % P:                              # behind the end: stale bytes
                nd[dst][:, :, :, n % P:] = 0xFF
                npar[dst].view(np.uint16)[:, :, :, n % P:] = 0xFFFF
        idx += [dst for _, dst in listed]
        cnts.append(len(listed))
        start.append(f * P)
    ring = dict(c, data=nd, param=npar, indptr=np.cumsum([0] + cnts).astype(np.int32), indices=np.asarray(idx, dtype=np.int32))
    return ring, np.asarray(start, dtype=np.int32), SP + R


@pytest.mark.parametrize("S,Wn,P,nkv,G", [(1, 1, 16, 2, 1), (4, 16, 16, 2, 4), (16, 63, 48, 2, 4), (17, 100, 48, 2, 1), (64, 16, 16, 4, 7),
                                          (64, 16, 48, 2, 4), (4, 100, 128, 2, 4), (17, 16, 256, 2, 1)])
def test_ring_list_equals_the_unreleased_list_bit_for_bit(S, Wn, P, nkv, G):
    """the _sink op on sink pages + ring pages (stale slots 0xFF) against the _sink op with kv_start = NULL on the full list: equal
    contents, shifts and split count, so equal bits -- decode and chunks, both RoPE forms"""
    from atom_amd import ops
    from atom_amd._lib import lib
    table = ops.rope_table(1e4 ** (-np.arange(64) / 64.0), DEV)
    for lens, qo_ref, qo, max_q, q_lens in _problems(S, Wn, RING_CHUNKS):
        c = A.build_needle(lens, nkv, P, seed=3)
        q = torch.from_numpy(A.needle_queries(int(qo_ref[-1]), nkv * G, 3)).to(DEV)
        shifts = _shifts(lens, q_lens, S, Wn)
        rc, start, slots = _sink_ring(c, S, Wn, q_lens, 1 if qo is None else MAX_ADD)
        if qo is None:
            plans = [lib().atom_batch_decode_gqa_i4_sink_splits(len(lens), nkv * G, nkv, P, mp, Wn) for mp in (slots, FULL_PAGES)]
        else:
            plans = [lib().atom_batch_prefill_gqa_i4_sink_workspace_bytes(int(qo[-1]), len(lens), nkv * G, nkv, P, max_q, mp, Wn)
                     for mp in (slots, FULL_PAGES)]
        assert plans[0] == plans[1]
        ring, full = _dev_kv(rc, slots, kv_start=start, sinks=S, window=Wn), _dev_kv(c, FULL_PAGES)
        for rope in ({}, dict(rope_table=table)):
            got = _run(ring, q, qo, max_q, S, Wn, shifts, **rope)
            assert torch.isfinite(got).all() and torch.equal(got, _run(full, q, qo, max_q, S, Wn, shifts, **rope)), (qo is not None, bool(rope))


def _step_ref(table, slots, lens, add, Wn, S, P):
    """atom_kv_step_sink_i4 in numpy: (lens', indptr, indices, lpo, kv_start, pos_shift, overflow)"""
    SP, new, rows, over = -(-S // P), [], [], False
    for b, n0 in enumerate(lens):
        for n, a in ((n0 + add, add), (n0, 0)):               # the step, or -- refused -- a step of 0 tokens to the old length
            lo, l = n - max(a, 1) - Wn + 1, (n - 1) // P
            f = max(SP, max(lo, 0) // P)
            if n <= 0 or (min(SP, l + 1) <= min(SP, slots[b]) and l - f + 1 <= slots[b] - SP):
                break
            over = True
        pages = [] if n <= 0 else [table[b, g] for g in range(min(SP, l + 1))] + [table[b, SP + (g - SP) % (slots[b] - SP)] for g in range(f, l + 1)]
        new.append(n)
        rows.append((pages, (n - 1) % P + 1 if n > 0 else 0, (f if n > 0 else SP) * P, max(lo - S, 0) if n > 0 else 0))
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return (i32(new), i32(np.cumsum([0] + [len(r[0]) for r in rows])), i32([x for r in rows for x in r[0]]), i32([r[1] for r in rows]),
            i32([r[2] for r in rows]), i32([r[3] for r in rows]), over)


@pytest.mark.parametrize("batch,P,Wn,S,add,short", [(1, 16, 1, 1, 1, None), (3, 16, 17, 4, 1, None), (65, 48, 100, 17, 1, None),
                                                    (130, 16, 63, 64, 1, None), (3, 16, 17, 4, 3, None), (3, 16, 17, 4, 1, 1)])
def test_sink_step_against_numpy(batch, P, Wn, S, add, short):
    """single-token steps (one case: steps of 3 on rings sized for 3) until the ring has wrapped twice: lengths, kv_indptr, kv_indices,
    last_page_offset, kv_start, pos_shift after every launch.  ``short``: a sequence with one ring slot -- it overflows, is flagged and
    not advanced, and every index it lists comes from its own row."""
    from atom_amd._lib import KV_STEP_OVERFLOW, current_stream, lib
    SP, R = -(-S // P), -(-(Wn - 1 + add) // P) + 1
    cap = SP + R
    table = np.random.default_rng(batch).permutation(batch * cap + 5)[:batch * cap].reshape(batch, cap).astype(np.int32)
    slots = [SP + 1 if b == short else cap for b in range(batch)]
    lens = np.asarray([(0, Wn - 1, S + Wn + 2 * P + 3)[b % 3] if b != short else 0 for b in range(batch)])
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)
    d_table, d_rows, dev = i32(table), i32(slots), i32(list(lens) + [0] * batch + [0, 0, 0, 0])
    out = torch.full((batch + 1 + batch * cap + 3 * batch,), -7, dtype=torch.int32, device=DEV)
    indptr, indices = out[:batch + 1], out[batch + 1:batch + 1 + batch * cap]
    lpo, start, shift = out[-3 * batch:-2 * batch], out[-2 * batch:-batch], out[-batch:]
    seen_over = False
    for _ in range(-(-2 * R * P // add) + SP * P + 2):
        st = lib().atom_kv_step_sink_i4(d_table.data_ptr(), d_rows.data_ptr(), dev.data_ptr(), indptr.data_ptr(), indices.data_ptr(),
                                        lpo.data_ptr(), dev[2 * batch:].data_ptr(), batch, cap, P, add, Wn, S, start.data_ptr(),
                                        shift.data_ptr(), current_stream(DEV))
        assert st == 0
        want = _step_ref(table, slots, lens, add, Wn, S, P)
        seen_over |= want[6]
        host, got = dev.tolist(), out.cpu().numpy()
        parity = host[2 * batch + 1] & 1
        assert host[2 * batch] == (KV_STEP_OVERFLOW if seen_over else 0) and host[2 * batch + 2] == 0
        assert host[parity * batch:(parity + 1) * batch] == want[0].tolist()
        assert np.array_equal(got[:batch + 1], want[1]) and np.array_equal(got[batch + 1:batch + 1 + want[1][-1]], want[2])
        for g, w in zip((lpo, start, shift), want[3:6]):
            assert g.cpu().tolist() == w.tolist()
        if short is not None:
            assert set(want[2][want[1][short]:want[1][short + 1]]) <= set(table[short, :slots[short]])
        lens = want[0]
    assert seen_over == (short is not None)
    assert short is None or lens[short] < lens[0]             # (both started empty)


PAGE = 16


def _cfg(heads, kv_heads, **extra):
    return types.SimpleNamespace(hidden_size=128 * heads, num_attention_heads=heads, num_key_value_heads=kv_heads, intermediate_size=512,
                                 rms_norm_eps=1e-5, rope_theta=1e4, num_hidden_layers=2, vocab_size=1000, pad_token_id=None, **extra)


def _pool(kv_heads, capacity):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(2, kv_heads, 128, capacity, PAGE, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def test_generate_streaming_equals_the_eager_loop_on_an_unreleased_cache():
    """two layers, 4 / 2 heads of 128, S = 4, W = 40, pages of 16, prompts of 5 and 90 tokens, 150 new tokens (the ring wraps more than
    once) out of a pool of exactly batch * (SP + R') pages; the model's streaming state is restored"""
    from atom_amd.e2e import LlamaForCausalLM, StreamingParams, generate
    from atom_amd.e2e.generate import _prefill
    from atom_amd.utils import BatchedKvCacheInt4, BatchLenInfo, KvCacheInt4
    S, Wn, new = 4, 40, 150
    torch.manual_seed(0)
    model, g = LlamaForCausalLM(_cfg(4, 2)).cuda(), torch.Generator().manual_seed(100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
    prompts = [torch.randint(0, 1000, (n,), generator=g).tolist() for n in (5, 90)]
    ring_pages = len(prompts) * (-(-S // PAGE) + -(-Wn // PAGE) + 1)
    pool = _pool(2, ring_pages)
    got = generate(model, prompts, new, pool, streaming=StreamingParams(sinks=S, window=Wn))
    assert model.streaming is None and all(layer.self_attn.window is None for layer in model.model.layers)
    assert pool.num_free_blocks == ring_pages and [len(row) for row in got] == [new, new]
    with pytest.raises(ValueError, match="streaming does not combine with rolling_kv"):
        generate(model, prompts, 4, pool, streaming=StreamingParams(S, Wn), rolling_kv=True)
    big = _pool(2, sum(-(-(len(p) + new) // PAGE) for p in prompts))
    seqs = [KvCacheInt4(big, 0) for _ in prompts]
    model.set_streaming(S, Wn)
    try:
        logits, last = _prefill(model, prompts, seqs, DEV)
        tok = logits.index_select(0, last.to(DEV)).argmax(-1)
        want = [tok]
        for _ in range(new - 1):
            for c in seqs:
                c.acquire_one()
            kv = BatchedKvCacheInt4(seqs)
            kv.pos_shift = torch.tensor([max(0, c.seqlen - 1 - Wn + 1 - S) for c in seqs], dtype=torch.int32, device=DEV)
            tok = model(tok, BatchLenInfo([], len(seqs), DEV), None, kv)[0].argmax(-1)
            want.append(tok)
    finally:
        model.set_streaming(None)
    assert got == torch.stack(want).t().tolist()
    assert len({t for row in got for t in row}) >= 8          # (not a model stuck on one token)


def test_refusals():
    from atom_amd import ops
    from atom_amd.e2e import LlamaForCausalLM, LlamaForCausalLMWithLora, MixtralForCausalLM
    from atom_amd.utils import KvCacheInt4, RollingKvCacheInt4
    with pytest.raises(ValueError, match="trained sliding window"):
        LlamaForCausalLM(_cfg(2, 1, sliding_window=40)).set_streaming(4, 40)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        LlamaForCausalLM(types.SimpleNamespace(**{**vars(_cfg(4, 2)), "hidden_size": 256})).set_streaming(4, 40)       # 4 heads of 64
    for cls, extra in ((MixtralForCausalLM, dict(num_local_experts=2, num_experts_per_tok=1)), (LlamaForCausalLMWithLora, {})):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(_cfg(2, 1, **extra)).set_streaming(4, 40)
    pool = _pool(1, 12)
    kv = RollingKvCacheInt4([KvCacheInt4(pool, 50)], 40, sinks=4)
    q = torch.zeros((1, 2, 128), dtype=torch.float16, device=DEV)
    for kw, msg in ((dict(sinks=4), "sinks needs window"), (dict(window=40), "serves only calls with sinks=4"),
                    (dict(window=40, sinks=5), "does not serve"), (dict(window=30, sinks=4), "needs pos_shift=")):
        with pytest.raises(ValueError, match=msg):
            ops.batch_decode_i4(q, kv, 0, **kw)
    kv.close()
    assert pool.num_free_blocks == 12
