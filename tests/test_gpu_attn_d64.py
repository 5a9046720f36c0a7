"""GPU tests of head size 64 in the INT4 paged-KV path (csrc/attn_d64.hip): quantiser and append bit for bit against the rule in fp32
torch; attention against a plain FP64 reference within the bound for fp16 MFMA operands, 4e-3 * max|ref| + 1e-3; the model.  Caches are
built by hand: scrambled page order, every byte outside a sequence's tokens 0xFF (codes 15, NaN scale and zero)."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REL, ABS = 4e-3, 1e-3


def quant_ref(x):
    """[.., 64] -> (codes uint8 [.., 64], (scale, zero) fp16 [.., 2]): scale = (hi - lo) / 15, zero = -lo, round half away, clamp"""
    x = x.float().cpu()
    lo, hi = x.amin(-1, keepdim=True), x.amax(-1, keepdim=True)
    scale, zero = (hi - lo) / 15.0, -lo
    t = (x + zero) * (1.0 / scale)
    tr = torch.trunc(t)
    tr = torch.where((t - tr).abs() >= 0.5, tr + torch.copysign(torch.ones_like(t), t), tr).clamp(0, 15)
    codes = torch.where(scale == 0, torch.zeros_like(tr), torch.nan_to_num(tr)).to(torch.uint8)
    return codes, torch.cat([scale, zero], -1).half()


def pack(codes):
    return codes[..., 0::2] | (codes[..., 1::2] << 4)


def dequant(codes, sz):
    return codes.double() * sz[..., 0:1].double() - sz[..., 1:2].double()


def tables(kv, lens, P):
    """the pool of `kv` with sequence b listing the first ceil(lens[b] / P) of its own pages"""
    pages = [pg[:max(-(-n // P), 1)] for pg, n in zip(kv.pages, lens)]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    return types.SimpleNamespace(data=kv.data, param=kv.param, pages=kv.pages, indptr=i32(np.cumsum([0] + [len(pg) for pg in pages])),
                                 indicies=i32(sum(pages, [])), last_page_offset=i32([n - (len(pg) - 1) * P for n, pg in zip(lens, pages)]),
                                 max_pages=max(len(pg) for pg in pages))


def make_cache(tokens, lens, P, layers=2, layer=1, seed=0):
    """tokens[b]: (k, v) fp16 [n_b, heads, 64] with n_b >= lens[b] (tokens past the length land in the last page's free slots).  The
    pool as ops takes it, and the de-quantised float64 (K, V) [lens[b], heads, 64] of every sequence."""
    heads = tokens[0][0].shape[1]
    npages = [max(-(-n // P), 1) for n in lens]
    order = torch.randperm(sum(npages) + 3, generator=torch.Generator().manual_seed(seed)).tolist()
    data = torch.full((len(order), layers, 2, heads, P, 32), 0xFF, dtype=torch.uint8)
    param = torch.full((len(order), layers, 2, heads, P, 2), float("nan"), dtype=torch.float16)
    pages, deq = [], []
    for (k, v), n, count in zip(tokens, lens, npages):
        own = [order.pop() for _ in range(count)]
        assert k.shape[0] <= count * P
        (kc, ks), (vc, vs) = quant_ref(k), quant_ref(v)
        for j in range(k.shape[0]):
            pg, e = own[j // P], j % P
            data[pg, layer, 0, :, e], data[pg, layer, 1, :, e] = pack(kc[j]), pack(vc[j])
            param[pg, layer, 0, :, e], param[pg, layer, 1, :, e] = ks[j], vs[j]
        pages.append(own)
        deq.append((dequant(kc, ks)[:n].numpy(), dequant(vc, vs)[:n].numpy()))
    return tables(types.SimpleNamespace(data=data.to(DEV), param=param.to(DEV), pages=pages), lens, P), deq


def random_tokens(lens, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return [tuple(torch.randn(n, heads, 64, generator=g).half() for _ in range(2)) for n in lens]


def rope64(x, pos, inv):
    """x float64 [S, .., 64] at positions pos [S]: pairs (i, i + 32) turned by pos * inv[i] radians"""
    ang = (np.asarray(pos, dtype=np.float64)[:, None] * inv[None, :]).reshape((len(pos),) + (1,) * (x.ndim - 2) + (32,))
    c, s, x1, x2 = np.cos(ang), np.sin(ang), x[..., :32], x[..., 32:]
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)


THETA_INV = 1e4 ** (-np.arange(32, dtype=np.float64) / 32)


def ref_attn(q, deq, qo, G, inv=THETA_INV, scale=1.0):
    """q fp16 [T, heads * G, 64]; sequence b's queries are rows qo[b] .. qo[b + 1] at its last positions -> float64 [T, heads * G, 64]"""
    q, out = q.double().cpu().numpy(), []
    for b, (K, V) in enumerate(deq):
        n, nq = K.shape[0], qo[b + 1] - qo[b]
        pos = np.arange(n - nq, n)
        Kr, qr = rope64(K, np.arange(n), inv), rope64(q[qo[b]:qo[b + 1]], pos, inv)
        s = np.einsum("qhd,khd->hqk", qr, np.repeat(Kr, G, axis=1)) * (scale / 8.0)
        s = np.where(np.arange(n)[None, None, :] > pos[None, :, None], -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        out.append(np.einsum("hqk,khd->qhd", p / p.sum(-1, keepdims=True), np.repeat(V, G, axis=1)))
    return np.concatenate(out)


def assert_close(got, ref, what=""):
    err, bound = np.abs(got.double().cpu().numpy() - ref).max(), REL * np.abs(ref).max() + ABS
    print(f"{what}: max|err| {err:.4g}, bound {bound:.4g}")
    assert err <= bound, what


def queries(rows, heads, seed):
    return torch.randn(rows, heads, 64, generator=torch.Generator().manual_seed(seed)).half().to(DEV)


@pytest.mark.parametrize("P", [16, 48])
def test_quantiser_and_append_bit_for_bit(P):
    from atom_amd import ops
    heads, lens = 3, [1, P, P + 1, 2 * P + 5]                          # init_kv_i4 writes these; append_kv_i4 one more token each
    na = sum(lens)
    x = torch.randn(na + len(lens), heads, 64, generator=torch.Generator().manual_seed(P)).half()
    x[0, 0] = 0.75                                                     # constant: scale 0, all codes 0
    x[0, 1] = 0; x[0, 1, 37] = -300.0                                  # a single spike
    x[1, 0] = (torch.arange(64).half() * 0.5 - 3).clamp(max=27.0)      # lo -3, hi 27, scale 2: every other value is a tie at .5
    k, v = x.to(DEV), x.flip(0).contiguous().to(DEV)
    got = [ops.kv_quant_u4(t) for t in (k, v)]
    for t, (codes, sz) in zip((k, v), got):
        wc, ws = quant_ref(t)
        assert torch.equal(codes.cpu(), pack(wc)) and torch.equal(sz.cpu().view(torch.int16), ws.view(torch.int16))
    assert got[0][0][0, 0].eq(0).all() and got[0][0][1, 0].cpu().unique().numel() > 8
    # the bytes land in the right page and slot: the hand-built cache of the same tokens is the expected pool, byte for byte
    off = np.concatenate([[0], np.cumsum(lens)])
    tok = [torch.cat([torch.arange(off[b], off[b + 1]), torch.tensor([na + b])]) for b in range(len(lens))]
    want, _ = make_cache([(x[t], x.flip(0)[t]) for t in tok], [n + 1 for n in lens], P)
    pool = tables(want, lens, P)                                       # the sequences before their last token, on an untouched pool
    pool.data, pool.param = torch.full_like(want.data, 0xFF), torch.full_like(want.param, float("nan"))
    (kc, ks), (vc, vs) = got
    ops.init_kv_i4(pool, kc[:na], vc[:na], ks[:na], vs[:na], torch.tensor(off, dtype=torch.int32, device=DEV), 1)
    grown = tables(pool, [n + 1 for n in lens], P)
    ops.append_kv_i4(grown, kc[na:], vc[na:], ks[na:], vs[na:], 1)
    assert torch.equal(pool.data, want.data) and torch.equal(pool.param.view(torch.int16), want.param.view(torch.int16))


LENS = [1, 127, 128, 129, 16, 17, 48, 2111]


@pytest.mark.parametrize("known", [True, False], ids=["max_pages", "no_split"])
@pytest.mark.parametrize("G,heads", [(1, 2), (4, 2), (8, 1), (7, 1)])
def test_decode_against_fp64(G, heads, known):
    from atom_amd import ops
    kv, deq = make_cache(random_tokens(LENS, heads, 1), LENS, 16)
    kv.max_pages = kv.max_pages if known else 0
    assert (ops.decode_splits(len(LENS), kv, heads * G) >= 2) == known
    q, qo = queries(len(LENS), heads * G, 2), list(range(len(LENS) + 1))
    ref = ref_attn(q, deq, qo, G)
    o = ops.batch_decode_i4(q, kv, 1)
    assert_close(o, ref, "decode")
    op = ops.batch_prefill_i4(q, torch.tensor(qo, dtype=torch.int32, device=DEV), kv, 1, max_q_len=1)
    assert_close(op, o.double().cpu().numpy(), "one query per sequence vs the decode entry")


SHAPE = [(0, 1), (0, 15), (0, 65), (0, 130), (1000, 1), (1000, 15), (1003, 65), (1005, 130), (31, 17)]      # (prefix, queries)


@pytest.mark.parametrize("G", [1, 4])
def test_prefill_against_fp64(G):
    from atom_amd import _lib, ops
    lens, qo = [p + n for p, n in SHAPE], np.concatenate([[0], np.cumsum([n for _, n in SHAPE])]).tolist()
    kv, deq = make_cache(random_tokens(lens, 2, 3), lens, 16)
    q = queries(qo[-1], 2 * G, 4)
    ref = ref_attn(q, deq, qo, G)
    assert _lib.lib().atom_batch_prefill_gqa_i4_d64_splits(qo[-1], len(lens), 2 * G, 2, 16, 130, kv.max_pages) >= 2
    for max_pages in (kv.max_pages, 0):                               # split, then unsplit
        kv.max_pages = max_pages
        o = ops.batch_prefill_i4(q, torch.tensor(qo, dtype=torch.int32, device=DEV), kv, 1, max_q_len=130)
        assert_close(o, ref, f"prefill, max_pages {max_pages}")


def test_mask_is_sharp_around_a_planted_key():
    """len 200, queries at 197 .. 199.  The key at 199 matches every query hugely and carries V = 6: it owns the row at 199 and must not
    move the rows at 197 and 198 (p + 1 and p + 2 for them); the same bytes sit at position 200, past the end, among NaN parameters."""
    from atom_amd import ops
    n, G = 200, 2
    (k, v), = random_tokens([n + 1], 1, 5)
    q = queries(3, G, 6)
    q[:, 1] = q[:, 0]
    target = q[2:3, :1].double().cpu().numpy()                                        # the last row's q: the others are it, turned back
    for r in (0, 1):
        q[r, :] = torch.from_numpy(rope64(target, [2 - r], THETA_INV)[0]).half().to(DEV)
    for j in (n - 1, n):
        k[j, 0] = torch.from_numpy(rope64(target, [(n - 1) - j], THETA_INV)[0, 0] * 4).half()
        v[j, 0] = 6.0
    kv, deq = make_cache([(k, v)], [n], 16)
    ref = ref_attn(q, deq, [0, 3], G)
    assert np.abs(ref[2] - 6.0).max() < 0.05 and np.abs(ref[:2]).max() < 3.0
    o = ops.batch_prefill_i4(q, torch.tensor([0, 3], dtype=torch.int32, device=DEV), kv, 1)
    assert torch.isfinite(o).all()
    assert_close(o, ref, "planted key")
    kv.last_page_offset -= 1                                                          # decode at p = 198: the key at 199 is now past the end
    deq = [(deq[0][0][:-1], deq[0][1][:-1])]
    assert_close(ops.batch_decode_i4(q[1:2].contiguous(), kv, 1), ref_attn(q[1:2], deq, [0, 1], G), "decode, planted key past the end")


def test_rope_table():
    from atom_amd import ops
    from atom_amd.e2e.rope import rope_init
    lens = [2111, 2200, 5]
    kv, deq = make_cache(random_tokens(lens, 2, 7), lens, 16)
    q, qo = queries(3, 4, 8), [0, 1, 2, 3]
    plain = ops.rope_table(THETA_INV, DEV, 64)
    assert plain.shape == (32,)
    assert_close(ops.batch_decode_i4(q, kv, 1, rope_table=plain), ref_attn(q, deq, qo, 2), "a table of plain theta")
    cfg = dict(rope_theta=5e5, rope_scaling=dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                                 original_max_position_embeddings=1024))
    inv = rope_init(cfg, 64)[2]
    assert inv.shape == (32,) and (inv < 5e5 ** (-np.arange(32) / 32) * 0.5).any()
    table = ops.rope_table(inv, DEV, 64)
    ref = ref_attn(q, deq, qo, 2, inv=table.double().cpu().numpy() * 2 * math.pi, scale=1.3)
    assert_close(ops.batch_decode_i4(q, kv, 1, rope_table=table, attn_scale=1.3), ref, "llama3 table, decode")
    qi = torch.tensor(qo, dtype=torch.int32, device=DEV)
    assert_close(ops.batch_prefill_i4(q, qi, kv, 1, rope_table=table, attn_scale=1.3), ref, "llama3 table, prefill")
    with pytest.raises(TypeError):
        ops.batch_decode_i4(q, kv, 1, rope_table=torch.zeros(64, device=DEV))
    ring = types.SimpleNamespace(**vars(kv), kv_start=kv.indptr)
    for c, kw in ((kv, dict(window=64)), (kv, dict(merge=False)), (kv, dict(append_kv=(None, None))), (ring, {})):      # left out at 64: raises
        with pytest.raises(NotImplementedError):
            ops.batch_decode_i4(q, c, 1, **kw)
    with pytest.raises(NotImplementedError):
        ops.batch_prefill_i4(q, qi, ring, 1)


VOCAB, NEW, PROMPTS = 320, 8, [5, 19, 33]


def _model(seed=0):
    from atom_amd.e2e import LlamaForCausalLM
    cfg = types.SimpleNamespace(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, intermediate_size=1408, rms_norm_eps=1e-5,
                                rope_theta=1e4, num_hidden_layers=2, vocab_size=VOCAB, pad_token_id=None)
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    return model


def _eager(model, pool, prompts, steps, forward=None):
    """prefill + `steps` decode steps, greedy, each through ``forward(counts, decode, ids, blen, prefill_kv, decode_kv)`` -> logits"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    forward = forward or (lambda counts, decode, *a: model(*a)[0])
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    logits = forward(lens, False, ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    toks = [logits[torch.tensor(lens).cumsum(0) - 1].argmax(-1)]
    for _ in range(steps):
        for c in seqs:
            c.acquire_one()
        kv = BatchedKvCacheInt4(seqs)
        kv.max_pages = max(-(-(n + NEW - 1) // 16) for n in lens)
        toks.append(forward([1] * len(seqs), True, toks[-1], BatchLenInfo([], len(seqs), DEV), None, kv).argmax(-1))
    for c in seqs:
        c.release()
    return torch.stack(toks).t().tolist()


QUANTISERS = {"rmsnorm_fp16_i4": "norm1", "reorder_fp16_i4": "attn_q", "add_rmsnorm_fp16_i4": "norm2", "activate_fp16_i4": "act"}
KV_OPS = {"init_kv_i4": "write", "append_kv_i4": "write", "batch_prefill_i4": "attn", "batch_decode_i4": "attn"}
STAGES = ["rmsnorm_fp16_i4", "q", "k", "kv_quant_u4", "v", "kv_quant_u4", "write", "attn", "reorder_fp16_i4", "o", "add_rmsnorm_fp16_i4", "gate",
          "up", "activate_fp16_i4", "down"]


def test_model_against_a_staged_reference_and_generate(monkeypatch):
    """Prefill + 4 decode steps of LlamaForCausalLM (2 layers, hidden 512, 8 heads on 2 K/V heads of 64), one launch per stage, every
    launch captured by the layer tests' spy and checked teacher-forced against the same weights in the oracle's form: q / k / v are
    the projections of norm1 (exact sums, the GEMM bound), the quantiser reads k then v, the cache write takes its outputs at this
    layer, attention is FP64 over the de-quantised k / v the test keeps per sequence (de-quantised cache, the layer tests' bound for
    matrix-core rows), o_proj reads the attention output re-ordered with the attention's index and is bounded, the residual adds the
    layer's input; the logits are lm_head on the returned hidden states.  Then generate() by graph replay returns the eager tokens."""
    from oracle import atom_oracle as O
    from atom_amd.e2e import generate
    from atom_amd.e2e.llama import FUSION
    from atom_amd.utils import KvPoolInt4
    from tests import layer_ref as R, test_gpu_layer_ref as T
    from tests.helpers import t2n
    monkeypatch.setattr(T, "SPIED", T.SPIED + ("kv_quant_u4",))
    model, hist = _model(), {}
    layers = model.model.layers
    W = [{n: dict(q4=O.unpack_int4(t2n(b4).view(np.uint8)), q8=t2n(b8), s4=t2n(sb), s8=t2n(sb8))
          for n, m in T._projections(layer).items() for b4, b8, sb, sb8 in [m.packed()]} for layer in layers]

    def forward(counts, decode, *a):
        with T._Spy() as spy:
            logits, hidden = model(*a)
        rows, qo, per = sum(counts), np.concatenate([[0], np.cumsum(counts)]).tolist(), len(spy.calls) // 2
        for li, layer in enumerate(layers):
            by_w = {m.weight_int8.data_ptr(): n for n, m in T._projections(layer).items()}
            made, c, recoded = {}, [], None
            for name, args, ptrs, outs in spy.calls[li * per:(li + 1) * per]:
                if name == "repack_act_f6":                          # LinearInt4 re-codes its activation first
                    recoded = args[0]
                    continue
                if name == "dense_layer_gemm_i4_fp16":
                    name, src = by_w[ptrs[5]], made[T.READS[by_w[ptrs[5]]]]
                    assert T._same(args[0] if recoded is None else recoded, src[1]) and T._same(args[4], src[0]), name + " reads another stage"
                    if name in "qkvo":
                        ok, msg = R._check_gemm(t2n(outs[0]), R.gemm(T._quant(src, rows), W[li][name]))
                        assert ok, (name, msg)
                    recoded = None
                made[QUANTISERS.get(name)] = outs[1:] if name == "add_rmsnorm_fp16_i4" else outs
                c.append((KV_OPS.get(name, name), args, ptrs, outs))
            assert [x[0] for x in c] == STAGES and c[6][1][-1] == c[7][1][-1] == li
            x, q, k, v = c[0][1][0], c[1][3][0], c[2][3][0], c[4][3][0]
            assert T._same(c[3][1][0], k.view(rows, 2, 64)) and T._same(c[5][1][0], v.view(rows, 2, 64)), "the quantiser reads k, then v"
            assert all(T._same(a, w) for a, w in zip(c[6][1][1:5], (c[3][3][0], c[5][3][0], c[3][3][1], c[5][3][1]))), "the cache write"
            kd, vd = (dequant(*quant_ref(t.view(rows, 2, 64))).numpy() for t in (k, v))
            for b in range(len(counts)):
                old = hist.get((li, b), (np.zeros((0, 2, 64)),) * 2)
                hist[li, b] = tuple(np.concatenate([h, t[qo[b]:qo[b + 1]]]) for h, t in zip(old, (kd, vd)))
            assert T._same(c[7][1][0], q.view(rows, 8, 64))
            assert_close(c[7][3][0], ref_attn(q.view(rows, 8, 64), [hist[li, b] for b in range(len(counts))], qo, 4), f"layer {li}, decode {decode}")
            assert T._same(c[8][1][0], c[7][3][0].view(rows, 512)) and c[8][2][1] == layer.self_attn.reorder_index.data_ptr()
            assert T._same(c[10][1][0], c[9][3][0]) and T._same(c[10][1][1], x), "the residual is o + the layer's input"
        ok, msg = R._check_logits(t2n(logits), t2n(hidden), t2n(model.lm_head.weight))
        assert ok, msg
        return logits

    for mod in model.modules():                                      # one launch per stage (the process-wide DecodeFusion is untouched)
        if hasattr(mod, "fusion"):
            mod.fusion = T._unfused()
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPTS]
    _eager(model, KvPoolInt4(2, 2, 64, 16, 16, DEV), prompts, 4, forward)
    for mod in model.modules():
        if hasattr(mod, "fusion"):
            mod.fusion = FUSION
    want = _eager(model, KvPoolInt4(2, 2, 64, 16, 16, DEV), prompts, NEW - 1)
    assert len({t for row in want for t in row}) >= 6, "the tiny model collapsed: pick another seed"
    pool = KvPoolInt4(2, 2, 64, 16, 16, DEV)
    assert generate(model, prompts, NEW, pool) == want
    with pytest.raises(NotImplementedError):
        generate(model, prompts, 4, pool, num_beams=2)
