"""GPU tests of the prefill / chunked-prefill attention over the INT4 paged KV cache (atom_batch_prefill_i4, csrc/prefill_i4.hip):
against an FP64 restatement (below), against the decode op, robustness (NaN past the end, read-only cache, graph capture, rejected
arguments), and chunked prefill through the decoder layer and the model."""
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests.helpers import t2n

pytestmark = pytest.mark.gpu


def _setup(seqlens, layers=2, heads=4, block=16, seed=0, extra_blocks=3):
    """test_gpu_kv._setup restated: a random cache (codes and (scale, zero) everywhere, also past the ends), plus page numbers in a
    scrambled order."""
    from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    g = torch.Generator(device="cuda").manual_seed(seed)
    cap = sum(-(-s // block) for s in seqlens) + extra_blocks
    pool = KvPoolInt4(layers, heads, 128, cap, block, torch.device("cuda"))
    pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device="cuda", generator=g, dtype=torch.uint8))
    pool.param.copy_((torch.rand(pool.param.shape, device="cuda", generator=g) * 0.2 + 0.01).half())
    cs = [KvCacheInt4(pool, s) for s in seqlens]
    kv = BatchedKvCacheInt4(cs)
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(cap)).to(device="cuda", dtype=torch.int32)
    kv.indicies = perm[kv.indicies.long()].contiguous()
    return pool, cs, kv, g


def _ref(q, pool, kv, qo, layer, theta=1e4):
    """FP64: sequence b's queries at its last q_b positions, causal, RoPE on q and on every key at its own position."""
    qn = t2n(q).astype(np.float64)
    data, param = t2n(pool.buf), t2n(pool.param)
    indptr, indices, lpo = t2n(kv.indptr), t2n(kv.indicies), t2n(kv.last_page_offset)
    P = data.shape[4]
    T, N, D = qn.shape
    out = np.zeros((T, N, D))
    for b in range(len(lpo)):
        S = O.kv_seq_len(indptr, lpo, P, b)
        r0, r1 = int(qo[b]), int(qo[b + 1])
        pos = np.arange(S - (r1 - r0), S)
        pages = [int(x) for x in indices[int(indptr[b]):int(indptr[b + 1])]]
        for h in range(N):
            kp = np.concatenate([data[pg, layer, 0, h] for pg in pages], axis=0)[:S]
            vp = np.concatenate([data[pg, layer, 1, h] for pg in pages], axis=0)[:S]
            kq = np.concatenate([param[pg, layer, 0, h] for pg in pages], axis=0)[:S]
            vq = np.concatenate([param[pg, layer, 1, h] for pg in pages], axis=0)[:S]
            kf = O._rope_llama(O._dequant_u4_rows(kp, kq), np.arange(S), theta)
            vf = O._dequant_u4_rows(vp, vq)
            qf = O._rope_llama(qn[r0:r1, h], pos, theta)
            s = qf @ kf.T / np.sqrt(D)
            s[np.arange(S)[None, :] > pos[:, None]] = -np.inf
            pr = np.exp(s - s.max(axis=1, keepdims=True))
            out[r0:r1, h] = (pr / pr.sum(axis=1, keepdims=True)) @ vf
    return out


def _case(prefixes, qlens, heads, block, seed):
    pool, cs, kv, g = _setup([a + n for a, n in zip(prefixes, qlens)], heads=heads, block=block, seed=seed)
    qo = np.cumsum([0] + list(qlens)).astype(np.int32)
    q = torch.randn((int(qo[-1]), heads, 128), device="cuda", generator=g).half()
    return pool, kv, q, qo, torch.from_numpy(qo).cuda()


def _bound(o, ref, rel=4e-3):
    err = np.abs(t2n(o).astype(np.float64) - ref).max()
    return err <= rel * np.abs(ref).max() + 1e-3, (err, np.abs(ref).max())


# (prefix, q_len) per sequence: every prefix of {0, 1, 15, 16, 300, 2000} and every q_len of {1, 7, 16, 63, 64, 65, 200, 1000} at
# least once, several sequences of different lengths per call; heads 1 / 4 / 32 / 40, pages of 16 / 48 / 64 tokens
CASES = [
    ([0, 1, 15], [7, 64, 16], 4, 16),
    ([16, 0], [63, 65], 1, 48),
    ([300, 0, 15], [1, 200, 64], 32, 16),
    ([0], [1000], 4, 64),
    ([2000, 16, 1], [7, 1, 65], 40, 48),
    ([0, 300], [16, 63], 32, 64),
]


@pytest.mark.parametrize("prefixes,qlens,heads,block", CASES)
def test_prefill_matches_fp64(prefixes, qlens, heads, block):
    from atom_amd import ops
    pool, kv, q, qo, qo_d = _case(prefixes, qlens, heads, block, seed=len(qlens) + heads)
    for layer in (0, 1):
        o = ops.batch_prefill_i4(q, qo_d, kv, layer, max_q_len=max(qlens))
        ok, info = _bound(o, _ref(q, pool, kv, qo, layer))
        assert ok, (layer, info)


@pytest.mark.parametrize("prefixes,qlens,heads", [([2000], [8], 32), ([300, 2000, 16], [7, 16, 1], 4)])
def test_prefill_kv_split_and_no_split(prefixes, qlens, heads):
    """Short chunks on long prefixes split their KV range (partial states + the decode op's merge); with max_pages = 0 the host
    cannot see the length and no split is made.  Both meet the FP64 bound and agree with each other."""
    from atom_amd import ops
    from atom_amd._lib import lib
    pool, kv, q, qo, qo_d = _case(prefixes, qlens, heads, 16, seed=7)
    T = q.size(0)
    assert lib().atom_batch_prefill_i4_workspace_bytes(T, len(qlens), heads, 16, max(qlens), kv.max_pages) > 0   # the split path runs
    o_split = ops.batch_prefill_i4(q, qo_d, kv, 1, max_q_len=max(qlens))
    kv.max_pages = 0
    assert lib().atom_batch_prefill_i4_workspace_bytes(T, len(qlens), heads, 16, max(qlens), 0) == 0
    o_one = ops.batch_prefill_i4(q, qo_d, kv, 1, max_q_len=max(qlens))
    ref = _ref(q, pool, kv, qo, 1)
    for o in (o_split, o_one):
        ok, info = _bound(o, ref)
        assert ok, info
    assert (o_split.float() - o_one.float()).abs().max().item() <= 4e-3 * np.abs(ref).max() + 1e-3
    # max_q_len left to its default (the row count): more workgroups, the same rows
    assert torch.equal(ops.batch_prefill_i4(q, qo_d, kv, 1), o_one)


@pytest.mark.parametrize("seqlens,heads,block", [([37, 5, 16, 1], 4, 16), ([300, 17, 260, 33, 1, 290, 128, 64], 32, 16),
                                                  ([2000, 7], 4, 16), ([210, 97, 5], 5, 48)])
def test_one_query_per_sequence_is_decode(seqlens, heads, block):
    from atom_amd import ops
    pool, cs, kv, g = _setup(seqlens, heads=heads, block=block, seed=len(seqlens))
    q = torch.randn((len(seqlens), heads, 128), device="cuda", generator=g).half()
    qo = torch.arange(len(seqlens) + 1, dtype=torch.int32, device="cuda")
    for layer in (0, 1):
        d = ops.batch_decode_i4(q, kv, layer).float()
        o = ops.batch_prefill_i4(q, qo, kv, layer, max_q_len=1).float()
        assert (o - d).abs().max().item() <= 4e-3 * d.abs().max().item(), layer


def test_rows_match_decode_on_truncated_caches():
    """Row i of a chunk on a cached prefix = batch_decode_i4 on the same pages with the sequence cut after position prefix + i."""
    from atom_amd import ops
    prefix, n, heads, P = 300, 40, 8, 16
    pool, cs, kv, g = _setup([prefix + n], heads=heads, block=P, seed=11)
    q = torch.randn((n, heads, 128), device="cuda", generator=g).half()
    o = ops.batch_prefill_i4(q, torch.tensor([0, n], dtype=torch.int32, device="cuda"), kv, 0).float()
    pages = kv.indicies.tolist()
    lens = [prefix + i + 1 for i in range(n)]
    npg = [-(-s // P) for s in lens]
    cut = types.SimpleNamespace(data=kv.data, param=kv.param, max_pages=max(npg),
                                indptr=torch.tensor(np.cumsum([0] + npg), dtype=torch.int32, device="cuda"),
                                indicies=torch.tensor([pg for k in npg for pg in pages[:k]], dtype=torch.int32, device="cuda"),
                                last_page_offset=torch.tensor([(s - 1) % P + 1 for s in lens], dtype=torch.int32, device="cuda"))
    d = ops.batch_decode_i4(q, cut, 0).float()
    assert (o - d).abs().max().item() <= 4e-3 * d.abs().max().item()


def test_nan_past_the_end_and_cache_is_read_only():
    from atom_amd import ops
    prefixes, qlens = [300, 0, 2000], [7, 65, 8]
    pool, kv, q, qo, qo_d = _case(prefixes, qlens, 4, 48, seed=5)
    data0, param0 = pool.buf.clone(), pool.param.clone()
    clean = ops.batch_prefill_i4(q, qo_d, kv, 1)
    assert torch.equal(pool.buf, data0) and torch.equal(pool.param.view(torch.int16), param0.view(torch.int16))
    # every slot no sequence owns: unused pages and the tail of each last page
    used = set(kv.indicies.tolist())
    for pg in range(pool.buf.size(0)):
        if pg not in used:
            pool.param[pg] = float("nan")
            pool.buf[pg] = 0xFF
    ip, idx, lpo = kv.indptr.tolist(), kv.indicies.tolist(), kv.last_page_offset.tolist()
    for b in range(len(qlens)):
        last = idx[ip[b + 1] - 1]
        pool.param[last, :, :, :, lpo[b]:] = float("inf")
        pool.param[last, :, 1, :, lpo[b]:] = float("nan")
    o = ops.batch_prefill_i4(q, qo_d, kv, 1)
    kv.max_pages = 0
    o2 = ops.batch_prefill_i4(q, qo_d, kv, 1)
    assert torch.isfinite(o).all() and torch.isfinite(o2).all()
    assert torch.equal(o, clean)


def test_graph_capture_equals_eager():
    from atom_amd import ops
    pool, kv, q, qo, qo_d = _case([2000, 16], [8, 40], 32, 16, seed=3)
    eager = ops.batch_prefill_i4(q, qo_d, kv, 0, max_q_len=40)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.batch_prefill_i4(q, qo_d, kv, 0, max_q_len=40)       # warm-up: the stream's workspace
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.batch_prefill_i4(q, qo_d, kv, 0, max_q_len=40)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_rejected_arguments():
    from atom_amd import _lib as L
    from atom_amd import ops
    pool, kv, q, qo, qo_d = _case([20, 3], [5, 4], 4, 16, seed=1)
    o = torch.empty_like(q)
    lib = L.lib()
    T = q.size(0)

    def call(**kw):
        a = dict(o=o.data_ptr(), q=q.data_ptr(), qo=qo_d.data_ptr(), T=T, mq=5, data=kv.data.data_ptr(), param=kv.param.data_ptr(),
                 indptr=kv.indptr.data_ptr(), indices=kv.indicies.data_ptr(), lpo=kv.last_page_offset.data_ptr(), batch=2, L=2, layer=0,
                 N=4, P=16, D=128, theta=1e4, scale=1.0)
        a.update(kw)
        st = lib.atom_batch_prefill_i4(a["o"], a["q"], a["qo"], a["T"], a["mq"], a["data"], a["param"], a["indptr"], a["indices"],
                                       a["lpo"], a["batch"], a["L"], a["layer"], a["N"], a["P"], a["D"], a["theta"], a["scale"], 0, None, 0,
                                       L.current_stream(q.device))
        return st
    assert call() == L.OK
    for kw, want in [(dict(D=64), L.ERR_SHAPE), (dict(P=24), L.ERR_SHAPE), (dict(P=8), L.ERR_SHAPE), (dict(layer=2), L.ERR_SHAPE),
                     (dict(T=0), L.ERR_SHAPE), (dict(mq=0), L.ERR_SHAPE), (dict(batch=0), L.ERR_SHAPE), (dict(N=0), L.ERR_SHAPE),
                     (dict(qo=None), L.ERR_INVALID_ARG), (dict(q=None), L.ERR_INVALID_ARG), (dict(o=None), L.ERR_INVALID_ARG),
                     (dict(data=None), L.ERR_INVALID_ARG), (dict(indices=None), L.ERR_INVALID_ARG), (dict(lpo=None), L.ERR_INVALID_ARG),
                     (dict(theta=0.0), L.ERR_INVALID_ARG), (dict(theta=-1.0), L.ERR_INVALID_ARG), (dict(scale=0.0), L.ERR_INVALID_ARG),
                     (dict(q=q.data_ptr() + 2), L.ERR_ALIGN), (dict(o=o.data_ptr() + 8), L.ERR_ALIGN),
                     (dict(data=kv.data.data_ptr() + 4), L.ERR_ALIGN), (dict(param=kv.param.data_ptr() + 2), L.ERR_ALIGN),
                     (dict(qo=qo_d.data_ptr() + 2), L.ERR_ALIGN)]:
        st = call(**kw)
        assert st == want, (kw, st)
        with pytest.raises(L.AtomHipError, match=f"status {want}"):
            L.check(st, "atom_batch_prefill_i4")
    # through the Python op
    with pytest.raises(L.AtomHipError, match=f"status {L.ERR_SHAPE}"):
        ops.batch_prefill_i4(q, qo_d, kv, 2)
    with pytest.raises(L.AtomHipError, match=f"status {L.ERR_INVALID_ARG}"):
        ops.batch_prefill_i4(q, qo_d, kv, 0, rope_theta=0.0)
    with pytest.raises(L.AtomHipError):
        ops.batch_prefill_i4(q.cpu(), qo_d, kv, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ chunked prefill, layer and model
def _cfg(layers=1):
    return types.SimpleNamespace(hidden_size=512, num_attention_heads=4, intermediate_size=1408, rms_norm_eps=1e-5, rope_theta=1e4,
                                 num_hidden_layers=layers, vocab_size=1000, pad_token_id=None)


def _load_weights(model, seed):
    g = torch.Generator().manual_seed(seed)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()


LENS = [37, 16]
CHUNKS = [[20, 5], [10, 6], [7, 5]]          # three chunks per sequence (sums: 37, 16)


def test_chunked_prefill_through_decoder_layer():
    """S = 37 + 16 tokens prefilled in three chunks (KvCacheInt4.acquire between them: the later chunks attend to a cached prefix)
    equal the same tokens prefilled in one go, row by row, at the attention's output; and the one-go HIP op equals the torch route."""
    from atom_amd import ops
    from atom_amd.e2e import LlamaDecoderLayer
    from atom_amd.e2e.llama import DecodeFusion
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    torch.manual_seed(3)
    cfg, dev = _cfg(), torch.device("cuda")
    fusion = DecodeFusion(prefill_attn=True)
    layer = LlamaDecoderLayer(cfg, layer_idx=1, fusion=fusion).cuda()
    _load_weights(layer, 5)
    x = [(torch.randn(n, cfg.hidden_size) * 0.7).half().cuda() for n in LENS]
    attn_in = []
    orig = ops.reorder_fp16_i4

    def spy(a, idx, **kw):
        if idx is layer.self_attn.reorder_index:
            attn_in.append(a.clone())
        return orig(a, idx, **kw)

    def pool():
        return KvPoolInt4(num_layers=2, num_heads=4, head_dim=128, capacity=16, block_len=16, device=dev)
    ops.reorder_fp16_i4 = spy
    try:
        # chunked
        p1 = pool()
        cs = [KvCacheInt4(p1, 0) for _ in LENS]
        beg = [0, 0]
        for ch in CHUNKS:
            for c, n in zip(cs, ch):
                c.acquire(n)
            xs = torch.cat([xi[b:b + n] for xi, b, n in zip(x, beg, ch)])
            layer(xs, BatchLenInfo(ch, 0, dev), BatchedKvCacheInt4(cs), None)
            beg = [b + n for b, n in zip(beg, ch)]
        chunked = [[], []]
        for a, ch in zip(attn_in, CHUNKS):
            chunked[0].append(a[:ch[0]])
            chunked[1].append(a[ch[0]:])
        chunked = torch.cat([torch.cat(chunked[0]), torch.cat(chunked[1])]).float()
        # one go, HIP op and torch route
        outs = []
        for flag in (True, False):
            fusion.prefill_attn = flag
            attn_in.clear()
            p2 = pool()
            layer(torch.cat(x), BatchLenInfo(LENS, 0, dev), BatchedKvCacheInt4([KvCacheInt4(p2, n) for n in LENS]), None)
            outs.append(attn_in[0].float())
    finally:
        ops.reorder_fp16_i4 = orig
        fusion.prefill_attn = True
    one_go, torch_route = outs
    scale = one_go.abs().max().item()
    assert (chunked - one_go).abs().max().item() <= 2e-3 * scale
    assert (one_go - torch_route).abs().max().item() <= 4e-3 * scale


def test_chunked_prefill_then_decode_model():
    """LlamaForCausalLM, 2 layers: chunked prefill + 4 decode steps gives the decode logits of one-shot prefill + the same 4 steps.
    (One-shot through the HIP op too: against the torch route the two layers' W4A4 quantisers turn the fp16-operand differences of the
    attention into flipped codes, up to ~0.2 of the logit scale on this model.)"""
    from atom_amd.e2e import LlamaForCausalLM
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    torch.manual_seed(4)
    cfg, dev = _cfg(2), torch.device("cuda")
    model = LlamaForCausalLM(cfg).cuda()
    _load_weights(model, 6)
    g = torch.Generator().manual_seed(9)
    ids = [torch.randint(0, cfg.vocab_size, (n,), generator=g).cuda() for n in LENS]
    steps = torch.randint(0, cfg.vocab_size, (4, len(LENS)), generator=g).cuda()

    def run(chunks):
        p = KvPoolInt4(num_layers=2, num_heads=4, head_dim=128, capacity=16, block_len=16, device=dev)
        cs = [KvCacheInt4(p, 0) for _ in LENS]
        beg = [0, 0]
        for ch in chunks:
            for c, n in zip(cs, ch):
                c.acquire(n)
            model(torch.cat([i[b:b + n] for i, b, n in zip(ids, beg, ch)]), BatchLenInfo(ch, 0, dev), BatchedKvCacheInt4(cs), None)
            beg = [b + n for b, n in zip(beg, ch)]
        logits = []
        for t in range(steps.size(0)):
            for c in cs:
                c.acquire_one()
            lg, _ = model(steps[t], BatchLenInfo([], len(LENS), dev), None, BatchedKvCacheInt4(cs))
            logits.append(lg.float())
        return torch.stack(logits)
    import atom_amd.e2e.llama as E
    flag, E.FUSION.prefill_attn = E.FUSION.prefill_attn, True    # the one-shot prefill on the same op (chunks with a prefix take it anyway)
    try:
        chunked, one_shot = run(CHUNKS), run([LENS])
    finally:
        E.FUSION.prefill_attn = flag
    assert torch.isfinite(chunked).all()
    scale = one_shot.abs().max().item()
    assert (chunked - one_shot).abs().max().item() <= 0.15 * scale
