"""The sparse MoE block on MX operands on the GPU: the routed MXFP4 GEMM bit for bit against float64 on operands whose
partial sums are exact, and against the dense tile kernel on quantiser output; the SiLU x up quantiser against tests/mx_ref.py; the
block against its op-by-op composition, a staged float64 reference and its own graph replay; the model switch."""
import itertools
import types

import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import moe_ref
from tests import mx_ref as R
from tests.test_gpu_mx import exact_operand, plain_np, random_layer

pytestmark = pytest.mark.gpu

E, TOP = 4, 2


def dev(plain):
    return ops.mx_from_plain(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in plain))


def stack(ws):                                               # MxOperands of the experts -> the stacked triple
    return tuple(torch.stack([getattr(w, f) for w in ws]) for f in ("q4", "sc", "q8"))


def planted_route(T):
    """every token's first choice is expert 1; tokens 0 .. 4 take expert 0 second, the rest expert 3; expert 2 gets nothing"""
    logits = torch.full((T, E), -8.0)
    logits[:, 1] = 4.0
    logits[:5, 0] = 2.0
    logits[5:, 3] = 2.0
    route = ops.moe_route_topk(logits.half().cuda(), TOP)
    indptr = route.expert_indptr.cpu().tolist()
    assert indptr == [0, min(T, 5), min(T, 5) + T, min(T, 5) + T, 2 * T]
    return route, indptr, route.row_token.cpu().numpy()


def parity(got, ref):
    return (np.abs(got - ref) / (1e-2 * np.maximum(np.abs(ref), np.sqrt((ref ** 2).mean())))).max()


@pytest.mark.parametrize("T,K,N_seg,nseg,gather", list(itertools.product([1, 5, 70], [256, 640], [64, 192], [1, 2], [True, False])))
def test_routed_gemm_exact_sums_bit_for_bit(T, K, N_seg, nseg, gather):
    route, indptr, row_token = planted_route(T)
    rows, N = TOP * T, nseg * N_seg
    a = exact_operand(T if gather else rows, K, 125, seed=T)
    ws = [exact_operand(N, K, 124, seed=100 * e + N + K) for e in range(E)]
    outs = ops.moe_gemm_mxfp4(dev(a), stack([dev(w) for w in ws]), route, gather=gather, nseg=nseg)
    got = np.concatenate([o.cpu().numpy() for o in outs], axis=1)
    want = np.empty((rows, N), np.float16)
    for e in range(E):
        r = np.arange(indptr[e], indptr[e + 1])
        src = row_token[r] if gather else r
        if len(r):
            want[r] = R.gemm_ref(tuple(t[src] for t in a), ws[e]).astype(np.float16)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), np.argwhere(got.view(np.uint16) != want.view(np.uint16))[:4]


@pytest.mark.parametrize("T,N,K", [(5, 64, 256), (70, 192, 640)])
def test_routed_rows_equal_the_dense_tile_kernel(T, N, K):
    route, indptr, row_token = planted_route(T)
    x, _, idx = random_layer(T, N, K, seed=T + N + K)
    xd, idd = torch.from_numpy(x).cuda(), torch.from_numpy(idx).cuda()
    ws = [ops.quant_weight_mx(torch.from_numpy(random_layer(1, N, K, seed=7 + e)[1]).cuda()) for e in range(E)]
    a_mx = ops.reorder_quant_mx(xd, idd)
    (got,) = ops.moe_gemm_mxfp4(a_mx, stack(ws), route, gather=True)
    a = plain_np(a_mx)
    for e in range(E):
        lo, hi = indptr[e], indptr[e + 1]
        if hi == lo:
            continue
        src = torch.from_numpy(row_token[lo:hi]).cuda().long()
        xe = torch.cat([xd[src], xd.new_zeros((max(17 - (hi - lo), 0), K))])
        assert ops.gemm_mxfp4_route(len(xe), N, K) == "tile"
        dense = ops.gemm_mxfp4(ops.reorder_quant_mx(xe, idd), ws[e])[: hi - lo]
        assert torch.equal(got[lo:hi].view(torch.int16), dense.view(torch.int16))
        ref = R.gemm_ref(tuple(t[row_token[lo:hi]] for t in a), plain_np(ws[e]))
        assert parity(got[lo:hi].cpu().numpy().astype(np.float64), ref) <= 1.0


@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("rows", [1, 17])
def test_silu_mul_quant_mx(rows, K):
    rng = np.random.default_rng(1000 * rows + K)              # (seeds checked on the CPU against the condition below)
    g, u = rng.standard_normal((rows, K)) * 2, rng.standard_normal((rows, K))
    g[:, rng.choice(K, 3, replace=False)] *= 12               # a few large channels
    u[:, rng.choice(K, 3, replace=False)] *= 20
    g, u = g.astype(np.float16), u.astype(np.float16)
    v = g.astype(np.float64) / (1 + np.exp(-g.astype(np.float64))) * u.astype(np.float64)
    m = np.frexp(np.abs(v).reshape(rows, -1, 32).max(-1))[0]  # in [0.5, 1); a condition on the inputs, not a tolerance: no block
    assert (m - 0.5 > 2.0 ** -21).all() and (1 - m > 2.0 ** -20).all()   # maximum within relative 2^-20 of a power of two
    o = ops.silu_mul_quant_mx(torch.from_numpy(g).cuda(), torch.from_numpy(u).cuda())
    assert (o.rows, o.k) == (rows, K)
    got = plain_np(o)
    want = R.quantise_plain(v)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    err, best = np.abs(R.dequant(got) - v), np.abs(R.dequant(want) - v)
    bad = err > best * (1 + 2.0 ** -10) + 2.0 ** -20 * np.abs(v)
    assert not bad.any(), (np.argwhere(bad)[:4], err[bad][:4], best[bad][:4])
    if rows % 16:                                             # the rows that pad the last tile: zero blocks
        codes, scales, k8, s8 = plain_np(ops.MxOperand(o.q4[-1:], o.sc[-1:], o.q8[-1:], 16, K))
        assert not codes[rows % 16:].any() and not k8[rows % 16:].any() and (scales[rows % 16:] == 127).all() and (s8[rows % 16:] == 127).all()


# ------------------------------------------------------------------------------------------------------------------- the block
H_, F_ = 256, 384


def _cfg(**kw):
    return types.SimpleNamespace(hidden_size=H_, num_attention_heads=2, num_key_value_heads=1, intermediate_size=F_, rms_norm_eps=1e-5,
                                 rope_theta=1e4, num_hidden_layers=2, vocab_size=500, pad_token_id=None, num_local_experts=E,
                                 num_experts_per_tok=TOP, sliding_window=None, **kw)


def _load_moe(moe, g):
    for j in range(moe.num_experts):
        w1, w3 = [(torch.randn(F_, H_, generator=g) * 0.05).half().cuda() for _ in range(2)]
        moe.load_expert_fp16(j, w1, w3, (torch.randn(H_, F_, generator=g) * 0.05).half().cuda())
    moe.gate.weight.data = (torch.randn(E, H_, generator=g) * 0.1).half().cuda()


@pytest.fixture(scope="module")
def moe_block():
    from atom_amd.e2e import MixtralSparseMoeMxfp4
    moe = MixtralSparseMoeMxfp4(_cfg()).cuda()
    _load_moe(moe, torch.Generator().manual_seed(3))
    return moe


def _inputs(T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, H_), generator=g)
    x[:, :4] *= 10
    return x.half().cuda(), torch.randn((T, H_), generator=g).half().cuda()


@pytest.mark.parametrize("T", [1, 19])
def test_block_composition_reference_and_replay(moe_block, T):
    moe = moe_block
    idx = torch.randperm(H_, generator=torch.Generator().manual_seed(T)).to(torch.int16).cuda()
    x, residual = _inputs(T, 40 + T)
    got = moe(x, idx, residual)
    # op by op
    route = ops.moe_route_topk(torch.nn.functional.linear(x, moe.gate.weight), TOP)
    x_mx = ops.reorder_quant_mx(x, idx)
    w13, w2 = (moe.w13_fp4, moe.w13_scale, moe.w13_fp8), (moe.w2_fp4, moe.w2_scale, moe.w2_fp8)
    gate, up = ops.moe_gemm_mxfp4(x_mx, w13, route, gather=True, nseg=2)
    h_mx = ops.silu_mul_quant_mx(gate, up)
    (y,) = ops.moe_gemm_mxfp4(h_mx, w2, route, gather=False)
    assert torch.equal(got.view(torch.int16), ops.moe_combine(y, route, residual).view(torch.int16))
    # staged float64 reference: the kernel's own quantised operands at each GEMM, the router's own tables
    indptr, rt = route.expert_indptr.cpu().tolist(), route.row_token.cpu().numpy()
    a, h = plain_np(x_mx), plain_np(h_mx)
    expert = lambda w, e, n, k: plain_np(ops.MxOperand(w[0][e], w[1][e], w[2][e], n, k))   # noqa: E731
    gu_ref, y_ref = np.zeros((TOP * T, 2 * F_)), np.zeros((TOP * T, H_))
    for e in range(E):
        lo, hi = indptr[e], indptr[e + 1]
        if hi > lo:
            gu_ref[lo:hi] = R.gemm_ref(tuple(t[rt[lo:hi]] for t in a), expert(w13, e, 2 * F_, H_))
            y_ref[lo:hi] = R.gemm_ref(tuple(t[lo:hi] for t in h), expert(w2, e, H_, F_))
    gu = torch.cat([gate, up], 1).cpu().numpy().astype(np.float64)
    assert parity(gu, gu_ref) <= 1.0 and parity(y.cpu().numpy().astype(np.float64), y_ref) <= 1.0
    want = moe_ref.combine(torch.from_numpy(y_ref).half(), route.topk_ids.cpu().long(), route.topk_w.cpu(), route.slot_row.cpu().tolist(),
                           residual.cpu())
    assert parity(got.cpu().numpy().astype(np.float64), want.numpy().astype(np.float64)) <= 1.0
    # one capture, replayed on new inputs
    sx, sr, graph = x.clone(), residual.clone(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = moe(sx, idx, sr)
    for seed in (7, 8):
        x2, r2 = _inputs(T, seed)
        sx.copy_(x2), sr.copy_(r2)
        graph.replay()
        assert torch.equal(out.view(torch.int16), moe(x2, idx, r2).view(torch.int16))


def test_model_switch_and_generate():
    from atom_amd.e2e import MixtralForCausalLM, generate
    from atom_amd.utils import KvCacheInt4
    from tests.test_gpu_moe import _eager_decode, _pages, _pool, _prefill
    assert type(MixtralForCausalLM(_cfg()).model.layers[0].block_sparse_moe).__name__ == "MixtralSparseMoeInt4"
    torch.manual_seed(0)
    model = MixtralForCausalLM(_cfg(expert_format="mxfp4")).cuda()
    g = torch.Generator().manual_seed(100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "MixtralSparseMoeMxfp4":
            _load_moe(mod, g)
    new, gp = 4, torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 500, (n,), generator=gp).tolist() for n in (7, 19)]
    cap, capacity = max(-(-(len(p) + new - 1) // 16) for p in prompts), _pages([len(p) for p in prompts], 16, new) + 2
    seqs, first, _ = _prefill(model, prompts, _pool(2, 1, capacity, 16))
    toks, _ = _eager_decode(model, seqs, first, new - 1, cap)
    pg = _pool(2, 1, capacity, 16)
    got = generate(model, prompts, new, pg, caches=[KvCacheInt4(pg, 0) for _ in prompts])
    assert got == torch.cat([first[None], toks]).t().tolist()
