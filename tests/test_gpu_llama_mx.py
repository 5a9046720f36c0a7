"""Dense Llama on MX operands on the GPU: the fused gate/up SiLU-quantising GEMM and the RMSNorm quantisers against
float64 through tests/mx_ref.py, the residual add of the GEMM bit for bit, the decoder layer against its op-by-op composition, a staged
float64 reference and its own graph replay, generate() against the eager loop, the config switch."""
import types

import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import mx_ref as R
from tests.test_gpu_mx import exact_operand, plain_np, random_layer

pytestmark = pytest.mark.gpu


def dev(plain):
    return ops.mx_from_plain(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in plain))


def pow2_clear(v, margin):
    """the input condition of the quantiser comparisons: no block maximum within relative `margin` of a power of two"""
    m = np.frexp(np.abs(v).reshape(len(v), -1, 32).max(-1))[0]
    m = m[m > 0]                                              # (an all-zero block has scale byte 127 whatever the arithmetic)
    return bool((m - 0.5 > margin / 2).all() and (1 - m > margin).all())


def assert_quantised(o, v, margin):
    """scale bytes equal the reference's; per element no further from v than the best code by more than the value's own error"""
    got, want = plain_np(o), R.quantise_plain(v)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    err, best = np.abs(R.dequant(got) - v), np.abs(R.dequant(want) - v)
    bad = err > best * (1 + 2.0 ** -10) + margin * np.abs(v)
    assert not bad.any(), (np.argwhere(bad)[:4], err[bad][:4], best[bad][:4])
    rows, K = v.shape
    if rows % 16:                                             # the rows that pad the last tile: zero blocks
        codes, scales, k8, s8 = plain_np(ops.MxOperand(o.q4[-1:], o.sc[-1:], o.q8[-1:], 16, K))
        assert not codes[rows % 16:].any() and not k8[rows % 16:].any() and (scales[rows % 16:] == 127).all() and (s8[rows % 16:] == 127).all()


# ------------------------------------------------------------------------------------------------------------ fused gate / up
# Scale bytes from 123 (weights at K = 640: 122): every product is a multiple of 2^-10 (2^-11) and every partial sum below 2^21 of them
# (the argument of tests/test_gpu_mx.py), so g and u are exact in FP32 in every summation order, with a standard deviation of 3 to 4.
def gate_up_case(M, K, F):
    lo = 123 - (K > 256)
    a, wg, wu = exact_operand(M, K, 123, seed=M + K), exact_operand(F, K, lo, seed=F + K), exact_operand(F, K, lo, seed=F + K + 1)
    g, u = R.gemm_ref(a, wg), R.gemm_ref(a, wu)
    return a, wg, wu, g / (1 + np.exp(-g)) * u


@pytest.mark.parametrize("F", [256, 384])
@pytest.mark.parametrize("K", [256, 640])
@pytest.mark.parametrize("M", [1, 16, 17, 129])
def test_gate_up_silu_quant_mx(M, K, F):
    assert ops.gate_up_silu_quant_mx_route(M, F, K) == ("decode" if M <= 16 else "tile")
    a, wg, wu, v = gate_up_case(M, K, F)
    assert pow2_clear(v, 2.0 ** -20)                          # (seeds checked on the CPU)
    o = ops.gate_up_silu_quant_mx(dev(a), ops.fuse_gate_up_mx(dev(wg), dev(wu)))
    assert (o.rows, o.k) == (M, F)
    assert_quantised(o, v, 2.0 ** -20)


@pytest.mark.parametrize("M", [1, 17])
def test_gate_and_up_are_not_interchangeable(M):
    a, wg, wu, v = gate_up_case(M, 256, 256)
    a_mx, g_mx, u_mx = dev(a), dev(wg), dev(wu)
    o, swapped = ops.gate_up_silu_quant_mx(a_mx, ops.fuse_gate_up_mx(g_mx, u_mx)), ops.gate_up_silu_quant_mx(a_mx, ops.fuse_gate_up_mx(u_mx, g_mx))
    assert_quantised(o, v, 2.0 ** -20)
    assert not torch.equal(o.q4, swapped.q4) and not torch.equal(o.q8, swapped.q8)


# ---------------------------------------------------------------------------------------------------------- RMSNorm quantisers
# The kernel's value carries at most about 24 FP32 roundings (the summation tree: 8 fused steps per chunk, the chunks of a thread, 6
# butterfly stages, 3 wave sums; mean, + eps, root, reciprocal; two products): below 24 * 2^-24 < 2^-19 relative; 2^-18 covers it twice.
RMS_MARGIN = 2.0 ** -18
EPS = 1e-5


def rms_case(M, K, add):
    rng = np.random.default_rng(10 * M + K + add)
    x, _, idx = random_layer(M, 64, K, seed=M + K)
    res = rng.standard_normal((M, K)).astype(np.float16)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    s = (x.astype(np.float64) + res.astype(np.float64)).astype(np.float16) if add else x
    s64 = s.astype(np.float64)
    v = (s64 * w.astype(np.float64) / np.sqrt((s64 ** 2).mean(-1, keepdims=True) + EPS))[:, idx]
    return x, res, w, idx, s, v


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("M", [1, 17])
def test_rmsnorm_quant_mx(M, K, add):
    x, res, w, idx, s, v = rms_case(M, K, add)
    assert pow2_clear(v, RMS_MARGIN)                          # (seeds checked on the CPU)
    xd, wd, idd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(idx).cuda()
    if add:
        rd = torch.from_numpy(res).cuda()
        o = ops.add_rmsnorm_quant_mx(xd, rd, wd, idd, EPS)
        assert np.array_equal(rd.cpu().numpy().view(np.uint16), s.view(np.uint16))
    else:
        o = ops.rmsnorm_quant_mx(xd, wd, idd, EPS)
    assert_quantised(o, v, RMS_MARGIN)


# ----------------------------------------------------------------------------------------------------------- gemm_mxfp4(add=)
@pytest.mark.parametrize("M", [1, 17])
def test_gemm_add_bit_for_bit(M):
    N, K = 192, 640
    a, w = exact_operand(M, K, 125, seed=M), exact_operand(N, K, 124, seed=N + K)
    # sums are multiples of 2^-7 below 2^14 (tests/test_gpu_mx.py); a residual of multiples of 2^-3 up to 128 keeps acc + residual exact in FP32
    res = (np.random.default_rng(M).integers(-1024, 1025, (M, N)) / 8.0).astype(np.float16)
    want = (R.gemm_ref(a, w) + res.astype(np.float64)).astype(np.float16)
    got = ops.gemm_mxfp4(dev(a), dev(w), add=torch.from_numpy(res).cuda()).cpu().numpy()
    assert np.isfinite(want).all() and np.array_equal(got.view(np.uint16), want.view(np.uint16))


# ------------------------------------------------------------------------------------------------------------- layer and model
H_, F_ = 256, 384


def _cfg(**kw):
    base = dict(hidden_size=H_, num_attention_heads=2, num_key_value_heads=1, intermediate_size=F_, rms_norm_eps=1e-5, rope_theta=1e4,
                num_hidden_layers=2, vocab_size=500, pad_token_id=None, sliding_window=None)
    return types.SimpleNamespace(**{**base, **kw})


@pytest.fixture(scope="module")
def model():
    from atom_amd.e2e import LlamaForCausalLM
    torch.manual_seed(0)
    m = LlamaForCausalLM(_cfg(linear_format="mxfp4")).cuda()
    g = torch.Generator().manual_seed(100)
    for mod in m.modules():
        if type(mod).__name__ == "LinearMxfp4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
    return m


def _hidden(T, seed):
    x = torch.randn((T, H_), generator=torch.Generator().manual_seed(seed))
    x[:, :4] *= 10
    return x.half().cuda()


def parity(got, ref):
    return (np.abs(got.cpu().numpy().astype(np.float64) - ref) / (1e-2 * np.maximum(np.abs(ref), np.sqrt((ref ** 2).mean())))).max()


@pytest.mark.parametrize("T", [1, 19])
def test_layer_equals_its_composition_and_the_staged_reference(model, T):
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    from tests.test_gpu_moe import _pool
    layer = model.model.layers[0]
    at, mlp, il, pl = layer.self_attn, layer.mlp, layer.input_layernorm, layer.post_attention_layernorm
    blen, x = BatchLenInfo([T], 0, "cuda"), _hidden(T, 40 + T)
    got = layer(x.clone(), blen, BatchedKvCacheInt4([KvCacheInt4(_pool(2, 1, 4, 16), T)]), None)
    # op by op, into a cache of its own; each GEMM against float64 on the operands the kernel read
    kv, h = BatchedKvCacheInt4([KvCacheInt4(_pool(2, 1, 4, 16), T)]), x.clone()
    x_mx = ops.rmsnorm_quant_mx(h, il.weight, il.reorder_index, il.variance_epsilon)
    qkv = ops.gemm_mxfp4(x_mx, at.qkv_mx())
    assert parity(qkv, R.gemm_ref(plain_np(x_mx), plain_np(at.qkv_mx()))) <= 1.0
    q, k, v = (t.contiguous().view(T, -1, 128) for t in qkv.split([H_, 128, 128], dim=1))
    (k4, ksz), (v4, vsz) = ops.kv_quant_u4(k), ops.kv_quant_u4(v)
    ops.init_kv_i4(kv, k4, v4, ksz, vsz, blen.indptr, 0)
    attn = ops.batch_prefill_i4(q, blen.indptr, kv, 0, rope_theta=at.rope_theta, max_q_len=T).view(T, H_)
    a_mx = ops.reorder_quant_mx(attn, at.reorder_index)
    o = ops.gemm_mxfp4(a_mx, at.o_proj.weight_mx())
    assert parity(o, R.gemm_ref(plain_np(a_mx), plain_np(at.o_proj.weight_mx()))) <= 1.0
    n_mx = ops.add_rmsnorm_quant_mx(o, h, pl.weight, pl.reorder_index, pl.variance_epsilon)
    assert torch.equal(h.view(torch.int16), (x + o).view(torch.int16))
    act = ops.gate_up_silu_quant_mx(n_mx, mlp.gate_up_mx())
    want = ops.gemm_mxfp4(act, mlp.down_proj.weight_mx(), add=h)
    down_ref = R.gemm_ref(plain_np(act), plain_np(mlp.down_proj.weight_mx())) + h.cpu().numpy().astype(np.float64)
    assert parity(want, down_ref) <= 1.0
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_layer_capture_replays_on_new_inputs(model):
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    from tests.test_gpu_moe import _pool
    layer, seq = model.model.layers[0], KvCacheInt4(_pool(2, 1, 4, 16), 7)
    layer(_hidden(7, 1), BatchLenInfo([7], 0, "cuda"), BatchedKvCacheInt4([seq]), None)
    seq.acquire_one()
    kv, blen = BatchedKvCacheInt4([seq]), BatchLenInfo([], 1, "cuda")
    sx, graph = _hidden(1, 2), torch.cuda.CUDAGraph()
    layer(sx.clone(), blen, None, kv)
    with torch.cuda.graph(graph):
        out = layer(sx, blen, None, kv)                       # (the layer overwrites sx with the post-attention stream)
    for seed in (7, 8):
        x2 = _hidden(1, seed)
        sx.copy_(x2)
        graph.replay()
        assert torch.equal(out.view(torch.int16), layer(x2.clone(), blen, None, kv).view(torch.int16))


def test_generate_equals_the_eager_loop(model):
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    from tests.test_gpu_moe import _eager_decode, _pages, _pool, _prefill
    new, gp = 4, torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 500, (n,), generator=gp).tolist() for n in (7, 19)]
    cap, capacity = max(-(-(len(p) + new - 1) // 16) for p in prompts), _pages([len(p) for p in prompts], 16, new) + 2
    seqs, first, _ = _prefill(model, prompts, _pool(2, 1, capacity, 16))
    toks, _ = _eager_decode(model, seqs, first, new - 1, cap)
    pg = _pool(2, 1, capacity, 16)
    got = generate(model, prompts, new, pg, caches=[KvCacheInt4(pg, 0) for _ in prompts])
    assert got == torch.cat([first[None], toks]).t().tolist()


def test_config_switch():
    from atom_amd.e2e import LlamaForCausalLM, MixtralForCausalLM
    assert type(LlamaForCausalLM(_cfg()).model.layers[0].mlp.gate_proj).__name__ == "LinearInt4"
    assert type(LlamaForCausalLM(_cfg(linear_format="mxfp4")).model.layers[0]).__name__ == "LlamaDecoderLayerMxfp4"
    with pytest.raises(ValueError):
        LlamaForCausalLM(_cfg(linear_format="fp8"))
    with pytest.raises(NotImplementedError):
        MixtralForCausalLM(_cfg(linear_format="mxfp4", num_local_experts=4, num_experts_per_tok=2))
    with pytest.raises(NotImplementedError):
        LlamaForCausalLM(_cfg(linear_format="mxfp4", num_attention_heads=4))   # head size 64
