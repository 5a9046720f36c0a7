"""MXFP6 activations (W4A6) on the GPU against float64 through tests/mx6_ref.py."""
import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import mx6_ref as R6
from tests import mx_ref as R
from tests.test_gpu_llama_mx import EPS, RMS_MARGIN, _cfg, _hidden, pow2_clear, rms_case
from tests.test_gpu_mx import FACTOR, bound, exact_operand, plain_np

pytestmark = pytest.mark.gpu

GRID = R.decode(np.arange(32), "e2m3")


def dev(plain):
    return ops.mx_from_plain(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in plain))


def planted(rows, k, seed):
    """Block b of row r by (b + r) % 6: random; zero; the grid's 31 midpoints (ties, both parities) beside a pinning 7.5, + / -; values
    that saturate; -0.0 and negatives that round to the negative-zero code."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, k // 32, 32)) * np.exp2(rng.integers(-6, 6, (rows, k // 32, 1)))
    ties = np.append((GRID[1:] + GRID[:-1]) / 2, 7.5)
    for r in range(rows):
        for b in range(k // 32):
            kind, s, v = (b + r) % 6, np.exp2(float(rng.integers(-8, 8))), x[r, b]
            if kind == 1:
                v[:] = 0
            elif kind in (2, 3):
                v[:] = ties * s * (1 if kind == 2 else -1)
            elif kind == 4:
                v[:] = rng.uniform(-7.5, 7.5, 32) * s
                v[:4] = np.array([7.75, 7.875, -7.8125, 7.625]) * s
            elif kind == 5:
                v[:8] = np.array([-0.0, -0.0, -0.03125, -0.0625, 0.0625, -0.1875, 7.0, -0.0]) * s
    return x.reshape(rows, k).astype(np.float16)


def assert_quantised(o, v, margin):
    """tests/test_gpu_llama_mx.py's rule: scale bytes equal; per element no further from v than the best code by more than v's own error"""
    got, want = plain_np(o), R6.quantise_plain(v)
    assert got[0].shape == want[0].shape and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    err, best = np.abs(R6.dequant(got) - v), np.abs(R6.dequant(want) - v)
    assert not (err > best * (1 + 2.0 ** -10) + margin * np.abs(v)).any()


def pads_are_zero_blocks(o, M, K):
    pad = plain_np(ops.MxOperand(o.q4[-1:], o.sc[-1:], o.q8[-1:], 16, K))
    return not pad[0][M % 16:].any() and not pad[2][M % 16:].any() and (pad[1][M % 16:] == 127).all() and (pad[3][M % 16:] == 127).all()


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("M", [1, 17])
def test_quantisers(M, K, reorder):
    xr = planted(M, K, seed=M + K)
    idx = np.random.default_rng(K).permutation(K) if reorder else np.arange(K)
    idd = torch.from_numpy(idx.astype(np.int16)).cuda() if reorder else None
    x = np.empty_like(xr)
    x[:, idx] = xr
    o = ops.reorder_quant_mx(torch.from_numpy(x).cuda(), idd, act_format="mxfp6")
    for name, g, w in zip(("codes", "scales", "keeper codes", "keeper scales"), plain_np(o), R6.quantise_plain(xr)):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:4])
    assert pads_are_zero_blocks(o, M, K)
    for add in (False, True):
        xn, res, w, pidx, s, v = rms_case(M, K, add)
        if not reorder:
            v = v[:, np.argsort(pidx)]
        assert pow2_clear(v, RMS_MARGIN)
        xd, wd, rd = torch.from_numpy(xn).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(res).cuda()
        pid = torch.from_numpy(pidx).cuda() if reorder else None
        if add:
            o = ops.add_rmsnorm_quant_mx(xd, rd, wd, pid, EPS, act_format="mxfp6")
            assert np.array_equal(rd.cpu().numpy().view(np.uint16), s.view(np.uint16))
        else:
            o = ops.rmsnorm_quant_mx(xd, wd, pid, EPS, act_format="mxfp6")
        assert_quantised(o, v, RMS_MARGIN)


def ones_weight(N, K):
    return (np.full((N, (K - 128) // 2), 0x22, np.uint8), np.full((N, (K - 128) // 32), 127, np.uint8), np.full((N, 128), 0x38, np.uint8),
            np.full((N, 4), 127, np.uint8))


def test_layout_one_hot():
    """One row tile per (row, channel, bit) with a single non-zero code (1 << bit; 0x21 for the sign bit, 0x20 alone being -0) times an
    all-ones weight: that output row, and no other, is the code's value."""
    row, ch, bit = (t.reshape(-1) for t in np.meshgrid(np.arange(16), np.arange(128), np.arange(6), indexing="ij"))
    n, code = len(row), np.where(bit == 5, 0x21, 1 << bit).astype(np.uint8)
    codes = np.zeros((16 * n, 128), np.uint8)
    codes[16 * np.arange(n) + row, ch] = code
    a = (R6.pack6(codes), np.full((16 * n, 4), 127, np.uint8), np.zeros((16 * n, 128), np.uint8), np.full((16 * n, 4), 127, np.uint8))
    want = np.zeros((16 * n, 64))
    want[16 * np.arange(n) + row] = R.decode(code, "e2m3")[:, None]
    got = ops.gemm_mxfp4(dev(a), dev(ones_weight(64, 256))).cpu().numpy().astype(np.float64)
    bad = np.argwhere((got != want).any(1))
    assert len(bad) == 0, [(row[i // 16], ch[i // 16], bit[i // 16], i % 16, got[i, 0]) for i in bad[:6, 0]]


# E2M3 codes are multiples of 1/8 up to 7.5, E2M1 of 1/2 up to 6, scale bytes 125 .. 127 and 124 .. 126: every product is a multiple of
# u = 2^-9 and at most 11520 u, so any partial sum of K <= 640 channels is an integer below 2^23 times u: exact in FP32 in every order.
def exact_operand6(rows, K, lo, seed):
    _, scales, k8, s8 = exact_operand(rows, K, lo, seed)
    return np.random.default_rng(seed + 1).integers(0, 256, (rows, 24 * (K - 128) // 32), dtype=np.uint8), scales, k8, s8


@pytest.mark.parametrize("K", [256, 640])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 16, 17, 129])
def test_gemm_exact_sums_bit_for_bit(M, N, K):
    a, w = exact_operand6(M, K, 125, seed=M), exact_operand(N, K, 124, seed=N + K)
    ref = R6.dequant(a) @ R.dequant(w).T
    got = ops.gemm_mxfp4(dev(a), dev(w)).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), ref.astype(np.float16).view(np.uint16)), np.abs(got - ref).max()
    if (N, K) == (192, 640) and M in (16, 129):               # add=: multiples of 2^-3 up to 128 keep acc + residual exact in FP32
        res = (np.random.default_rng(M).integers(-1024, 1025, (M, N)) / 8.0).astype(np.float16)
        got = ops.gemm_mxfp4(dev(a), dev(w), add=torch.from_numpy(res).cuda()).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), (ref + res.astype(np.float64)).astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("M,N,K", [(16, 192, 640), (17, 64, 640), (129, 192, 640)])
def test_gemm_on_quantiser_output(M, N, K):
    """tests/test_gpu_mx.py's bound and the parity limit; RMS error against x . dequant(W)^T below half of MXFP4's (float64: ~0.26)"""
    rng = np.random.default_rng(M + N + K)
    x, wt = rng.standard_normal((M, K)).astype(np.float16), (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    xd, w_mx = torch.from_numpy(x).cuda(), ops.quant_weight_mx(torch.from_numpy(wt).cuda())
    dw, rms = R.dequant(plain_np(w_mx)), {}
    for fmt, deq in (("mxfp4", R.dequant), ("mxfp6", R6.dequant)):
        a_mx = ops.reorder_quant_mx(xd, None, act_format=fmt)
        got, da = ops.gemm_mxfp4(a_mx, w_mx).cpu().numpy().astype(np.float64), deq(plain_np(a_mx))
        ref = da @ dw.T
        err, blocks = np.abs(got - ref), sum(np.abs(da[:, k:k + 32] @ dw[:, k:k + 32].T) for k in range(0, K, 32))
        ratio, parity = (err / bound(ref, blocks, K)).max(), (err / (1e-2 * np.maximum(np.abs(ref), np.sqrt((ref ** 2).mean())))).max()
        rms[fmt] = np.sqrt(((got - x.astype(np.float64) @ dw.T) ** 2).mean())
        print(f"{fmt} {M}x{N}x{K}: worst error / bound = {ratio:.3f}, error / parity limit = {parity:.4f}, rms error vs x.W^T = {rms[fmt]:.5f}")
        assert ratio <= FACTOR and parity <= 1.0
    assert rms["mxfp6"] < 0.5 * rms["mxfp4"]


# scale bytes from 123: g and u are exact in FP32 in every order (products multiples of 2^-12, partial sums below 2^22 of them)
@pytest.mark.parametrize("in6", [True, False])
@pytest.mark.parametrize("F", [256, 384])
@pytest.mark.parametrize("M", [1, 17])
def test_gate_up_silu_quant_mx6(M, F, in6):
    K = 256
    a = exact_operand6(M, K, 123, seed=M + K) if in6 else exact_operand(M, K, 123, seed=M + K)
    wg, wu = exact_operand(F, K, 123, seed=F + K), exact_operand(F, K, 123, seed=F + K + 1)
    da = (R6.dequant if in6 else R.dequant)(a)
    g, u = da @ R.dequant(wg).T, da @ R.dequant(wu).T
    v = g / (1 + np.exp(-g)) * u
    assert pow2_clear(v, 2.0 ** -20)                          # (seeds checked on the CPU)
    o = ops.gate_up_silu_quant_mx(dev(a), ops.fuse_gate_up_mx(dev(wg), dev(wu)), out_format="mxfp6")
    assert (o.rows, o.k) == (M, F) and tuple(o.q4.shape) == ((M + 15) // 16, F // 128 - 1, 96, 16)
    assert_quantised(o, v, 2.0 ** -20)
    assert pads_are_zero_blocks(o, M, F)


@pytest.fixture(scope="module")
def model():
    from atom_amd.e2e import LlamaForCausalLM
    m, g = LlamaForCausalLM(_cfg(linear_format="mxfp4", activation_format="mxfp6")).cuda(), torch.Generator().manual_seed(100)
    for mod in m.modules():
        if type(mod).__name__ == "LinearMxfp4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
    return m


@pytest.mark.parametrize("T", [1, 19])
def test_layer_equals_its_composition(model, T):
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    from tests.test_gpu_moe import _pool
    layer = model.model.layers[0]
    at, mlp, il, pl = layer.self_attn, layer.mlp, layer.input_layernorm, layer.post_attention_layernorm
    blen, x = BatchLenInfo([T], 0, "cuda"), _hidden(T, 40 + T)
    got = layer(x.clone(), blen, BatchedKvCacheInt4([KvCacheInt4(_pool(2, 1, 4, 16), T)]), None)
    kv, h = BatchedKvCacheInt4([KvCacheInt4(_pool(2, 1, 4, 16), T)]), x.clone()
    x_mx = ops.rmsnorm_quant_mx(h, il.weight, il.reorder_index, il.variance_epsilon, act_format="mxfp6")
    q, k, v = (t.contiguous().view(T, -1, 128) for t in ops.gemm_mxfp4(x_mx, at.qkv_mx()).split([256, 128, 128], dim=1))
    (k4, ksz), (v4, vsz) = ops.kv_quant_u4(k), ops.kv_quant_u4(v)
    ops.init_kv_i4(kv, k4, v4, ksz, vsz, blen.indptr, 0)
    attn = ops.batch_prefill_i4(q, blen.indptr, kv, 0, rope_theta=at.rope_theta, max_q_len=T).view(T, 256)
    o = ops.gemm_mxfp4(ops.reorder_quant_mx(attn, at.reorder_index, act_format="mxfp6"), at.o_proj.weight_mx())
    n_mx = ops.add_rmsnorm_quant_mx(o, h, pl.weight, pl.reorder_index, pl.variance_epsilon, act_format="mxfp6")
    act = ops.gate_up_silu_quant_mx(n_mx, mlp.gate_up_mx(), out_format="mxfp6")
    assert all(t.q4.shape[2] == 96 for t in (x_mx, n_mx, act))
    assert torch.equal(got.view(torch.int16), ops.gemm_mxfp4(act, mlp.down_proj.weight_mx(), add=h).view(torch.int16))


def test_capture_replay_and_generate_equal_eager(model):
    from atom_amd.e2e import generate
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    from tests.test_gpu_moe import _eager_decode, _pages, _pool, _prefill
    layer, seq = model.model.layers[0], KvCacheInt4(_pool(2, 1, 4, 16), 7)
    layer(_hidden(7, 1), BatchLenInfo([7], 0, "cuda"), BatchedKvCacheInt4([seq]), None)
    seq.acquire_one()
    kv, blen = BatchedKvCacheInt4([seq]), BatchLenInfo([], 1, "cuda")
    sx, graph = _hidden(1, 2), torch.cuda.CUDAGraph()
    layer(sx.clone(), blen, None, kv)
    with torch.cuda.graph(graph):
        out = layer(sx, blen, None, kv)
    for seed in (7, 8):
        x2 = _hidden(1, seed)
        sx.copy_(x2)
        graph.replay()
        assert torch.equal(out.view(torch.int16), layer(x2.clone(), blen, None, kv).view(torch.int16))
    new, gp = 4, torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 500, (n,), generator=gp).tolist() for n in (7, 19)]
    cap, capacity = max(-(-(len(p) + new - 1) // 16) for p in prompts), _pages([len(p) for p in prompts], 16, new) + 2
    seqs, first, _ = _prefill(model, prompts, _pool(2, 1, capacity, 16))
    toks, _ = _eager_decode(model, seqs, first, new - 1, cap)
    pg = _pool(2, 1, capacity, 16)
    assert generate(model, prompts, new, pg, caches=[KvCacheInt4(pg, 0) for _ in prompts]) == torch.cat([first[None], toks]).t().tolist()


@pytest.mark.parametrize("kw", [dict(activation_format="mxfp6"), dict(linear_format="mxfp4", activation_format="fp8")])
def test_activation_format_is_checked(kw):
    from atom_amd.e2e import LlamaForCausalLM
    with pytest.raises(ValueError):
        LlamaForCausalLM(_cfg(**kw))
