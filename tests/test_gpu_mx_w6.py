"""MXFP6 weights (W6A4 / W6A6) on the GPU against float64 through tests/mx_ref.py and tests/mx6_ref.py."""
import numpy as np
import pytest
import torch

from atom_amd import ops
from tests import mx6_ref as R6
from tests import mx_ref as R
from tests.test_gpu_llama_mx import _cfg, pow2_clear
from tests.test_gpu_mx import FACTOR, INT8_CODES, bound, plain_np
from tests.test_gpu_mx6 import assert_quantised, dev, pads_are_zero_blocks, planted
from tests.test_gpu_mx6 import test_capture_replay_and_generate_equal_eager as replay_and_generate_equal_eager
from tests.test_gpu_mx6 import test_layer_equals_its_composition as layer_equals_its_composition

pytestmark = pytest.mark.gpu
DEQ = {"mxfp4": R.dequant, "mxfp6": R6.dequant}


@pytest.mark.parametrize("M", [16, 17])                       # the decode and the tile geometry
def test_layout_one_hot_first_operand(M):
    """One weight row tile per (row, channel, bit) with a single non-zero E2M3 code (1 << bit; 0x21 for the sign bit, 0x20 alone being
    -0) times an all-ones activation: that output feature, and no other, is the code's value for every token."""
    row, ch, bit = (t.reshape(-1) for t in np.meshgrid(np.arange(16), np.arange(128), np.arange(6), indexing="ij"))
    n, code = len(row), np.where(bit == 5, 0x21, 1 << bit).astype(np.uint8)
    codes = np.zeros((16 * n, 128), np.uint8)
    codes[16 * np.arange(n) + row, ch] = code
    w = (R6.pack6(codes), np.full((16 * n, 4), 127, np.uint8), np.zeros((16 * n, 128), np.uint8), np.full((16 * n, 4), 127, np.uint8))
    ones = (np.full((M, 64), 0x22, np.uint8), np.full((M, 4), 127, np.uint8), np.full((M, 128), 0x38, np.uint8), np.full((M, 4), 127, np.uint8))
    want = np.zeros(16 * n)
    want[16 * np.arange(n) + row] = R.decode(code, "e2m3")
    got = ops.gemm_mxfp4(dev(ones), dev(w)).cpu().numpy().astype(np.float64)
    bad = np.argwhere((got != want[None]).any(0))
    assert len(bad) == 0, [(row[i // 16], ch[i // 16], bit[i // 16], i % 16, got[0, i]) for i in bad[:6, 0]]


@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("N", [1, 17])
def test_weight_quantiser(N, K):
    w = planted(N, K, seed=N + K)                             # ties, saturation, zero blocks, negative zeros: exact in fp16, so codes are equal
    o = ops.quant_weight_mx(torch.from_numpy(w).cuda(), weight_format="mxfp6")
    assert tuple(o.q4.shape) == ((N + 15) // 16, K // 128 - 1, 96, 16) and pads_are_zero_blocks(o, N, K)
    for name, g, r in zip(("codes", "scales", "keeper codes", "keeper scales"), plain_np(o), R6.quantise_plain(w)):
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:4])


# E2M3 codes are multiples of 2^-3 up to 7.5 (E2M1: of 2^-1 up to 6).  With bulk scale bytes lo .. lo + span - 1 on either side every
# bulk product is a multiple of u = 2^-6 2^(lo_a - 127) 2^(lo_w - 127) and at most 56.25 x 4 / 2^-6 = 14400 u (span 2 on both sides);
# keeper codes are integers up to 8 under scale bytes lo - 3 .. lo - 3 + span - 1, so a keeper product is a multiple of u and at most
# 64 x 4 u.  K <= 640, spans 2, 2: 512 x 14400 + 128 x 256 < 2^23.  K = 1280, spans 1 (activation), 2 (weight): 1152 x 7200 + 128 x 128
# = 8310784 < 2^23 = 8388608.  Every partial sum is an integer below 2^23 times u: exact in FP32 in any order.
def exact_operand(rows, K, lo, span, fmt, seed):
    rng, s = np.random.default_rng(seed), K // 128 - 1
    return (rng.integers(0, 256, (rows, (96 if fmt == "mxfp6" else 64) * s), dtype=np.uint8), rng.integers(lo, lo + span, (rows, 4 * s)).astype(np.uint8),
            rng.choice(INT8_CODES, (rows, 128)), rng.integers(lo - 3, lo - 3 + span, (rows, 4)).astype(np.uint8))


@pytest.mark.parametrize("act", ["mxfp4", "mxfp6"])
@pytest.mark.parametrize("M,N,K", [(M, N, K) for M in (1, 16, 17, 129) for N in (64, 192) for K in (256, 640)] + [(1, 64, 1280)])
def test_gemm_exact_sums_bit_for_bit(M, N, K, act):
    a, w = exact_operand(M, K, 126, 1 if K == 1280 else 2, act, seed=M), exact_operand(N, K, 124, 2, "mxfp6", seed=N + K)
    ref = DEQ[act](a) @ R6.dequant(w).T
    got = ops.gemm_mxfp4(dev(a), dev(w)).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), ref.astype(np.float16).view(np.uint16)), np.abs(got - ref).max()
    if (N, K) == (192, 640) and M in (16, 129):               # add=: multiples of 2^-3 up to 128 keep acc + residual exact in FP32
        res = (np.random.default_rng(M).integers(-1024, 1025, (M, N)) / 8.0).astype(np.float16)
        got = ops.gemm_mxfp4(dev(a), dev(w), add=torch.from_numpy(res).cuda()).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), (ref + res.astype(np.float64)).astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("M,N,K", [(16, 192, 640), (17, 64, 640), (129, 192, 640)])
def test_gemm_on_quantiser_output(M, N, K):
    """tests/test_gpu_mx.py's bound and the parity limit for W6A4 and W6A6; RMS error against the unquantised x . w^T: W6A6 below half of
    W4A4's and below both mixed forms.  The float64 reference alone on these seeds (quantise, dequantise, multiply; no kernel) gives
    W6A6 / W4A4 = 0.282, 0.267, 0.273, W6A6 / W4A6 = 0.379, 0.370, 0.368 and W6A6 / W6A4 = 0.384, 0.385, 0.376 at the three shapes."""
    rng = np.random.default_rng(M + N + K)
    x, wt = rng.standard_normal((M, K)).astype(np.float16), (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    xd, wd, exact, rms = torch.from_numpy(x).cuda(), torch.from_numpy(wt).cuda(), x.astype(np.float64) @ wt.astype(np.float64).T, {}
    for wf, af in [(wf, af) for wf in DEQ for af in DEQ]:
        a_mx, w_mx = ops.reorder_quant_mx(xd, None, act_format=af), ops.quant_weight_mx(wd, weight_format=wf)
        got, da, dw = ops.gemm_mxfp4(a_mx, w_mx).cpu().numpy().astype(np.float64), DEQ[af](plain_np(a_mx)), DEQ[wf](plain_np(w_mx))
        ref, blocks = da @ dw.T, sum(np.abs(da[:, k:k + 32] @ dw[:, k:k + 32].T) for k in range(0, K, 32))
        ratio, parity = (np.abs(got - ref) / bound(ref, blocks, K)).max(), (np.abs(got - ref) / (1e-2 * np.maximum(np.abs(ref), np.sqrt((ref ** 2).mean())))).max()
        rms[wf, af] = np.sqrt(((got - exact) ** 2).mean())
        print(f"W {wf} A {af} {M}x{N}x{K}: worst error / bound = {ratio:.3f}, error / parity limit = {parity:.4f}, rms error vs x.w^T = {rms[wf, af]:.5f}")
        assert wf == "mxfp4" or (ratio <= FACTOR and parity <= 1.0)
    w6a6 = rms["mxfp6", "mxfp6"]
    print(f"W6A6 / W4A4 = {w6a6 / rms['mxfp4', 'mxfp4']:.3f}, / W4A6 = {w6a6 / rms['mxfp4', 'mxfp6']:.3f}, / W6A4 = {w6a6 / rms['mxfp6', 'mxfp4']:.3f}")
    assert w6a6 < 0.5 * rms["mxfp4", "mxfp4"] and w6a6 < rms["mxfp4", "mxfp6"] and w6a6 < rms["mxfp6", "mxfp4"]


@pytest.mark.parametrize("act", ["mxfp4", "mxfp6"])
@pytest.mark.parametrize("F", [256, 384])
@pytest.mark.parametrize("M", [1, 17])
def test_gate_up_silu_quant_w6(M, F, act):
    K = 256                                                   # g and u are exact (exact_operand's argument at 128 bulk channels)
    a, wg, wu = exact_operand(M, K, 126, 2, act, seed=M + K), exact_operand(F, K, 124, 2, "mxfp6", seed=F + K), exact_operand(F, K, 124, 2, "mxfp6", seed=F + K + 1)
    g, u = DEQ[act](a) @ R6.dequant(wg).T, DEQ[act](a) @ R6.dequant(wu).T
    v = g / (1 + np.exp(-g)) * u
    assert pow2_clear(v, 2.0 ** -20)                          # (seeds checked on the CPU)
    o = ops.gate_up_silu_quant_mx(dev(a), ops.fuse_gate_up_mx(dev(wg), dev(wu), weight_format="mxfp6"), out_format="mxfp6")
    assert (o.rows, o.k) == (M, F) and tuple(o.q4.shape) == ((M + 15) // 16, F // 128 - 1, 96, 16) and pads_are_zero_blocks(o, M, F)
    assert_quantised(o, v, 2.0 ** -20)


@pytest.fixture(scope="module", params=["mxfp6", {"down_proj": "mxfp6"}], ids=["all", "down_proj"])
def model(request):
    from atom_amd.e2e import LlamaForCausalLM
    m = LlamaForCausalLM(_cfg(linear_format="mxfp4", activation_format="mxfp6", weight_format=request.param)).cuda()
    g, mlp = torch.Generator().manual_seed(100), m.model.layers[0].mlp
    for mod in m.modules():
        if type(mod).__name__ == "LinearMxfp4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
    assert (mlp.gate_up_mx().q4.shape[2], mlp.down_proj.weight_mx().q4.shape[2]) == ((96, 96) if request.param == "mxfp6" else (64, 96))
    return m


# the checks of tests/test_gpu_mx6.py on the models built here (the ops read every weight's format off its operand): the layer against
# its op-by-op composition; a captured decode step replayed against the eager call and generate() against the eager loop
@pytest.mark.parametrize("T", [1, 19])
def test_layer_equals_its_composition(model, T):
    layer_equals_its_composition(model, T)


def test_capture_replay_and_generate_equal_eager(model):
    replay_and_generate_equal_eager(model)
