"""GPU: the planted rows of tests/quant_planted.py through every form of the activation quantisers, bit for bit against the unmutated
oracle -- codes, keeper, scales and the de-quantised tensor; packed, wide and BF6 stores; with and without a reorder index; the
RMSNorm ops at two eps and two hidden sizes (4096: the instances with compile-time LDS buffers); and the quantisers inside
atom_gemm_w4a4_multi_q (csrc/gemvq_w4a4.hip and the decode-batch form: separate implementations) at one and two tokens.
tests/test_quant_planted_cpu.py shows that each deliberate error (wrong rounding rule, lower clamp, clip on the keeper, maximum
without abs, reciprocal of the stored scale, product order, eps, zero-group rule, FP32 scale in the de-quantised tensor) moves these
rows' reference, so a kernel that made one could not pass here."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import quant_planted as P
from tests.helpers import assert_quant_equal, bits16, rand_gemm_operands, t2n, to_device

pytestmark = pytest.mark.gpu

FORMATS = [False, True, "f6"]


def _ops():
    from atom_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _tail_case(mode, clip):
    y = P.tail_rows(mode, clip)
    return y, P.run("reorder", (y, None), mode, clip)


@pytest.mark.parametrize("with_index", [False, True], ids=["in-order", "gathered"])
@pytest.mark.parametrize("mode,clip", P.MODE_CLIPS)
def test_reorder_on_planted_rows(mode, clip, with_index):
    ops = _ops()
    y, ref = _tail_case(mode, clip)
    idx = P.perm(y.shape[1]) if with_index else None
    x = _dev(P.scatter(y, idx) if with_index else y)
    it = _dev(idx) if with_index else None
    for fmt in FORMATS:
        outs = ops.reorder_fp16_i4(x, it, quant_mode=mode, clip=clip, scale_layout="plain", return_dequant=True, wide_codes=fmt)
        assert_quant_equal(outs, ref, len(y), fmt=fmt, xq_ref=ref["xq"], what=f"reorder {mode} {clip} fmt={fmt}")
    outs = ops.reorder_fp16_i4(x, it, quant_mode=mode, clip=clip, scale_layout="ref")                  # without the de-quantised output: other instances
    assert_quant_equal(outs, ref, len(y), layout="ref", what=f"reorder {mode} {clip} ref layout")


@pytest.mark.parametrize("mode,clip", P.MODE_CLIPS)
def test_silu_mul_on_saturated_gates(mode, clip):
    """gates from {0} u [17, 48]: silu(a) = a in FP32 (the CPU test shows the oracle gives exactly a * b), so the SiLU op is compared
    bit for bit (exact), ties, clamp and zero groups included"""
    ops = _ops()
    a, b = P.silu_planted(mode, clip)
    ref = P.run("silu_mul", (a, b), mode, clip)
    at, bt = _dev(a), _dev(b)
    for fmt in FORMATS:
        outs = ops.activate_fp16_i4(at, bt, quant_mode=mode, clip=clip, scale_layout="plain", return_dequant=True, wide_codes=fmt)
        assert_quant_equal(outs, ref, len(a), fmt=fmt, xq_ref=ref["xq"], what=f"silu_mul {mode} {clip} fmt={fmt}")
    outs = ops.activate_fp16_i4(at, bt, quant_mode=mode, clip=clip, scale_layout="ref")
    assert_quant_equal(outs, ref, len(a), layout="ref", what=f"silu_mul {mode} {clip} ref layout")


@pytest.mark.parametrize("H", P.NORM_HS)
@pytest.mark.parametrize("eps", P.EPS)
@pytest.mark.parametrize("mode,clip", P.NORM_MODE_CLIPS)
def test_rmsnorm_and_add_rmsnorm_on_planted_rows(mode, clip, eps, H):
    ops = _ops()
    x, w, idx = P.norm_rows(H, mode, clip, eps)
    ref = P.run("rmsnorm", (x, w, eps, idx), mode, clip)
    wt, it = _dev(w), _dev(idx)
    what = f"{mode} {clip} eps={eps} H={H}"
    outs = ops.rmsnorm_fp16_i4(_dev(x), wt, it, eps, quant_mode=mode, clip=clip, scale_layout="plain", return_dequant=True)
    assert_quant_equal(outs, ref, len(x), xq_ref=ref["xq"], what="rmsnorm " + what)
    xa, res = P.add_split(x)                                  # x + residual == the same rows, both finite
    outs = ops.add_rmsnorm_fp16_i4(_dev(xa), _dev(res), wt, it, eps, quant_mode=mode, clip=clip, scale_layout="plain", return_dequant=True)
    assert np.array_equal(bits16(t2n(outs[0])), bits16(x)), "add_rmsnorm: the residual stream"
    assert_quant_equal(outs[1:], ref, len(x), xq_ref=ref["xq"], what="add_rmsnorm " + what)
    for fmt in FORMATS[1:]:
        outs = ops.rmsnorm_fp16_i4(_dev(x), wt, it, eps, quant_mode=mode, clip=clip, scale_layout="plain", wide_codes=fmt)
        assert_quant_equal(outs, ref, len(x), fmt=fmt, what=f"rmsnorm {what} fmt={fmt}")


def _fused(N, K, nseg):
    ops = _ops()
    devs = [to_device(rand_gemm_operands(4, N, K, seed=51 + i), "ref") for i in range(nseg)]
    mods = [types.SimpleNamespace(weight_int4=torch.nn.Parameter(dv[1], requires_grad=False), weight_int8=torch.nn.Parameter(dv[5], requires_grad=False),
                                  scale_int4=torch.nn.Parameter(dv[3], requires_grad=False), scale_int8=torch.nn.Parameter(dv[7], requires_grad=False),
                                  packed=None) for dv in devs]
    for md in mods:
        md.packed = (lambda md=md: (md.weight_int4.data, md.weight_int8.data, md.scale_int4.data, md.scale_int8.data))
    return ops.fuse_projection_weights(mods)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("clip", [1.0, 0.9])
@pytest.mark.parametrize("op,N,K,nseg", P.MULTI_Q_CASES + P.MULTI_Q_ROUTE_CASES)
def test_quantisers_inside_the_gemm_launch_on_planted_rows(op, N, K, nseg, clip, M):
    """atom_gemm_w4a4_multi_q: the planted rows, M at a time, against the separate quantiser op followed by atom_gemm_w4a4_multi, bit
    for bit (in the summation order the separate entry points take for the token count: see
    test_quantiser_inside_the_gemm_launch_equals_quantiser_then_gemm).  The separate op's operand is first compared with the
    oracle, so the chain reaches the oracle: a quantiser inside the launch that broke a tie the other way, took the reciprocal of the
    stored scale or mishandled a zero group would give another operand and, on these rows, other sums."""
    ops = _ops()
    assert ops.multi_q_gemm_fits(op, M, N, nseg, K)
    eps, mode = 1e-5, "kernel"
    fused = _fused(N, K, nseg)
    res = None
    if op == "reorder":
        idx = P.perm(K)
        y = P.tail_rows(mode, clip, K)
        x, x2 = P.scatter(y, idx), None
        ref = P.run("reorder", (x, idx), mode, clip)
    elif op == "silu_mul":
        idx = None
        x, x2 = P.silu_planted(mode, clip, K)
        ref = P.run("silu_mul", (x, x2), mode, clip)
    else:
        s, x2, idx = P.norm_rows(K, mode, clip, eps)
        ref = P.run("rmsnorm", (s, x2, eps, idx), mode, clip)
        x, res = P.add_split(s) if op == "add_rmsnorm" else (s, None)
    R = len(x)
    xt, x2t = _dev(x), (None if x2 is None else _dev(x2))
    it, rt = (None if idx is None else _dev(idx)), (None if res is None else _dev(res))

    def separate(rows):
        """the quantiser op on the given rows -> (keeper, codes, keeper scales, group scales), x + residual"""
        if op == "reorder":
            return ops.reorder_fp16_i4(xt[rows], it, clip=clip), None
        if op == "rmsnorm":
            return ops.rmsnorm_fp16_i4(xt[rows], x2t, it, eps, clip=clip), None
        if op == "silu_mul":
            return ops.activate_fp16_i4(xt[rows], x2t[rows], clip=clip), None
        out = ops.add_rmsnorm_fp16_i4(xt[rows], rt[rows], x2t, it, eps, clip=clip)
        return out[1:], out[0]

    every = torch.arange(R, device="cuda")
    qt, _ = separate(every)
    assert_quant_equal(qt, ref, R, layout="ref", what=f"{op} (separate op) clip={clip} K={K}")
    dot = ops.L.lib().atom_gemm_w4a4_packed_order(M, N * nseg, K, 0) == 64
    assert dot == (M == 1 or K > P.MULTI_Q_DOT_K), "the planted rows no longer reach the quantiser of the kernel this case is here for"
    rep = 1 if dot else 2                                      # the decode-batch kernel needs two rows more: the tokens twice over
    for r0 in range(0, R - M + 1, M):
        rows = every[r0:r0 + M]
        (outlier, norms, outlier_scales, norm_scales), res_want = separate(rows.repeat(rep))
        assert_quant_equal((outlier, norms, outlier_scales, norm_scales), {k: np.tile(ref[k][r0:r0 + M], (rep,) + (1,) * (ref[k].ndim - 1)) for k in ("q4", "q8", "s4", "s8")},
                           M * rep, layout="ref", what=f"{op} rows {r0}..")
        want = [t[:M] for t in ops.dense_layer_gemm_i4_multi(norms, norm_scales, outlier, outlier_scales, fused)]
        kw = dict(clip=clip)
        if op != "silu_mul":
            kw["reorder_index"] = it
        if op in ("rmsnorm", "add_rmsnorm"):
            kw.update(x2=x2t, eps=eps)
        if op == "add_rmsnorm":
            kw["residual"] = rt[rows].contiguous()
        if op == "silu_mul":
            kw["x2"] = x2t[rows].contiguous()
        got, res_out = ops.dense_layer_gemm_i4_multi_q(op, xt[rows].contiguous(), fused, **kw)
        for i in range(nseg):
            assert got[i].dtype == want[i].dtype and torch.equal(got[i].view(torch.int16), want[i].view(torch.int16)), (op, M, clip, r0, i)
        if op == "add_rmsnorm":
            assert torch.equal(res_out.view(torch.int16), res_want[:M].view(torch.int16)), (op, M, r0)
            assert np.array_equal(bits16(t2n(res_out)), bits16(s[r0:r0 + M]))
