"""MXFP4 W4A4 against the shipped INT4 / BF6 routes on one GPU (profiles/mxfp4/README.md).

  python tools/mx_bench.py [--reps 5] [--iters 50]
  python tools/mx_bench.py --mlp       the fused gate/up SiLU-quantising launch against gemm_mxfp4 x 2 + silu_mul_quant_mx
  python tools/mx_bench.py --act mxfp6 MXFP6 activations (W4A6) against the MXFP4 ones: GEMM, fused gate/up, quantiser
  python tools/mx_bench.py --weight mxfp6   MXFP6 weights against the MXFP4 ones under either activation: GEMM, fused gate/up

Every figure is the median over --reps repetitions of the mean time of --iters replays of a captured graph holding one launch (hot:
operands stay in L2 / MALL where they fit), the two sides of a comparison alternating inside one repetition; the spread printed beside
a median is (max - min) over the repetitions of the same binary.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def time_graphs(graphs, reps, iters):
    """[median us, spread us] per graph; the graphs alternate inside a repetition"""
    t = [[] for _ in graphs]
    for g, _ in graphs:
        for _ in range(5):
            g.replay()
    for _ in range(reps):
        for i, (g, _) in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                g.replay()
            b.record()
            b.synchronize()
            t[i].append(a.elapsed_time(b) * 1e3 / iters)
    return [(statistics.median(x), max(x) - min(x)) for x in t]


def operands(M, N, K, dev):
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    x = torch.randn((M, K), generator=g, device=dev, dtype=torch.float16)
    x[:, -128:] *= 20
    w = (torch.randn((N, K), generator=g, device=dev, dtype=torch.float16) * 0.05)
    return x, w


def gemm_pair(M, N, K, dev):
    """(MX GEMM, the shipped route on its fastest operand form for the shape) as callables"""
    x, w = operands(M, N, K, dev)
    a_mx, w_mx = ops.reorder_quant_mx(x), ops.quant_weight_mx(w)
    b4, b8, sb, sb8 = ops.quant_weight_w4(w)
    o8, o4, s8, s4 = ops.reorder_fp16_i4(x, None, scale_layout="plain")
    if M > 256:                                                # prefill: both operands in the BF6 form (the headline kernel's own)
        a6, w6 = ops.repack_act_f6(o4.view(torch.uint8), s4, scale_layout="plain"), ops.repack_weight_f6(b4, sb)
        ref = lambda: ops.dense_layer_gemm_i4_fp16(a6, w6, s4, sb, o8, b8, s8, sb8, scale_layout="plain", a_wide="f6")   # noqa: E731
    else:
        ref = lambda: ops.dense_layer_gemm_i4_fp16(o4, b4, s4, sb, o8, b8, s8, sb8, scale_layout="plain")   # noqa: E731
    return (lambda: ops.gemm_mxfp4(a_mx, w_mx)), ref


def mlp(args, dev):
    """Llama-7B MLP shapes: one fused launch against the three launches it replaces, on the same operands"""
    K, F = 4096, 11008
    for M in (1, 16, 256, 2048):
        x, wg = operands(M, F, K, dev)
        _, wu = operands(M + 1, F, K, dev)
        a_mx, g_mx, u_mx = ops.reorder_quant_mx(x), ops.quant_weight_mx(wg), ops.quant_weight_mx(wu)
        gu_mx = ops.fuse_gate_up_mx(g_mx, u_mx)
        fused = lambda: ops.gate_up_silu_quant_mx(a_mx, gu_mx)                                                          # noqa: E731
        three = lambda: ops.silu_mul_quant_mx(ops.gemm_mxfp4(a_mx, g_mx), ops.gemm_mxfp4(a_mx, u_mx))                   # noqa: E731
        (t_f, s_f), (t_3, s_3), (t_f2, _) = time_graphs([graph_of(fused), graph_of(three), graph_of(fused)], args.reps, args.iters)
        print(json.dumps({"what": "mlp gate/up", "M": M, "F": F, "K": K, "route": ops.gate_up_silu_quant_mx_route(M, F, K),
                          "fused_us": round(t_f, 2), "fused_spread_us": round(s_f, 2), "fused_again_us": round(t_f2, 2),
                          "three_launches_us": round(t_3, 2), "three_spread_us": round(s_3, 2), "ratio": round(t_f / t_3, 3)}))


def act6(args, dev):
    """W4A6 against W4A4 on the same data: the FP6-activation graph alternates with the FP4 one (the FP4 graph twice: its own spread)"""
    def row(what, M, f4, f6, **kw):
        (t4, s4), (t6, s6), (t4b, _) = time_graphs([graph_of(f4), graph_of(f6), graph_of(f4)], args.reps, args.iters)
        print(json.dumps({"what": what, "M": M, **kw, "mxfp4_us": round(t4, 2), "mxfp4_spread_us": round(s4, 2), "mxfp4_again_us": round(t4b, 2),
                          "mxfp6_us": round(t6, 2), "mxfp6_spread_us": round(s6, 2), "ratio": round(t6 / t4, 3)}))
    N = K = 4096
    for M in (4096, 256, 16, 1):
        x, w = operands(M, N, K, dev)
        w_mx, a4, a6 = ops.quant_weight_mx(w), ops.reorder_quant_mx(x), ops.reorder_quant_mx(x, act_format="mxfp6")
        row("gemm a6", M, lambda: ops.gemm_mxfp4(a4, w_mx), lambda: ops.gemm_mxfp4(a6, w_mx), N=N, K=K, route=ops.gemm_mxfp4_route(M, N, K))
        gu_mx = ops.fuse_gate_up_mx(w_mx, ops.quant_weight_mx(operands(M + 1, N, K, dev)[1]))
        row("gate/up a6", M, lambda: ops.gate_up_silu_quant_mx(a4, gu_mx), lambda: ops.gate_up_silu_quant_mx(a6, gu_mx, out_format="mxfp6"), F=N, K=K)
    x, _ = operands(2048, 64, 4096, dev)
    idx = torch.randperm(4096, device=dev).to(torch.int16)
    row("quantiser a6", 2048, lambda: ops.reorder_quant_mx(x, idx), lambda: ops.reorder_quant_mx(x, idx, act_format="mxfp6"), K=4096)


def weight6(args, dev):
    """MXFP6 weights against MXFP4 ones on the same data, per activation format: W6A4 against W4A4, W6A6 against W4A6 (the MXFP4-weight
    graph twice: its own spread)"""
    def row(what, M, f4, f6, **kw):
        (t4, s4), (t6, s6), (t4b, _) = time_graphs([graph_of(f4), graph_of(f6), graph_of(f4)], args.reps, args.iters)
        print(json.dumps({"what": what, "M": M, **kw, "w4_us": round(t4, 2), "w4_spread_us": round(s4, 2), "w4_again_us": round(t4b, 2),
                          "w6_us": round(t6, 2), "w6_spread_us": round(s6, 2), "ratio": round(t6 / t4, 3)}))
    N = K = 4096
    for M in (4096, 256, 16, 1):
        x, w = operands(M, N, K, dev)
        wu = operands(M + 1, N, K, dev)[1]
        w4, w6 = ops.quant_weight_mx(w), ops.quant_weight_mx(w, weight_format="mxfp6")
        gu4 = ops.fuse_gate_up_mx(w4, ops.quant_weight_mx(wu))
        gu6 = ops.fuse_gate_up_mx(w6, ops.quant_weight_mx(wu, weight_format="mxfp6"), weight_format="mxfp6")
        for act in ("mxfp4", "mxfp6"):
            a = ops.reorder_quant_mx(x, act_format=act)
            row("gemm w6", M, lambda: ops.gemm_mxfp4(a, w4), lambda: ops.gemm_mxfp4(a, w6), act=act, N=N, K=K, route=ops.gemm_mxfp4_route(M, N, K))
            row("gate/up w6", M, lambda: ops.gate_up_silu_quant_mx(a, gu4, out_format=act), lambda: ops.gate_up_silu_quant_mx(a, gu6, out_format=act),
                act=act, F=N, K=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--act", choices=["mxfp4", "mxfp6"], default="mxfp4")
    ap.add_argument("--weight", choices=["mxfp4", "mxfp6"], default="mxfp4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    if args.weight == "mxfp6":
        return weight6(args, dev)
    if args.act == "mxfp6":
        return act6(args, dev)
    if args.mlp:
        return mlp(args, dev)
    for M, N, K in [(4096, 4096, 4096), (1, 4096, 4096), (16, 4096, 4096), (256, 4096, 4096)]:
        mx, ref = gemm_pair(M, N, K, dev)
        # the same MX graph twice: the spread of two runs of the same binary beside the difference
        (t_mx, s_mx), (t_ref, s_ref), (t_mx2, _) = time_graphs([graph_of(mx), graph_of(ref), graph_of(mx)], args.reps, args.iters)
        print(json.dumps({"what": "gemm", "M": M, "N": N, "K": K, "route": ops.gemm_mxfp4_route(M, N, K), "mx_us": round(t_mx, 2),
                          "mx_spread_us": round(s_mx, 2), "mx_again_us": round(t_mx2, 2), "shipped_us": round(t_ref, 2),
                          "shipped_spread_us": round(s_ref, 2), "mx_tflops": round(2.0 * M * N * K / t_mx * 1e-6, 1)}))
    x, _ = operands(2048, 64, 4096, dev)
    idx = torch.randperm(4096, device=dev).to(torch.int16)
    (t_mx, s_mx), (t_ref, s_ref) = time_graphs([graph_of(lambda: ops.reorder_quant_mx(x, idx)),
                                                graph_of(lambda: ops.reorder_fp16_i4(x, idx, scale_layout="plain"))], args.reps, args.iters)
    print(json.dumps({"what": "quantiser", "M": 2048, "K": 4096, "mx_us": round(t_mx, 2), "mx_spread_us": round(s_mx, 2),
                      "reorder_fp16_i4_us": round(t_ref, 2), "shipped_spread_us": round(s_ref, 2)}))


if __name__ == "__main__":
    main()
