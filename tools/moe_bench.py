"""The sparse mixture-of-experts block at Mixtral-8x7B shapes (hidden 4096, intermediate 14336, 8 experts, top-2) against what a user of
the library could write before the routed kernels existed: the reference's per-expert Python loop (model/qMixtralLayer.py:302-350)
over ops.dense_layer_gemm_i4_fp16 with gathers and index_add_.

    python tools/moe_bench.py [tokens,tokens,...] [--blocks N] [--out FILE]

Per token count (default 1, 16, 64, 2048), us per block:
    new/graph   MixtralSparseMoeInt4.forward captured in a HIP graph and replayed (router matmul + 5 launches, no host work)
    new/eager   the same calls issued from Python, event-timed
    loop/eager  the per-expert loop, event-timed (it reads the routing back on the host once per expert, so it cannot be captured)
each "hot" (one block's weights in every call: what fits stays in the Infinity Cache) and "cold" (cycling through N distinct blocks,
N x 0.69 GB of expert weights, so every call streams its experts from HBM).  Launch counts: calls into libatom_hip.so and torch
operators dispatched per block call.  Also prints the largest difference between the two outputs on the same inputs (the loop's dense
GEMMs may sum the K steps in another order at prefill sizes: include/atom_hip.h, atom_gemm_w4a4_packed_order)."""
import argparse
import os
import sys
import types

import torch
import torch.utils._python_dispatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from atom_amd import _lib as L  # noqa: E402
from atom_amd import ops  # noqa: E402
from atom_amd.e2e import MixtralSparseMoeInt4  # noqa: E402

H, F, E, K = 4096, 14336, 8, 2
dev = torch.device("cuda", 0)


def make_block(seed):
    cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=F, num_local_experts=E, num_experts_per_tok=K)
    moe = MixtralSparseMoeInt4(cfg).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for name, p in moe.named_parameters():
        if p.dtype == torch.uint8:
            p.data.copy_(torch.randint(0, 256, p.shape, device=dev, generator=g, dtype=torch.uint8))
        elif p.dtype == torch.int8:
            p.data.copy_(torch.randint(-128, 128, p.shape, device=dev, generator=g, dtype=torch.int16).to(torch.int8))
        elif "scale" in name:                                  # channel pairs share their int4 scales (weight_channel_group = 2)
            s = torch.rand(p.shape[:-1] + (p.shape[-1] // 2,), device=dev, generator=g) * 0.004 + 0.001
            p.data.copy_(s.repeat_interleave(2, dim=-1).half())
        else:
            p.data.copy_((torch.randn(p.shape, device=dev, generator=g) * 0.1).half())
    # the loop's per-expert operands as tensor objects that live as long as the block: ops tags a weight's scale tensor and keys its
    # cached BF6 form by the tensor, so a fresh view per call would pay a device round trip each time
    names = ("w13_int4", "w13_scale_int4", "w13_int8", "w13_scale_int8", "w2_int4", "w2_scale_int4", "w2_int8", "w2_scale_int8")
    moe.per_expert = [tuple(getattr(moe, n).data[e] for n in names) for e in range(E)]
    return moe


def loop_block(moe, x_q, gate_in, residual):
    """what the parent commit offers: route in torch, then per expert gather -> dense GEMM -> SiLU x up quantiser -> dense GEMM ->
    scale by the routing weight -> index_add_ (plain scale layout, so that a token's scales can be gathered)"""
    o8, o4, s8, s4 = x_q
    p = torch.softmax(torch.nn.functional.linear(gate_in, moe.gate.weight).float(), dim=-1)
    w, ids = torch.topk(p, K, dim=-1)
    w = (w / w.sum(dim=-1, keepdim=True)).half()
    acc = torch.zeros_like(residual)
    for e in range(E):
        t, k = torch.nonzero(ids == e, as_tuple=True)          # host read: the row count sizes the launches
        if t.numel() == 0:
            continue
        b4, sb, b8, sb8, c4, sc, c8, sc8 = moe.per_expert[e]
        gu = ops.dense_layer_gemm_i4_fp16(o4[t], b4, s4[:, t].contiguous(), sb, o8[t], b8, s8[t], sb8, scale_layout="plain")
        a8, a4, t8, t4 = ops.activate_fp16_i4(gu[:, :F].contiguous(), gu[:, F:].contiguous(), scale_layout="plain")
        y = ops.dense_layer_gemm_i4_fp16(a4, c4, t4, sc, a8, c8, t8, sc8, scale_layout="plain")
        acc.index_add_(0, t, y * w[t, k][:, None])
    return residual + acc


class LaunchCount(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def count_launches(fn):
    """(calls into libatom_hip.so, torch operators dispatched) of one call of fn"""
    lib, n = L.lib(), [0]
    saved = {}
    for name in L.SIGNATURES:
        f = getattr(lib, name)
        if f.restype is not L._int or not f.argtypes or f.argtypes[-1] is not L._vp:
            continue                                           # host-side queries take no stream

        def wrap(*a, _f=f):
            n[0] += 1
            return _f(*a)
        saved[name] = f
        setattr(lib, name, wrap)
    try:
        with LaunchCount() as c:
            fn()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    torch.cuda.synchronize()
    return n[0], c.n


def event_time(fns, iters):
    for f in fns:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(3):
        e0.record()
        for i in range(iters):
            fns[i % len(fns)]()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def graph_time(fns, iters):
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fns[i % len(fns)]()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(3):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tokens", nargs="?", default="1,16,64,2048")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    blocks = [make_block(s) for s in range(a.blocks)]
    lines = [f"# sparse MoE block, H {H} F {F} E {E} top-{K}; us per block; cold = cycling through {a.blocks} blocks "
             f"({a.blocks} x {sum(p.numel() * p.element_size() for p in blocks[0].parameters()) / 1e9:.2f} GB)",
             "| tokens | new/graph hot | new/graph cold | new/eager hot | new/eager cold | loop/eager hot | loop/eager cold | launches new (lib + torch) "
             "| launches loop (lib + torch) | active experts | max abs diff |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    for T in (int(v) for v in a.tokens.split(",")):
        g = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn((T, H), device=dev, generator=g)
        x[:, -128:] *= 10
        x = x.half()
        gate_in = torch.randn((T, H), device=dev, generator=g).half()
        residual = torch.randn((T, H), device=dev, generator=g).half()
        xq_ref, xq_plain = ops.reorder_fp16_i4(x, None), ops.reorder_fp16_i4(x, None, scale_layout="plain")
        new = [lambda m=m: m(xq_ref, gate_in, residual) for m in blocks]
        loop = [lambda m=m: loop_block(m, xq_plain, gate_in, residual) for m in blocks]
        iters = max(a.blocks, 16 if T <= 64 else 4)
        iters -= iters % a.blocks
        r = [graph_time(new[:1], iters), graph_time(new, iters), event_time(new[:1], iters), event_time(new, iters),
             event_time(loop[:1], iters), event_time(loop, iters)]
        ln, ll = count_launches(new[0]), count_launches(loop[0])
        active = int((ops.moe_route_topk(torch.nn.functional.linear(gate_in, blocks[0].gate.weight), K).expert_indptr.diff() > 0).sum())
        diff = (new[0]().float() - loop[0]().float()).abs().max().item()
        row = f"| {T} | " + " | ".join(f"{v:.1f}" for v in r) + f" | {ln[0]} + {ln[1]} | {ll[0]} + {ll[1]} | {active} | {diff:.4g} |"
        print(row, flush=True)
        lines.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
