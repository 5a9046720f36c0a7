"""Times of beam search on Llama-7B dimensions (hidden 4096, 32 heads of 128, pages of 16), context 1024 + 8 tokens so that every row
has a partial page, W beams per prompt:

    fork    ops.kv_beam_fork_i4 by graph replay, `calls` forks per graph: `rotate` (parent b + 1: EVERY row copies its partial page -- the
            worst case), `identity` (no row copies: the table gather and the copy back alone), against `naive`: the fork that copies
            every page of the parent (torch index_select + index_copy_ over rows that own all their pages).  Pool of --fork-layers layers.
    select  ops.beam_select by graph replay, `groups` x W rows with C = W candidates each
    step    the replayed beam step per token (BeamDecodeGraph: kv.step, forward on groups x W rows, ops.logprob, ops.beam_select, fork)
            against the greedy DecodeGraph step at batch groups x W, their repetitions alternating in one process.  Model of --layers layers.

    python tools/beam_bench.py [--part fork|select|step|all] [--beams 2,4,8] [--groups 1] [--ctx 1032] [--layers 8] [--fork-layers 32]
                               [--calls 20] [--reps 10] [--steps 64]

fork / select: a repetition is one replay between two device events, a figure is microseconds per call.  step: `steps` tokens timed by
the host clock around work that ends in a device synchronise.  One JSON line per (part, W).  The fork's bytes are what it must move:
rows that copy x one page of both pool buffers, read and written.  Run each part under a time limit of its own (timeout ... --part X)."""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4, StaticBeamKvCacheInt4  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["fork", "select", "step", "all"], default="all")
ap.add_argument("--beams", default="2,4,8")
ap.add_argument("--groups", type=int, default=1)
ap.add_argument("--ctx", type=int, default=1032)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--fork-layers", type=int, default=32)
ap.add_argument("--vocab", type=int, default=32000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=64)
args = ap.parse_args()
dev = torch.device("cuda", 0)
P, WARM = 16, 8


def replayed(fn):
    """(median, min, max) microseconds per call of fn, captured args.calls times"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.calls):
            fn()
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
    us = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / args.calls)
    return [round(x, 2) for x in (sorted(us)[len(us) // 2], min(us), max(us))]


def pool_of(layers, pages):
    pool = KvPoolInt4(num_layers=layers, num_heads=32, head_dim=128, capacity=pages, block_len=P, device=dev)
    pool.buf.random_(0, 255)
    pool.param.copy_(torch.rand(pool.param.shape, device=dev).mul_(0.05).add_(0.01).half())
    return pool


def beam_cache(layers, W, reserve):
    G, ctx = args.groups, args.ctx
    pages = G * -(-ctx // P) + G * W * (-(-(ctx + reserve) // P) - ctx // P + 1) + 2
    pool = pool_of(layers, pages)
    return pool, StaticBeamKvCacheInt4([KvCacheInt4(pool, ctx) for _ in range(G)], W, reserve)


def part_fork(W):
    G, rows = args.groups, args.groups * W
    pool, skv = beam_cache(args.fork_layers, W, 8)
    rotate = torch.tensor([(b + 1) % W for b in range(W)] * G, dtype=torch.int32, device=dev)
    identity = torch.tensor(list(range(W)) * G, dtype=torch.int32, device=dev)
    rot, idt = replayed(lambda: skv.fork(rotate)), replayed(lambda: skv.fork(identity))
    skv.close()
    page_bytes = pool.buf[0].numel() + pool.param[0].numel() * 2
    # the naive fork: every row owns ceil(ctx / P) pages and receives a copy of all of its parent's
    n = -(-args.ctx // P)
    naive_pool = pool_of(args.fork_layers, rows * n)
    own = torch.arange(rows * n, dtype=torch.int64, device=dev).view(rows, n)
    src = own[torch.tensor([r - r % W + (r % W + 1) % W for r in range(rows)], device=dev)].reshape(-1)
    dst = own.reshape(-1)

    def naive():
        naive_pool.buf.index_copy_(0, dst, naive_pool.buf.index_select(0, src))
        naive_pool.param.index_copy_(0, dst, naive_pool.param.index_select(0, src))
    nv = replayed(naive)
    moved = 2 * rows * page_bytes
    print(json.dumps({"part": "fork", "beams": W, "groups": G, "ctx": args.ctx, "layers": args.fork_layers, "page_bytes": page_bytes,
                      "rotate_us": rot, "identity_us": idt, "naive_us": nv, "fork_bytes": moved,
                      "fork_GBps": round(moved / rot[0] / 1e3, 1), "naive_bytes": moved * n, "naive_GBps": round(moved * n / nv[0] / 1e3, 1),
                      "naive_over_fork": round(nv[0] / rot[0], 1), "calls": args.calls, "reps": args.reps,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def part_select(W):
    rows = args.groups * W
    g = torch.Generator(device=dev).manual_seed(W)
    lp = -torch.rand((rows, W), generator=g, device=dev).mul_(10).sort(dim=1).values
    ids = torch.randint(0, args.vocab, (rows, W), generator=g, device=dev)
    cum = -torch.rand(rows, generator=g, device=dev).mul_(30)
    fin, length = torch.zeros(rows, dtype=torch.int32, device=dev), torch.ones(rows, dtype=torch.int32, device=dev)
    out = tuple(torch.zeros(rows, dtype=d, device=dev) for d in (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32))
    us = replayed(lambda: ops.beam_select(ids, lp, cum, fin, length, None, W, out=out))
    print(json.dumps({"part": "select", "beams": W, "groups": args.groups, "candidates": W, "select_us": us, "calls": args.calls,
                      "reps": args.reps, "device": torch.cuda.get_device_name(0)}), flush=True)


def build_model():
    from atom_amd.e2e import LlamaForCausalLM
    cfg = types.SimpleNamespace(hidden_size=4096, num_attention_heads=32, intermediate_size=11008, rms_norm_eps=1e-5, rope_theta=1e4,
                                num_hidden_layers=args.layers, vocab_size=args.vocab, pad_token_id=None)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g, device=dev) * 0.05).half())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g, device=dev)).half()
    return model


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def part_step(model, W):
    from atom_amd.e2e import BeamDecodeGraph, DecodeGraph
    rows, total = args.groups * W, WARM + args.reps * args.steps
    _, bkv = beam_cache(args.layers, W, total)
    bg = BeamDecodeGraph(model, bkv, total)
    bg.length.fill_(1)
    gpool = pool_of(args.layers, rows * (-(-(args.ctx + total) // P) + 1))
    skv = StaticBatchedKvCacheInt4([KvCacheInt4(gpool, args.ctx) for _ in range(rows)], reserve=total)
    dg = DecodeGraph(model, skv, total)
    timed(bg.step, WARM)                                      # the eager first step, the capture, six replays
    timed(dg.step, WARM)
    beam_us, greedy_us = [], []
    for _ in range(args.reps):
        beam_us.append(timed(bg.step, args.steps))
        greedy_us.append(timed(dg.step, args.steps))
    copied = int((bg.parents != torch.arange(W, device=dev, dtype=torch.int32).repeat(args.groups)).sum())
    bkv.close()
    skv.close()
    med = lambda us: round(sorted(us)[len(us) // 2], 1)
    print(json.dumps({"part": "step", "beams": W, "groups": args.groups, "rows": rows, "ctx": args.ctx, "layers": args.layers,
                      "steps": args.steps, "beam_us_per_token": [round(u, 1) for u in beam_us], "beam_median": med(beam_us),
                      "greedy_us_per_token": [round(u, 1) for u in greedy_us], "greedy_median": med(greedy_us),
                      "beam_minus_greedy_us": round(med(beam_us) - med(greedy_us), 1),
                      "rows_with_another_parent": copied, "row_steps": int(bg.parents.numel()),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    beams = [int(w) for w in args.beams.split(",")]
    with torch.no_grad():
        if args.part in ("fork", "all"):
            for W in beams:
                part_fork(W)
        if args.part in ("select", "all"):
            for W in beams:
                part_select(W)
        if args.part in ("step", "all"):
            model = build_model()
            for W in beams:
                part_step(model, W)


if __name__ == "__main__":
    main()
