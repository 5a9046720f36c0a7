"""Time of ops.logprob (atom_logprob_f16) by graph replay, hot, against what a user would otherwise write on the device and against
one pass over the rows:

    logprob  ops.logprob(logits, targets, top_n): one launch
    torch    log_softmax(float32) -> gather of the targets' log-probabilities -> topk(top_n) (no rank: the composition does less)
    argmax   torch.argmax over the same rows, the floor for one pass

    python tools/logprob_bench.py [--vocabs 32000,128256] [--rows 1,16,64,2048] [--tops 0,5,20] [--calls 20] [--reps 20]
                                  [--decode] [--batches 1,16] [--layers 8] [--ctx 1024] [--steps 64]

Each is captured `calls` times into one graph; a repetition is one replay between two device events, so a figure is microseconds per
call with no launch gap beyond the graph's own.  The logits are N(0, 3^2) fp16, the same for the three; up to 64 rows they stay in L2
between calls ("hot": in the decode step the lm_head GEMM has just written them).  One JSON line per shape.
--decode times the replayed decode step of tools/generate_bench.py (Llama-7B-width layers) three ways, the repetitions alternating in
one process: greedy, greedy with logprobs=5, and sampled (what ops.sample adds, the yardstick for what ops.logprob may add).
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--rows", default="1,16,64,2048")
ap.add_argument("--tops", default="0,5,20")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--decode", action="store_true")
ap.add_argument("--batches", default="1,16")
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
args = ap.parse_args()
dev = torch.device("cuda", 0)
WARM = 8


def torch_composition(logits, targets, top_n):
    lsm = torch.log_softmax(logits.float(), dim=-1)
    lp = lsm.gather(-1, targets.unsqueeze(-1)).squeeze(-1)
    return (lp,) + (tuple(lsm.topk(top_n, dim=-1)) if top_n else ())


def replayed(fn):
    """median, min, max microseconds per call of fn, captured args.calls times"""
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
    return sorted(us)[len(us) // 2], min(us), max(us)


def op_times():
    for vocab in (int(v) for v in args.vocabs.split(",")):
        for rows in (int(b) for b in args.rows.split(",")):
            g = torch.Generator(device=dev).manual_seed(vocab + rows)
            logits = (torch.randn((rows, vocab), generator=g, device=dev) * 3.0).half()
            targets = torch.randint(0, vocab, (rows,), generator=g, device=dev)
            with torch.no_grad():
                a = replayed(lambda: torch.argmax(logits, dim=-1))
                for top_n in (int(t) for t in args.tops.split(",")):
                    out = ops.logprob(logits, targets, top_n)
                    k = replayed(lambda: ops.logprob(logits, targets, top_n, out=out))
                    t = replayed(lambda: torch_composition(logits, targets, top_n))
                    print(json.dumps({"vocab": vocab, "rows": rows, "top_n": top_n, "calls": args.calls, "reps": args.reps,
                                      "logprob_us": round(k[0], 2), "logprob_min_max": [round(k[1], 2), round(k[2], 2)],
                                      "torch_us": round(t[0], 2), "argmax_us": round(a[0], 2), "torch_over_logprob": round(t[0] / k[0], 2),
                                      "logprob_over_argmax": round(k[0] / a[0], 2), "row_GBps": round(vocab * 2 / k[0] / 1e3, 2),
                                      "total_GBps": round(rows * vocab * 2 / k[0] / 1e3, 2), "device": torch.cuda.get_device_name(0)}),
                          flush=True)


def decode_times():
    from atom_amd.e2e import DecodeGraph, LlamaForCausalLM, SamplingParams
    from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4
    for vocab in (int(v) for v in args.vocabs.split(",")):
        cfg = types.SimpleNamespace(hidden_size=4096, num_attention_heads=32, intermediate_size=11008, rms_norm_eps=1e-5, rope_theta=1e4,
                                    num_hidden_layers=args.layers, vocab_size=vocab, pad_token_id=None)
        torch.manual_seed(0)
        model = LlamaForCausalLM(cfg).to(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        for mod in model.modules():
            if type(mod).__name__ == "LinearInt4":
                mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g, device=dev) * 0.05).half())
            elif type(mod).__name__ == "LlamaRMSNormInt4":
                mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g, device=dev)).half()

        def timed(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6

        for batch in (int(b) for b in args.batches.split(",")):
            total = WARM + args.reps * args.steps
            graphs = []
            with torch.no_grad():
                for kw in ({}, {"logprobs": 5}, {"sampler": [SamplingParams(0.8, 50, 0.95, seed=b + 1) for b in range(batch)]}):
                    pages = batch * (-(-(args.ctx + total) // 16) + 1)
                    pool = KvPoolInt4(num_layers=args.layers, num_heads=32, head_dim=128, capacity=pages, block_len=16, device=dev)
                    pool.buf.random_(0, 255)
                    pool.param.copy_(torch.rand(pool.param.shape, device=dev).mul_(0.05).add_(0.01).half())
                    skv = StaticBatchedKvCacheInt4([KvCacheInt4(pool, args.ctx) for _ in range(batch)], reserve=total)
                    dg = DecodeGraph(model, skv, total, **kw)
                    timed(dg.step, WARM)
                    graphs.append((dg, skv))
                us = ([], [], [])
                for _ in range(args.reps):
                    for (dg, _), out in zip(graphs, us):
                        out.append(timed(dg.step, args.steps))
                for _, skv in graphs:
                    skv.close()
            med = [sorted(u)[len(u) // 2] for u in us]
            print(json.dumps({"decode": True, "vocab": vocab, "batch": batch, "ctx": args.ctx, "layers": args.layers, "steps": args.steps,
                              "greedy_us": [round(u, 1) for u in us[0]], "logprobs5_us": [round(u, 1) for u in us[1]],
                              "sampled_us": [round(u, 1) for u in us[2]], "medians": [round(m, 1) for m in med],
                              "logprobs5_adds_us": round(med[1] - med[0], 1), "sample_adds_us": round(med[2] - med[0], 1),
                              "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    decode_times() if args.decode else op_times()
