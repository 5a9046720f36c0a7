"""Time of ops.sample (atom_sample_f16) by graph replay, hot, against the launch it replaces and against a sampler written in torch:

    sample  ops.sample: temperature 0.8, top-k 50, top-p 0.95 (or --plain: T = 1, both cuts off), a seed per row, the step read from a
            device counter -- one launch
    argmax  torch.argmax over the same rows (what the greedy decode step does)
    torch   sort -> softmax -> cumsum -> top-k / top-p mask -> multinomial -> gather, the usual torch sampler, on the same rows

    python tools/sample_bench.py [--vocabs 32000,128256] [--batches 1,16,64] [--calls 50] [--reps 20] [--plain]

Each of the three is captured `calls` times into one graph; a repetition is one replay between two device events, so a figure is
microseconds per call with no launch gap beyond the graph's own.  The logits are N(0, 3^2) fp16, the same for the three; they stay
in L2 between calls at these sizes ("hot": in the decode step the lm_head GEMM has just written them).  One JSON line per shape with
the medians, the ratios, and the bytes of logits a call reads over its time -- per row (one workgroup owns a row) and in all.
The per-token cost inside a decode step is tools/generate_bench.py --mode pair.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--batches", default="1,16,64")
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--plain", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
T, K, P = (1.0, 0, 1.0) if args.plain else (0.8, 50, 0.95)


def torch_sampler(logits):
    vals, idx = torch.sort(logits.float() / T, dim=-1, descending=True)
    probs = torch.softmax(vals, dim=-1)
    cum = probs.cumsum(-1)
    drop = (cum - probs) >= P                                  # tokens in front already hold P: the shortest prefix reaching it stays
    if K > 0:
        drop[:, K:] = True
    probs = probs.masked_fill(drop, 0.0)
    return idx.gather(-1, torch.multinomial(probs, 1)).squeeze(-1)


def replayed(fn):
    """median microseconds per call of fn, captured args.calls times"""
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


def main():
    for vocab in (int(v) for v in args.vocabs.split(",")):
        for batch in (int(b) for b in args.batches.split(",")):
            g = torch.Generator(device=dev).manual_seed(vocab + batch)
            logits = (torch.randn((batch, vocab), generator=g, device=dev) * 3.0).half()
            temp = torch.full((batch,), T, dtype=torch.float32, device=dev)
            top_k = torch.full((batch,), K, dtype=torch.int32, device=dev)
            top_p = torch.full((batch,), P, dtype=torch.float32, device=dev)
            seeds = torch.arange(1, batch + 1, dtype=torch.int64, device=dev)
            step = torch.zeros(1, dtype=torch.int64, device=dev)
            out = torch.empty(batch, dtype=torch.int64, device=dev)
            with torch.no_grad():
                s = replayed(lambda: ops.sample(logits, temp, top_k, top_p, seeds, step=step, step_offset=1, out=out))
                a = replayed(lambda: torch.argmax(logits, dim=-1))
                t = replayed(lambda: torch_sampler(logits))
            row_bytes = vocab * 2
            print(json.dumps({"vocab": vocab, "batch": batch, "T": T, "top_k": K, "top_p": P, "calls": args.calls, "reps": args.reps,
                              "sample_us": round(s[0], 2), "sample_min_max": [round(s[1], 2), round(s[2], 2)],
                              "argmax_us": round(a[0], 2), "torch_sampler_us": round(t[0], 2),
                              "sample_over_argmax": round(s[0] / a[0], 2), "torch_over_sample": round(t[0] / s[0], 2),
                              "row_GBps": round(row_bytes / s[0] / 1e3, 2), "total_GBps": round(batch * row_bytes / s[0] / 1e3, 2),
                              "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
