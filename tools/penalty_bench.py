"""Time of ops.penalize (atom_penalize_f16) by graph replay, hot, against a plain copy of the same rows and against the penalties
written in torch:

    penalize  ops.penalize: repetition 1.1, presence 0.5, frequency 0.3 on every row, 5 % of the tokens seen (half of them prompt
              tokens, half generated 1 .. 4 times), 16 bias entries per row, one token per row counted -- one launch
    nobias    the same without the bias table (the build without the LDS stage)
    neutral   the same launch with neutral parameters and no bias: every row copied, one state word per row touched
    copy      out.copy_(logits) on the same rows
    torch     the gather / scatter formulation on the same rows: scatter_add of the fed token into an int32 count table, gather of the
              seen tokens' logits, where(> 0, / rep, * rep), scatter back, minus frequency * counts and presence * (counts > 0),
              scatter_add of the bias

    python tools/penalty_bench.py [--vocabs 32000,128256] [--batches 1,16,64] [--calls 50] [--reps 20]

Each form is captured `calls` times into one graph; a repetition is one replay between two device events, so a figure is microseconds
per call with no launch gap beyond the graph's own.  The logits are N(0, 3^2) fp16; they stay in L2 between calls at these sizes
("hot": in the decode step the lm_head GEMM has just written them).  The count of the fed token saturates at 32767 long before the
replays end, which costs nothing: the saturated owner skips one 2-byte store.  One JSON line per shape with the medians, the ratios, and
the bytes a call moves (logits read + state read + out written = 6 bytes per element) over its time.
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
args = ap.parse_args()
dev = torch.device("cuda", 0)
REP, PRES, FREQ, SEEN, NBIAS = 1.1, 0.5, 0.3, 0.05, 16


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


def torch_penalties(logits, counts, prompt, fed, bias_ids, bias_vals, out):
    counts.scatter_add_(1, fed.unsqueeze(1), torch.ones_like(fed, dtype=torch.int32).unsqueeze(1))
    x = logits.float()
    seen = (counts > 0) | prompt
    x = torch.where(seen, torch.where(x > 0, x / REP, x * REP), x)
    x = x - FREQ * counts.float() - PRES * (counts > 0).float()
    x.scatter_add_(1, bias_ids, bias_vals)
    out.copy_(x)


def main():
    for vocab in (int(v) for v in args.vocabs.split(",")):
        for batch in (int(b) for b in args.batches.split(",")):
            g = torch.Generator(device=dev).manual_seed(vocab + batch)
            logits = (torch.randn((batch, vocab), generator=g, device=dev) * 3.0).half()
            pick = torch.rand((batch, vocab), generator=g, device=dev)
            prompt = pick < SEEN / 2
            counts = torch.where((pick >= SEEN / 2) & (pick < SEEN), torch.randint(1, 5, (batch, vocab), generator=g, device=dev), 0).int()
            ld = -(-vocab // 8) * 8
            state = torch.zeros((batch, ld), dtype=torch.int16, device=dev)
            state[:, :vocab] = (counts + prompt.int() * -32768).to(torch.int16)
            fed = torch.randint(0, vocab, (batch,), generator=g, device=dev)
            f32 = lambda v: torch.full((batch,), v, dtype=torch.float32, device=dev)
            rep, pres, freq = f32(REP), f32(PRES), f32(FREQ)
            one, zero = f32(1.0), f32(0.0)
            bias_ids = torch.stack([torch.randperm(vocab, generator=g, device=dev)[:NBIAS] for _ in range(batch)])
            bias_vals = torch.randn((batch, NBIAS), generator=g, device=dev)
            ids32 = bias_ids.int()
            out = torch.empty((batch, vocab), dtype=torch.float16, device=dev)
            with torch.no_grad():
                p = replayed(lambda: ops.penalize(logits, state, fed, rep, pres, freq, ids32, bias_vals, out=out))
                nb = replayed(lambda: ops.penalize(logits, state, fed, rep, pres, freq, out=out))
                ne = replayed(lambda: ops.penalize(logits, state, fed, one, zero, zero, out=out))
                c = replayed(lambda: out.copy_(logits))
                t = replayed(lambda: torch_penalties(logits, counts, prompt, fed, bias_ids, bias_vals, out))
            moved = batch * vocab * 6
            print(json.dumps({"vocab": vocab, "batch": batch, "seen": SEEN, "bias": NBIAS, "calls": args.calls, "reps": args.reps,
                              "penalize_us": round(p[0], 2), "penalize_min_max": [round(p[1], 2), round(p[2], 2)],
                              "nobias_us": round(nb[0], 2), "neutral_us": round(ne[0], 2), "copy_us": round(c[0], 2),
                              "torch_us": round(t[0], 2), "penalize_over_copy": round(p[0] / c[0], 2),
                              "torch_over_penalize": round(t[0] / p[0], 2), "GBps": round(moved / p[0] / 1e3, 1),
                              "workgroups": batch * -(-vocab // ops.PENALTY_TILE), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
