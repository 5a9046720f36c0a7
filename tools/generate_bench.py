"""Per-token wall time of greedy decoding, two ways, on Llama-7B-width layers (hidden 4096, 32 heads, intermediate 11008):

    eager   the loop a user writes without atom_amd.e2e.generate: acquire_one on every sequence, a new BatchedKvCacheInt4 (three
            host-to-device copies), one forward, argmax -- per token
    replay  atom_amd.e2e.DecodeGraph: the page tables stepped on the device (atom_kv_step_i4) and the whole step replayed from one graph
    sampled the same with a sampler (ops.sample in place of argmax: T = 0.8, top-k 50, top-p 0.95, one seed per sequence)
    pair    replay, sampled and penalised, their repetitions alternating in one process (the fair comparison of the three)
    penalised  sampled with logit penalties in front (ops.penalize: repetition 1.1, presence 0.5, frequency 0.3, 16 bias entries per
            sequence, 5 % of the vocabulary flagged as prompt tokens); pair leaves it out where --tree has no LogitPenalties

    python tools/generate_bench.py [--mode eager|replay|sampled|pair|both] [--batches 1,16] [--ctx 1024] [--steps 64] [--reps 5] [--layers 8]
                                   [--tree DIR]

Every repetition is `steps` tokens timed by the host clock around work that ends in a device synchronise; the context grows from
`ctx` on, the same way in both modes.  One JSON line per (mode, batch) with every repetition's microseconds per token.  `--tree DIR`
imports atom_amd from another checkout (built there), to time the eager loop -- which needs nothing newer -- on another commit.
The page-table step's kernel time comes from a tracer run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/generate_bench.py --mode replay --reps 1   (kernel kv_step_kernel)
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["eager", "replay", "sampled", "pair", "both"], default="both")
ap.add_argument("--batches", default="1,16")
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--vocab", type=int, default=32000)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from atom_amd.e2e import LlamaForCausalLM  # noqa: E402
from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4  # noqa: E402

dev = torch.device("cuda", 0)
WARM = 8                                                      # untimed tokens in front of the first repetition


def build_model():
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


def sequences(batch, total_tokens):
    pages = batch * (-(-(args.ctx + total_tokens) // 16) + 1)
    pool = KvPoolInt4(num_layers=args.layers, num_heads=32, head_dim=128, capacity=pages, block_len=16, device=dev)
    pool.buf.random_(0, 255)
    pool.param.copy_(torch.rand(pool.param.shape, device=dev).mul_(0.05).add_(0.01).half())
    return pool, [KvCacheInt4(pool, args.ctx) for _ in range(batch)]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def eager(model, batch):
    pool, seqs = sequences(batch, WARM + args.reps * args.steps)
    blen = BatchLenInfo([], batch, dev)
    state = {"ids": torch.zeros(batch, dtype=torch.int64, device=dev)}

    def step():
        for c in seqs:
            c.acquire_one()
        logits, _ = model(state["ids"], blen, None, BatchedKvCacheInt4(seqs))
        state["ids"] = logits.argmax(-1)
    timed(step, WARM)
    return [timed(step, args.steps) for _ in range(args.reps)]


def replay_graph(model, batch, sampled, penalised=False):
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    total = WARM + args.reps * args.steps
    pool, seqs = sequences(batch, total)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=total)
    kw = {}
    if sampled:
        from atom_amd.e2e import SamplingParams
        kw["sampler"] = [SamplingParams(0.8, 50, 0.95, seed=b + 1) for b in range(batch)]
    if penalised:
        from atom_amd.e2e import LogitPenalties
        bias = {t * (args.vocab // 16): -1.0 for t in range(16)}
        kw["sampler"] = [SamplingParams(0.8, 50, 0.95, seed=b + 1, repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.3,
                                        logit_bias=bias) for b in range(batch)]
        kw["penalties"] = LogitPenalties(batch, args.vocab, dev, kw["sampler"])
        kw["penalties"].reset([list(range(b, args.vocab, 20)) for b in range(batch)])
    dg = DecodeGraph(model, skv, total, **kw)
    timed(dg.step, WARM)                                      # the eager first step, the capture, six replays
    return dg, skv


def replay(model, batch, sampled=False):
    dg, skv = replay_graph(model, batch, sampled)
    us = [timed(dg.step, args.steps) for _ in range(args.reps)]
    skv.close()
    return us


def pair(model, batch):
    """greedy, sampled and (where the tree has them) penalised replay, one repetition of each in turn"""
    import atom_amd.e2e
    forms = [(False, False), (True, False)] + ([(True, True)] if hasattr(atom_amd.e2e, "LogitPenalties") else [])
    graphs = [replay_graph(model, batch, *form) for form in forms]
    us = tuple([] for _ in graphs)
    for _ in range(args.reps):
        for (dg, _), out in zip(graphs, us):
            out.append(timed(dg.step, args.steps))
    for _, skv in graphs:
        skv.close()
    return us


def main():
    model = build_model()
    modes = ["eager", "replay"] if args.mode == "both" else [args.mode]
    for batch in (int(b) for b in args.batches.split(",")):
        results = []
        for mode in modes:
            with torch.no_grad():
                if mode == "pair":
                    results += list(zip(("replay", "sampled", "penalised"), pair(model, batch)))
                else:
                    results.append((mode, eager(model, batch) if mode == "eager" else replay(model, batch, mode == "sampled")))
        for mode, us in results:
            print(json.dumps({"mode": mode, "batch": batch, "ctx": args.ctx, "layers": args.layers, "steps": args.steps,
                              "us_per_token": [round(u, 1) for u in us], "median": round(sorted(us)[len(us) // 2], 1),
                              "device": torch.cuda.get_device_name(0), "tree": os.path.abspath(args.tree)}), flush=True)


if __name__ == "__main__":
    main()
