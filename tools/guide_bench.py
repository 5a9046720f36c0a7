"""What guided decoding costs, hot:

    kernels  ops.guide_mask at every vocabulary and batch, beside ops.penalize on the same shape (non-neutral rows with state: it moves
             more bytes per element), a plain device copy of the rows and the torch formulation torch.where(bool_mask[state], logits,
             -inf); ops.guide_advance beside a one-element torch kernel standing for an empty launch.  20 calls per graph, device events
             around a replay, the forms alternating; the whole set is taken twice for the run-to-run spread
    step     the replayed DecodeGraph step with and without a guide on Llama-7B-width layers (hidden 4096, 32 heads, intermediate
             11008; the layer stack and the pool of tools/spec_bench.py), context 1024, their repetitions alternating in one process

    python tools/guide_bench.py [--part kernels|step|all] [--batches 1,16,64] [--vocabs 32000,128256] [--step-batches 1,16] [--ctx 1024]
                                [--steps 64] [--reps 5] [--layers 8] [--forms plain,guided]

`step` times with the host clock around work that ends in a device synchronise.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["kernels", "step", "all"], default="all")
ap.add_argument("--batches", default="1,16,64")
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--step-batches", default="1,16")
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--vocab", type=int, default=32000, help="the step part's vocabulary")
ap.add_argument("--states", type=int, default=64, help="mask rows of the kernels part")
ap.add_argument("--forms", default="plain,guided", help="the step part's graphs (one of them alone: for a kernel trace of that form)")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.e2e import DecodeGraph, LlamaForCausalLM, LogitGuide, TokenAutomaton  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4  # noqa: E402

dev = torch.device("cuda", 0)
WARM = 8                                                      # untimed steps in front of the first repetition


def emit(**kw):
    print(json.dumps(dict(kw, device=torch.cuda.get_device_name(0))), flush=True)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def graph_of(fn, calls=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, calls=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(forms, replays=10):
    """{name: (median, min, max) microseconds per call}: every form captured 20 times into a graph of its own, the replays in turn"""
    graphs = {name: graph_of(fn) for name, fn in forms.items()}
    out = {name: [] for name in forms}
    for _ in range(replays):
        for name, g in graphs.items():
            out[name].append(replay_us(g))
    return {name: (round(median(v), 2), round(min(v), 2), round(max(v), 2)) for name, v in out.items()}


def part_kernels():
    S = args.states
    for vocab in (int(v) for v in args.vocabs.split(",")):
        g = torch.Generator(device=dev).manual_seed(5)
        words = -(-(-(-vocab // 32)) // 4) * 4
        mask = torch.randint(-2 ** 31, 2 ** 31, (S, words), device=dev, generator=g, dtype=torch.int64).to(torch.int32)   # half the tokens
        bool_mask = ((mask.view(S, words, 1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).bool().view(S, words * 32)[:, :vocab].contiguous()
        # advance: every state has the even tokens as its edges, each leading to the next state
        indptr = torch.arange(S + 1, device=dev, dtype=torch.int32) * (vocab // 2)
        edge_tok = (torch.arange(vocab // 2, device=dev, dtype=torch.int32) * 2).repeat(S)
        edge_next = ((torch.arange(S, device=dev, dtype=torch.int32) + 1) % S).repeat_interleave(vocab // 2)
        neg_inf = torch.tensor(float("-inf"), dtype=torch.float16, device=dev)
        for batch in (int(b) for b in args.batches.split(",")):
            logits = torch.randn((batch, vocab), device=dev, generator=g).half()
            out = torch.empty_like(logits)
            state = torch.randint(0, S, (batch,), device=dev, generator=g, dtype=torch.int32)
            state64 = state.to(torch.int64)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            pen_state = torch.zeros((batch, -(-vocab // 8) * 8), dtype=torch.int16, device=dev)
            pen_state[:, ::3] = 2
            fed = torch.randint(0, vocab, (batch,), device=dev, generator=g)
            rep = torch.full((batch,), 1.3, dtype=torch.float32, device=dev)
            tokens = torch.randint(0, vocab // 2, (batch,), device=dev, generator=g) * 2
            one = torch.zeros(1, device=dev)
            work = logits.clone()
            forms = {
                "guide_mask": lambda: ops.guide_mask(logits, state, mask, out=out, status=status),
                "guide_mask_in_place": lambda: ops.guide_mask(work, state, mask, out=work, status=status),
                "penalize": lambda: ops.penalize(logits, pen_state, fed, rep, out=out),
                "copy": lambda: out.copy_(logits),
                "torch_where": lambda: torch.where(bool_mask[state64], logits, neg_inf),
                "guide_advance": lambda: ops.guide_advance(state, tokens, indptr, edge_tok, edge_next, status=status),
                "one_element_kernel": lambda: one.add_(0),
            }
            want = torch.where(bool_mask[state64], logits, neg_inf)
            same = bool(torch.equal(ops.guide_mask(logits, state, mask).view(torch.int16), want.view(torch.int16)))
            for take in (0, 1):                               # the same measurement again: the run-to-run spread
                state.copy_(state64.to(torch.int32))          # (the captured advance moves the states: start each take alike)
                res = alternate(forms)
                # bytes the mask needs: the row read and written, one mask bit per element
                need = batch * vocab * (2 + 2) + batch * vocab // 8
                emit(part="kernels", vocab=vocab, batch=batch, take=take, us_median_min_max=res, mask_equals_torch_where=same,
                     mask_bytes=need, mask_gb_per_s=round(need / res["guide_mask"][0] / 1e3, 1),
                     penalize_bytes=batch * vocab * 6, status=int(status.item()))


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


def sequences(batch, reserve):
    """a pool whose first ctx tokens per sequence are random, the same on every call (seeded), and its sequences"""
    pages = batch * (-(-(args.ctx + reserve) // 16) + 1)
    pool = KvPoolInt4(num_layers=args.layers, num_heads=32, head_dim=128, capacity=pages, block_len=16, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    pool.buf.random_(0, 255, generator=g)
    pool.param.copy_(torch.rand(pool.param.shape, device=dev, generator=g).mul_(0.05).add_(0.01).half())
    return pool, [KvCacheInt4(pool, args.ctx) for _ in range(batch)]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def part_step(model):
    """the guide: two states, the even tokens lead from 0 to 1 and the odd ones back -- half the vocabulary allowed at every step, and a
    run that never leaves the language"""
    v = np.arange(args.vocab)
    auto = TokenAutomaton(2, np.stack([v % 2, v, 1 - v % 2], axis=1).tolist(), 0, args.vocab)
    total = WARM + args.reps * args.steps
    for batch in (int(b) for b in args.step_batches.split(",")):
        graphs, caches = {}, []
        for form in args.forms.split(","):
            pool, seqs = sequences(batch, total)
            skv = StaticBatchedKvCacheInt4(seqs, reserve=total)
            guide = LogitGuide(batch, args.vocab, dev, auto) if form == "guided" else None
            graphs[form] = DecodeGraph(model, skv, total, guide=guide)
            graphs[form].input_ids.fill_(4)
            caches.append((skv, guide))
            status = guide
            timed(graphs[form].step, WARM)
        us = {form: [] for form in graphs}
        for _ in range(args.reps):                            # one repetition of each in turn
            for form, dg in graphs.items():
                us[form].append(timed(dg.step, args.steps))
        med = {form: round(median(v), 1) for form, v in us.items()}
        emit(part="step", batch=batch, ctx=args.ctx, layers=args.layers, vocab=args.vocab, steps=args.steps,
             us_per_step={form: [round(u, 1) for u in v] for form, v in us.items()}, median=med,
             overhead_us=round(med["guided"] - med["plain"], 1) if len(med) == 2 else None,
             status=None if status is None else status.status_bits())
        for skv, _ in caches:
            skv.close()


def main():
    with torch.no_grad():
        if args.part in ("kernels", "all"):
            part_kernels()
        if args.part in ("step", "all"):
            part_step(build_model())


if __name__ == "__main__":
    main()
