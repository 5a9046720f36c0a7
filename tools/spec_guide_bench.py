"""What guided speculative decoding costs and what forced drafts win, on Llama-7B-width layers (hidden 4096, 32 heads,
intermediate 11008; the layer stack and the pool of tools/spec_bench.py), context 1024, hot:

    walk     ops.guide_walk_rows alone for every batch and Q: 20 calls per graph, device events around a replay; a chain automaton
             (every draft forced: Q searches and Q - 1 stores per sequence) and one whose states allow 1000 tokens (Q searches of depth 10)
    mask     ops.guide_mask over batch * Q rows of `vocab` logits into a second buffer, as the verify step calls it, beside batch rows
    step     the replayed guided speculative step against the replayed unguided speculative step AND the replayed guided one-token
             step at the same batch, their repetitions alternating in one process
    forced   tokens per second on a from_sequences guide with ONE long choice (every draft forced and accepted) at K, against the guided
             one-token step on the same guide, and with force_drafts=False under a drafter that is always wrong

    python tools/spec_guide_bench.py [--part walk|mask|step|forced|all] [--batches 1,16] [--qs 3,5,9] [--k 4] [--ctx 1024] [--steps 64]
                                     [--reps 5] [--layers 8]

`step` and `forced` time with the host clock around work that ends in a device synchronise.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["walk", "mask", "step", "forced", "all"], default="all")
ap.add_argument("--batches", default="1,16")
ap.add_argument("--qs", default="3,5,9")
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--vocab", type=int, default=32000)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.e2e import DecodeGraph, LlamaForCausalLM, LogitGuide, SpecDecodeGraph, SpeculativeParams, TokenAutomaton  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4  # noqa: E402

dev = torch.device("cuda", 0)
WARM = 8                                                      # untimed steps in front of the first repetition
BATCHES = [int(b) for b in args.batches.split(",")]


def emit(**kw):
    print(json.dumps(dict(kw, ctx=args.ctx, layers=args.layers, vocab=args.vocab, device=torch.cuda.get_device_name(0))), flush=True)


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
    pages = batch * (-(-(args.ctx + reserve) // 16) + 1)
    pool = KvPoolInt4(num_layers=args.layers, num_heads=32, head_dim=128, capacity=pages, block_len=16, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    pool.buf.random_(0, 255, generator=g)
    pool.param.copy_(torch.rand(pool.param.shape, device=dev, generator=g).mul_(0.05).add_(0.01).half())
    return pool, [KvCacheInt4(pool, args.ctx) for _ in range(batch)]


def prompts(batch):
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, args.vocab, (args.ctx,), generator=g).tolist() for _ in range(batch)]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def median(xs):
    return sorted(xs)[len(xs) // 2]


def graph_us(fn, calls=20, replays=10):
    """microseconds per call of `fn`, captured `calls` times into one graph: (median, min, max) over the replays"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return round(median(out), 2), round(min(out), 2), round(max(out), 2)


class ConstDrafter:
    def __init__(self, token):
        self.token = int(token)

    def propose(self, hist, hist_len, n_out, out):
        out.fill_(self.token)


def wide_automaton():
    """two states that allow 1000 tokens each and lead to each other: never forced, never dead under its own mask"""
    edges = [(0, t, 1) for t in range(1000)] + [(1, t, 0) for t in range(1000, 2000)]
    return TokenAutomaton(2, edges, 0, args.vocab)


def chain_automaton(length=64):
    """one choice of `length` tokens, then EOS for ever: every state allows exactly one token"""
    return TokenAutomaton.from_sequences([list(range(300, 300 + length))], args.vocab - 1, args.vocab)


def part_walk():
    for batch in BATCHES:
        for name, auto, first in (("chain", chain_automaton(), 300), ("wide", wide_automaton(), 5)):
            guide = LogitGuide(batch, args.vocab, dev, auto)
            for Q in (int(q) for q in args.qs.split(",")):
                rows = torch.zeros((batch, Q), dtype=torch.int32, device=dev)
                adds = torch.zeros(batch, dtype=torch.int32, device=dev)
                ids = torch.full((batch, Q), first, dtype=torch.int64, device=dev)
                if name == "wide":                            # a path the automaton takes: 5, 1005, 5, ..
                    ids[:, 1::2] += 1000
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                call = lambda: ops.guide_walk_rows(guide.state, adds, rows, ids, guide.indptr, guide.edge_tok, guide.edge_next, status=status)
                us = graph_us(call)
                emit(part="walk", automaton=name, batch=batch, Q=Q, us_median_min_max=us, last_row_state=int(rows[0, -1]), status=int(status.item()))
        guide = LogitGuide(batch, args.vocab, dev, wide_automaton())
        tokens = torch.full((batch,), 5, dtype=torch.int64, device=dev)
        emit(part="walk", automaton="wide", batch=batch, Q=None, op="guide_advance",
             us_median_min_max=graph_us(lambda: ops.guide_advance(guide.state, tokens, guide.indptr, guide.edge_tok, guide.edge_next)))


def part_mask():
    g = torch.Generator(device=dev).manual_seed(5)
    ld = -(-args.vocab // 8) * 8
    for batch in BATCHES:
        guide = LogitGuide(batch, args.vocab, dev, wide_automaton())
        for Q in [1] + [int(q) for q in args.qs.split(",")]:
            logits = torch.randn((batch * Q, args.vocab), device=dev, generator=g).half()
            out = torch.zeros((batch * Q, ld), dtype=torch.float16, device=dev)[:, :args.vocab]
            state = torch.zeros(batch * Q, dtype=torch.int32, device=dev)
            us = graph_us(lambda: ops.guide_mask(logits, state, guide.mask_bits, out=out, status=guide.status))
            emit(part="mask", batch=batch, Q=Q, rows=batch * Q, us_median_min_max=us, bytes_moved=4 * batch * Q * args.vocab,
                 gb_per_s=round(4 * batch * Q * args.vocab / us[0] / 1e3, 1))


def spec_graph(model, batch, K, max_new, drafter, auto=None, first=5, force=True):
    pool, seqs = sequences(batch, max_new + K)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=max_new + K)
    guide = None if auto is None else LogitGuide(batch, args.vocab, dev, auto)
    sg = SpecDecodeGraph(model, skv, max_new, params=SpeculativeParams(num_draft_tokens=K, guided=auto is not None, force_drafts=force),
                         drafter=drafter, guide=guide)
    sg.start(prompts(batch), torch.full((batch,), first, dtype=torch.int64, device=dev))
    return sg, skv, guide


def plain_graph(model, batch, total, auto, first):
    pool, seqs = sequences(batch, total)
    pkv = StaticBatchedKvCacheInt4(seqs, reserve=total)
    guide = LogitGuide(batch, args.vocab, dev, auto)
    dg = DecodeGraph(model, pkv, total, guide=guide)
    dg.input_ids.fill_(first)
    return dg, pkv, guide


def part_step(model):
    K, total = args.k, WARM + args.reps * args.steps
    wrong = ConstDrafter(args.vocab - 2)
    for batch in BATCHES:
        max_new = total * (K + 1) + 2
        forms = {"guided_one_token": plain_graph(model, batch, total, wide_automaton(), 5),
                 "spec": spec_graph(model, batch, K, max_new, wrong),
                 "spec_guided": spec_graph(model, batch, K, max_new, wrong, wide_automaton())}
        us = {name: [] for name in forms}
        for name, (g, _, _) in forms.items():
            timed(g.step, WARM)
        for _ in range(args.reps):                            # one repetition of each in turn
            for name, (g, _, _) in forms.items():
                us[name].append(timed(g.step, args.steps))
        med = {name: median(v) for name, v in us.items()}
        for name, (g, kv, guide) in forms.items():
            emit(part="step", form=name, batch=batch, K=K, steps=args.steps, us_per_step=[round(u, 1) for u in us[name]],
                 median=round(med[name], 1), over_spec=round(med[name] / med["spec"], 4), over_spec_us=round(med[name] - med["spec"], 1),
                 over_guided_one_token=round(med[name] / med["guided_one_token"], 3),
                 status=None if guide is None else guide.status_bits())
            if name != "guided_one_token":
                g.commit()
            kv.close()


def part_forced(model):
    K, steps = args.k, args.steps
    auto, wrong = chain_automaton(), ConstDrafter(args.vocab - 2)
    for batch in BATCHES:
        dg, pkv, guide = plain_graph(model, batch, WARM + steps, auto, 300)
        timed(dg.step, WARM)
        us = timed(dg.step, steps)
        emit(part="forced", form="guided_one_token", batch=batch, steps=steps, us_per_step=round(us, 1), tokens_per_step=1.0,
             tokens_per_s=round(batch / us * 1e6, 1), tokens_per_s_per_seq=round(1 / us * 1e6, 1), status=guide.status_bits())
        pkv.close()
        for force in (True, False):
            max_new = (steps + WARM) * (K + 1) + 2
            sg, skv, guide = spec_graph(model, batch, K, max_new, wrong, auto, first=300, force=force)
            timed(sg.step, WARM)
            n0, a0 = sg.n_out.tolist(), sg.accepted.tolist()
            us = timed(sg.step, steps)
            n1, a1 = sg.n_out.tolist(), sg.accepted.tolist()
            tokens = sum(n1) - sum(n0)
            emit(part="forced", form="spec_guided", force_drafts=force, batch=batch, K=K, steps=steps, us_per_step=round(us, 1),
                 accepted_per_step=round((sum(a1) - sum(a0)) / (steps * batch), 3), tokens_per_step=round(tokens / (steps * batch), 3),
                 tokens_per_s=round(tokens / (us * steps) * 1e6, 1), tokens_per_s_per_seq=round(tokens / batch / (us * steps) * 1e6, 1),
                 status=guide.status_bits())
            sg.commit()
            skv.close()


def main():
    with torch.no_grad():
        if args.part in ("walk", "all"):
            part_walk()
        if args.part in ("mask", "all"):
            part_mask()
        if args.part in ("step", "forced", "all"):
            model = build_model()
            if args.part in ("step", "all"):
                part_step(model)
            if args.part in ("forced", "all"):
                part_forced(model)


if __name__ == "__main__":
    main()
