"""What speculative decoding costs and what it can win, on Llama-7B-width layers (hidden 4096, 32 heads, intermediate 11008; the layer
stack and the pool of tools/generate_bench.py), context 1024, hot:

    step     the replayed SpecDecodeGraph step for every K and batch against the replayed DecodeGraph step at the same batch, their
             repetitions alternating in one process: r = t_spec / t_plain, which is also the break-even mean tokens per step
    forced   tokens per second at 0, K/2 and K accepted drafts per step, forced with a table drafter: a first run records the tokens the
             verify forward chooses, the table repeats them with every (a + 1)-th one corrupted; what was really accepted is reported
    kernels  the three new kernels alone (ops.spec_draft_ngram, ops.spec_accept, ops.kv_step_rows_i4) beside the plain step's fixed
             additions of the same kind (ops.kv_step_i4, argmax): 20 calls per graph, device events around a replay

    python tools/spec_bench.py [--part step|forced|kernels|all] [--batches 1,4,16] [--ks 2,4,8] [--ctx 1024] [--steps 64] [--reps 5] [--layers 8]

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
ap.add_argument("--part", choices=["step", "forced", "kernels", "all"], default="all")
ap.add_argument("--batches", default="1,4,16")
ap.add_argument("--ks", default="2,4,8")
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--vocab", type=int, default=32000)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.e2e import DecodeGraph, LlamaForCausalLM, SpecDecodeGraph, SpeculativeParams  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4  # noqa: E402

dev = torch.device("cuda", 0)
WARM = 8                                                      # untimed steps in front of the first repetition


def emit(**kw):
    print(json.dumps(dict(kw, ctx=args.ctx, layers=args.layers, device=torch.cuda.get_device_name(0))), flush=True)


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


def sequences(batch, reserve, layers=None):
    """a pool whose first ctx tokens per sequence are random, the same on every call (seeded), and its sequences"""
    layers = args.layers if layers is None else layers
    pages = batch * (-(-(args.ctx + reserve) // 16) + 1)
    pool = KvPoolInt4(num_layers=layers, num_heads=32, head_dim=128, capacity=pages, block_len=16, device=dev)
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


class ConstDrafter:
    """K copies of one token: (almost) never accepted"""

    def __init__(self, token):
        self.token = int(token)

    def propose(self, hist, hist_len, n_out, out):
        out.fill_(self.token)


class TableDrafter:
    """drafts from a [batch, max_new + K] table at n_out + j"""

    def __init__(self, table, K):
        self.table, self.cols = table, torch.arange(K, dtype=torch.int64, device=dev).unsqueeze(0)

    def propose(self, hist, hist_len, n_out, out):
        out.copy_(self.table.gather(1, n_out.to(torch.int64).unsqueeze(1) + self.cols))


def spec_graph(model, batch, K, max_new, drafter):
    """a started SpecDecodeGraph with a budget of `max_new` tokens per sequence"""
    pool, seqs = sequences(batch, max_new + K)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=max_new + K)
    sg = SpecDecodeGraph(model, skv, max_new, params=SpeculativeParams(num_draft_tokens=K), drafter=drafter)
    sg.start(prompts(batch), torch.full((batch,), 5, dtype=torch.int64, device=dev))
    return sg, skv


def part_step(model):
    total = WARM + args.reps * args.steps
    for batch in (int(b) for b in args.batches.split(",")):
        pool, seqs = sequences(batch, total)
        pkv = StaticBatchedKvCacheInt4(seqs, reserve=total)
        plain = DecodeGraph(model, pkv, total)
        timed(plain.step, WARM)
        graphs = {}
        for K in (int(k) for k in args.ks.split(",")):
            graphs[K] = spec_graph(model, batch, K, total * (K + 1) + 2, ConstDrafter(args.vocab - 1))   # room for steps that accept everything
            timed(graphs[K][0].step, WARM)
        us = {"plain": []}
        us.update({K: [] for K in graphs})
        for _ in range(args.reps):                            # one repetition of each in turn
            us["plain"].append(timed(plain.step, args.steps))
            for K, (sg, _) in graphs.items():
                us[K].append(timed(sg.step, args.steps))
        emit(part="step", form="plain", batch=batch, steps=args.steps, us_per_step=[round(u, 1) for u in us["plain"]],
             median=round(median(us["plain"]), 1))
        for K, (sg, skv) in graphs.items():
            r = median(us[K]) / median(us["plain"])
            emit(part="step", form="spec", batch=batch, K=K, steps=args.steps, us_per_step=[round(u, 1) for u in us[K]],
                 median=round(median(us[K]), 1), r=round(r, 3), break_even_tokens_per_step=round(r, 3), can_win=bool(r < K + 1),
                 accepted_by_chance=sg.accepted.tolist())
            sg.commit()
            skv.close()
        pkv.close()


def part_forced(model):
    steps = args.steps
    for batch in (int(b) for b in args.batches.split(",")):
        for K in (int(k) for k in args.ks.split(",")):
            # what the verify forward chooses: every token comes from a row that saw the tokens before it, whatever the drafts were
            max_new = (steps + WARM) * (K + 1) + 2            # what steps + WARM steps emit when every draft is accepted
            sg, skv = spec_graph(model, batch, K, max_new, ConstDrafter(args.vocab - 1))
            while sg.steps_done < sg.max_steps:
                sg.step()
            truth = sg.tokens.clone()
            sg.commit()
            skv.close()
            for a in sorted({0, K // 2, K}):
                table = torch.zeros((batch, truth.size(1) + K), dtype=torch.int64, device=dev)
                table[:, :truth.size(1)] = truth
                wrong = (torch.arange(table.size(1), device=dev) - 1) % (a + 1) == a
                table[:, wrong] = (table[:, wrong] + 1) % args.vocab
                sg, skv = spec_graph(model, batch, K, max_new, TableDrafter(table, K))   # the same reserve: the same KV split
                timed(sg.step, WARM)
                n0, a0 = sg.n_out.tolist(), sg.accepted.tolist()
                us = timed(sg.step, steps)
                n1, a1 = sg.n_out.tolist(), sg.accepted.tolist()
                tokens = sum(n1) - sum(n0)
                emit(part="forced", batch=batch, K=K, forced_accepts=a, steps=steps, us_per_step=round(us, 1),
                     accepted_per_step=round((sum(a1) - sum(a0)) / (steps * batch), 3), tokens_per_step=round(tokens / (steps * batch), 3),
                     tokens_per_s=round(tokens / (us * steps) * 1e6, 1), tokens_per_s_per_seq=round(tokens / batch / (us * steps) * 1e6, 1))
                sg.commit()
                skv.close()


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


def part_kernels():
    hist_cap = args.ctx + 1024
    for batch in (int(b) for b in args.batches.split(",")):
        pool, seqs = sequences(batch, 4096, layers=1)
        skv = StaticBatchedKvCacheInt4(seqs, reserve=4096)
        zeros = torch.zeros(batch, dtype=torch.int32, device=dev)
        g = torch.Generator(device=dev).manual_seed(5)
        hist = torch.randint(0, args.vocab, (batch, hist_cap), device=dev, generator=g, dtype=torch.int32)
        hist_len = torch.full((batch,), args.ctx + 300, dtype=torch.int32, device=dev)
        logits = torch.randn((batch, args.vocab), device=dev, generator=g).half()
        res = {"kv_step_i4": graph_us(lambda: ops.kv_step_i4(skv, 0)), "argmax[batch]": graph_us(lambda: logits.argmax(-1))}
        for twice in (0, 1):                                  # the same measurement again: the run-to-run spread
            for K in (int(k) for k in args.ks.split(",")):
                Q = K + 1
                ids = torch.zeros((batch, Q), dtype=torch.int64, device=dev)
                targets = torch.randint(0, args.vocab, (batch, Q), device=dev, generator=g)
                tokens = torch.zeros((batch, 64), dtype=torch.int64, device=dev)
                n_out, steps, accepted = zeros.clone(), zeros.clone(), zeros.clone()
                budget = torch.full((batch,), 2 ** 30, dtype=torch.int32, device=dev)
                hl, adds, done = hist_len.clone(), zeros.clone(), torch.zeros(1, dtype=torch.int32, device=dev)
                draw = torch.zeros(batch, dtype=torch.int64, device=dev)
                wide = torch.randn((batch * Q, args.vocab), device=dev, generator=g).half()
                one = {
                    "spec_draft_ngram": graph_us(lambda: ops.spec_draft_ngram(hist, hist_len, ids[:, 1:], ngram_max=3, ngram_min=1)),
                    "spec_accept": graph_us(lambda: ops.spec_accept(targets, ids, n_out, budget, tokens, hist, hl, adds, draw, accepted, steps, done)),
                    "kv_step_rows_i4": graph_us(lambda: ops.kv_step_rows_i4(skv, zeros, Q)),
                    "argmax[batch*Q]": graph_us(lambda: wide.argmax(-1)),
                    "kv_step_i4": graph_us(lambda: ops.kv_step_i4(skv, 0)), "argmax[batch]": graph_us(lambda: logits.argmax(-1)),
                }
                new3 = sum(one[k][0] for k in ("spec_draft_ngram", "spec_accept", "kv_step_rows_i4"))
                plain2 = one["kv_step_i4"][0] + one["argmax[batch]"][0]
                emit(part="kernels", batch=batch, K=K, take=twice, us_median_min_max=one, new_three_us=round(new3, 2),
                     plain_kv_step_plus_argmax_us=round(plain2, 2), hist_len=args.ctx + 300)
        emit(part="kernels", batch=batch, first=res)
        skv.close()


def main():
    with torch.no_grad():
        if args.part in ("kernels", "all"):
            part_kernels()
        if args.part in ("step", "forced", "all"):
            model = build_model()
            if args.part in ("step", "all"):
                part_step(model)
            if args.part in ("forced", "all"):
                part_forced(model)


if __name__ == "__main__":
    main()
