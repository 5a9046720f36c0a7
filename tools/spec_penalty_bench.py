"""What penalties under speculative decoding cost, hot, on one GPU:

    rows     ops.penalize_rows over batch sequences of Q verify rows (20 calls per graph, device events around a replay, the replays of the three forms alternating), against
             (1) ops.penalize over the same batch * Q rows with a state row EACH -- less work: no drafts, no commit -- and
             (2) what a user would launch without the op: a copy of the state into a scratch buffer, then Q strided ops.penalize(fed=)
                 calls, call j over row j of every sequence with draft j fed into the scratch (no commit either)
    step     the replayed penalised speculative step against the replayed unpenalised one at the same batch (Llama-7B-width layers:
             hidden 4096, 32 heads, intermediate 11008; the layer stack and pool of tools/spec_bench.py), their repetitions
             alternating in one process, a drafter that is always wrong

    python tools/spec_penalty_bench.py [--part rows|step|all] [--batches 1,4,16] [--qs 3,5,9] [--k 4] [--ctx 1024] [--steps 64] [--reps 5]
                                       [--layers 8] [--vocab 32000] [--big 128256]

`step` times with the host clock around work that ends in a device synchronise.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["rows", "step", "all"], default="all")
ap.add_argument("--batches", default="1,4,16")
ap.add_argument("--step-batches", default="1,16")
ap.add_argument("--qs", default="3,5,9")
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--vocab", type=int, default=32000)
ap.add_argument("--big", type=int, default=128256, help="a second vocabulary, timed at 16 sequences of 5 rows (0: none)")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.e2e import LlamaForCausalLM, LogitPenalties, SamplingParams, SpecDecodeGraph, SpeculativeParams  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, StaticBatchedKvCacheInt4  # noqa: E402

dev = torch.device("cuda", 0)
WARM = 8                                                      # untimed steps in front of the first repetition


def emit(**kw):
    print(json.dumps(dict(kw, device=torch.cuda.get_device_name(0))), flush=True)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def graphs_us(fns, calls=20, replays=10):
    """microseconds per call of every function of `fns`, each captured `calls` times into a graph of its own; the replays of the
    graphs alternate.  {name: (median, min, max) over the replays}"""
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(replays):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {name: (round(median(v), 2), round(min(v), 2), round(max(v), 2)) for name, v in out.items()}


def rows_case(batch, Q, vocab, max_bias):
    g = torch.Generator(device=dev).manual_seed(5)
    ld = -(-vocab // 8) * 8
    logits = torch.randn((batch * Q, vocab), device=dev, generator=g).mul_(3).half()
    out = torch.zeros((batch * Q, ld), dtype=torch.float16, device=dev)[:, :vocab]
    seen = torch.rand((batch, ld), device=dev, generator=g) < 0.05            # 5 % of the vocabulary seen: a context of ~1,600 tokens
    state = torch.where(seen, torch.randint(1, 4, (batch, ld), device=dev, generator=g), 0).to(torch.int16)
    ids = torch.randint(0, vocab, (batch, Q), device=dev, generator=g)
    pending = torch.randint(0, vocab, (batch, Q), device=dev, generator=g)
    counts = torch.full((batch,), Q, dtype=torch.int32, device=dev)
    rep, pres, freq = (torch.full((batch,), v, dtype=torch.float32, device=dev) for v in (1.3, 0.4, 0.7))
    bias = (None, None)
    if max_bias:
        bias = (torch.randint(0, vocab, (batch, max_bias), device=dev, generator=g).to(torch.int32),
                torch.randn((batch, max_bias), device=dev, generator=g))
    # (1) the same rows with a state row each
    state_rows = state.repeat_interleave(Q, 0).contiguous()
    per_row = [t.repeat_interleave(Q).contiguous() for t in (rep, pres, freq)]
    bias_rows = tuple(None if t is None else t.repeat_interleave(Q, 0).contiguous() for t in bias)
    # (2) a scratch copy of the state and Q strided calls: call j takes row j of every sequence and feeds draft j into the scratch
    scratch = torch.zeros((batch, ld), dtype=torch.int16, device=dev)
    l3, o3 = logits.view(batch, Q, vocab), out.view(batch, Q, vocab)
    fed = [ids[:, j].contiguous() for j in range(Q)]

    def rows_op():
        ops.penalize_rows(logits, state, ids, pending, counts, rep, pres, freq, *bias, out=out)

    def per_row_op():
        ops.penalize(logits, state_rows, None, *per_row, *bias_rows, out=out)

    def strided():
        scratch.copy_(state)
        for j in range(Q):
            ops.penalize(l3[:, j], scratch, fed[j] if j else None, rep, pres, freq, *bias, out=o3[:, j])

    forms = graphs_us({"penalize_rows": rows_op, "penalize_same_rows": per_row_op, "copy_and_strided_penalize": strided})
    moved = (4 * Q + 2) * batch * vocab
    for name, us in forms.items():
        emit(part="rows", form=name, batch=batch, Q=Q, vocab=vocab, max_bias=max_bias, us_median_min_max=us,
             over_rows_op=round(us[0] / forms["penalize_rows"][0], 3),
             gb_per_s=round(moved / us[0] / 1e3, 1) if name == "penalize_rows" else None)


def part_rows():
    for batch in (int(b) for b in args.batches.split(",")):
        for Q in (int(q) for q in args.qs.split(",")):
            for max_bias in (0, 16):
                rows_case(batch, Q, args.vocab, max_bias)
    if args.big:
        for max_bias in (0, 16):
            rows_case(16, 5, args.big, max_bias)


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


class ConstDrafter:
    def __init__(self, token):
        self.token = int(token)

    def propose(self, hist, hist_len, n_out, out):
        out.fill_(self.token)


def spec_graph(model, batch, K, max_new, penalised):
    pool, seqs = sequences(batch, max_new + K)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=max_new + K)
    sampling = SamplingParams(temperature=0.8, top_k=50, top_p=0.95, seed=1, repetition_penalty=1.3, presence_penalty=0.4,
                              frequency_penalty=0.7, logit_bias={7: -1.0} if penalised else None)
    pen = None
    if penalised:
        pen = LogitPenalties(batch, args.vocab, dev, sampling)
        pen.reset(prompts(batch))
    sg = SpecDecodeGraph(model, skv, max_new, params=SpeculativeParams(num_draft_tokens=K, penalised=penalised),
                         drafter=ConstDrafter(args.vocab - 2), sampler=sampling, penalties=pen)
    sg.start(prompts(batch), torch.full((batch,), 5, dtype=torch.int64, device=dev))
    return sg, skv


def part_step(model):
    K, total = args.k, WARM + args.reps * args.steps
    for batch in (int(b) for b in args.step_batches.split(",")):
        max_new = total * (K + 1) + 2
        forms = {"spec_sampled": spec_graph(model, batch, K, max_new, False), "spec_sampled_penalised": spec_graph(model, batch, K, max_new, True)}
        us = {name: [] for name in forms}
        for name, (g, _) in forms.items():
            timed(g.step, WARM)
        for _ in range(args.reps):                            # one repetition of each in turn
            for name, (g, _) in forms.items():
                us[name].append(timed(g.step, args.steps))
        med = {name: median(v) for name, v in us.items()}
        for name, (g, kv) in forms.items():
            emit(part="step", form=name, batch=batch, K=K, steps=args.steps, ctx=args.ctx, layers=args.layers, vocab=args.vocab,
                 us_per_step=[round(u, 1) for u in us[name]], median=round(med[name], 1),
                 over_spec=round(med[name] / med["spec_sampled"], 4), over_spec_us=round(med[name] - med["spec_sampled"], 1),
                 paired_us=[round(a - b, 1) for a, b in zip(us[name], us["spec_sampled"])])
            g.commit()
            kv.close()


def main():
    with torch.no_grad():
        if args.part in ("rows", "all"):
            part_rows()
        if args.part in ("step", "all"):
            part_step(build_model())


if __name__ == "__main__":
    main()
