"""Times of the LoRA ops and of a decoder layer with adapters (profiles/lora/README.md), Llama-7B widths, rank 16.

  ops    add_lora 4096 -> 16 -> 4096 at 1 / 16 / 64 one-row segments with distinct adapters, against torch on the same GPU (adapters
         gathered per row + two torch.bmm), and at 4 segments x 512 rows against two F.linear per segment
  layer  one LlamaDecoderLayerWithLora (hidden 4096, 32 heads, intermediate 11008) at batch 1 and 16, context 1024, with q_proj / v_proj
         adapters against the same layer after set_adapters(None)

Method: every case is captured in a HIP graph of REPS back-to-back calls (the launch overhead of the eager call is not the subject;
the op allocates its rank-wide intermediate inside the capture like any caller's step would); a timed sample is one replay between
two events divided by REPS; WARM untimed replays, then SAMPLES samples; REPLAYS replays per sample, the samples of the two sides of a
comparison alternating; the median and the min .. max range are printed, plus one JSON
line per case.  The ops read the same operands every call, i.e. these are warm (L2 / MALL resident where they fit) numbers.
usage: python tools/lora_bench.py [ops|layer|all] [--out FILE]"""
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, SAMPLES, REPLAYS = 20, 5, 30, 10
DEV = torch.device("cuda")


def timed(fn, reps=REPS):
    return timed_alt({"x": fn}, reps)["x"]


def timed_alt(fns, reps=REPS):
    """{name: median / min / max microseconds per call}: every function captured as a graph of ``reps`` calls; a sample is REPLAYS
    replays between two events; the samples of the functions ALTERNATE, so a drift of the machine hits all of them alike"""
    graphs = {}
    for name, fn in fns.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(reps):
                fn()
        for _ in range(WARM):
            graphs[name].replay()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(SAMPLES):
        for name, graph in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPLAYS):
                graph.replay()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / (reps * REPLAYS))
    return {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for name, v in out.items()}


def report(results, name, ours, ref=None, **extra):
    r = {"case": name, "ours": ours, **extra}
    if ref is not None:
        r["torch"] = ref
        r["ratio_torch_over_ours"] = round(ref["median_us"] / ours["median_us"], 2)
    results.append(r)
    print(json.dumps(r), flush=True)


def bench_ops(results):
    from atom_amd import ops
    h1, h2, r, cap, layers, layer = 4096, 4096, 16, 64, 2, 1
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: (torch.randn(s, device="cuda", generator=g) * 0.05).half()
    wa, wb = rn(cap, layers, r, h1), rn(cap, layers, h2, r)
    for rows in (1, 16, 64):
        x, y = rn(rows, h1), rn(rows, h2)
        ids = torch.arange(rows, dtype=torch.int32, device="cuda")                         # distinct adapters
        idl = ids.long()

        def ours():
            ops.add_lora(y, x, wa, wb, ids, layer, 1.0)

        def ref():
            a, b = wa[idl, layer], wb[idl, layer]                                             # gather [rows, r, h1], [rows, h2, r]
            t = torch.bmm(x.unsqueeze(1), a.transpose(1, 2))
            y.add_(torch.bmm(t, b.transpose(1, 2)).squeeze(1))

        t = timed_alt({"ours": ours, "torch": ref})
        report(results, f"add_lora {rows} one-row segments", t["ours"], t["torch"], rows=rows, h1=h1, h2=h2, rank=r)
    seg, nseg = 512, 4
    rows = seg * nseg
    x, y = rn(rows, h1), rn(rows, h2)
    ids = torch.arange(nseg, dtype=torch.int32, device="cuda")
    ptr = torch.arange(0, rows + 1, seg, dtype=torch.int32, device="cuda")

    def ours():
        ops.add_lora(y, x, wa, wb, ids, layer, 1.0, seg_indptr=ptr)

    def ref():
        for s in range(nseg):
            sl = slice(s * seg, (s + 1) * seg)
            y[sl].add_(torch.nn.functional.linear(torch.nn.functional.linear(x[sl], wa[s, layer]), wb[s, layer]))

    bytes_min = rows * h1 * 2 + 2 * rows * h2 * 2                                             # x once, y read and written
    tt = timed_alt({"ours": ours, "torch": ref}, reps=5)
    o = tt["ours"]
    report(results, f"add_lora {nseg} segments x {seg} rows", o, tt["torch"], rows=rows, h1=h1, h2=h2, rank=r,
           min_bytes=bytes_min, ours_gbps_of_min_bytes=round(bytes_min / o["median_us"] / 1e3, 1))
    t = torch.empty((rows, r), dtype=torch.float16, device="cuda")

    def shrink():
        ops.bgmv(t, x, wa, ids, layer, 1.0, seg_indptr=ptr)

    def expand():
        ops.bgmv(y, t, wb, ids, layer, 1.0, seg_indptr=ptr)

    report(results, "  its shrink pass alone (bgmv, reads x: 16.8 MB)", timed(shrink, reps=5))
    report(results, "  its expand pass alone (bgmv, reads and writes y: 33.6 MB)", timed(expand, reps=5))


def bench_layer(results):
    from atom_amd.e2e import LlamaForCausalLMWithLora
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4
    from atom_amd.utils.lora import LlamaLoraManager
    cfg = types.SimpleNamespace(hidden_size=4096, num_attention_heads=32, intermediate_size=11008, rms_norm_eps=1e-5, rope_theta=1e4,
                                num_hidden_layers=1, vocab_size=64, pad_token_id=None)
    torch.manual_seed(0)
    model = LlamaForCausalLMWithLora(cfg).cuda()
    g = torch.Generator().manual_seed(1)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.02).half().cuda())
    mgr = LlamaLoraManager(cfg, capacity=16, lora_rank=16, device=DEV)
    for a in range(16):
        w = mgr.alloc()
        for m in mgr.target_modules:
            mgr.load(w, 0, m, torch.randn(16, 4096, generator=g) * 0.02, torch.randn(4096, 16, generator=g) * 0.02, alpha=32)
    layer, ctx = model.model.layers[0], 1024
    for batch in (1, 16):
        pool = KvPoolInt4(1, 32, 128, batch * (ctx // 16 + 1) + 1, 16, DEV)
        pool.buf.random_(0, 256)
        pool.param.copy_((torch.rand(pool.param.shape, device="cuda") * 0.2 + 0.01).half())
        seqs = [KvCacheInt4(pool, ctx) for _ in range(batch)]
        kv = BatchedKvCacheInt4(seqs)
        blen = BatchLenInfo([], batch, DEV)
        h = (torch.randn((batch, 4096), device="cuda") * 0.5).half()
        # the three sides share the model's id buffer (a replay reads what it holds THEN), so they are timed one after the other, not
        # alternating; every call re-writes the same last cache slot
        times = {}
        for name, ids in (("base", None), ("lora", list(range(batch))), ("lora_path_no_adapter", [-1] * batch)):
            model.set_adapters(ids, mgr)
            times[name] = timed(lambda: layer(h, blen, None, kv), reps=10)
        model.set_adapters(None)
        report(results, f"decoder layer, decode batch {batch}, context {ctx}: q_proj + v_proj adapters", times["lora"], base=times["base"],
               unfused_path_with_ids_minus_1=times["lora_path_no_adapter"],
               ratio_lora_over_base=round(times["lora"]["median_us"] / times["base"]["median_us"], 2))
        for c in seqs:
            c.release()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "all"
    results = []
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps_per_graph": REPS, "warm_replays": WARM, "samples": SAMPLES}))
    if what in ("ops", "all"):
        bench_ops(results)
    if what in ("layer", "all"):
        bench_layer(results)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
