"""Bench of grouped-query attention (GQA) over the INT4 paged KV cache (atom_batch_decode_gqa_i4 / atom_batch_prefill_gqa_i4,
csrc/prefill_i4.hip), 32 query heads on 8 K/V heads, pages of 16 tokens, warm caches:
    python tools/gqa_bench.py [--iters K] [--warmup W] [--only decode|prefill|layer|NAME] [--rope-table [--theta-only] | --window W]   (on the GPU box)

Per shape, on the same box in one run:
  gqa        the GQA op: 32 query heads on the 8-head cache
  mha_kv     the MHA op on a cache of 8 heads (8 query heads: the same KV bytes)
  mha_rep    the MHA op on the cache replicated to 32 heads (the only way to run a GQA model before the GQA ops)
and a Llama-3-8B-shaped decode layer (hidden 4096, 32 / 8 heads, intermediate 14336) at context 1024: one decode step per batch size.
Prints one line per shape and a JSON line with everything.

--rope-table: instead, the Llama-3.1-8B shapes (batch 1 at contexts 1,024 / 8,192 / 32,768 / 131,072 and batch 16 up to 32,768; a decode
step and a 512-token chunk at the end of each context) with the THETA path (rope_theta = 5e5) and the TABLE path (the Llama 3.1
frequency table, ops.rope_table) of the same op in one run, each timed twice in alternation (the two figures of a path show the
run-to-run difference).  --theta-only skips the table path: the same figures from a build that has none.

--window W: instead, sliding-window attention (atom_batch_decode_gqa_i4_win / atom_batch_prefill_gqa_i4_win).  Per batch 1 / 16 / 64
the windowed decode op at contexts 4 W and 8 W against the un-windowed op of the same build at context W (the same keys staged) and at
the full context, and the windowed prefill of 1 x 2 W against the un-windowed one; every figure timed twice in alternation (the two
figures of the un-windowed op at context W are the spread the comparison is read against)."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.utils import BatchLenInfo  # noqa: E402
from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4  # noqa: E402

NQ, NKV, BLOCK = 32, 8, 16
G = NQ // NKV
DECODE = {f"decode_b{b}_c{c}": (b, c) for c in (1024, 4096) for b in (1, 16, 64)}
PREFILL = {"1x2048": [(0, 2048)], "8x512": [(0, 512)] * 8, "8_on_4000": [(4000, 8)]}
LAYER = {f"layer_b{b}_c1024": b for b in (1, 16, 64)}


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _caches(seqlens, heads=NKV, layers=1):
    """a random cache of `heads` heads, and the same contents replicated to NQ heads"""
    dev = torch.device("cuda")
    pool = KvPoolInt4(layers, heads, 128, sum(-(-s // BLOCK) for s in seqlens) + 1, BLOCK, dev)
    pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device=dev, dtype=torch.uint8))
    pool.param.copy_((torch.rand(pool.param.shape, device=dev) * 0.2 + 0.01).half())
    kv = BatchedKvCacheInt4([KvCacheInt4(pool, s) for s in seqlens])
    rep = types.SimpleNamespace(data=kv.data.repeat_interleave(G, dim=3).contiguous(), param=kv.param.repeat_interleave(G, dim=3).contiguous(),
                                indptr=kv.indptr, indicies=kv.indicies, last_page_offset=kv.last_page_offset, max_pages=kv.max_pages)
    return pool, kv, rep


def decode(name, batch, ctx, iters, warmup):
    pool, kv, rep = _caches([ctx] * batch)
    q = torch.randn((batch, NQ, 128), device="cuda").half()
    q8 = q[:, :NKV].contiguous()
    r = {"shape": name, "batch": batch, "ctx": ctx, "kv_bytes": batch * ctx * NKV * 136,       # K + V codes and (scale, zero) halves
         "splits_gqa": ops.decode_splits(batch, kv, NQ), "splits_mha_rep": ops.decode_splits(batch, rep)}
    r["gqa_us"] = _time(lambda: ops.batch_decode_i4(q, kv, 0), iters, warmup)
    r["mha_kv_us"] = _time(lambda: ops.batch_decode_i4(q8, kv, 0), iters, warmup)
    r["mha_rep_us"] = _time(lambda: ops.batch_decode_i4(q, rep, 0), iters, warmup)
    r["gqa_over_mha_kv"] = r["gqa_us"] / r["mha_kv_us"]
    r["gqa_over_mha_rep"] = r["gqa_us"] / r["mha_rep_us"]
    print(f"DECODE  {name:18s} gqa {r['gqa_us']:8.1f} us  mha(8 heads) {r['mha_kv_us']:8.1f} us ({r['gqa_over_mha_kv']:.2f}x)  "
          f"mha(replicated 32) {r['mha_rep_us']:8.1f} us ({r['gqa_over_mha_rep']:.2f}x)  splits {r['splits_gqa']}", flush=True)
    return r


def prefill(name, seqs, iters, warmup):
    seqlens = [a + n for a, n in seqs]
    qlens = [n for _, n in seqs]
    pool, kv, rep = _caches(seqlens)
    T, mq = sum(qlens), max(qlens)
    q = torch.randn((T, NQ, 128), device="cuda").half()
    q8 = q[:, :NKV].contiguous()
    qo = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    r = {"shape": name, "seqs": len(seqs), "prefix": seqs[0][0], "q_len": qlens[0]}
    r["gqa_us"] = _time(lambda: ops.batch_prefill_i4(q, qo, kv, 0, max_q_len=mq), iters, warmup)
    r["mha_kv_us"] = _time(lambda: ops.batch_prefill_i4(q8, qo, kv, 0, max_q_len=mq), iters, warmup)
    r["mha_rep_us"] = _time(lambda: ops.batch_prefill_i4(q, qo, rep, 0, max_q_len=mq), iters, warmup)
    r["gqa_over_mha_rep"] = r["gqa_us"] / r["mha_rep_us"]
    print(f"PREFILL {name:18s} gqa {r['gqa_us']:8.1f} us  mha(8 heads) {r['mha_kv_us']:8.1f} us  mha(32 heads) {r['mha_rep_us']:8.1f} us "
          f"({r['gqa_over_mha_rep']:.2f}x)", flush=True)
    return r


def layer(name, batch, iters, warmup):
    from atom_amd.e2e import LlamaDecoderLayer
    cfg = types.SimpleNamespace(hidden_size=4096, num_attention_heads=NQ, num_key_value_heads=NKV, intermediate_size=14336, rms_norm_eps=1e-5,
                                rope_theta=5e5)
    dev = torch.device("cuda")
    lay = LlamaDecoderLayer(cfg, layer_idx=0).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for mod in lay.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, device=dev, generator=g) * 0.02).half())
    pool, kv, _ = _caches([1024] * batch)          # 1024 tokens per sequence, the last one the slot every timed step writes
    x = (torch.randn(batch, 4096, device=dev) * 0.5).half()
    blen = BatchLenInfo([], batch, dev)
    r = {"shape": name, "batch": batch, "ctx": 1024}
    r["layer_us"] = _time(lambda: lay(x, blen, None, kv), iters, warmup)
    print(f"LAYER   {name:18s} Llama-3-8B-shaped decode layer {r['layer_us']:8.1f} us", flush=True)
    return r


ROPE_SHAPES = [(1, c) for c in (1024, 8192, 32768, 131072)] + [(16, c) for c in (1024, 8192, 32768)]
LLAMA31 = dict(rope_parameters=dict(rope_type="llama3", rope_theta=5e5, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                    original_max_position_embeddings=8192))


def rope_table(iters, warmup, theta_only):
    """theta path against table path, per shape: decode and a 512-token chunk"""
    paths = {"theta": dict(rope_theta=5e5)}
    if not theta_only:
        from atom_amd.e2e.rope import rope_init
        paths["table"] = dict(rope_theta=5e5, rope_table=ops.rope_table(rope_init(LLAMA31)[2], "cuda"))
    out = []
    for batch, ctx in ROPE_SHAPES:
        pool, kv, _ = _caches([ctx] * batch)
        q = torch.randn((batch, NQ, 128), device="cuda").half()
        chunk = 512
        qc = torch.randn((batch * chunk, NQ, 128), device="cuda").half()
        qo = torch.arange(batch + 1, dtype=torch.int32, device="cuda") * chunk
        it = max(3, iters // 4) if batch * ctx >= 1 << 18 else iters          # (the long chunks take milliseconds)
        r = {"batch": batch, "ctx": ctx, "splits": ops.decode_splits(batch, kv, NQ)}
        for rnd in (1, 2):
            for name, kw in paths.items():
                r[f"decode_{name}_us_{rnd}"] = _time(lambda: ops.batch_decode_i4(q, kv, 0, **kw), iters, warmup)
                r[f"chunk_{name}_us_{rnd}"] = _time(lambda: ops.batch_prefill_i4(qc, qo, kv, 0, max_q_len=chunk, **kw), it, warmup)
        line = f"ROPE    b{batch:<3d} c{ctx:<7d}"
        for op in ("decode", "chunk"):
            th = [r[f"{op}_theta_us_{i}"] for i in (1, 2)]
            line += f" {op}: theta {th[0]:9.1f} / {th[1]:9.1f} us"
            if not theta_only:
                tb = [r[f"{op}_table_us_{i}"] for i in (1, 2)]
                r[f"{op}_table_over_theta"] = min(tb) / min(th)
                line += f"  table {tb[0]:9.1f} / {tb[1]:9.1f} us ({r[f'{op}_table_over_theta']:.3f}x) "
        print(line, flush=True)
        out.append(r)
        del pool, kv
    return out


def window(W, iters, warmup):
    """windowed decode at 4 W / 8 W against un-windowed at W and at the full context; windowed prefill of 1 x 2 W against un-windowed"""
    out = {"window": W, "decode": [], "prefill": []}
    for batch in (1, 16, 64):
        q = torch.randn((batch, NQ, 128), device="cuda").half()
        pool0, kv0, _ = _caches([W] * batch)
        r = {"batch": batch, "base_ctx": W, "splits_base": ops.decode_splits(batch, kv0, NQ)}
        runs = {"base": (kv0, {})}
        pools = [pool0]
        for ctx in (4 * W, 8 * W):
            pool, kv, _ = _caches([ctx] * batch)
            pools.append(pool)
            runs[f"win_c{ctx}"] = (kv, {"window": W})
            runs[f"full_c{ctx}"] = (kv, {})
            r[f"splits_win_c{ctx}"] = ops.decode_splits(batch, kv, NQ, window=W)
            r[f"splits_full_c{ctx}"] = ops.decode_splits(batch, kv, NQ)
        for rnd in (1, 2):
            for name, (kv, kw) in runs.items():
                r[f"{name}_us_{rnd}"] = _time(lambda: ops.batch_decode_i4(q, kv, 0, **kw), iters, warmup)
        base = [r["base_us_1"], r["base_us_2"]]
        line = f"WINDOW  decode b{batch:<3d} W {W}: un-windowed at ctx {W} {base[0]:8.1f} / {base[1]:8.1f} us (splits {r['splits_base']})"
        for ctx in (4 * W, 8 * W):
            wn, fl = [r[f"win_c{ctx}_us_{i}"] for i in (1, 2)], [r[f"full_c{ctx}_us_{i}"] for i in (1, 2)]
            r[f"win_c{ctx}_over_base"] = min(wn) / min(base)
            r[f"win_c{ctx}_over_full"] = min(wn) / min(fl)
            line += (f" | ctx {ctx}: windowed {wn[0]:8.1f} / {wn[1]:8.1f} us (splits {r[f'splits_win_c{ctx}']}, {r[f'win_c{ctx}_over_base']:.3f}x of base) "
                     f"un-windowed {fl[0]:8.1f} / {fl[1]:8.1f} us")
        print(line, flush=True)
        out["decode"].append(r)
        del pools, runs, kv0
    n = 2 * W
    pool, kv, _ = _caches([n])
    q = torch.randn((n, NQ, 128), device="cuda").half()
    qo = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    r = {"q_len": n}
    it = max(3, iters // 4)
    for rnd in (1, 2):
        r[f"win_us_{rnd}"] = _time(lambda: ops.batch_prefill_i4(q, qo, kv, 0, max_q_len=n, window=W), it, warmup)
        r[f"full_us_{rnd}"] = _time(lambda: ops.batch_prefill_i4(q, qo, kv, 0, max_q_len=n), it, warmup)
    r["win_over_full"] = min(r["win_us_1"], r["win_us_2"]) / min(r["full_us_1"], r["full_us_2"])
    print(f"WINDOW  prefill 1x{n} W {W}: windowed {r['win_us_1']:9.1f} / {r['win_us_2']:9.1f} us  un-windowed {r['full_us_1']:9.1f} / "
          f"{r['full_us_2']:9.1f} us ({r['win_over_full']:.3f}x)", flush=True)
    out["prefill"].append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--rope-table", action="store_true", help="theta path against table path on the Llama-3.1-8B shapes")
    ap.add_argument("--theta-only", action="store_true", help="with --rope-table: the theta path alone")
    ap.add_argument("--window", type=int, default=None, help="sliding-window attention with this window (4096: Mistral-7B-v0.1)")
    a = ap.parse_args()
    if a.window is not None:
        print(json.dumps({"gqa_bench_window": window(a.window, a.iters, a.warmup)}))
        return
    if a.rope_table:
        print(json.dumps({"gqa_bench_rope_table": rope_table(a.iters, a.warmup, a.theta_only)}))
        return

    def want(kind, name):
        return a.only in (None, kind, name)
    out = {"decode": [decode(n, b, c, a.iters, a.warmup) for n, (b, c) in DECODE.items() if want("decode", n)],
           "prefill": [prefill(n, s, a.iters, a.warmup) for n, s in PREFILL.items() if want("prefill", n)],
           "layer": [layer(n, b, a.iters, a.warmup) for n, b in LAYER.items() if want("layer", n)]}
    print(json.dumps({"gqa_bench": out}))


if __name__ == "__main__":
    main()
