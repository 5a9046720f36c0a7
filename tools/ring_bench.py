"""Rolling KV cache of a sliding-window model: what the ring costs and what it saves.

    python tools/ring_bench.py [--iters K] [--warmup W] [--only step|decode|generate]   (on the GPU box)

step      ops.kv_step_ring_i4 against ops.kv_step_i4 on the same batch and row width: a rebuild (add = 0) of tables that list the
          same number of pages per sequence -- a static cache of W tokens, a rolling cache of 8 W tokens with window W.
decode    atom_batch_decode_gqa_i4_ring against atom_batch_decode_gqa_i4_win at context 32,768, W = 4096, pages of 16, 32 / 8 heads,
          batch 1 / 16 / 64.  Both ops read the SAME pool bytes: the _win op through the full page list, the _ring op through the list
          of the last ceil(W / 16) + 1 pages with kv_start in front of them.  Timed in alternation, twice each: the two figures of an op
          are the spread that the comparison is read against.
generate  tokens generated per pool page: generate(rolling_kv=True) against the default on a tiny windowed Llama (W = 4096), one
          prompt of 128 tokens, 8192 new tokens; the pages are the most the pool ever had out (counted in KvPoolInt4.alloc_block).
One JSON line at the end."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atom_amd import ops  # noqa: E402
from atom_amd.utils import KvCacheInt4, KvPoolInt4, RollingKvCacheInt4, StaticBatchedKvCacheInt4  # noqa: E402
from atom_amd.utils.kvcache import BatchedKvCacheInt4  # noqa: E402

NQ, NKV, BLOCK, WINDOW, CTX = 32, 8, 16, 4096, 32768
DEV = torch.device("cuda")


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


def step(iters, warmup):
    out = []
    R = -(-WINDOW // BLOCK) + 1
    for batch in (1, 16, 64, 256):
        pool = KvPoolInt4(1, 1, 128, batch * (R + 8 * WINDOW // BLOCK) + 2, BLOCK, DEV)
        static = StaticBatchedKvCacheInt4([KvCacheInt4(pool, WINDOW) for _ in range(batch)], reserve=BLOCK)      # R pages per row
        rolling = RollingKvCacheInt4([KvCacheInt4(pool, 8 * WINDOW) for _ in range(batch)], WINDOW)
        assert static.max_pages == rolling.max_pages == R
        r = {"batch": batch, "row_pages": R}
        for rnd in (1, 2):
            r[f"static_us_{rnd}"] = _time(lambda: static.step(0), iters, warmup)
            r[f"ring_us_{rnd}"] = _time(lambda: rolling.step(0), iters, warmup)
        static.close()
        rolling.close()
        print(f"STEP    b{batch:<4d} rows of {R}: kv_step_i4 {r['static_us_1']:7.2f} / {r['static_us_2']:7.2f} us   "
              f"kv_step_ring_i4 {r['ring_us_1']:7.2f} / {r['ring_us_2']:7.2f} us", flush=True)
        out.append(r)
    return out


def decode(iters, warmup):
    out = []
    pages = CTX // BLOCK
    R = -(-WINDOW // BLOCK) + 1
    for batch in (1, 16, 64):
        pool = KvPoolInt4(1, NKV, 128, batch * pages + 1, BLOCK, DEV)
        pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device=DEV, dtype=torch.uint8))
        pool.param.copy_((torch.rand(pool.param.shape, device=DEV) * 0.2 + 0.01).half())
        full = BatchedKvCacheInt4([KvCacheInt4(pool, CTX) for _ in range(batch)])
        f = (CTX - WINDOW) // BLOCK                           # first live page of a decode step at this length
        cnt = pages - f
        lists = full.indicies.view(batch, pages)[:, f:].contiguous()
        ring = types.SimpleNamespace(data=full.data, param=full.param, indicies=lists.view(-1), last_page_offset=full.last_page_offset,
                                     indptr=torch.arange(batch + 1, dtype=torch.int32, device=DEV) * cnt, max_pages=R, window=WINDOW,
                                     kv_start=torch.full((batch,), f * BLOCK, dtype=torch.int32, device=DEV))
        q = torch.randn((batch, NQ, 128), device=DEV).half()
        r = {"batch": batch, "ctx": CTX, "window": WINDOW, "splits_win": ops.decode_splits(batch, full, NQ, window=WINDOW),
             "splits_ring": ops.decode_splits(batch, ring, NQ, window=WINDOW)}
        r["bit_identical"] = bool(torch.equal(ops.batch_decode_i4(q, full, 0, window=WINDOW), ops.batch_decode_i4(q, ring, 0, window=WINDOW)))
        for rnd in (1, 2):
            r[f"win_us_{rnd}"] = _time(lambda: ops.batch_decode_i4(q, full, 0, window=WINDOW), iters, warmup)
            r[f"ring_us_{rnd}"] = _time(lambda: ops.batch_decode_i4(q, ring, 0, window=WINDOW), iters, warmup)
        r["ring_over_win"] = (r["ring_us_1"] + r["ring_us_2"]) / (r["win_us_1"] + r["win_us_2"])
        print(f"DECODE  b{batch:<3d} ctx {CTX} W {WINDOW}: _win {r['win_us_1']:8.1f} / {r['win_us_2']:8.1f} us (splits {r['splits_win']})   "
              f"_ring {r['ring_us_1']:8.1f} / {r['ring_us_2']:8.1f} us (splits {r['splits_ring']})   ring / win {r['ring_over_win']:.3f}   "
              f"bit-identical {r['bit_identical']}", flush=True)
        out.append(r)
        del pool, full, ring
    return out


def generate(new=8192, prompt=128):
    import time
    from atom_amd.e2e import LlamaForCausalLM, generate as gen
    cfg = types.SimpleNamespace(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=1408, rms_norm_eps=1e-5,
                                rope_theta=1e4, num_hidden_layers=2, vocab_size=1000, pad_token_id=None, sliding_window=WINDOW)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).cuda()
    g = torch.Generator().manual_seed(100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
    prompts = [torch.randint(0, 1000, (prompt,), generator=g).tolist()]
    out = {"new_tokens": new, "prompt": prompt, "window": WINDOW, "page": BLOCK}
    tokens = {}
    for name, rolling in (("default", False), ("rolling", True)):
        pool = KvPoolInt4(2, 2, 128, -(-(prompt + new) // BLOCK) + 2, BLOCK, DEV)
        capacity, low, alloc = pool.num_free_blocks, [pool.num_free_blocks], pool.alloc_block

        def counted():
            idx = alloc()
            low[0] = min(low[0], pool.num_free_blocks)
            return idx
        pool.alloc_block = counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tokens[name] = gen(model, prompts, new, pool, rolling_kv=rolling)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert pool.num_free_blocks == capacity
        peak = capacity - low[0]
        out[name] = {"peak_pages": peak, "tokens_per_page": new / peak, "seconds": dt, "us_per_token": dt / new * 1e6}
        print(f"GENERATE {name:8s}: {new} new tokens on at most {peak} pool pages -> {new / peak:6.1f} tokens per page; "
              f"{dt:.2f} s ({dt / new * 1e6:.0f} us per token)", flush=True)
    out["same_tokens"] = tokens["default"] == tokens["rolling"]
    print(f"GENERATE same tokens: {out['same_tokens']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("step", "decode", "generate"))
    a = ap.parse_args()
    res = {}
    if a.only in (None, "step"):
        res["step"] = step(a.iters, a.warmup)
    if a.only in (None, "decode"):
        res["decode"] = decode(a.iters, a.warmup)
    if a.only in (None, "generate"):
        res["generate"] = generate()
    print(json.dumps({"ring_bench": res}))


if __name__ == "__main__":
    main()
