"""Bench of the prefill attention over the INT4 paged KV cache (csrc/prefill_i4.hip) against the torch route it replaces, Llama-7B heads
(32 x 128), pages of 16 tokens:  python tools/prefill_bench.py [--iters K] [--warmup W] [--only NAME]   (on the GPU box).

Per shape: ops.batch_prefill_i4, and the torch route timed with events on the same cache --
  * prompts from an empty cache: what LlamaAttention runs today (FP32 de-quantisation of the new tokens, then per request RoPE +
    FP32 scaled_dot_product_attention, causal);
  * chunks on a cached prefix (no torch route exists): the whole sequence de-quantised from the pages, RoPE at every position,
    SDPA with the offset causal mask.
Chunks on long prefixes also time batch_decode_i4 on the same cache (the op should cost at most ~2 of those).  Prints one
PREFILL line per shape and a JSON line with everything."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from atom_amd import ops  # noqa: E402
from atom_amd.e2e.llama import dequant_kv_u4, rope_llama  # noqa: E402
from atom_amd.utils.kvcache import BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4  # noqa: E402

PEAK_F16 = 2.5e15
HEADS, BLOCK = 32, 16
SHAPES = {                      # name: (prefix, q_len) per sequence
    "1x2048": [(0, 2048)],
    "8x512": [(0, 512)] * 8,
    "32x128": [(0, 128)] * 32,
    "256_on_1792": [(1792, 256)],
    "8_on_4000": [(4000, 8)],
}


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


def _torch_empty(q, k, v, ks, vs, qlens):
    """llama.py LlamaAttention.forward's prefill branch (after init_kv_i4)"""
    nh, hd = q.shape[1], q.shape[2]
    kf, vf = dequant_kv_u4(k, ks), dequant_kv_u4(v, vs)
    outs, beg = [], 0
    for n in qlens:
        sl = slice(beg, beg + n)
        pos = torch.arange(n, device=q.device)
        qq = rope_llama(q[sl].float(), pos).transpose(0, 1)
        kk = rope_llama(kf[sl], pos).transpose(0, 1)
        o = torch.nn.functional.scaled_dot_product_attention(qq, kk, vf[sl].transpose(0, 1), is_causal=True)
        outs.append(o.transpose(0, 1).reshape(n, nh * hd).to(q.dtype))
        beg += n
    return torch.cat(outs)


def _torch_prefix(q, kv, qlens, pages, seqlens):
    """the whole sequence de-quantised from its pages, SDPA with the offset causal mask"""
    nh, hd = q.shape[1], q.shape[2]
    outs, beg = [], 0
    for n, pg, S in zip(qlens, pages, seqlens):
        blk = kv.data[pg, 0]                                   # [np, 2, N, P, 64]
        prm = kv.param[pg, 0]
        k = blk[:, 0].permute(0, 2, 1, 3).reshape(-1, nh, hd // 2)[:S]
        v = blk[:, 1].permute(0, 2, 1, 3).reshape(-1, nh, hd // 2)[:S]
        kp = prm[:, 0].permute(0, 2, 1, 3).reshape(-1, nh, 2)[:S]
        vp = prm[:, 1].permute(0, 2, 1, 3).reshape(-1, nh, 2)[:S]
        kf = rope_llama(dequant_kv_u4(k, kp), torch.arange(S, device=q.device)).transpose(0, 1)
        vf = dequant_kv_u4(v, vp).transpose(0, 1)
        qq = rope_llama(q[beg:beg + n].float(), torch.arange(S - n, S, device=q.device)).transpose(0, 1)
        mask = torch.arange(S, device=q.device)[None, :] <= torch.arange(S - n, S, device=q.device)[:, None]
        o = torch.nn.functional.scaled_dot_product_attention(qq, kf, vf, attn_mask=mask)
        outs.append(o.transpose(0, 1).reshape(n, nh * hd).to(q.dtype))
        beg += n
    return torch.cat(outs)


def run(name, seqs, iters, warmup):
    dev = torch.device("cuda")
    seqlens = [a + n for a, n in seqs]
    qlens = [n for _, n in seqs]
    pool = KvPoolInt4(1, HEADS, 128, sum(-(-s // BLOCK) for s in seqlens), BLOCK, dev)
    pool.buf.copy_(torch.randint(0, 256, pool.buf.shape, device=dev, dtype=torch.uint8))
    pool.param.copy_((torch.rand(pool.param.shape, device=dev) * 0.2 + 0.01).half())
    cs = [KvCacheInt4(pool, s) for s in seqlens]
    kv = BatchedKvCacheInt4(cs)
    T = sum(qlens)
    q = torch.randn((T, HEADS, 128), device=dev).half()
    qo = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    mq = max(qlens)
    res = {"shape": name, "seqs": len(seqs), "prefix": seqs[0][0], "q_len": qlens[0], "heads": HEADS, "page": BLOCK}
    res["op_us"] = _time(lambda: ops.batch_prefill_i4(q, qo, kv, 0, max_q_len=mq), iters, warmup)
    flop = sum(4 * 128 * HEADS * sum(a + i + 1 for i in range(n)) for a, n in seqs)
    res["gflop"] = flop / 1e9
    res["peak_fraction"] = flop / (res["op_us"] * 1e-6) / PEAK_F16
    if all(a == 0 for a, _ in seqs):
        # the new tokens' codes as the layer holds them (the cache slots, gathered once outside the timing)
        pages = [torch.tensor(c.indicies, device=dev) for c in cs]
        k = torch.cat([pool.buf[pg, 0, 0].permute(0, 2, 1, 3).reshape(-1, HEADS, 64)[:s] for pg, s in zip(pages, seqlens)])
        v = torch.cat([pool.buf[pg, 0, 1].permute(0, 2, 1, 3).reshape(-1, HEADS, 64)[:s] for pg, s in zip(pages, seqlens)])
        ks = torch.cat([pool.param[pg, 0, 0].permute(0, 2, 1, 3).reshape(-1, HEADS, 2)[:s] for pg, s in zip(pages, seqlens)])
        vs = torch.cat([pool.param[pg, 0, 1].permute(0, 2, 1, 3).reshape(-1, HEADS, 2)[:s] for pg, s in zip(pages, seqlens)])
        res["torch_route"] = "empty-cache route of LlamaAttention"
        res["torch_us"] = _time(lambda: _torch_empty(q, k, v, ks, vs, qlens), max(iters // 4, 3), 2)
    else:
        pages = [torch.tensor(c.indicies, device=dev) for c in cs]
        res["torch_route"] = "whole-sequence dequant + SDPA, offset causal mask"
        res["torch_us"] = _time(lambda: _torch_prefix(q, kv, qlens, pages, seqlens), max(iters // 4, 3), 2)
        if mq <= 16:
            qd = q[qo[1:].long() - 1].contiguous()                  # one query per sequence: a decode step on the same cache
            res["decode_us"] = _time(lambda: ops.batch_decode_i4(qd, kv, 0), iters, warmup)
    res["speedup_vs_torch"] = res["torch_us"] / res["op_us"]
    extra = f"  decode {res['decode_us']:7.1f} us ({res['op_us'] / res['decode_us']:.2f}x)" if "decode_us" in res else ""
    print(f"PREFILL {name:12s} op {res['op_us']:8.1f} us  {res['peak_fraction']:.3f} of f16 peak  torch {res['torch_us']:9.1f} us "
          f"({res['speedup_vs_torch']:.1f}x){extra}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    out = [run(n, s, a.iters, a.warmup) for n, s in SHAPES.items() if a.only in (None, n)]
    print(json.dumps({"prefill_bench": out}))


if __name__ == "__main__":
    main()
