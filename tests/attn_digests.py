"""Output digests of the INT4 paged-KV attention ops, one small case per host path (plan -> launch -> merge): decode in one launch,
decode split and merged by each decode_merge_kernel instantiation, the waves-of-one-workgroup decode, merge=False, the append inside
the launch, prefill and grouped-query prefill / decode split and unsplit, and every split case again through the C ABI with a workspace
one byte short (the unsplit fall-back).  Inputs are seeded on the CPU and copied over; no op uses atomics, so the bytes are a function
of the inputs and of the plan alone.  tests/test_gpu_attn_digests.py compares against tests/golden/attn_digests.json, recorded on the
GPU at the commit BEFORE the host paths were folded into one:

    python -m tests.attn_digests tests/golden/attn_digests.json

Every case: 128-dimensional heads, pages of 16 tokens, 2 layers (layer 1 is read)."""
import hashlib
import json
import sys
import types

import numpy as np
import torch

P, D, LAYERS, LAYER = 16, 128, 2, 1


def _cache(seqlens, heads, seed):
    """a random cache (codes and (scale, zero) everywhere, also past the ends) with its pages in a scrambled order, and the generator"""
    rng = np.random.default_rng(seed)
    counts = [-(-s // P) for s in seqlens]
    cap = sum(counts) + 3
    shape = (cap, LAYERS, 2, heads, P)
    dev = lambda a: torch.from_numpy(a).cuda()
    kv = types.SimpleNamespace(
        data=dev(rng.integers(0, 256, shape + (D // 2,), dtype=np.uint8)),
        param=dev((rng.random(shape + (2,)) * 0.2 + 0.01).astype(np.float16)),
        indptr=dev(np.cumsum([0] + counts).astype(np.int32)),
        indicies=dev(rng.permutation(cap)[:sum(counts)].astype(np.int32)),
        last_page_offset=dev(np.array([(s - 1) % P + 1 for s in seqlens], dtype=np.int32)),
        max_pages=max(counts))
    return kv, rng


def _q(rng, rows, heads):
    return torch.from_numpy(rng.standard_normal((rows, heads, D)).astype(np.float16)).cuda()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _kv_args(kv):
    return (kv.data.data_ptr(), kv.param.data_ptr(), kv.indptr.data_ptr(), kv.indicies.data_ptr(), kv.last_page_offset.data_ptr())


def _short_ws(nbytes):
    """the workspace the op asked for, declared one byte short: the op must run unsplit"""
    assert nbytes > 0
    return torch.empty(nbytes // 4, dtype=torch.float32, device="cuda"), nbytes - 1


def _decode_short(q, kv, nq=None):
    from atom_amd import _lib as L
    lib = L.lib()
    B, N = q.size(0), kv.data.size(3)
    o = torch.empty_like(q)
    tail = (D, 1e4, 1.0, kv.max_pages)
    if nq is None:
        ws, wsb = _short_ws(lib.atom_batch_decode_i4_workspace_bytes(B, N, P, kv.max_pages))
        st = lib.atom_batch_decode_i4(o.data_ptr(), q.data_ptr(), *_kv_args(kv), B, LAYERS, LAYER, N, P, *tail, ws.data_ptr(), wsb,
                                      L.current_stream(q.device))
    else:
        ws, wsb = _short_ws(lib.atom_batch_decode_gqa_i4_workspace_bytes(B, nq, N, P, kv.max_pages))
        st = lib.atom_batch_decode_gqa_i4(o.data_ptr(), q.data_ptr(), *_kv_args(kv), B, LAYERS, LAYER, nq, N, P, *tail, ws.data_ptr(), wsb,
                                          L.current_stream(q.device))
    L.check(st, "decode with a short workspace")
    return o


def _prefill_short(q, qo, kv, max_q, gqa):
    from atom_amd import _lib as L
    lib = L.lib()
    T, nq, B, N = q.size(0), q.size(1), qo.numel() - 1, kv.data.size(3)
    o = torch.empty_like(q)
    tail = (P, D, 1e4, 1.0, kv.max_pages)
    if not gqa:
        ws, wsb = _short_ws(lib.atom_batch_prefill_i4_workspace_bytes(T, B, N, P, max_q, kv.max_pages))
        st = lib.atom_batch_prefill_i4(o.data_ptr(), q.data_ptr(), qo.data_ptr(), T, max_q, *_kv_args(kv), B, LAYERS, LAYER, N, *tail,
                                       ws.data_ptr(), wsb, L.current_stream(q.device))
    else:
        ws, wsb = _short_ws(lib.atom_batch_prefill_gqa_i4_workspace_bytes(T, B, nq, N, P, max_q, kv.max_pages))
        st = lib.atom_batch_prefill_gqa_i4(o.data_ptr(), q.data_ptr(), qo.data_ptr(), T, max_q, *_kv_args(kv), B, LAYERS, LAYER, nq, N, *tail,
                                           ws.data_ptr(), wsb, L.current_stream(q.device))
    L.check(st, "prefill with a short workspace")
    return o


def split_contexts():
    """pages of a batch-1, 4-head decode whose partial-state count falls in each merge instantiation's range (the first that does), and of
    a 4-on-1 grouped-query decode that is split at all: chosen by the library's own queries"""
    from atom_amd._lib import lib
    found = {}
    for pages in range(1, 200):
        s = lib().atom_batch_decode_i4_splits(1, 4, P, pages)
        for name, lo, hi in (("2_8", 2, 8), ("9_16", 9, 16), ("17_64", 17, 64)):
            if lo <= s <= hi:
                found.setdefault(name, pages)
        if lib().atom_batch_decode_gqa_i4_splits(1, 4, 1, P, pages) >= 2:
            found.setdefault("gqa", pages)
    assert sorted(found) == ["17_64", "2_8", "9_16", "gqa"], found
    return found


def compute():
    """{case: sha256 of the output bytes}, in a fixed order"""
    from atom_amd import ops
    from atom_amd._lib import lib
    L = lib()
    ctx = split_contexts()
    out = {}

    kv, rng = _cache([5, 37], 4, 1)
    assert ops.decode_splits(2, kv) == 1
    out["decode_unsplit"] = _sha(ops.batch_decode_i4(_q(rng, 2, 4), kv, LAYER))

    for i, name in enumerate(("2_8", "9_16", "17_64")):
        kv, rng = _cache([ctx[name] * P - 3], 4, 10 + i)
        q = _q(rng, 1, 4)
        lo, hi = (int(x) for x in name.split("_"))
        assert lo <= ops.decode_splits(1, kv) <= hi
        out[f"decode_split_{name}"] = _sha(ops.batch_decode_i4(q, kv, LAYER))
        out[f"decode_split_{name}_short_ws"] = _sha(_decode_short(q, kv))
        if name == "2_8":
            part = ops.batch_decode_i4(q, kv, LAYER, merge=False)
            assert part.shape == (1, 4, ops.decode_splits(1, kv), 130)
            out["decode_split_2_8_unmerged"] = _sha(part)
            k32, v32 = (torch.from_numpy(rng.standard_normal((1, 4 * D)).astype(np.float32)).cuda() for _ in range(2))
            o = ops.batch_decode_i4(q, kv, LAYER, append_kv=(k32, v32))              # (last: it writes the cache)
            out["decode_split_2_8_append"] = _sha(o, kv.data, kv.param)

    # 8 waves per pair in workgroups of four: 2 partial states per pair
    kv, rng = _cache([32 * P], 4, 20)
    assert kv.max_pages == 32 and L.atom_batch_decode_i4_splits(1, 4, P, 32) == 2
    q = _q(rng, 1, 4)
    out["decode_inner"] = _sha(ops.batch_decode_i4(q, kv, LAYER))
    out["decode_inner_short_ws"] = _sha(_decode_short(q, kv))

    # 16 tiles in 4 splits that are waves of one workgroup (4 divides 12, 256 pairs): one launch, the workspace unused.  The query
    # cannot know `o` and reports the 4 partial states a call WITHOUT `o` leaves (merge=False: the route through the workspace)
    kv, rng = _cache([256] * 8, 32, 30)
    assert L.atom_batch_decode_i4_splits(8, 32, P, 16) == 4 and L.atom_batch_decode_i4_workspace_bytes(8, 32, P, 16) == 8 * 32 * 4 * 130 * 4
    q = _q(rng, 8, 32)
    out["decode_wgm"] = _sha(ops.batch_decode_i4(q, kv, LAYER))
    out["decode_wgm_unmerged"] = _sha(ops.batch_decode_i4(q, kv, LAYER, merge=False))

    for gqa, heads, nq in ((False, 4, 4), (True, 1, 4)):
        tag = "prefill_gqa" if gqa else "prefill"
        ws_bytes = (lambda T, B, mq, mp: L.atom_batch_prefill_gqa_i4_workspace_bytes(T, B, nq, heads, P, mq, mp) if gqa
                    else L.atom_batch_prefill_i4_workspace_bytes(T, B, heads, P, mq, mp))
        kv, rng = _cache([17, 23], heads, 40 + gqa)
        qo = torch.tensor([0, 17, 20], dtype=torch.int32).cuda()
        assert ws_bytes(20, 2, 17, kv.max_pages) == 0
        out[f"{tag}_unsplit"] = _sha(ops.batch_prefill_i4(_q(rng, 20, nq), qo, kv, LAYER, max_q_len=17))
        kv, rng = _cache([2008], heads, 50 + gqa)
        qo = torch.tensor([0, 8], dtype=torch.int32).cuda()
        q = _q(rng, 8, nq)
        assert ws_bytes(8, 1, 8, kv.max_pages) > 0
        out[f"{tag}_split"] = _sha(ops.batch_prefill_i4(q, qo, kv, LAYER, max_q_len=8))
        out[f"{tag}_split_short_ws"] = _sha(_prefill_short(q, qo, kv, 8, gqa))

    kv, rng = _cache([ctx["gqa"] * P - 5], 1, 60)
    q = _q(rng, 1, 4)
    assert ops.decode_splits(1, kv, 4) >= 2
    out["decode_gqa_split"] = _sha(ops.batch_decode_i4(q, kv, LAYER))
    part = ops.batch_decode_i4(q, kv, LAYER, merge=False)
    assert part.shape == (1, 4, ops.decode_splits(1, kv, 4), 130)
    out["decode_gqa_split_unmerged"] = _sha(part)
    out["decode_gqa_split_short_ws"] = _sha(_decode_short(q, kv, nq=4))
    kv, rng = _cache([20], 1, 61)
    assert ops.decode_splits(1, kv, 4) == 1
    out["decode_gqa_unsplit"] = _sha(ops.batch_decode_i4(_q(rng, 1, 4), kv, LAYER))
    torch.cuda.synchronize()
    return {"contexts": ctx, "sha256": out}


if __name__ == "__main__":
    res = compute()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
