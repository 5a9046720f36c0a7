"""What the host side of the INT4 paged-KV attention ops answers without a GPU: the plan queries (workspace bytes, split counts) over a
fixed grid, and the error code of calls that are rejected before any launch -- single faults, and double faults that pin the ORDER of
the argument checks.  tests/test_attn_host_tables_cpu.py compares the library against tests/golden/attn_host_tables.json, recorded at
the commit BEFORE the host paths were folded into one:

    python -m tests.attn_host_tables tests/golden/attn_host_tables.json

The calls of the matrix run on host memory: every one must come back before the library would launch (the generator refuses to record a
call that returns ATOM_OK or ATOM_ERR_LAUNCH)."""
import ctypes
import itertools
import json
import sys

BATCH = (1, 2, 8, 16, 64, 200, 300)
KV_HEADS = (1, 4, 8, 32)
GROUP = (1, 2, 4, 7)
PAGE = (16, 32, 48)
MAX_PAGES = (0, 1, 2, 6, 16, 64, 125, 256, 300, 8192)
PREFILL = ((1, 1), (5, 1), (8, 8), (100, 60), (2048, 2048), (64, 4096))       # (total_q, max_q_len)


def plan_tables(L):
    """the six queries over the grid, each table a flat list in the order of its loops"""
    t = {"decode": [], "prefill": [], "decode_gqa": [], "prefill_gqa": []}
    for b, n, p, mp in itertools.product(BATCH, KV_HEADS, PAGE, MAX_PAGES):
        t["decode"] += [L.atom_batch_decode_i4_workspace_bytes(b, n, p, mp), L.atom_batch_decode_i4_splits(b, n, p, mp)]
        t["prefill"] += [L.atom_batch_prefill_i4_workspace_bytes(T, b, n, p, mq, mp) for T, mq in PREFILL]
        for g in GROUP:
            t["decode_gqa"] += [L.atom_batch_decode_gqa_i4_workspace_bytes(b, n * g, n, p, mp), L.atom_batch_decode_gqa_i4_splits(b, n * g, n, p, mp)]
            t["prefill_gqa"] += [L.atom_batch_prefill_gqa_i4_workspace_bytes(T, b, n * g, n, p, mq, mp) for T, mq in PREFILL]
    return t


# rejected inputs of the queries: batch 0, heads 0, page size 8, query heads no multiple of the K/V heads, negative head counts
REJECTED = (
    [("atom_batch_decode_i4_workspace_bytes", a) for a in ((0, 4, 16, 64), (1, 0, 16, 64), (1, 4, 8, 64), (1, -4, 16, 64))] +
    [("atom_batch_decode_i4_splits", a) for a in ((0, 4, 16, 64), (1, 0, 16, 64), (1, 4, 8, 64), (1, -4, 16, 64))] +
    [("atom_batch_prefill_i4_workspace_bytes", a) for a in ((8, 0, 4, 16, 8, 256), (8, 1, 0, 16, 8, 256), (8, 1, 4, 8, 8, 256), (8, 1, -4, 16, 8, 256),
                                                            (0, 1, 4, 16, 8, 256), (8, 1, 4, 16, 0, 256))] +
    [(f, a) for f in ("atom_batch_decode_gqa_i4_workspace_bytes", "atom_batch_decode_gqa_i4_splits")
     for a in ((0, 8, 4, 16, 64), (1, 0, 4, 16, 64), (1, 8, 0, 16, 64), (1, 8, 4, 8, 64), (1, 6, 4, 16, 64), (1, -8, 4, 16, 64), (1, 8, -4, 16, 64),
               (1, -8, -4, 16, 64), (0, 4, 4, 16, 64), (1, 4, 4, 8, 64))] +
    [("atom_batch_prefill_gqa_i4_workspace_bytes", a) for a in ((8, 0, 8, 4, 16, 8, 256), (8, 1, 0, 4, 16, 8, 256), (8, 1, 8, 0, 16, 8, 256),
                                                                (8, 1, 8, 4, 8, 8, 256), (8, 1, 6, 4, 16, 8, 256), (8, 1, -8, 4, 16, 8, 256),
                                                                (8, 1, 8, -4, 16, 8, 256), (0, 1, 8, 4, 16, 8, 256), (8, 1, 8, 4, 16, 0, 256),
                                                                (8, 0, 4, 4, 16, 8, 256), (8, 1, 4, 4, 8, 8, 256))])

# ---- the error-code matrix.  A call = an entry point, and what it changes in that entry point's valid argument list below.  Pointer
# arguments are "mem" (a 64-byte-aligned host buffer), "+n" (n bytes into it) or "null"; "nan" is the float.
_KV = [("kv_data", "mem"), ("kv_param", "mem"), ("kv_indptr", "mem"), ("kv_indices", "mem"), ("last_page_offset", "mem")]
_DIMS = [("batch", 2), ("num_layers", 2), ("layer_idx", 1)]
_ROPE = [("rope_theta", 1e4), ("rope_scale", 1.0), ("max_pages_per_seq", 0), ("workspace", "null"), ("workspace_bytes", 0), ("stream", "null")]
_MHA = _DIMS + [("num_heads", 4), ("page_size", 16), ("head_dim", 128)]
_GQA = _DIMS + [("num_qo_heads", 8), ("num_kv_heads", 4), ("page_size", 16), ("head_dim", 128)]
VALID = {
    "atom_kv_append_i4": _KV + [("k", "mem"), ("v", "mem"), ("k_param", "mem"), ("v_param", "mem"), ("append_indptr", "mem"), ("total_tokens", 3)] +
                         _MHA + [("stream", "null")],
    "atom_kv_quant_append_f32": _KV + [("k_f32", "mem"), ("v_f32", "mem")] + _MHA + [("stream", "null")],
    "atom_batch_decode_i4": [("o", "mem"), ("q", "mem")] + _KV + _MHA + _ROPE,
    "atom_batch_decode_append_i4": [("o", "mem"), ("q", "mem"), ("k_f32", "mem"), ("v_f32", "mem")] + _KV + _MHA + _ROPE,
    "atom_batch_prefill_i4": [("o", "mem"), ("q", "mem"), ("qo_indptr", "mem"), ("total_q", 3), ("max_q_len", 2)] + _KV + _MHA + _ROPE,
    "atom_batch_decode_gqa_i4": [("o", "mem"), ("q", "mem")] + _KV + _GQA + _ROPE,
    "atom_batch_prefill_gqa_i4": [("o", "mem"), ("q", "mem"), ("qo_indptr", "mem"), ("total_q", 3), ("max_q_len", 2)] + _KV + _GQA + _ROPE,
}
_ALIGN4 = ("kv_param", "qo_indptr", "k_param", "v_param")      # pointers the library wants 4-byte aligned; the other checked ones 16


def matrix():
    """[(entry point, {argument: value})]: every call carries at least one fault"""
    calls = []
    for fn, valid in VALID.items():
        names = [n for n, _ in valid]
        gqa, prefill = "num_kv_heads" in names, "total_q" in names
        decode = "rope_theta" in names and not prefill
        ptrs = [n for n, v in valid if v == "mem"]
        one = lambda **kw: calls.append((fn, kw))
        for p in ptrs:                                          # (o = null: the un-merged form, refused where the KV range is not split)
            one(**{p: "null"})
        for p in ptrs:
            if p not in ("kv_indptr", "kv_indices", "last_page_offset", "append_indptr"):
                one(**{p: "+2" if p in _ALIGN4 else "+8"})
        one(head_dim=64)
        for layer in (-1, 2):
            one(layer_idx=layer)
        for ps in (8, 24):
            one(page_size=ps)
        for k, v in (("batch", 0), ("num_layers", 0)):
            one(**{k: v})
        if gqa:
            for nq, nkv in ((6, 4), (8, 0), (0, 4), (8, -4), (-8, -4), (-8, 4)):
                one(num_qo_heads=nq, num_kv_heads=nkv)
            one(num_qo_heads=6, kv_data="null")                                 # the ratio is checked before any pointer
            one(num_qo_heads=6, kv_data="+8", q="null", head_dim=64)
            # G = 1: the MHA entry point's checks in the MHA entry point's order
            one(num_qo_heads=4, q="null")
            one(num_qo_heads=4, o="+8")
            one(num_qo_heads=4, o="+8", kv_param="+2", page_size=24)
            one(num_qo_heads=4, kv_data="null", head_dim=64)
            one(num_qo_heads=4, rope_theta=0.0, q="+8")
            one(num_qo_heads=4, num_kv_heads=4, **({"total_q": 0, "o": "+8"} if prefill else {"o": "null", "q": "+8"}))
        else:
            for n in (0, -4):
                one(num_heads=n)
        one(kv_data="null", head_dim=64)                        # null pointer + bad shape
        one(last_page_offset="null", page_size=8, kv_data="+8")
        one(page_size=24, kv_data="+8")                         # bad shape + misalignment
        one(layer_idx=2, kv_param="+2")
        if "rope_theta" in names:
            for k in ("rope_theta", "rope_scale"):
                for v in (0.0, -1.0, "nan"):
                    one(**{k: v})
            one(q="null", o="+8")
            one(rope_scale="nan", q="+8")
            one(rope_theta=-1.0, kv_data="+8")                  # the cache's alignment is checked with the cache, before the rest
            one(q="null", head_dim=64)
        if decode:
            one(o="null", q="+8")                               # alignment before "un-merged needs a split"
            one(o="null", max_pages_per_seq=64)                 # split by the plan, but no workspace: unsplit, so refused
            one(o="null", max_pages_per_seq=64, workspace="mem", workspace_bytes=64)
            one(o="null", max_pages_per_seq=8192, workspace="+8", workspace_bytes=1 << 30)
        if prefill:
            for k, v in (("total_q", 0), ("total_q", 1 << 31), ("total_q", (1 << 31) + 5), ("max_q_len", 0), ("max_q_len", -3)):
                one(**{k: v})
            one(total_q=0, o="+8")                              # shape before alignment
            one(max_q_len=0, qo_indptr="+2")
            one(total_q=0, q="null")                            # null pointer before shape
            one(total_q=0, rope_theta=0.0)
            one(total_q=(1 << 31) - 1)                          # rows x heads past 2^31: refused behind every other check
            one(total_q=(1 << 31) - 1, o="+8")
            one(total_q=(1 << 31) - 1, max_q_len=1 << 30, batch=64)
        if fn == "atom_batch_decode_gqa_i4":
            one(batch=1 << 30)                                  # the grid past 2^31
            one(batch=1 << 30, q="+8")
            one(batch=1 << 30, o="null")
        if fn == "atom_batch_decode_append_i4":
            one(k_f32="null", kv_data="null", head_dim=64)      # the new token's operands are checked first
            one(k_f32="+8", kv_data="null")
            one(v_f32="+8", k_f32="null")
            one(v_f32="+8", page_size=8)
        if fn == "atom_kv_quant_append_f32":
            one(k_f32="null", kv_data="+8")                     # the cache first, all of it
            one(v_f32="+8", k_f32="null")
            one(k_f32="+8", layer_idx=-1)
        if fn == "atom_kv_append_i4":
            for tt in (0, -1, 1 << 31):
                one(total_tokens=tt)
            one(append_indptr="null", total_tokens=3)           # one token per sequence needs total_tokens == batch
            one(append_indptr="null", total_tokens=3, k="+8")
            one(k="null", total_tokens=0)
            one(total_tokens=0, k="+8")
            one(v_param="+2", k_param="null")
            one(k="null", kv_param="+2")
    return calls


_mem = ctypes.create_string_buffer((1 << 16) + 64)
_base = (ctypes.addressof(_mem) + 63) & ~63


def _value(v):
    if v == "mem":
        return _base
    if v == "null":
        return None
    if v == "nan":
        return float("nan")
    if isinstance(v, str):
        return _base + int(v)
    return v


def call(L, fn, changes):
    names = [n for n, _ in VALID[fn]]
    assert changes and set(changes) <= set(names), (fn, changes)
    return getattr(L, fn)(*(_value(changes.get(n, v)) for n, v in VALID[fn]))


def record(L):
    from atom_amd import _lib
    errors = []
    for fn, changes in matrix():
        st = call(L, fn, changes)
        assert st in (_lib.ERR_INVALID_ARG, _lib.ERR_SHAPE, _lib.ERR_ALIGN), f"{fn} {changes}: status {st} -- not rejected before the launch"
        errors.append([fn, changes, st])
    return {"plan": plan_tables(L), "rejected": [[f, list(a), getattr(L, f)(*a)] for f, a in REJECTED], "errors": errors}


if __name__ == "__main__":
    from atom_amd._lib import lib
    res = record(lib())
    with open(sys.argv[1], "w") as f:
        f.write("{\n")
        f.write(',\n'.join(f' "plan.{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in res["plan"].items()))
        for key in ("rejected", "errors"):
            f.write(f',\n "{key}": [\n' + ",\n".join("  " + json.dumps(e) for e in res[key]) + "\n ]")
        f.write("\n}\n")
    print({k: len(v) for k, v in res["plan"].items()}, len(res["rejected"]), "rejected queries,", len(res["errors"]), "rejected calls")
