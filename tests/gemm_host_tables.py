"""What the host side of the W4A4 GEMM entry points answers without a GPU: the route and workspace queries over a fixed grid of
shapes, the queries on inputs they reject, and the error code of calls that are refused before any launch -- single faults, and double
faults that pin the ORDER of the argument checks.  tests/test_gemm_host_tables_cpu.py compares the library against
tests/golden/gemm_host_tables.json, recorded at the commit BEFORE the route decision was folded into one function:

    python -m tests.gemm_host_tables tests/golden/gemm_host_tables.json

Small-valued tables are stored one character per value (ALPHABET[index into the table's sorted value list]); the two byte counts are
multiples of 256 on the grid (N is a multiple of 64) and are stored divided by it.  The calls of the matrix run on host memory: every
one must come back before the library would launch (the generator refuses to record a call that returns ATOM_OK or ATOM_ERR_LAUNCH)."""
import ctypes
import itertools
import json
import string
import sys

M_GRID = (1, 2, 3, 7, 8, 16, 17, 32, 33, 64, 65, 128, 129, 200, 256, 257, 300, 512, 513, 768, 1024, 1500, 2048, 4096, 65536)
N_GRID = (64, 128, 1024, 1088, 2048, 4096, 5120, 8192, 11008, 13824, 16384, 28672)
K_GRID = (256, 384, 640, 1152, 2176, 4096, 4224, 5120, 8192, 11008, 11264, 11392, 12288, 13824, 14336, 14464, 28672)
ORDERS = (1, 2, 8, 63, 64, 102, 103, 104, 108)                 # every value atom_gemm_w4a4_packed_order can return on the grid

# the segmented entry points' fits queries: K on both sides of 4096, 8192, 12288 and 14464
SEG_M = (1, 2, 3, 16, 17, 256, 257)
SEG_N = (8, 16, 24, 4096, 13824)
SEG_NSEG = (0, 1, 2, 3, 4)
SEG_K = (256, 4096, 4224, 8192, 8320, 12288, 12416, 14464, 14592)
Q_OPS = (0, 1, 2, 3, 4, 5)
MERGE_SPLITS = (1, 2, 4, 16, 17)

ALPHABET = string.digits + string.ascii_letters


def shapes():
    return list(itertools.product(M_GRID, N_GRID, K_GRID))


def seg_shapes():
    return list(itertools.product(SEG_M, SEG_N, SEG_NSEG, SEG_K))


def plan_tables(L):
    """{table: list of values}, each in the order of shapes() / seg_shapes() (and of the innermost parameter where there is one)"""
    t = {k: [] for k in ("f6_order", "packed_order_0", "packed_order_1", "packed_order_2", "workspace_bytes", "ws_recodes", "ws_recodes_cached",
                         "o4_workspace_bytes", "multi_fits", "multi_q_fits", "multi_merge_q_fits")}
    for m, n, k in shapes():
        t["f6_order"].append(L.atom_gemm_w4a4_f6_order(m, n, k))
        for ws in (0, 1, 2):
            t[f"packed_order_{ws}"].append(L.atom_gemm_w4a4_packed_order(m, n, k, ws))
        t["workspace_bytes"].append(L.atom_gemm_w4a4_workspace_bytes(m, n, k))
        t["ws_recodes"].append(L.atom_gemm_w4a4_ws_recodes(m, n, k))
        t["ws_recodes_cached"].append(L.atom_gemm_w4a4_ws_recodes_cached(m, n, k))
        t["o4_workspace_bytes"].append(L.atom_gemm_w4a4_o4_workspace_bytes(m, n, k))
    for m, n, nseg, k in seg_shapes():
        t["multi_fits"].append(L.atom_gemm_w4a4_multi_fits(m, n, nseg, k))
        t["multi_q_fits"] += [L.atom_gemm_w4a4_multi_q_fits(q, m, n, nseg, k) for q in Q_OPS]
        t["multi_merge_q_fits"] += [L.atom_gemm_w4a4_multi_merge_q_fits(m, n, nseg, k, s) for s in MERGE_SPLITS]
    return t


BYTE_TABLES = ("workspace_bytes", "o4_workspace_bytes")


def encode(name, values):
    if name in BYTE_TABLES:
        assert all(v % 256 == 0 for v in values), name
        return [v // 256 for v in values]
    alphabet = sorted(set(values))
    assert len(alphabet) <= len(ALPHABET), name
    return {"values": alphabet, "codes": "".join(ALPHABET[alphabet.index(v)] for v in values)}


def decode(name, stored):
    if name in BYTE_TABLES:
        return [v * 256 for v in stored]
    return [stored["values"][ALPHABET.index(c)] for c in stored["codes"]]


# ---- rejected inputs of the queries: M = 0, N = 32, K = 128, K = 4000, N = 96 and negative values, one at a time, in two valid shapes
def _bad_shapes(m, n, k):
    return [(0, n, k), (m, 32, k), (m, n, 128), (m, n, 4000), (m, 96, k), (-m, n, k), (m, -n, k), (m, n, -k), (-m, -n, -k)]


def rejected():
    out = []
    for base in ((300, 4096, 4096), (16, 4096, 4096)):
        for a in _bad_shapes(*base):
            for f in ("atom_gemm_w4a4_f6_order", "atom_gemm_w4a4_workspace_bytes", "atom_gemm_w4a4_ws_recodes", "atom_gemm_w4a4_ws_recodes_cached",
                      "atom_gemm_w4a4_o4_workspace_bytes"):
                out.append((f, a))
            out += [("atom_gemm_w4a4_packed_order", a + (ws,)) for ws in (0, 1, 2)]
    for m, n, k in _bad_shapes(2, 4096, 4096) + [(2, 8, 4096), (2, 24, 4096)]:
        out.append(("atom_gemm_w4a4_multi_fits", (m, n, 2, k)))
        out.append(("atom_gemm_w4a4_multi_q_fits", (1, m, n, 2, k)))
        out.append(("atom_gemm_w4a4_multi_merge_q_fits", (m, n, 2, k, 2)))
    for nseg in (0, 4, -1):
        out.append(("atom_gemm_w4a4_multi_fits", (2, 4096, nseg, 4096)))
        out.append(("atom_gemm_w4a4_multi_q_fits", (1, 2, 4096, nseg, 4096)))
        out.append(("atom_gemm_w4a4_multi_merge_q_fits", (2, 4096, nseg, 4096, 2)))
    out += [("atom_gemm_w4a4_multi_q_fits", (q, 2, 4096, 2, 4096)) for q in (-1, 0, 5, 6)]
    out += [("atom_gemm_w4a4_multi_merge_q_fits", (1, 4096, 1, 4096, s)) for s in (-1, 0, 1, 17)]
    return out


# ---- the error-code matrix.  A call = an entry point, and what it changes in that entry point's valid argument list below.  Pointer
# arguments are "mem" / "mem2" / "mem3" (distinct 64-byte-aligned host buffers), "+n" (n bytes into the first) or "null"; "nan" is the float.
A_WIDE, AB_F6, B_F6S, WS_VERIFY, B_SCALE_PAIRS = 0x100, 0x200, 0x400, 0x4000, 0x2000
_OPS8 = [(n, "mem") for n in ("A4", "B4", "sA", "sB", "A8", "B8", "sA8", "sB8")]
_DIMS = [("M", 4), ("N", 256), ("K_total", 640), ("group", 128), ("keeper", 128), ("scale_layout", 0)]
_WS = [("workspace", "mem"), ("workspace_bytes", 1 << 30)]
_SEG_OUT = [("out0", "mem"), ("out1", "mem"), ("out2", "null"), ("f32_mask", 0), ("add0_f16", "null")]
_SEG_DIMS = [("M", 1), ("N_seg", 128), ("nseg", 2), ("K_total", 640), ("group", 128), ("keeper", 128)]
_WEIGHT = [(n, "mem") for n in ("B4", "sB", "B8", "sB8")]
VALID = {
    "atom_gemm_w4a4_f16": _OPS8 + [("D", "mem")] + _DIMS + [("stream", "null")],
    "atom_gemm_w4a4_f16_ws": _OPS8 + [("D", "mem"), ("M", 512), ("N", 4096), ("K_total", 4096)] + _DIMS[3:] + _WS + [("stream", "null")],
    "atom_gemm_w4a4_o4": _OPS8 + [("D_u4", "mem"), ("D_scale_zero", "mem")] + _DIMS + [("stream", "null")],
    "atom_gemm_w4a4_o4_ws": _OPS8 + [("D_u4", "mem"), ("D_scale_zero", "mem")] + _DIMS + _WS + [("stream", "null")],
    "atom_gemm_w4a4_f32": _OPS8 + [("D_f32", "mem")] + _DIMS + [("stream", "null")],
    "atom_gemm_w4a4_multi": _OPS8 + _SEG_OUT + _SEG_DIMS + [("scale_layout", 0), ("stream", "null")],
    "atom_gemm_w4a4_multi_q": [("q_op", 1), ("x", "mem"), ("x2", "null"), ("residual", "null"), ("residual_out", "null"), ("reorder_index", "mem"),
                               ("eps", 1e-5), ("clip", 1.0)] + _WEIGHT + _SEG_OUT + _SEG_DIMS + [("stream", "null")],
    "atom_gemm_w4a4_multi_merge_q": [("partials_f32", "mem"), ("splits", 2), ("reorder_index", "mem"), ("clip", 1.0)] + _WEIGHT + _SEG_OUT +
                                    _SEG_DIMS + [("stream", "null")],
    "atom_gemm_w4a4_silu_mul_quant_f6": [("A_f6", "mem"), ("Bgu_f6s", "mem"), ("A8", "mem"), ("Bgu8", "mem"), ("sA8", "mem"), ("sBgu8", "mem"),
                                         ("M", 4), ("N_inter", 256), ("K_total", 640), ("group", 128), ("keeper", 128), ("quant_mode", 0),
                                         ("clip", 1.0), ("scale_layout", 0), ("o_outliers", "mem"), ("o_norms_f6", "mem"),
                                         ("outlier_scales", "mem"), ("norm_scales", "mem"), ("xq", "null"), ("stream", "null")],
}
_ALIGN4 = ("sB", "sB8", "sBgu8")                                # pointers the ABI wants 4-byte aligned: "+2" is their fault
_UNCHECKED = ("sA", "sA8", "outlier_scales", "norm_scales", "D_scale_zero", "partials_f32")   # ... and those whose alignment it does not check


def matrix():
    """[(entry point, {argument: value})]: every call carries at least one fault"""
    calls = []
    for fn, valid in VALID.items():
        names = [n for n, _ in valid]
        one = lambda **kw: calls.append((fn, kw))
        seg, q, merge, gu = "nseg" in names, "q_op" in names, "splits" in names, "N_inter" in names
        ndim = "N_seg" if seg else ("N_inter" if gu else "N")
        ptrs = [n for n, v in valid if v == "mem" and n != "workspace"]
        for p in ptrs:
            if p != "reorder_index":                            # (optional)
                one(**{p: "null"})
        for p in ptrs:
            if p not in _UNCHECKED:
                one(**{p: "+2" if p in _ALIGN4 else "+8"})
        for k, v in (("M", 0), ("M", -1), (ndim, 0), (ndim, -256), ("K_total", 128), ("K_total", 4000), ("K_total", -640),
                     ("M", (1 << 24) + 1), ("K_total", (1 << 20) + 128), ("group", 64), ("keeper", 64)):
            one(**{k: v})
        if not seg:                                             # (two segments of 32 or 96 features are a legal N)
            one(**{ndim: 32})
            one(**{ndim: 96})
        if "scale_layout" in names:
            one(scale_layout=2)
            one(scale_layout=A_WIDE | AB_F6)
            one(scale_layout=B_F6S)
            one(scale_layout=2, **{ndim: 32})                   # bad flag + bad shape
            one(scale_layout=A_WIDE | AB_F6, K_total=4000)
            one(scale_layout=2, group=64)
        first, second = ptrs[0], ptrs[1]
        one(**{first: "null", second: "+8"})                    # null + misaligned
        one(**{second: "null", first: "+8"})
        one(**{first: "null", "K_total": 4000})                 # null + bad shape
        one(**{first: "+8", "K_total": 4000})                   # bad shape + misaligned
        one(**{first: "+8", "group": 64})
        one(sB8="+2", M=0) if "sB8" in names else one(sBgu8="+2", M=0)
        one(group=64, K_total=4000)
        if fn in ("atom_gemm_w4a4_f16", "atom_gemm_w4a4_f16_ws"):
            one(D="null", A4="null")
            one(D="null", K_total=4000)
            one(D="+8", K_total=4000)
            one(D="+8", B4="+8")
            one(D="null", scale_layout=2)
        if fn == "atom_gemm_w4a4_f16_ws":
            one(workspace="+8")
            one(workspace="+8", D="+8")
            one(N=4100)
            for flags in (WS_VERIFY, WS_VERIFY | 0x1000, WS_VERIFY | B_SCALE_PAIRS):
                one(scale_layout=flags, workspace="null")
                one(scale_layout=flags, workspace_bytes=8)
                one(scale_layout=flags, workspace="+8")
                one(scale_layout=flags, workspace="null", A4="null")       # the operands are checked before the assertions
                one(scale_layout=flags, workspace_bytes=8, K_total=4000)
                one(scale_layout=flags | 2, workspace="null")
            # a workspace too small, or none: the plain entry point's checks
            one(workspace="null", D="null")
            one(workspace_bytes=8, D="+8")
            one(workspace_bytes=0, K_total=4000)
        if fn in ("atom_gemm_w4a4_o4", "atom_gemm_w4a4_o4_ws"):
            one(N=192)                                          # N % 128
            one(N=192, D_u4="+8")
            one(N=192, scale_layout=A_WIDE)
            one(scale_layout=A_WIDE)
            one(scale_layout=AB_F6)
            one(scale_layout=AB_F6 | B_F6S)
            one(scale_layout=A_WIDE, D_u4="+8")
            one(D_u4="null", A4="null")
            one(D_scale_zero="null", K_total=4000)
        if fn == "atom_gemm_w4a4_o4_ws":
            one(workspace="+8")
            one(workspace="+8", D_u4="+8")
            one(workspace="null", D_u4="null")
            one(workspace_bytes=8, D_u4="+8")
            one(workspace="+8", N=192)
        if fn == "atom_gemm_w4a4_f32":
            one(M=300, N=4096, K_total=4096)                    # a shape outside the decode-batch kernel's
            one(M=64, N=4096, K_total=14592)
            one(M=300, N=4096, K_total=4096, D_f32="+8")
            one(scale_layout=A_WIDE)
            one(scale_layout=AB_F6)
            one(scale_layout=A_WIDE, D_f32="null")
            one(scale_layout=A_WIDE, A4="null")
        if seg:
            for k, v in (("nseg", 0), ("nseg", 4), ("nseg", -1), ("N_seg", 8), ("N_seg", 24)):
                one(**{k: v})
            one(out0="null")
            one(out1="null")
            one(nseg=3)                                         # out2 missing
            one(out1="+8")
            one(nseg=3, out2="+8")
            one(add0_f16="+8")
            one(f32_mask=1, add0_f16="mem")
            one(f32_mask=1, add0_f16="mem", N_seg=24)           # the segment's size is checked before the addend
            one(f32_mask=1, add0_f16="mem", K_total=4000)
            one(nseg=0, N_seg=24)                               # bad segment count + bad segment size
            one(nseg=4, K_total=4000)                           # bad segment + bad shape
            one(N_seg=24, K_total=4000)
            one(N_seg=24, M=0)
            one(N_seg=8, B4="null")
            one(N_seg=24, out0="+8")
            one(nseg=0, B4="+8")
            one(out0="+8", K_total=4000)
            one(out0="+8", B4="+8")
            one(M=300, N_seg=4096, K_total=4096)                # a shape the kernels behind it do not take
            one(M=300, N_seg=4096, K_total=4096, out0="+8")
        if fn == "atom_gemm_w4a4_multi":
            one(scale_layout=A_WIDE)
            one(scale_layout=AB_F6)
            one(scale_layout=A_WIDE, nseg=0)
            one(scale_layout=A_WIDE, N_seg=24)
            one(scale_layout=2, N_seg=24)
            one(M=17, K_total=8448)                             # more than 64 K items with more than one token block
        if q:
            for v in (0, 5, -1):
                one(q_op=v)
            one(x="null", q_op=0)
            for op in (2, 3, 4):
                one(q_op=op)                                    # x2 (and the residual pair) missing
            one(q_op=3, x2="mem")
            one(q_op=3, x2="mem", residual="mem2")
            one(q_op=3, x2="mem", residual="mem2", residual_out="mem2")     # residual_out == residual
            one(q_op=3, x2="mem", residual="mem2", residual_out="mem")      # residual_out == x
            one(q_op=4, x2="mem")                               # a reorder index with SiLU
            one(q_op=4, x2="mem", reorder_index="null", clip=0.0)
            one(q_op=4, x2="+8", reorder_index="null")
            one(q_op=3, x2="mem", residual="+8", residual_out="mem3")
            one(q_op=3, x2="mem", residual="mem2", residual_out="+8")
            for k, v in (("clip", 0.0), ("clip", "nan"), ("clip", -1.0), ("eps", -1.0), ("eps", "nan")):
                one(**{k: v})
            one(clip=0.0, nseg=0)
            one(clip=0.0, N_seg=24)
            one(clip=0.0, f32_mask=1, add0_f16="mem")
            one(clip=0.0, K_total=4000)
            one(eps=-1.0, B4="null")
            one(M=3)                                            # the quantiser in front: one or two tokens
            one(M=3, x="+8")
            one(x="+8", out0="+8")
            one(reorder_index="+8", x="+8")
            one(q_op=0, nseg=0)
        if merge:
            for s in (1, 17, 0, -2):
                one(splits=s)
            one(splits=1, out0="+8")
            one(splits=17, K_total=4000)
            one(splits=1, B4="+8")
            for v in (0.0, "nan", -1.0):
                one(clip=v)
            one(clip=0.0, N_seg=24)
            one(clip=0.0, partials_f32="null")
            one(clip=0.0, f32_mask=1, add0_f16="mem")
            one(M=3)
            one(reorder_index="+8", out0="+8")
            one(partials_f32="+8", splits=1)
        if gu:
            for v in (7, -1, 2):
                one(quant_mode=v)
            for v in (0.0, "nan", 1.5, -1.0):
                one(clip=v)
            one(N_inter=128)
            one(N_inter=320)                                    # N_inter % 128
            one(xq="+8")
            one(scale_layout=B_SCALE_PAIRS | 2)
            one(scale_layout=A_WIDE)
            one(quant_mode=7, scale_layout=2)
            one(quant_mode=7, clip=1.5)
            one(quant_mode=7, A_f6="null")
            one(clip=1.5, group=64)
            one(clip=1.5, K_total=4000)
            one(quant_mode=7, N_inter=320)
            one(N_inter=320, A_f6="+8")
            one(o_norms_f6="+8", A_f6="null")
            one(o_outliers="+8", K_total=4000)
    return calls


_mem = ctypes.create_string_buffer((1 << 16) + 64)
_base = (ctypes.addressof(_mem) + 63) & ~63


def _value(v):
    if v == "null":
        return None
    if v == "nan":
        return float("nan")
    if isinstance(v, str):
        return _base + {"mem": 0, "mem2": 4096, "mem3": 8192}[v] if v.startswith("mem") else _base + int(v)
    return v


def call(L, fn, changes):
    names = [n for n, _ in VALID[fn]]
    assert changes and set(changes) <= set(names), (fn, changes)
    return getattr(L, fn)(*(_value(changes.get(n, v)) for n, v in VALID[fn]))


def record(L):
    from atom_amd import _lib
    errors = [[fn, changes, call(L, fn, changes)] for fn, changes in matrix()]
    passed = [e for e in errors if e[2] not in (_lib.ERR_INVALID_ARG, _lib.ERR_SHAPE, _lib.ERR_ALIGN)]
    assert not passed, f"not rejected before the launch: {passed}"
    return {"plan": plan_tables(L), "rejected": [[f, list(a), getattr(L, f)(*a)] for f, a in rejected()], "errors": errors}


if __name__ == "__main__":
    from atom_amd._lib import lib
    res = record(lib())
    assert set(res["plan"]["packed_order_0"] + res["plan"]["packed_order_1"] + res["plan"]["packed_order_2"]) == set(ORDERS)
    with open(sys.argv[1], "w") as f:
        f.write("{\n")
        f.write(',\n'.join(f' "plan.{k}": {json.dumps(encode(k, v), separators=(",", ":"))}' for k, v in res["plan"].items()))
        f.write(',\n "rejected": [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in res["rejected"]) + "\n ]")
        # the calls are matrix(), in its order: their codes alone are stored
        f.write(',\n "errors": ' + json.dumps([st for _, _, st in res["errors"]], separators=(",", ":")))
        f.write("\n}\n")
    print({k: len(v) for k, v in res["plan"].items()}, len(res["rejected"]), "rejected queries,", len(res["errors"]), "rejected calls")
