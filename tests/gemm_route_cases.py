"""Output digests of the W4A4 GEMM entry points, one small case per route of DESIGN.md section 5 (operands, rows -> kernel, order): for
each route the shape of smallest M x N x K that the recorded host tables (tests/gemm_host_tables.py) map to it, found by a CPU search
over the queries.  Every case is one call of the C ABI -- one launch, or one chain (re-code + GEMM, GEMM + split-K reduce, the fall-back
of a refused launcher) -- on operands from a seeded numpy generator.  No kernel uses atomics, so the output bytes are a function of the
inputs and of the route alone.  tests/test_gpu_gemm_route_digests.py compares against tests/golden/gemm_route_digests.json, recorded on
the GPU at the commit BEFORE the route decision was folded into one function:

    python -m tests.gemm_route_cases tests/golden/gemm_route_digests.json

tools/gemm_routes.py runs the same cases once under a kernel trace.  A case whose call is refused is digested as its status code;
cases with a workspace digest the workspace behind the output (a weight-cached call that takes no re-coding route must leave it alone)."""
import hashlib
import json
import sys

import numpy as np

G128 = 128
PLAIN, REF = 1, 0
A_WIDE, AB_F6, B_F6S, CACHED, PAIRS = 0x100, 0x200, 0x400, 0x1000, 0x2000

# (name, entry point, M, N, K, options).  Options: flags; layout (PLAIN unless given); ws = "need" (what the query asks for), "short" (one
# byte less), "weight" (need, the weight's BF6 form put there by atom_repack_weight_f6s first) or a byte count; order = what
# atom_gemm_w4a4_packed_order(M, N, K, 0 / 1 / 2 for no / a free / a weight-cached workspace) must say; shift = {operand: bytes} moves
# an operand off its 16-byte alignment; status = the code a refused call returns.
CASES = [
    # ---- packed operands, no workspace
    ("dot_1tok", "f16", 1, 64, 256, dict(order=64)),
    ("dot_2tok_long_k", "f16", 2, 64, 4224, dict(order=64)),
    ("decode_2tok", "f16", 2, 64, 256, dict(order=8)),
    ("decode_16tok", "f16", 16, 64, 256, dict(order=8, layout=REF)),
    ("decode_16tok_8_slots", "f16", 16, 64, 7296, dict(order=8)),           # the three instances by K items per wave: <= 4, <= 8, <= 14
    ("decode_16tok_14_slots", "f16", 16, 64, 13440, dict(order=8)),
    ("decode_33tok", "f16", 33, 64, 384, dict(order=8)),
    ("decode_200tok", "f16", 200, 64, 384, dict(order=8)),
    ("mid_int8", "f16", 129, 2048, 4352, dict(order=1)),
    ("staged_dot", "f16", 3, 64, 14464, dict(order=63)),
    ("tiles_2wave", "f16", 257, 64, 256, dict(order=1)),                    # INT8 tiles: 64x128 (2 waves), 64x64 (1 wave), 256x128
    ("tiles_1_wave", "f16", 1024, 2176, 256, dict(order=1, layout=REF)),
    ("tiles_256x128", "f16", 4096, 4096, 256, dict(order=1)),
    # ---- packed operands with a workspace
    ("recode_mid", "f16_ws", 257, 2048, 1152, dict(ws="need", order=1, recodes=1)),
    ("recode_two_groups", "f16_ws", 513, 4096, 1152, dict(ws="need", order=2, recodes=1, flags=PAIRS)),
    ("recode_256x128", "f16_ws", 257, 11008, 1152, dict(ws="need", order=1, recodes=1)),
    ("recode_256x256", "f16_ws", 513, 11008, 1152, dict(ws="need", order=1, recodes=1, flags=PAIRS)),
    ("recode_256x256_own_scales", "f16_ws", 513, 11008, 1152, dict(ws="need", order=1, recodes=1)),
    ("recode_128x128", "f16_ws", 1500, 11008, 1152, dict(ws="need", order=1, recodes=1, layout=REF)),
    ("cached_64_rows", "f16_ws", 64, 13824, 5120, dict(ws="weight", flags=CACHED, order=1, recodes=0, recodes_cached=1)),
    ("cached_129_rows_two_groups", "f16_ws", 129, 11008, 1152, dict(ws="weight", flags=CACHED, order=2, recodes_cached=1)),
    ("splitk_2", "f16_ws", 257, 64, 1152, dict(ws="need", order=102)),
    ("splitk_3", "f16_ws", 2048, 1088, 2176, dict(ws="need", order=103)),
    ("splitk_4", "f16_ws", 257, 64, 2176, dict(ws="need", order=104)),
    ("splitk_8", "f16_ws", 8, 64, 14464, dict(ws="need", order=108)),
    ("long_k_12_rows", "f16_ws", 12, 8192, 28672, dict(ws="need", order=108)),
    ("long_k_12_rows_cached", "f16_ws", 12, 8192, 28672, dict(ws="need", flags=CACHED, order=1)),
    ("short_workspace", "f16_ws", 513, 4096, 1152, dict(ws="short", order=1, ws_order=0)),
    ("no_workspace_needed", "f16_ws", 16, 64, 256, dict(ws=4096, order=8)),
    # ---- BF6 operands: the five geometries, float32 weight scales behind the codes (ATOM_B_F6S) or fp16 ones
    ("f6_mid", "f16", 257, 2048, 1152, dict(flags=AB_F6 | B_F6S)),
    ("f6_mid_f16_scales", "f16", 257, 2048, 1152, dict(flags=AB_F6)),
    ("f6_two_groups", "f16", 513, 4096, 1152, dict(flags=AB_F6 | B_F6S | PAIRS)),
    ("f6_two_groups_short_k", "f16", 513, 4096, 896, dict(flags=AB_F6 | B_F6S)),
    ("f6_two_groups_f16_scales", "f16", 513, 4096, 1152, dict(flags=AB_F6)),
    ("f6_256x128", "f16", 257, 11008, 1152, dict(flags=AB_F6 | B_F6S)),
    ("f6_256x128_f16_scales", "f16", 257, 11008, 1152, dict(flags=AB_F6)),
    ("f6_256x256_pairs", "f16", 513, 11008, 1152, dict(flags=AB_F6 | B_F6S | PAIRS)),
    ("f6_256x256", "f16", 513, 11008, 1152, dict(flags=AB_F6 | B_F6S)),
    ("f6_256x256_f16_scales", "f16", 513, 11008, 1152, dict(flags=AB_F6 | PAIRS)),
    ("f6_128x128", "f16", 1500, 11008, 1152, dict(flags=AB_F6 | B_F6S)),
    ("f6_128x128_third_workgroup", "f16", 4096, 4352, 256, dict(flags=AB_F6 | B_F6S)),
    ("f6_128x128_f16_scales", "f16", 1500, 11008, 1152, dict(flags=AB_F6)),
    ("f6_with_a_workspace", "f16_ws", 513, 4096, 1152, dict(flags=AB_F6 | B_F6S, ws="need")),
    # ---- pre-widened activations: the three tile picks, and split-K through the workspace
    ("wide_2wave", "f16", 257, 64, 256, dict(flags=A_WIDE)),
    ("wide_1_wave", "f16", 1024, 2176, 256, dict(flags=A_WIDE)),
    ("wide_256x256", "f16", 2048, 4096, 256, dict(flags=A_WIDE)),
    ("wide_splitk", "f16_ws", 257, 64, 1152, dict(flags=A_WIDE, ws="need")),
    ("wide_no_split", "f16_ws", 1024, 2176, 256, dict(flags=A_WIDE, ws=1 << 20)),
    ("wide_mid_shape_splits", "f16_ws", 129, 2048, 4352, dict(flags=A_WIDE, ws="need")),
    # ---- the u4 epilogue, FP32 sums, segmented outputs
    ("o4_tiles", "o4", 40, 128, 640, {}),
    ("o4_ws_decode", "o4_ws", 16, 128, 256, dict(ws="o4")),
    ("o4_ws_tiles", "o4_ws", 300, 384, 384, dict(ws=1 << 20)),
    ("f32_dot", "f32", 1, 64, 256, {}),
    ("f32_decode", "f32", 16, 64, 256, {}),
    ("multi_dot", "multi", 1, 64, 256, dict(nseg=3, f32_mask=4, add=True)),
    ("multi_decode", "multi", 16, 64, 256, dict(nseg=3, f32_mask=4, add=True, layout=REF)),
    ("multi_q_dot_1", "multi_q", 1, 64, 640, dict(nseg=2, q_op=1, f32_mask=2)),
    ("multi_q_dot_2", "multi_q", 1, 64, 640, dict(nseg=2, q_op=2)),
    ("multi_q_dot_3", "multi_q", 2, 64, 4224, dict(nseg=2, q_op=3, add=True)),
    ("multi_q_dot_4", "multi_q", 1, 64, 640, dict(nseg=2, q_op=4)),
    ("multi_q_decode_1", "multi_q", 2, 64, 640, dict(nseg=2, q_op=1, f32_mask=2)),
    ("multi_q_decode_2", "multi_q", 2, 64, 640, dict(nseg=2, q_op=2)),
    ("multi_q_decode_3", "multi_q", 2, 64, 640, dict(nseg=2, q_op=3, add=True)),
    ("multi_q_decode_4", "multi_q", 2, 64, 640, dict(nseg=2, q_op=4)),
    ("merge_q", "merge_q", 1, 64, 640, dict(nseg=2, splits=2, add=True)),
    ("gateup_sim", "gateup", 300, 256, 384, dict(mode=1, clip=0.9, flags=PAIRS)),
    ("gateup_kernel", "gateup", 300, 256, 384, dict(mode=0, clip=1.0, flags=PAIRS, layout=REF)),
    ("gateup_sim_own_scales", "gateup", 300, 256, 384, dict(mode=1, clip=0.9)),
    ("gateup_kernel_own_scales", "gateup", 300, 256, 384, dict(mode=0, clip=1.0)),
    # ---- what a launcher refuses and the route cannot see: weight scales 4 bytes off an 8-byte boundary are legal for the tile
    # kernels, which must take the call; entry points with no kernel behind the decode-batch one report the refusal.  (An output 8 bytes
    # off is refused by every entry point before any launcher is asked: ATOM_ERR_ALIGN.)
    ("decode_scales_off_8", "f16", 16, 64, 256, dict(shift={"sB": 4})),
    ("decode_keeper_scales_off_8", "f16", 16, 64, 256, dict(shift={"sB8": 4})),
    ("decode_output_off_16", "f16", 16, 64, 256, dict(shift={"D": 8}, status=-14)),
    ("f32_scales_off_8", "f32", 16, 64, 256, dict(shift={"sB": 4}, status=-33)),
    ("o4_ws_scales_off_8", "o4_ws", 16, 128, 256, dict(ws="o4", shift={"sB": 4})),
    ("multi_scales_off_8", "multi", 16, 64, 256, dict(nseg=3, shift={"sB": 4}, status=-33)),
    ("multi_q_scales_off_8", "multi_q", 2, 64, 640, dict(nseg=2, q_op=1, shift={"sB": 4}, status=-33)),
]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class _Dev:
    """numpy arrays on the device, by name; `shift` puts an array that many bytes into a larger allocation"""

    def __init__(self, shift):
        self.t, self.shift = {}, shift

    def put(self, name, a):
        import torch
        a = np.ascontiguousarray(a)
        off = self.shift.get(name, 0)
        raw = np.zeros(a.nbytes + 16, dtype=np.uint8)
        raw[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.t[name] = (torch.from_numpy(raw).cuda(), off, a.dtype, a.shape)
        return self.ptr(name)

    def ptr(self, name):
        return self.t[name][0].data_ptr() + self.t[name][1]

    def dev(self, name):
        """the array as a torch tensor on the device (a view)"""
        import torch
        t, off, dtype, shape = self.t[name]
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return t[off:off + n].view(torch.from_numpy(np.empty(0, dtype=dtype)).dtype).reshape(shape)

    def get(self, name):
        t, off, dtype, shape = self.t[name]
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return t.cpu().numpy()[off:off + n].view(dtype).reshape(shape)


_operand_cache = {}


def _operands(M, N, K, seed):
    """the packed operands of a shape (weight scales shared by channel pairs), made once per shape"""
    key = (M, N, K)
    if key not in _operand_cache:
        _operand_cache.clear()                                  # (cases of one shape are adjacent: keep one)
        rng = np.random.default_rng(seed)
        G = (K - G128) // G128
        sB = np.repeat(rng.uniform(0.005, 0.05, (G, N // 2)).astype(np.float16), 2, axis=1)
        _operand_cache[key] = dict(
            A4=rng.integers(0, 256, (M, (K - G128) // 2), dtype=np.uint8), B4=rng.integers(0, 256, (N, (K - G128) // 2), dtype=np.uint8),
            A8=rng.integers(-128, 128, (M, G128), dtype=np.int16).astype(np.int8), B8=rng.integers(-128, 128, (N, G128), dtype=np.int16).astype(np.int8),
            sB=sB, sB8=rng.uniform(0.005, 0.05, (N,)).astype(np.float16), rng=rng)
    return _operand_cache[key]


def check_route(lib, case):
    """the queries (CPU) say what the case is there for"""
    name, entry, M, N, K, o = case
    cached = o.get("flags", 0) & CACHED
    if "order" in o:
        assert lib.atom_gemm_w4a4_packed_order(M, N, K, o.get("ws_order", 0 if entry == "f16" else (2 if cached else 1))) == o["order"], name
    for q in ("recodes", "recodes_cached"):
        if q in o:
            assert getattr(lib, "atom_gemm_w4a4_ws_" + q)(M, N, K) == o[q], (name, q)
    if o.get("ws") in ("need", "short", "weight"):
        assert lib.atom_gemm_w4a4_workspace_bytes(M, N, K) > 0, name
    if entry in ("multi", "multi_q", "merge_q") and "status" not in o:
        fits = {"multi": lambda: lib.atom_gemm_w4a4_multi_fits(M, N, o["nseg"], K),
                "multi_q": lambda: lib.atom_gemm_w4a4_multi_q_fits(o.get("q_op", 0), M, N, o["nseg"], K),
                "merge_q": lambda: lib.atom_gemm_w4a4_multi_merge_q_fits(M, N, o["nseg"], K, o.get("splits", 0))}[entry]()
        assert fits == 1, name


def call(case, src=None, flags=None):
    """Make the call of one case and return (status, the device arrays by name, the names of its outputs in digest order).  `src`: the
    operands -- A4 (packed, or the wide form for a case with ATOM_A_WIDE), B4, A8, B8, sA [G, ld], sA8 [ld] in the case's scale layout,
    sB, sB8 -- in place of the seeded ones (tests/test_gpu_gemm_planted.py); `flags` in place of the case's own."""
    import torch
    from atom_amd import _lib
    lib = _lib.lib()
    name, entry, M, N, K, o = case
    layout, flags, shift = o.get("layout", PLAIN), o.get("flags", 0) if flags is None else flags, o.get("shift", {})
    G = (K - G128) // G128
    stream = _lib.current_stream(torch.device("cuda"))
    nseg = o.get("nseg", 1)
    n_all = N * nseg if entry != "gateup" else 2 * N
    given = src is not None
    if not given:
        src = _operands(M, n_all, K, seed=M * 1000003 + n_all * 1009 + K)
    rng = np.random.default_rng(len(name) + M + n_all + K)
    ld = lib.atom_scale_size(M, layout)
    d = _Dev(shift)
    for k in ("B4", "B8", "sB", "sB8", "A8"):
        d.put(k, src[k])
    if given:
        assert src["sA"].shape == (G, ld) and src["sA8"].shape == (ld,) and src["A4"].shape == (M, (K - G128) // (1 if flags & A_WIDE else 2))
        for k in ("sA", "sA8", "A4"):
            d.put(k, src[k])
    else:
        d.put("sA", rng.uniform(0.005, 0.05, (G, ld)).astype(np.float16))
        d.put("sA8", rng.uniform(0.005, 0.05, (ld,)).astype(np.float16))
        if flags & A_WIDE:
            d.put("A4", (rng.integers(-8, 8, (M, K - G128)) * 16).astype(np.int8))
        else:
            d.put("A4", src["A4"])
    check_route(lib, case)
    rows = lambda r: (r + 255) // 256 * 256
    if (flags & AB_F6) or entry == "gateup":                    # the BF6 operands, by the library's own re-coding kernels
        a6 = np.zeros((G, rows(M), 104), dtype=np.uint8)
        d.put("A6", a6)
        _lib.check(lib.atom_repack_act_f6(d.ptr("A4"), d.ptr("sA"), M, K, layout, d.ptr("A6"), stream), "atom_repack_act_f6")
        d.put("B6", np.zeros(lib.atom_f6_weight_bytes(n_all, K), dtype=np.uint8))
        if (flags & B_F6S) or entry == "gateup":
            _lib.check(lib.atom_repack_weight_f6s(d.ptr("B4"), d.ptr("sB"), n_all, K, d.ptr("B6"), stream), "atom_repack_weight_f6s")
        else:
            _lib.check(lib.atom_repack_weight_f6(d.ptr("B4"), n_all, K, d.ptr("B6"), stream), "atom_repack_weight_f6")
    a4, b4 = ("A6", "B6") if flags & AB_F6 else ("A4", "B4")
    ops8 = [d.ptr(k) for k in (a4, b4, "sA", "sB", "A8", "B8", "sA8", "sB8")]
    dims = [M, N, K, G128, G128, layout | flags]
    ws_args, outs = [], []
    if "ws" in o:
        need = lib.atom_gemm_w4a4_o4_workspace_bytes(M, N, K) if o["ws"] == "o4" else lib.atom_gemm_w4a4_workspace_bytes(M, N, K)
        nbytes = o["ws"] if isinstance(o["ws"], int) else need
        assert nbytes > 0, name
        d.put("ws", rng.integers(0, 256, nbytes, dtype=np.uint8))
        if o["ws"] == "weight":
            assert need >= lib.atom_f6_weight_bytes(N, K)
            _lib.check(lib.atom_repack_weight_f6s(d.ptr("B4"), d.ptr("sB"), N, K, d.ptr("ws"), stream), "atom_repack_weight_f6s")
        ws_args = [d.ptr("ws"), nbytes - 1 if o["ws"] == "short" else nbytes]
        outs.append("ws")

    def out(name_, shape, dtype):
        outs.insert(len(outs) - ("ws" in outs), name_)
        return d.put(name_, np.zeros(shape, dtype=dtype))

    def seg_outs():
        mask = o.get("f32_mask", 0)
        p = [out(f"out{i}", (M, N), np.float32 if (mask >> i) & 1 else np.float16) if i < nseg else None for i in range(3)]
        add = d.put("add", rng.standard_normal((M, N)).astype(np.float16)) if o.get("add") else None
        return p + [mask, add]

    if entry == "f16":
        st = lib.atom_gemm_w4a4_f16(*ops8, out("D", (M, N), np.float16), *dims, stream)
    elif entry == "f16_ws":
        st = lib.atom_gemm_w4a4_f16_ws(*ops8, out("D", (M, N), np.float16), *dims, *ws_args, stream)
    elif entry == "f32":
        st = lib.atom_gemm_w4a4_f32(*ops8, out("D", (M, N), np.float32), *dims, stream)
    elif entry in ("o4", "o4_ws"):
        o4 = [out("D4", (M, N // 2), np.uint8), out("Dsz", (M, N // 128 * 2), np.float16)]
        st = getattr(lib, "atom_gemm_w4a4_" + entry)(*ops8, *o4, *dims, *ws_args, stream)
    elif entry == "multi":
        st = lib.atom_gemm_w4a4_multi(*ops8, *seg_outs(), M, N, nseg, K, G128, G128, layout | flags, stream)
    elif entry == "multi_q":
        q = o["q_op"]
        x = rng.standard_normal((M, K)).astype(np.float16)
        x2 = {1: None, 2: rng.uniform(0.5, 1.5, (K,)), 3: rng.uniform(0.5, 1.5, (K,)), 4: rng.standard_normal((M, K))}[q]
        res = d.put("res", rng.standard_normal((M, K)).astype(np.float16)) if q == 3 else None
        res_out = out("res_out", (M, K), np.float16) if q == 3 else None
        idx = d.put("idx", rng.permutation(K).astype(np.int16)) if q != 4 else None
        st = lib.atom_gemm_w4a4_multi_q(q, d.put("x", x), None if x2 is None else d.put("x2", x2.astype(np.float16)), res, res_out, idx, 1e-5, 0.9,
                                        *(d.ptr(k) for k in ("B4", "sB", "B8", "sB8")), *seg_outs(), M, N, nseg, K, G128, G128, stream)
    elif entry == "merge_q":
        part = src["part"] if given and "part" in src else rng.uniform(0.1, 1.0, (M, K // 128, o["splits"], 130)).astype(np.float32)
        st = lib.atom_gemm_w4a4_multi_merge_q(d.put("part", part), o["splits"], d.put("idx", rng.permutation(K).astype(np.int16)), 0.9,
                                              *(d.ptr(k) for k in ("B4", "sB", "B8", "sB8")), *seg_outs(), M, N, nseg, K, G128, G128, stream)
    elif entry == "gateup":
        go = [out("o8", (M, G128), np.int8), out("o6", (N // 128 - 1, rows(M), 104), np.uint8), out("s8", (ld,), np.float16),
              out("s4", (N // 128 - 1, ld), np.float16), out("xq", (M, N), np.float16)]
        st = lib.atom_gemm_w4a4_silu_mul_quant_f6(d.ptr("A6"), d.ptr("B6"), d.ptr("A8"), d.ptr("B8"), d.ptr("sA8"), d.ptr("sB8"), M, N, K, G128, G128,
                                                  o["mode"], o["clip"], layout | flags, *go, stream)
    else:
        raise KeyError(entry)
    torch.cuda.synchronize()
    return st, d, outs


def run(case):
    """the digest of one case (and what the call returned)"""
    name, o = case[0], case[5]
    st, d, outs = call(case)
    assert st == o.get("status", 0), f"{name}: status {st}"
    return f"status {st}" if st != 0 else _sha(*(d.get(k) for k in outs))


def compute(cases=CASES):
    """{case: sha256 of the output bytes}, in the order of CASES"""
    return {c[0]: run(c) for c in cases}


if __name__ == "__main__":
    res = compute()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
