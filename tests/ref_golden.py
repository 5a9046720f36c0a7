"""ctypes view of oracle/_ref/libatom_ref.so: the reference's own CPU golden functions (run_cpu_reorder_fp16_i4,
run_cpu_activate_fp16_i4, run_cpu_rmsnorm_fp16_i4, its INT4 paged-KV restatements and the u4-output GEMM epilogue), compiled from
the reference source by oracle/Makefile.  Checker side only.

Where the library is not built (no reference tree on the machine) every function here replays what the library returned for the
same inputs, from tests/golden/ref_cpu_calls.npz (keyed by a hash of the function name and its inputs; written by
tests/golden/gen_golden_refcpu.py).  Where the library is built, its results are also checked against those recordings.

Most of those results are (nearly) what the repository's restatement (oracle/atom_oracle.py) computes for the same call, so an
array is stored as the XOR of its bytes with the restatement's prediction -- nearly all zeros -- beside the sha256 of the
reference's own bytes.  Replay rebuilds the bytes and checks that digest: a changed restatement cannot change what is replayed,
only make the replay fail.  Arrays without a prediction are stored as they are."""
import atexit
import ctypes
import hashlib
import os

import numpy as np

from oracle import atom_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "oracle", "_ref", "libatom_ref.so")
RECORDED = os.path.join(ROOT, "tests", "golden", "ref_cpu_calls.npz")
_RECORD_TO = os.environ.get("ATOM_REF_RECORD")      # set by gen_golden_refcpu.py: every library call made is added to that file
_lib = None
_recorded = None
_pending = {}


def lib_built() -> bool:
    return os.path.exists(_SO)


def _key(name, inputs):
    h = hashlib.sha256(name.encode())
    for a in inputs:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
        else:
            h.update(repr(a).encode())
    return h.hexdigest()[:32]


def _recordings():
    """{key: {field: stored array}}; a predicted field F is stored as F~x (XOR bytes), F~sha, F~shape, F~dtype."""
    global _recorded
    if _recorded is None:
        _recorded = {}
        if os.path.exists(RECORDED):
            z = np.load(RECORDED)
            for f in z.files:
                k, field = f.split(".", 1)
                _recorded.setdefault(k, {})[field] = z[f]
    return _recorded


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _encode(out, pred):
    """What is stored for one call: predicted fields as XOR against the prediction, the rest as they are."""
    rec = {}
    for f, a in out.items():
        a = np.ascontiguousarray(a)
        p = None if pred is None else pred.get(f)
        if p is not None and np.ascontiguousarray(p).nbytes == a.nbytes:
            rec[f + "~x"] = np.bitwise_xor(a.view(np.uint8).ravel(), np.ascontiguousarray(p).view(np.uint8).ravel())
            rec[f + "~sha"] = _sha(a)
            rec[f + "~shape"] = np.array(a.shape, np.int64)
            rec[f + "~dtype"] = np.array(a.dtype.str)
        else:
            rec[f] = a
    return rec


def _decode(name, rec, predict):
    out, pred = {}, None
    for f, a in rec.items():
        if "~" not in f:
            out[f] = a
        elif f.endswith("~x"):
            f = f[:-2]
            if pred is None:
                pred = predict()
            p = np.ascontiguousarray(pred[f]).view(np.uint8).ravel()
            b = np.bitwise_xor(p, a) if p.size == a.size else None
            if b is None or not np.array_equal(_sha(b), rec[f + "~sha"]):
                raise LookupError(f"the recording of the reference's {name}.{f} does not rebuild against oracle/atom_oracle.py's "
                                  "prediction: re-record with tests/golden/gen_golden_refcpu.py where oracle/_ref/libatom_ref.so is built")
            out[f] = b.view(np.dtype(str(rec[f + "~dtype"]))).reshape(tuple(rec[f + "~shape"]))
    return out


def _save_pending():
    if not _pending:
        return
    old = dict(np.load(_RECORD_TO)) if os.path.exists(_RECORD_TO) else {}
    for k, rec in _pending.items():
        old = {f: a for f, a in old.items() if not f.startswith(k + ".")}
        for field, a in rec.items():
            old[f"{k}.{field}"] = a
    np.savez_compressed(_RECORD_TO, **old)


if _RECORD_TO:
    atexit.register(_save_pending)


def _call(name, inputs, compute, predict=None):
    """compute() -> dict of arrays, run on the reference's library where it is built; else the recorded result of the same call.
    predict() -> the restatement's arrays for the same call (the fields it can predict), used to store and rebuild the recording."""
    k = _key(name, inputs)
    rec = _recordings().get(k)
    if lib_built():
        out = compute()
        if rec is not None:
            want = _decode(name, rec, predict)
            for field, a in out.items():
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(want[field]).view(np.uint8)), \
                    f"{RECORDED} disagrees with the reference's library on {name}.{field}"
        if _RECORD_TO:
            _pending[k] = _encode(out, None if predict is None else predict())
        return out
    if rec is None:
        raise LookupError(f"no recorded result of the reference's {name} for these inputs in {RECORDED}: record it with "
                          "tests/golden/gen_golden_refcpu.py where oracle/_ref/libatom_ref.so is built")
    return _decode(name, rec, predict)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_SO)
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.ref_cpu_reorder_fp16_i4.restype = None
        L.ref_cpu_reorder_fp16_i4.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp]
        L.ref_cpu_activate_fp16_i4.restype = None
        L.ref_cpu_activate_fp16_i4.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp]
        L.ref_cpu_rmsnorm_fp16_i4.restype = None
        L.ref_cpu_rmsnorm_fp16_i4.argtypes = [vp, vp, ctypes.c_float, i, i, i, vp, vp, vp, vp, vp]
        L.ref_cpu_append_paged_kv_i4.restype = None
        L.ref_cpu_append_paged_kv_i4.argtypes = [vp] * 5 + [i] * 6 + [vp] * 5
        L.ref_cpu_single_decode_i4.restype = None
        L.ref_cpu_single_decode_i4.argtypes = [vp] * 5 + [i, i, i, ctypes.c_float, ctypes.c_float, vp]
        L.ref_cpu_o4_epilogue.restype = None
        L.ref_cpu_o4_epilogue.argtypes = [vp, i, i, vp, vp]
        L.ref_scale_index.restype = i
        L.ref_scale_index.argtypes = [i]
        _lib = L
    return _lib


def scale_size(rows: int) -> int:
    """SCALE_SIZE_A (Reorder.cu:50)."""
    return rows // 16 * 64 + 64 - (1 - (rows % 16) // 8) * (8 - (rows % 8)) * 8


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def scale_index(r: int) -> int:
    """The reference's row -> scale position map (Reorder.cu)."""
    return int(_call("scale_index", [int(r)], lambda: {"v": np.array([lib().ref_scale_index(int(r))], np.int64)})["v"][0])


def _run(kind, x, b=None, w=None, idx=None, eps=0.0):
    """Returns dict(q4 int8 [M, K4] (unpacked), s4 f16 [M, G], q8 int8 [M, 128], s8 f16 [M]) read back from the reference's
    buffers: packed PackInt4 codes (low nibble = even element) and the replicated scale layout (first replica)."""
    x = np.ascontiguousarray(x, dtype=np.float16)
    M, H = x.shape
    G = H // 128 - 1
    ld = scale_size(M)
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.int16)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float16)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float16)

    def compute():
        o8 = np.zeros((M, 128), np.int8)
        o4 = np.zeros((M, (H - 128) // 2), np.uint8)
        s8 = np.zeros(ld, np.float16)
        s4 = np.zeros(G * ld, np.float16)
        L = lib()
        if kind == "reorder":
            L.ref_cpu_reorder_fp16_i4(_p(x), 128, H, M, _p(idx), _p(o8), _p(o4), _p(s8), _p(s4))
        elif kind == "activate":
            L.ref_cpu_activate_fp16_i4(_p(x), _p(b), 128, H, M, _p(o8), _p(o4), _p(s8), _p(s4))
        else:
            L.ref_cpu_rmsnorm_fp16_i4(_p(x), _p(w), float(eps), 128, H, M, _p(idx), _p(o8), _p(o4), _p(s8), _p(s4))
        rows = np.array([L.ref_scale_index(r) for r in range(M)], np.int64)
        return dict(o8=o8, o4=o4, s8=s8, s4=s4, rows=rows)

    def predict():                      # the restatement in kernel mode, in the reference's buffer layout
        if kind == "reorder":
            q = O.reorder_quant(x, idx, "kernel", 1.0)
        elif kind == "activate":
            q = O.silu_mul_quant(x, b, "kernel", 1.0)
        else:
            q = O.rmsnorm_reorder_quant(x, w, eps, idx, "kernel", 1.0)
        return dict(o8=np.asarray(q["q8"], np.int8), o4=O.pack_int4(q["q4"]),
                    s8=O.scales_to_ref_layout(np.asarray(q["s8"]).reshape(1, M)).ravel(),
                    s4=O.scales_to_ref_layout(np.ascontiguousarray(np.asarray(q["s4"]).T)).ravel(),
                    rows=np.array([O.scale_index(r) for r in range(M)], np.int64))
    r = _call(kind, [x, b, w, idx, float(eps)], compute, predict)
    o8, o4, s8, s4, rows = r["o8"], r["o4"], r["s8"], r["s4"], r["rows"]
    lo = (o4 & 0xF).astype(np.int8)
    hi = (o4 >> 4).astype(np.int8)
    q4 = np.stack([np.where(lo >= 8, lo - 16, lo), np.where(hi >= 8, hi - 16, hi)], axis=-1).reshape(M, H - 128).astype(np.int8)
    s4p = s4.reshape(G, ld)[:, rows].T.copy()
    # all four replicas of a scale must agree (rows + 2k)
    for k in range(1, 4):
        assert np.array_equal(s4.reshape(G, ld)[:, rows + 2 * k].T, s4p)
    return dict(q4=q4, s4=s4p, q8=o8, s8=s8[rows].copy(), raw_s4=s4, raw_s8=s8, packed4=o4)


def reorder(x, idx):
    return _run("reorder", x, idx=idx)


def activate(a, b):
    return _run("activate", a, b=b)


def rmsnorm(x, w, eps, idx):
    return _run("rmsnorm", x, w=w, idx=idx, eps=eps)


def o4_epilogue(c32):
    """The u4-output GEMM's epilogue as the reference CODE computes it (DenseLayerGEMM_i4_o4.cu:722-786 applied around the
    reference's own local_max_min, :72-80; oracle/ref/wrap.cpp) on FP32 sums [M, N] -> (u8 [M, N/2], f16 (scale, zero) [M, N/128, 2]).
    The reference casts round(...) to int8_t with no clamp (:766-767): out of the int8 range that is undefined behaviour on the host
    (and a saturating cvt on the device), so callers compare only where in_range() holds."""
    c32 = np.ascontiguousarray(c32, dtype=np.float32)
    M, N = c32.shape

    def compute():
        D = np.zeros((M, N // 2), np.uint8)
        sz = np.zeros((M, N // 128, 2), np.float16)
        lib().ref_cpu_o4_epilogue(_p(c32), M, N, _p(D), _p(sz))
        return dict(D=D, sz=sz)
    r = _call("o4_epilogue", [c32], compute, lambda: dict(zip(("D", "sz"), O.quant_o4(c32, ref_extrema=True))))
    return r["D"], r["sz"]


def o4_in_range(c32):
    """[M, N/128] bool: groups whose reference-code quotients (x + zero) * r all lie inside the int8 range (see o4_epilogue)."""
    g = np.asarray(c32, np.float32).reshape(c32.shape[0], -1, 128)
    a = np.abs(g)
    mx, mn = a.max(-1), a.min(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(1) / ((mx - mn) / np.float32(15)).astype(np.float32)
        q = ((g - mn[..., None]).astype(np.float32) * r[..., None]).astype(np.float32)
    return np.isfinite(q).all(-1) & (np.abs(q) < 127).all(-1)


# ---- INT4 paged KV cache: the reference's CPU restatements (kernels/src/flashinfer/cpu_reference.h)
def append_paged_kv_i4(data, param, indptr, indices, last_page_offset, k, v, k_param, v_param, layer, append_indptr):
    """In place on data u8 [pages, L, 2, N, P, D/2] / param f16 [pages, L, 2, N, P, 2]; k, v u8 [T, N, D/2]; k_param, v_param f16 [T, N, 2]."""
    assert data.flags.c_contiguous and param.flags.c_contiguous and data.dtype == np.uint8 and param.dtype == np.float16
    pages, Lr, _, N, P, Dh = data.shape
    c32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    ip, ix, lp, ap = c32(indptr), c32(indices), c32(last_page_offset), c32(append_indptr)
    k, v = np.ascontiguousarray(k, np.uint8), np.ascontiguousarray(v, np.uint8)
    kp, vpm = np.ascontiguousarray(k_param, np.float16), np.ascontiguousarray(v_param, np.float16)

    def compute():
        d, p = data.copy(), param.copy()
        lib().ref_cpu_append_paged_kv_i4(_p(d), _p(p), _p(ip), _p(ix), _p(lp), Lr, int(layer), N, P, Dh * 2, len(lp), _p(k), _p(v),
                                         _p(kp), _p(vpm), _p(ap))
        return dict(d=d, p=p)

    def predict():
        d, p = data.copy(), param.copy()
        O.kv_append_i4(d, p, ip, ix, lp, k, v, kp, vpm, int(layer), append_indptr=ap)
        return dict(d=d, p=p)
    r = _call("append_paged_kv_i4", [data, param.view(np.uint16), ip, ix, lp, k, v, kp.view(np.uint16), vpm.view(np.uint16), int(layer), ap],
              compute, predict)
    data[...] = r["d"]
    param[...] = r["p"]


def single_decode_i4(q16, k, v, k_param, v_param, theta=1e4):
    """q f16 [N, D]; k, v u8 [S, N, D/2]; k_param, v_param f16 [S, N, 2] -> float32 [N, D] (llama RoPE on q at S - 1 and on every key)."""
    q16 = np.ascontiguousarray(q16, np.float16)
    k, v = np.ascontiguousarray(k, np.uint8), np.ascontiguousarray(v, np.uint8)
    kp, vpm = np.ascontiguousarray(k_param, np.float16), np.ascontiguousarray(v_param, np.float16)
    S, N, Dh = k.shape

    def compute():
        out = np.empty((N, Dh * 2), np.float32)
        lib().ref_cpu_single_decode_i4(_p(q16), _p(k), _p(v), _p(kp), _p(vpm), S, N, Dh * 2, 1.0, float(theta), _p(out))
        return dict(out=out)
    return _call("single_decode_i4", [q16.view(np.uint16), k, v, kp.view(np.uint16), vpm.view(np.uint16), float(theta)], compute)["out"]
