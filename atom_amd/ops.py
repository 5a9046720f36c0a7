"""Native op wrappers with the call surface of the reference's ``punica.ops``
(/root/reference/e2e/punica-atom/punica/ops/__init__.py:137-219): same names, same positional arguments,
same return tuples and output shapes/dtypes.  Each call allocates its outputs with ``torch.empty`` and
enqueues one HIP kernel of libatom_hip.so on the current stream.

Keyword-only extras (defaults reproduce the reference CUDA kernels exactly):
  quant_mode   "kernel" (Reorder.cuh:137-178 arithmetic) | "sim" (model/quant.py arithmetic)
  clip         clip ratio applied to the INT4 groups' absmax (1.0 = none, the kernels' behaviour)
  scale_layout "ref" (ldmatrix-replicated layout, scale_size(M) halves per group) | "plain" ([G, M])
  return_dequant  also return the de-quantised FP16 tensor (what quantize_activation_wrapper returns)
  wide_codes   (activation ops) / a_wide (GEMM): the native activation format of include/atom_hip.h -- o_norms is
               int8 [bs, H-128] = code*16 with the even/odd channels of every 32-channel block de-interleaved, i.e.
               already the INT8 MFMA operand; the prefill GEMM then skips 2/3 of its widening instructions.
               wide_codes="f6" / a_wide="f6": the BF6 group-major format [G][f6_rows(bs)][104] of the block-scaled-MFMA
               prefill kernel; the GEMM then also wants the weight from repack_weight_f6
"""
from __future__ import annotations

import collections
import weakref

import torch

from . import _lib as L

GROUP_SIZE = 128

_MODES = {"kernel": L.QUANT_KERNEL, "sim": L.QUANT_SIM}
_LAYOUTS = {"ref": L.SCALE_LAYOUT_REF, "plain": L.SCALE_LAYOUT_PLAIN}


def scale_size(x: int) -> int:
    """punica/ops/__init__.py:137-138 (SCALE_SIZE_A, Reorder.cuh:50)."""
    return ((x) // 16 * 64 + 64 - (1 - (x % 16) // 8) * (8 - (x % 8)) * 8)


def _ld(rows: int, layout: str) -> int:
    return scale_size(rows) if layout == "ref" else rows


def _require_cuda_half(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise L.AtomHipError(f"{name} must live on the GPU: the Atom W4A4 path has no CPU fallback")
    if t.dtype != torch.float16:
        raise TypeError(f"{name} must be float16, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def f6_rows(rows: int) -> int:
    """Rows per group of an F6 operand buffer (include/atom_hip.h, ATOM_AB_F6): rows rounded up to 256."""
    return (rows + 255) // 256 * 256


def _alloc_act_outputs(bs, hidden_dim, device, layout, return_dequant, wide=False):
    # empty, like the reference's wrappers (punica/ops/__init__.py:189-196): the replicated layout has slots no row ever
    # writes, and no kernel here reads them (rows are clamped to M - 1); zero-filling them cost two fill launches per op
    alloc = torch.empty
    o_outlier = torch.empty((bs, GROUP_SIZE), dtype=torch.int8, device=device)
    if wide == "f6":        # [G][rows_pad][104] BF6 streams + in-row scales; pad rows are never read into a result
        o_norms = torch.empty((hidden_dim // GROUP_SIZE - 1, f6_rows(bs), L.F6_PITCH), dtype=torch.uint8, device=device)
    else:
        o_norms = torch.empty((bs, (hidden_dim - GROUP_SIZE) // (1 if wide else 2)), dtype=torch.int8, device=device)
    outlier_scales = alloc((_ld(bs, layout),), dtype=torch.float16, device=device)
    norm_scales = alloc((hidden_dim // GROUP_SIZE - 1, _ld(bs, layout)), dtype=torch.float16, device=device)
    xq = torch.empty((bs, hidden_dim), dtype=torch.float16, device=device) if return_dequant else None
    return o_outlier, o_norms, outlier_scales, norm_scales, xq


def _ret(o_outlier, o_norms, outlier_scales, norm_scales, xq):
    if xq is None:
        return o_outlier, o_norms, outlier_scales, norm_scales
    return o_outlier, o_norms, outlier_scales, norm_scales, xq


def _mode(quant_mode, wide_codes):
    """wide_codes: False (packed nibbles, the reference format) | True (int8 code*16) | "f6" (BF6 group-major)."""
    flag = L.QUANT_F6_CODES if wide_codes == "f6" else (L.QUANT_WIDE_CODES if wide_codes else 0)
    return _MODES[quant_mode] | flag


def activate_fp16_i4(a: torch.Tensor, b: torch.Tensor, *, quant_mode="kernel", clip=1.0, scale_layout="ref",
                     return_dequant=False, wide_codes=False):
    """quant(silu(a) * b) -> (o_outlier i8[bs,128], o_norms i8[bs,(H-128)/2], outlier_scales, norm_scales).
    Reference: punica/ops/__init__.py:141-156 -> run_activate_fp16_i4 (Activate.cuh:194-217).  Any H % 128 == 0
    (the reference is hard-instantiated for 11008, punica_ops.cc:76)."""
    _require_cuda_half(a, "a")
    _require_cuda_half(b, "b")
    bs, hidden_dim = a.shape
    assert b.shape == a.shape
    outs = _alloc_act_outputs(bs, hidden_dim, a.device, scale_layout, return_dequant, wide_codes)
    st = L.lib().atom_silu_mul_quant_f16(a.data_ptr(), b.data_ptr(), bs, hidden_dim, _mode(quant_mode, wide_codes), clip,
                                          _LAYOUTS[scale_layout], outs[0].data_ptr(), outs[1].data_ptr(),
                                          outs[2].data_ptr(), outs[3].data_ptr(), L.ptr(outs[4]),
                                          L.current_stream(a.device))
    L.check(st, "atom_silu_mul_quant_f16")
    return _ret(*outs)


def rmsnorm_fp16_i4(hidden_states: torch.Tensor, weight: torch.Tensor, reorder_index: torch.Tensor, eps: float, *,
                    quant_mode="kernel", clip=1.0, scale_layout="ref", return_dequant=False, wide_codes=False):
    """quant(index_select(RMSNorm(x)*w, reorder_index)).  Reference: punica/ops/__init__.py:183-200 ->
    run_rmsnorm_fp16_i4 (RMSNorm.cuh:255-285).  reorder_index is int16 [H] as in the reference."""
    _require_cuda_half(hidden_states, "hidden_states")
    _require_cuda_half(weight, "weight")
    assert reorder_index.dtype == torch.int16 and reorder_index.is_cuda
    bs, hidden_dim = hidden_states.shape
    outs = _alloc_act_outputs(bs, hidden_dim, hidden_states.device, scale_layout, return_dequant, wide_codes)
    st = L.lib().atom_rmsnorm_reorder_quant_f16(hidden_states.data_ptr(), weight.data_ptr(), float(eps),
                                                 reorder_index.data_ptr(), bs, hidden_dim,
                                                 _mode(quant_mode, wide_codes), clip,
                                                 _LAYOUTS[scale_layout], outs[0].data_ptr(), outs[1].data_ptr(),
                                                 outs[2].data_ptr(), outs[3].data_ptr(), L.ptr(outs[4]),
                                                 L.current_stream(hidden_states.device))
    L.check(st, "atom_rmsnorm_reorder_quant_f16")
    return _ret(*outs)


def add_rmsnorm_fp16_i4(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, reorder_index: torch.Tensor,
                        eps: float, *, inplace=False, quant_mode="kernel", clip=1.0, scale_layout="ref",
                        return_dequant=False, wide_codes=False):
    """NEW (no reference op): s = x + residual (fp16), then rmsnorm_fp16_i4(s, ...) -- the residual add
    of the decoder layer (llama.py:266-282) fused into the following RMSNorm-quant kernel.  Returns (s, *quant outputs);
    ``inplace`` writes s over ``residual``."""
    _require_cuda_half(x, "x")
    _require_cuda_half(residual, "residual")
    _require_cuda_half(weight, "weight")
    assert x.shape == residual.shape and reorder_index.dtype == torch.int16 and reorder_index.is_cuda
    bs, hidden_dim = x.shape
    s = residual if inplace else torch.empty_like(residual)
    outs = _alloc_act_outputs(bs, hidden_dim, x.device, scale_layout, return_dequant, wide_codes)
    st = L.lib().atom_add_rmsnorm_reorder_quant_f16(x.data_ptr(), residual.data_ptr(), s.data_ptr(), weight.data_ptr(),
                                                     float(eps), reorder_index.data_ptr(), bs, hidden_dim,
                                                     _mode(quant_mode, wide_codes), clip, _LAYOUTS[scale_layout],
                                                     outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                     outs[3].data_ptr(), L.ptr(outs[4]), L.current_stream(x.device))
    L.check(st, "atom_add_rmsnorm_reorder_quant_f16")
    return (s,) + tuple(_ret(*outs))


def reorder_fp16_i4(hidden_states: torch.Tensor, reorder_index, *, quant_mode="kernel", clip=1.0,
                    scale_layout="ref", return_dequant=False, wide_codes=False):
    """quant(index_select(x, reorder_index)).  Reference: punica/ops/__init__.py:203-219 ->
    run_reorder_fp16_i4 (Reorder.cuh:205-228).  ``reorder_index=None`` quantises x in its given channel order
    (the tail of quantize_activation_wrapper, model/quant.py:187-231)."""
    _require_cuda_half(hidden_states, "hidden_states")
    if reorder_index is not None:
        assert reorder_index.dtype == torch.int16 and reorder_index.is_cuda
    bs, hidden_dim = hidden_states.shape
    outs = _alloc_act_outputs(bs, hidden_dim, hidden_states.device, scale_layout, return_dequant, wide_codes)
    st = L.lib().atom_reorder_quant_f16(hidden_states.data_ptr(), L.ptr(reorder_index), bs, hidden_dim,
                                         _mode(quant_mode, wide_codes), clip, _LAYOUTS[scale_layout], outs[0].data_ptr(),
                                         outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), L.ptr(outs[4]),
                                         L.current_stream(hidden_states.device))
    L.check(st, "atom_reorder_quant_f16")
    return _ret(*outs)


_WS = {}
_WS_RETIRED = []               # buffers replaced during a graph capture: launches captured earlier still point at them


def _workspace(device, nbytes):
    """Scratch for split-K partial sums / re-coded operands / decode partials, per (device, stream): calls on one stream reuse it
    in stream order; calls on different streams never share a buffer.  Grown on demand (the old buffer is returned to the caching
    allocator, which keeps it alive for work already queued on its stream).  During HIP-graph capture a too small buffer is not
    freed -- launches captured earlier (also of an earlier graph captured on the same stream) reference it -- but retired, and
    the new one comes out of the capturing graph's memory pool like every other tensor allocated during capture.  Nothing is ever
    expected to SURVIVE in this buffer from one call to the next (round 3 kept a weight's re-coded form at its head and trusted
    that no other call had touched it -- unsafe under graph capture, and useless for a model whose projections share the buffer)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        if t is not None and torch.cuda.is_current_stream_capturing():
            _WS_RETIRED.append(t)
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


# ---- re-coded (F6) forms of PACKED weights that meet prefill-size batches through the reference-format entry points -------------------
# A caller of the reference's operator surface hands dense_layer_gemm_i4_fp16 the packed INT4 weight on every call (llama.py:61-68).
# From 257 rows on the fastest kernels want the F6 form; re-coding the weight on every call costs as much as re-coding the activation
# (12 vs 6 us at 4096 x 4096).  So the F6 form of every weight seen here is kept -- per WEIGHT (its own tensor, nothing shares it), keyed
# by the storage addresses and version counters of the packed weight and its scales, least recently used first out under a byte cap.
# A Llama-7B's 224 projections are 5.5 GB in this form (0.84 B per weight) next to 288 GB of HBM.
#   * an entry dies with the packed weight: weakref finalizers on the storages of the weight and of its scales drop it (so a cached
#     address is never handed to another tensor while its entry lives, and deleting a model frees its BF6 forms -- rounds 3-4 held
#     strong references);
#   * the byte cap defaults to an eighth of the device's memory, at most 32 GiB (set_weight_f6_cache_bytes changes it);
#   * an entry is complete before its first use on ANY stream: the stream that re-coded the weight is synchronised once, at creation;
#   * tensors made under torch.inference_mode() have no version counter: they count as version -1 (they cannot be written in place);
#   * a weight rewritten in place bumps its version counter -> miss (writes through a `.data` / `.detach()` alias do NOT bump it:
#     call forget_weight_f6(b) after such a write);
#   * HIP-graph capture: nothing executes during capture, so an entry is never CREATED there (the call takes the workspace route and
#     re-codes both operands inside the captured graph -- always right); a HIT during capture pins the entry for good, because the
#     captured launch keeps pointing at it.
_F6W = collections.OrderedDict()      # key -> [f6s tensor, finalizers, bytes, pinned]
_F6W_STATE = {"limit": None, "bytes": 0, "hits": 0, "misses": 0}


def _f6w_limit(device):
    if _F6W_STATE["limit"] is None:
        _F6W_STATE["limit"] = min(32 << 30, torch.cuda.get_device_properties(device).total_memory // 8)
    return _F6W_STATE["limit"]


def _version_of(t):
    try:
        return t._version
    except RuntimeError:                                     # inference tensors do not track a version counter
        return -1


def _drop_f6w(key):
    e = _F6W.pop(key, None)
    if e is not None:
        _F6W_STATE["bytes"] -= e[2]
        for f in e[1]:                                       # (a no-op for the finalizer that is calling us)
            f.detach()


def set_weight_f6_cache_bytes(limit: int):
    """Byte cap of the re-coded-weight cache (0 disables it: every call re-codes both operands in the workspace)."""
    _F6W_STATE["limit"] = int(limit)
    _evict_f6w()


def clear_weight_f6_cache():
    for e in _F6W.values():
        for f in e[1]:
            f.detach()
    _F6W.clear()
    _F6W_STATE.update(bytes=0, hits=0, misses=0)


def forget_weight_f6(b: torch.Tensor, b_scale: torch.Tensor = None):
    """Drop the cached F6 form(s) of the packed weight ``b`` (after writing it through an alias that keeps the version counter --
    ``.data`` / ``.detach()`` writes, inference tensors).  Pass the weight's scale tensor as well after such a write to IT: the
    channel-pair tag of ``_pairs_flag`` lives on that tensor object and is keyed by the same version counter."""
    for key in [k for k in _F6W if k[1] == b.data_ptr() and k[0] == b.device]:
        _drop_f6w(key)
    for t in (b, b_scale):
        if t is not None and getattr(t, "_atom_pairs", None) is not None:
            try:
                del t._atom_pairs
            except AttributeError:
                pass


def _evict_f6w():
    for key in list(_F6W):
        if _F6W_STATE["limit"] is None or _F6W_STATE["bytes"] <= _F6W_STATE["limit"]:
            break
        if not _F6W[key][3]:
            for f in _F6W[key][1]:
                f.detach()
            _drop_f6w(key)


def _weight_f6s(b, b_scale, n, k):
    """The cached F6 form (codes + float32 scales, ATOM_B_F6S) of a packed weight, or None when there is none and none may be made."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = (b.device, b.data_ptr(), _version_of(b), b_scale.data_ptr(), _version_of(b_scale), n, k)
    e = _F6W.get(key)
    if e is not None:
        _F6W.move_to_end(key)
        _F6W_STATE["hits"] += 1
        if capturing:
            e[3] = True
        return e[0]
    if capturing or _f6w_limit(b.device) <= 0:
        return None
    _F6W_STATE["misses"] += 1
    g = k // GROUP_SIZE - 1
    f6 = repack_weight_f6(b.view(torch.uint8), b_scale.reshape(-1)[:g * n])      # b_scale is read flat as [G][N] whatever its shape
    nbytes = f6.atom_f6s.numel()
    if nbytes > _F6W_STATE["limit"]:
        return f6
    torch.cuda.current_stream(b.device).synchronize()        # complete before any other stream (or a graph captured later) reads it
    fin = tuple(weakref.finalize(st, _drop_f6w, key) for st in (b.untyped_storage(), b_scale.untyped_storage()))
    if not all(f.alive for f in fin):
        # a torch whose untyped_storage() hands out a fresh wrapper per call: the finalizers have fired already and the entry could
        # never be dropped -- a recycled address would then hit a stale weight.  Do not cache (the call re-codes in the workspace).
        for f in fin:
            f.detach()
        return f6
    _F6W[key] = [f6, fin, nbytes, False]
    _F6W_STATE["bytes"] += nbytes
    _evict_f6w()
    return f6


def gemm_recodes_cached(m, n, k):
    """True where a packed activation of m rows should be re-coded to BF6 for a weight [n, k] whose BF6 form is at hand (the rule of
    ATOM_WS_WEIGHT_CACHED, atom_gemm_w4a4_ws_recodes_cached in include/atom_hip.h): what modules that own their weight's BF6 form ask,
    so that it is not made a second time in this module's per-weight cache."""
    return bool(L.lib().atom_gemm_w4a4_ws_recodes_cached(int(m), int(n), int(k)))


def _gemm_dims(a, b, a_keeper, a_wide=False, b_keeper=None):
    if a_wide == "f6":                                             # [G][rows_pad][104]: sizes come from the keepers
        return a_keeper.size(0), b_keeper.size(0), a.size(0) * GROUP_SIZE + a_keeper.size(1)
    m = a.size(0)
    n = b.size(0)
    k = a.size(1) * (1 if a_wide else 2) + a_keeper.size(1)       # punica_ops.cc:228-241
    return m, n, k


def dense_layer_gemm_i4_fp16(a, b, a_scale, b_scale, a_keeper, b_keeper, a_keeper_scale, b_keeper_scale, *,
                             scale_layout="ref", a_wide=False):
    """d[M,N] fp16 = W4A4 group-128 GEMM + INT8 keeper.  Reference: punica/ops/__init__.py:159-167 ->
    DenseLayerGEMM_i4<nv_half> (DenseLayerGEMM_i4.cu:722-791).  b_scale is read flat as [G][N] and b_keeper_scale
    as [N], exactly like the reference kernel (Dense_layer_gemm_i4_o16.cuh:497), whatever the tensor's shape."""
    for t in (a, b, a_scale, b_scale, a_keeper, b_keeper, a_keeper_scale, b_keeper_scale):
        if not t.is_cuda:
            raise L.AtomHipError("all GEMM operands must live on the GPU: no CPU fallback")
    m, n, k = _gemm_dims(a, b, a_keeper, a_wide, b_keeper)
    if a_wide == "f6":
        assert a.shape == (k // GROUP_SIZE - 1, f6_rows(m), L.F6_PITCH) and b.shape == (a.shape[0], f6_rows(n), L.F6_PITCH)
    d = torch.empty((m, n), dtype=torch.float16, device=a.device)
    lib = L.lib()
    # > 0 for skinny shapes that gain from split-K, and for packed operands of prefill size (re-coded to F6 in the workspace);
    # operands that are F6 already need none (the F6 kernels take no workspace)
    ws_bytes = lib.atom_gemm_w4a4_workspace_bytes(m, n, k) if not (a_wide == "f6" or (a_wide and m >= 2048)) else 0
    # packed operands of prefill size (the re-coding route): with the weight's F6 form cached (per weight, _weight_f6s) only the
    # activation is re-coded, into a fresh tensor, and the F6 kernel runs on the two -- the kernel and the bits of the workspace route
    # (with the weight's BF6 form cached the route starts at 129 rows, and at 17 where the decode-batch kernel does not take the shape
    # -- only the activation is re-coded and the mid-size-batch BF6 kernel beats what runs otherwise: ATOM_WS_WEIGHT_CACHED's rule,
    # atom_gemm_w4a4_ws_recodes_cached in include/atom_hip.h)
    if ws_bytes and not a_wide and lib.atom_gemm_w4a4_ws_recodes_cached(m, n, k):
        f6w = _weight_f6s(b, b_scale, n, k)
        if f6w is not None:
            a6 = repack_act_f6(a.view(torch.uint8), a_scale, scale_layout=scale_layout)
            return dense_layer_gemm_i4_fp16(a6, f6w, a_scale, b_scale, a_keeper, b_keeper, a_keeper_scale, b_keeper_scale,
                                            scale_layout=scale_layout, a_wide="f6")
    ws = _workspace(a.device, ws_bytes) if ws_bytes else None
    st = lib.atom_gemm_w4a4_f16_ws(a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(),
                                   a_keeper.data_ptr(), b_keeper.data_ptr(), a_keeper_scale.data_ptr(),
                                   b_keeper_scale.data_ptr(), d.data_ptr(), m, n, k, GROUP_SIZE, GROUP_SIZE,
                                   _LAYOUTS[scale_layout] | (L.AB_F6 if a_wide == "f6" else (L.A_WIDE if a_wide else 0))
                                   | (L.B_F6S if a_wide == "f6" and getattr(b, "atom_f6s", None) is not None else 0)
                                   | (L.B_SCALE_PAIRS if (getattr(b, "atom_pairs", False) if a_wide == "f6" else _pairs_flag(b_scale, n)) else 0),
                                   L.ptr(ws), ws_bytes,
                                   L.current_stream(a.device))
    L.check(st, "atom_gemm_w4a4_f16_ws")
    return d


def dense_layer_gemm_i4_o4(a, b, a_scale, b_scale, a_keeper, b_keeper, a_keeper_scale, b_keeper_scale, *,
                           scale_layout="ref", use_workspace=True, ref_extrema=False):
    """Same GEMM, output asymmetric-quantised to u4 per 128-column group: (d u8[M,N/2], d_scale f16[M,N/128*2]).
    Reference: punica/ops/__init__.py:170-180 -> DenseLayerGEMM_i4_o4 (DenseLayerGEMM_i4_o4.cu:808-856).
    Decode batches (the shapes of the decode-batch GEMM) go through atom_gemm_w4a4_o4_ws with the cached workspace (weight-streaming kernel + u4
    epilogue launch); ``use_workspace=False`` forces the tile kernel.  ``ref_extrema=True``: the epilogue exactly as the reference
    CODE computes it (extrema of |x|, 4-bit wrap instead of a clamp: ATOM_O4_REF_EXTREMA in include/atom_hip.h)."""
    m, n, k = _gemm_dims(a, b, a_keeper)
    assert n % 128 == 0
    d = torch.empty((m, n // 2), dtype=torch.uint8, device=a.device)
    d_scale = torch.empty((m, n // 128 * 2), dtype=torch.float16, device=a.device)
    lib = L.lib()
    ws_bytes = lib.atom_gemm_w4a4_o4_workspace_bytes(m, n, k) if use_workspace else 0
    ws = _workspace(a.device, ws_bytes) if ws_bytes else None
    st = lib.atom_gemm_w4a4_o4_ws(a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(),
                                  a_keeper.data_ptr(), b_keeper.data_ptr(), a_keeper_scale.data_ptr(),
                                  b_keeper_scale.data_ptr(), d.data_ptr(), d_scale.data_ptr(), m, n, k, GROUP_SIZE,
                                  GROUP_SIZE, _LAYOUTS[scale_layout] | (L.O4_REF_EXTREMA if ref_extrema else 0), L.ptr(ws), ws_bytes,
                                  L.current_stream(a.device))
    L.check(st, "atom_gemm_w4a4_o4_ws")
    return d, d_scale


def decode_gemm_fits(m: int, n: int, k: int) -> bool:
    """True when (m, n, k) is a shape the decode-batch GEMM takes, i.e. dense_layer_gemm_i4_f32 is available."""
    return m >= 1 and n % 128 == 0 and L.lib().atom_gemm_w4a4_o4_workspace_bytes(m, n, k) > 0


def dense_layer_gemm_i4_f32(a, b, a_scale, b_scale, a_keeper, b_keeper, a_keeper_scale, b_keeper_scale, *,
                            scale_layout="ref"):
    """NEW (no reference counterpart): the FP32 sums of the GEMM, float [M, N], for decode batches (decode_gemm_fits) --
    what the u4 epilogue quantises; feeds quant_append_kv_i4."""
    m, n, k = _gemm_dims(a, b, a_keeper)
    d = torch.empty((m, n), dtype=torch.float32, device=a.device)
    st = L.lib().atom_gemm_w4a4_f32(a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(),
                                    a_keeper.data_ptr(), b_keeper.data_ptr(), a_keeper_scale.data_ptr(),
                                    b_keeper_scale.data_ptr(), d.data_ptr(), m, n, k, GROUP_SIZE, GROUP_SIZE,
                                    _LAYOUTS[scale_layout], L.current_stream(a.device))
    L.check(st, "atom_gemm_w4a4_f32")
    return d


def fuse_projection_weights(mods):
    """Offline, once per layer: the packed weights of 2-3 ``LinearInt4`` modules that read the same activation (q / k / v; gate /
    up) as ONE operand for dense_layer_gemm_i4_multi, concatenated along the output features.  The codes are not duplicated: the
    modules' ``weight_int4`` / ``weight_int8`` parameters become views of the fused buffers (a later in-place load writes through;
    a re-assigned parameter changes the key and the operand is rebuilt; serialisers that refuse tensors sharing storage, e.g.
    safetensors' save_file, want ``.clone()``d parameters).  The scales (31 x N halves per projection) are copied.
    Returns a dict; ``fused_key(mods)`` tells whether it is current."""
    packs = [m.packed() for m in mods]
    n = packs[0][0].shape[0]
    assert all(pk[0].shape == packs[0][0].shape for pk in packs) and n % 16 == 0
    b4 = torch.cat([pk[0].view(torch.uint8) for pk in packs], 0).contiguous()
    b8 = torch.cat([pk[1] for pk in packs], 0).contiguous()
    g = packs[0][2].shape[0]
    sb = torch.cat([pk[2].reshape(g, n) for pk in packs], 1).contiguous()
    sb8 = torch.cat([pk[3].reshape(-1) for pk in packs], 0).contiguous()
    for i, m in enumerate(mods):                                   # the parameters now alias the fused storage
        m.weight_int4.data = b4[i * n:(i + 1) * n]
        m.weight_int8.data = b8[i * n:(i + 1) * n]
    return {"b4": b4, "b8": b8, "sb": sb, "sb8": sb8, "n_seg": n, "nseg": len(mods), "k": b4.shape[1] * 2 + GROUP_SIZE,
            "key": fused_key(mods)}


def fused_key(mods):
    return tuple((m.weight_int4.data_ptr(), m.weight_int4._version, m.weight_int8.data_ptr(), m.weight_int8._version,
                  m.scale_int4.data_ptr(), m.scale_int4._version, m.scale_int8.data_ptr(), m.scale_int8._version) for m in mods)


def multi_gemm_fits(m: int, n_seg: int, nseg: int, k: int) -> bool:
    return bool(L.lib().atom_gemm_w4a4_multi_fits(int(m), int(n_seg), int(nseg), int(k)))


def dense_layer_gemm_i4_multi(a, a_scale, a_keeper, a_keeper_scale, fused, *, f32_mask=0, add=None, scale_layout="ref"):
    """NEW (decode batches; no reference counterpart): the projections in ``fused`` (fuse_projection_weights) applied to one
    activation operand in ONE launch.  Returns a tuple of [M, n_seg] tensors, fp16 or (bits of ``f32_mask``) the FP32 sums;
    ``add`` (fp16 [M, n_seg]) is added to the first output the way torch adds two half tensors (the residual add).  Bit-identical to
    dense_layer_gemm_i4_f32 / the decode-batch kernel per projection (+ torch's add)."""
    m = a.size(0)
    n, nseg, k = fused["n_seg"], fused["nseg"], fused["k"]
    assert a.size(1) * 2 + a_keeper.size(1) == k
    outs = [torch.empty((m, n), dtype=torch.float32 if (f32_mask >> i) & 1 else torch.float16, device=a.device) for i in range(nseg)]
    if add is not None:
        _require_cuda_half(add, "add")
        assert add.shape == (m, n) and add.is_contiguous()
    st = L.lib().atom_gemm_w4a4_multi(a.data_ptr(), fused["b4"].data_ptr(), a_scale.data_ptr(), fused["sb"].data_ptr(), a_keeper.data_ptr(),
                                      fused["b8"].data_ptr(), a_keeper_scale.data_ptr(), fused["sb8"].data_ptr(), outs[0].data_ptr(),
                                      outs[1].data_ptr() if nseg > 1 else None, outs[2].data_ptr() if nseg > 2 else None,
                                      int(f32_mask), L.ptr(add), m, n, nseg, k, GROUP_SIZE, GROUP_SIZE, _LAYOUTS[scale_layout],
                                      L.current_stream(a.device))
    L.check(st, "atom_gemm_w4a4_multi")
    return tuple(outs)


_Q_OPS = {"reorder": L.Q_REORDER, "rmsnorm": L.Q_RMSNORM, "add_rmsnorm": L.Q_ADD_RMSNORM, "silu_mul": L.Q_SILU_MUL}


def multi_q_gemm_fits(q_op: str, m: int, n_seg: int, nseg: int, k: int) -> bool:
    """True when dense_layer_gemm_i4_multi_q(q_op, ...) takes the shape (the launcher's own predicate)."""
    return bool(L.lib().atom_gemm_w4a4_multi_q_fits(_Q_OPS[q_op], int(m), int(n_seg), int(nseg), int(k)))


def dense_layer_gemm_i4_multi_q(q_op: str, x, fused, *, x2=None, residual=None, reorder_index=None, eps=0.0, clip=1.0, f32_mask=0, add=None):
    """NEW (decode steps of one or two tokens; no reference counterpart): dense_layer_gemm_i4_multi with the quantiser that precedes
    it in the reference's call order INSIDE the launch -- ``q_op`` "reorder" (reorder_fp16_i4), "rmsnorm" (rmsnorm_fp16_i4, ``x2`` = the
    norm weight), "add_rmsnorm" (add_rmsnorm_fp16_i4: returns x + residual as well) or "silu_mul" (activate_fp16_i4, ``x2`` = the second
    factor); kernel-flavoured quantiser arithmetic.  ``x`` fp16 [M, K].  Returns (outs, residual_out).  The quantised operand is
    bit-identical to the quantiser op's, and the GEMM behind it sums in the order the SEPARATE entry points use for the token count
    (atom_gemm_w4a4_packed_order): the dot-product kernel's (64) for one token and for two with K > 4096 -- round 6, csrc/gemvq_w4a4.hip:
    one quantiser per CU in front of that kernel -- and the decode-batch kernel's (8) for two tokens with K <= 4096.  The outputs are
    therefore bit-identical to quantiser op + dense_layer_gemm_i4_multi throughout (tests/test_gpu_e2e.py); rounds 3-5 always ran the
    decode-batch kernel and were one fp16 ulp off where the separate path took the dot-product kernel."""
    _require_cuda_half(x, "x")
    code = _Q_OPS[q_op]
    m = x.size(0)
    n, nseg, k = fused["n_seg"], fused["nseg"], fused["k"]
    assert x.shape == (m, k) and x.is_contiguous()
    outs = [torch.empty((m, n), dtype=torch.float32 if (f32_mask >> i) & 1 else torch.float16, device=x.device) for i in range(nseg)]
    res_out = None
    if code == L.Q_ADD_RMSNORM:
        _require_cuda_half(residual, "residual")
        assert residual.shape == x.shape and residual.is_contiguous()
        res_out = torch.empty_like(x)                    # (never in place: every workgroup reads the residual, one writes the sum)
    if x2 is not None:
        _require_cuda_half(x2, "x2")
        assert x2.is_contiguous() and (x2.shape == x.shape if code == L.Q_SILU_MUL else x2.numel() == k)
    if reorder_index is not None:
        assert reorder_index.dtype == torch.int16 and reorder_index.numel() == k and reorder_index.is_cuda
    if add is not None:
        _require_cuda_half(add, "add")
        assert add.shape == (m, n) and add.is_contiguous()
    st = L.lib().atom_gemm_w4a4_multi_q(code, x.data_ptr(), L.ptr(x2), L.ptr(residual), L.ptr(res_out), L.ptr(reorder_index), float(eps),
                                        float(clip), fused["b4"].data_ptr(), fused["sb"].data_ptr(), fused["b8"].data_ptr(),
                                        fused["sb8"].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if nseg > 1 else None,
                                        outs[2].data_ptr() if nseg > 2 else None, int(f32_mask), L.ptr(add), m, n, nseg, k,
                                        GROUP_SIZE, GROUP_SIZE, L.current_stream(x.device))
    L.check(st, "atom_gemm_w4a4_multi_q")
    return tuple(outs), res_out


def merge_q_gemm_fits(m: int, n_seg: int, nseg: int, k: int, splits: int) -> bool:
    """True when dense_layer_gemm_i4_merge_q takes the shape and the KV-split count (atom_gemm_w4a4_multi_merge_q_fits)."""
    return bool(L.lib().atom_gemm_w4a4_multi_merge_q_fits(int(m), int(n_seg), int(nseg), int(k), int(splits)))


def dense_layer_gemm_i4_merge_q(partials: torch.Tensor, splits: int, fused, *, reorder_index=None, clip=1.0, f32_mask=0, add=None):
    """NEW (round 6; decode steps of one or two tokens, no reference counterpart): dense_layer_gemm_i4_multi_q("reorder", ...) on the
    decode attention's output while that is still in KV-split form -- ``partials`` float32 [M, heads, splits, 130] as
    ``batch_decode_i4(..., merge=False)`` returns it --, the split merge running in front of the reorder quantiser inside the
    projection's launch.  Bit-identical to batch_decode_i4 (merged) -> dense_layer_gemm_i4_multi_q("reorder", ...).  Returns outs."""
    if not partials.is_cuda:
        raise L.AtomHipError("merge_q needs GPU tensors: no CPU fallback")
    n, nseg, k = fused["n_seg"], fused["nseg"], fused["k"]
    m = partials.size(0)
    assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.shape == (m, k // 128, splits, 130)
    outs = [torch.empty((m, n), dtype=torch.float32 if (f32_mask >> i) & 1 else torch.float16, device=partials.device) for i in range(nseg)]
    if reorder_index is not None:
        assert reorder_index.dtype == torch.int16 and reorder_index.numel() == k and reorder_index.is_cuda
    if add is not None:
        _require_cuda_half(add, "add")
        assert add.shape == (m, n) and add.is_contiguous()
    st = L.lib().atom_gemm_w4a4_multi_merge_q(partials.data_ptr(), int(splits), L.ptr(reorder_index), float(clip), fused["b4"].data_ptr(),
                                              fused["sb"].data_ptr(), fused["b8"].data_ptr(), fused["sb8"].data_ptr(), outs[0].data_ptr(),
                                              outs[1].data_ptr() if nseg > 1 else None, outs[2].data_ptr() if nseg > 2 else None,
                                              int(f32_mask), L.ptr(add), m, n, nseg, k, GROUP_SIZE, GROUP_SIZE,
                                              L.current_stream(partials.device))
    L.check(st, "atom_gemm_w4a4_multi_merge_q")
    return tuple(outs)


def quant_weight_w4(weight: torch.Tensor, w_clip: float = 0.85, channel_group: int = 2, return_fake_quant=False):
    """NEW (no reference counterpart): quantise + pack a (column-reordered) FP16 weight [N,K] the
    way QLinearLayer.quant does (qLinearLayer.py:42-78).  Returns (B4 u8[N,K4/2], B8 i8[N,128], sB f16[G,N],
    sB8 f16[N][, Wq f16[N,K]])."""
    _require_cuda_half(weight, "weight")
    n, k = weight.shape
    dev = weight.device
    b4 = torch.empty((n, (k - GROUP_SIZE) // 2), dtype=torch.uint8, device=dev)
    b8 = torch.empty((n, GROUP_SIZE), dtype=torch.int8, device=dev)
    sb = torch.empty(((k - GROUP_SIZE) // GROUP_SIZE, n), dtype=torch.float16, device=dev)
    sb8 = torch.empty((n,), dtype=torch.float16, device=dev)
    wq = torch.empty_like(weight) if return_fake_quant else None
    st = L.lib().atom_quant_weight_w4(weight.data_ptr(), n, k, float(w_clip), int(channel_group), b4.data_ptr(),
                                       b8.data_ptr(), sb.data_ptr(), sb8.data_ptr(), L.ptr(wq),
                                       L.current_stream(dev))
    L.check(st, "atom_quant_weight_w4")
    return (b4, b8, sb, sb8, wq) if return_fake_quant else (b4, b8, sb, sb8)


def pack_weight_w4(weight_fq: torch.Tensor, channel_group: int = 2, strict: bool = True):
    """NEW: pack an ALREADY fake-quantised FP16 weight [N,K] -- the tensor GPTQ assigns to
    ``layer.weight.data`` (gptq.py:331) or ``QLinearLayer.quant`` leaves behind -- by recovering codes and fp16 scales.
    Returns (B4, B8, sB, sB8, bad) with ``bad`` = number of (channel_group x 128) blocks that are on no INT4/INT8 grid;
    ``strict`` raises when bad != 0 (costs one device->host sync; this is an offline op)."""
    _require_cuda_half(weight_fq, "weight_fq")
    n, k = weight_fq.shape
    dev = weight_fq.device
    w = weight_fq.contiguous()
    b4 = torch.empty((n, (k - GROUP_SIZE) // 2), dtype=torch.uint8, device=dev)
    b8 = torch.empty((n, GROUP_SIZE), dtype=torch.int8, device=dev)
    sb = torch.empty(((k - GROUP_SIZE) // GROUP_SIZE, n), dtype=torch.float16, device=dev)
    sb8 = torch.empty((n,), dtype=torch.float16, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    st = L.lib().atom_pack_weight_w4(w.data_ptr(), n, k, int(channel_group), b4.data_ptr(), b8.data_ptr(),
                                      sb.data_ptr(), sb8.data_ptr(), bad.data_ptr(), L.current_stream(dev))
    L.check(st, "atom_pack_weight_w4")
    nbad = int(bad.item())
    if strict and nbad:
        raise L.AtomHipError(f"pack_weight_w4: {nbad} weight blocks are not INT4-g128/INT8 fake-quantised values")
    return b4, b8, sb, sb8, nbad


# ------------------------------------------------------------------------------------------------ INT4 paged KV cache
def _kv_dims(kv):
    _c, num_layers, _2, num_heads, page_size, half_dim = kv.data.shape
    return num_layers, num_heads, page_size, half_dim * 2


def _require_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise L.AtomHipError("KV-cache operands must live on the GPU: no CPU fallback")


def _kv_args(kv, layer_idx, num_qo_heads=None):
    """The cache as every C entry point takes it: its five pointers; (batch, layers, layer, [query heads: the grouped-query entries,]
    K/V heads, page size, head dim); the host's bound of a sequence's pages (0: unknown -- no KV split)."""
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    ptrs = tuple(t.data_ptr() for t in (kv.data, kv.param, kv.indptr, kv.indicies, kv.last_page_offset))
    heads = (num_heads,) if num_qo_heads is None else (num_qo_heads, num_heads)
    dims = (kv.last_page_offset.numel(), num_layers, int(layer_idx)) + heads + (page_size, head_dim)
    return ptrs, dims, int(getattr(kv, "max_pages", 0))


def _kv_append(kv, k, v, k_param, v_param, append_indptr, layer_idx, what):
    _require_cuda(kv.data, kv.param, k, v, k_param, v_param)
    ptrs, dims, _ = _kv_args(kv, layer_idx)
    num_heads, head_dim = dims[3], dims[5]
    total = k.size(0)
    assert k.shape == v.shape == (total, num_heads, head_dim // 2) and k.dtype == v.dtype == torch.uint8
    assert k_param.numel() == v_param.numel() == total * num_heads * 2 and k_param.dtype == torch.float16
    st = L.lib().atom_kv_append_i4(*ptrs, k.contiguous().data_ptr(), v.contiguous().data_ptr(), k_param.contiguous().data_ptr(),
                                    v_param.contiguous().data_ptr(), L.ptr(append_indptr), total, *dims, L.current_stream(k.device))
    L.check(st, what)


def init_kv_i4(kv, k, v, k_param, v_param, seqlen_indptr, layer_idx: int):
    """Write the prefill tokens' quantised K/V into the pages.  Reference: punica/ops/__init__.py:33-45 ->
    FlashInferInitKvKernel_i4.  k, v uint8 [sum(len), heads, 64]; k_param, v_param fp16 [sum(len), heads, 2];
    seqlen_indptr int32 [batch+1]."""
    assert seqlen_indptr.dtype == torch.int32 and seqlen_indptr.is_cuda
    _kv_append(kv, k, v, k_param, v_param, seqlen_indptr, layer_idx, "atom_kv_append_i4 (init)")


def append_kv_i4(kv, k, v, k_param, v_param, layer_idx: int):
    """Append ONE token per sequence.  Reference: punica/ops/__init__.py:48-59 -> FlashInferAppendKvKernel_i4."""
    _kv_append(kv, k, v, k_param, v_param, None, layer_idx, "atom_kv_append_i4")


def _require_kv_f32(kv, k_f32, v_f32):
    """this step's FP32 k / v projections [batch, heads * 128] of the fused appends"""
    _require_cuda(k_f32, v_f32)
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    for t in (k_f32, v_f32):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (kv.last_page_offset.numel(), num_heads * head_dim)


def quant_append_kv_i4(kv, k_f32: torch.Tensor, v_f32: torch.Tensor, layer_idx: int):
    """NEW (fused decode step): quantise the FP32 k / v projections [batch, heads*128] per head (the _o4 epilogue) and
    append them as the last token of every sequence.  Same cache contents as dense_layer_gemm_i4_o4 + append_kv_i4."""
    _require_kv_f32(kv, k_f32, v_f32)
    ptrs, dims, _ = _kv_args(kv, layer_idx)
    st = L.lib().atom_kv_quant_append_f32(*ptrs, k_f32.data_ptr(), v_f32.data_ptr(), *dims, L.current_stream(k_f32.device))
    L.check(st, "atom_kv_quant_append_f32")


def _kv_step_tables(kv):
    """the seven device tables of a static cache as atom_kv_step_i4 / atom_kv_step_rows_i4 take them, checked: (tensors, batch, cap)"""
    tensors = (kv.page_table, kv.row_pages, kv.lengths, kv.indptr, kv.indicies, kv.last_page_offset, kv.state)
    for t in tensors:
        if not t.is_cuda:
            raise L.AtomHipError("KV-cache page tables must live on the GPU: no CPU fallback")
        assert t.dtype == torch.int32 and t.is_contiguous()
    batch, cap = kv.page_table.shape
    assert kv.row_pages.numel() == batch and kv.lengths.numel() == 2 * batch and kv.indptr.numel() == batch + 1
    assert kv.indicies.numel() == batch * cap and kv.last_page_offset.numel() == batch and kv.state.numel() == 4
    return tensors, batch, cap


def kv_step_i4(kv, add: int = 1):
    """NEW (page tables stepped on the device): every sequence of a utils.StaticBatchedKvCacheInt4 gains ``add`` tokens (0: none) and
    its ``indptr`` / ``indicies`` / ``last_page_offset`` are rebuilt in place from its padded page table (atom_kv_step_i4) -- one
    launch on the current stream, no host synchronisation, capturable.  A sequence that would outgrow its reserved pages keeps its
    length and sets the cache's status word (read by ``kv.sync_host()``)."""
    tensors, batch, cap = _kv_step_tables(kv)
    st = L.lib().atom_kv_step_i4(*(t.data_ptr() for t in tensors), batch, cap, kv.page_size, int(add),
                                  L.current_stream(kv.page_table.device))
    L.check(st, "atom_kv_step_i4")


def kv_step_rows_i4(kv, adds: torch.Tensor, lookahead: int = 0):
    """NEW (speculative decoding): ``kv_step_i4`` with a count per sequence -- ``adds`` int32 [batch] on the device, read by the launch --
    and ``lookahead`` >= 0 tentative slots (atom_kv_step_rows_i4).  The length a sequence keeps is ``len + adds[b]``; its tables are
    built for ``lookahead`` tokens more, so a verify step can write and attend to K + 1 tokens of which the next call commits only the
    accepted ones.  A negative count is taken as 0 and flagged; a sequence whose ``len + adds[b] + lookahead`` outgrows its reserved
    pages keeps its length and its tables (the cache's status word, read by ``kv.sync_host()``).  One launch, no host synchronisation,
    capturable."""
    tensors, batch, cap = _kv_step_tables(kv)
    if not adds.is_cuda:
        raise L.AtomHipError("adds must live on the GPU: no CPU fallback")
    if not (adds.dtype == torch.int32 and adds.shape == (batch,) and adds.is_contiguous()):
        raise TypeError(f"adds must be a contiguous int32 tensor of [{batch}], got {adds.dtype} {tuple(adds.shape)}")
    if int(lookahead) < 0:
        raise ValueError(f"lookahead must be non-negative, got {lookahead}")
    st = L.lib().atom_kv_step_rows_i4(*(t.data_ptr() for t in tensors), batch, cap, kv.page_size, adds.data_ptr(), int(lookahead),
                                       L.current_stream(kv.page_table.device))
    L.check(st, "atom_kv_step_rows_i4")


def kv_step_ring_i4(kv, add: int = 1):
    """NEW (rolling cache of a sliding-window model): ``kv_step_i4`` for a utils.RollingKvCacheInt4, whose page-table rows are RINGS --
    logical page g of a sequence lives in slot g % row_pages (atom_kv_step_ring_i4).  Every sequence gains ``add`` tokens; its tables
    list the pages that the step's new rows still see under ``kv.window``, in logical order, and ``kv.kv_start`` receives the position
    of each list's first token (what the attention ops then read).  The slot of the new last page is one whose previous tenant fell
    behind the window.  A sequence whose live pages would outnumber its ring keeps its length and sets the cache's status word.  One
    launch on the current stream, no host synchronisation, capturable."""
    tensors, batch, cap = _kv_step_tables(kv)
    start = kv.kv_start
    if not start.is_cuda:
        raise L.AtomHipError("KV-cache page tables must live on the GPU: no CPU fallback")
    assert start.dtype == torch.int32 and start.is_contiguous() and start.numel() == batch
    st = L.lib().atom_kv_step_ring_i4(*(t.data_ptr() for t in tensors), batch, cap, kv.page_size, int(add), int(kv.window),
                                       start.data_ptr(), L.current_stream(kv.page_table.device))
    L.check(st, "atom_kv_step_ring_i4")


def _ring_start(kv, window):
    """``kv.kv_start`` of a rolling cache (utils.RollingKvCacheInt4) for a call with ``window`` -- the call then takes the _ring entry
    points --, None for every other cache.  A rolling cache has released the pages behind ITS window: an un-windowed call, or one with
    a wider window, would silently read a truncated history and is refused."""
    start = getattr(kv, "kv_start", None)
    if start is None:
        return None
    if window is None or window > kv.window:
        raise ValueError(f"a rolling cache serves only windowed calls no wider than its own window ({kv.window}), got window={window!r}: "
                         f"the pages behind that window are released")
    return start


def _qo_heads(num_qo_heads: int, num_kv_heads: int) -> int:
    """grouped-query attention: query head h reads the cache's K/V head h // G -- the query head count must be a multiple of the cache's"""
    if num_qo_heads < 1 or num_qo_heads % num_kv_heads:
        raise ValueError(f"{num_qo_heads} query heads on a cache of {num_kv_heads} K/V heads: not a multiple (grouped-query attention)")
    return num_qo_heads


def _window_arg(window):
    """``window=`` of the attention ops, checked: None, or an int >= 1"""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"window must be None or an int >= 1 (keys p - window < j <= p), got {window!r}")
    return window


def decode_splits(batch: int, kv, num_qo_heads: int = None, window: int = None) -> int:
    """How many partial states per (sequence, head) batch_decode_i4 produces for this cache (1: none; small batches: one per workgroup of
    four KV-split waves).  ``num_qo_heads``: the query heads of a grouped-query call (default: the cache's head count).  ``window``:
    of the sliding-window call (atom_batch_decode_gqa_i4_win_splits, the grouped-query plan at every head ratio; on a rolling cache
    atom_batch_decode_gqa_i4_ring_splits, and a call without a window or with one wider than the cache's is a ``ValueError``)."""
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    max_pages = int(getattr(kv, "max_pages", 0))
    ring = _ring_start(kv, _window_arg(window)) is not None
    if _window_arg(window) is not None:
        nq = num_heads if num_qo_heads is None else _qo_heads(int(num_qo_heads), num_heads)
        query = L.lib().atom_batch_decode_gqa_i4_ring_splits if ring else L.lib().atom_batch_decode_gqa_i4_win_splits
        return int(query(int(batch), nq, num_heads, page_size, max_pages, window))
    if num_qo_heads is None or num_qo_heads == num_heads:
        return int(L.lib().atom_batch_decode_i4_splits(int(batch), num_heads, page_size, max_pages))
    nq = _qo_heads(int(num_qo_heads), num_heads)
    return int(L.lib().atom_batch_decode_gqa_i4_splits(int(batch), nq, num_heads, page_size, max_pages))


def _decode_outputs(q, merge, ws_bytes, splits):
    """(o, workspace, what the op returns) of a decode call.  merge=False: no `o`; the partial states go to a tensor of their own"""
    if merge:
        o = torch.empty_like(q)
        return o, (_workspace(q.device, ws_bytes) if ws_bytes else None), o
    batch, heads = q.shape[:2]
    assert splits >= 2 and ws_bytes == batch * heads * splits * 130 * 4, "merge=False needs a split KV range (decode_splits)"
    part = torch.empty((batch, heads, splits, 130), dtype=torch.float32, device=q.device)
    return None, part, part


def rope_table(inv_freq, device) -> torch.Tensor:
    """The per-pair frequency table of ``batch_decode_i4`` / ``batch_prefill_i4`` (``rope_table=``) from HF-style ``inv_freq`` -- 64
    values in RADIANS per position, pair i = dims (i, i + 64): divided by 2 pi in float64 and rounded ONCE to fp32, on ``device``.  The
    kernels work in revolutions and use the table as loaded, so the fp32 values returned here are the definition of the angles."""
    import numpy as np
    f = inv_freq.detach().cpu().numpy() if isinstance(inv_freq, torch.Tensor) else inv_freq
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    if f.shape != (64,):
        raise ValueError(f"inv_freq must hold 64 values (head_dim 128), got {f.shape[0]}")
    return torch.from_numpy((f / (2.0 * np.pi)).astype(np.float32)).to(device)


def _rope_args(rope_table, attn_scale, device):
    """(rope_table pointer or None, attn_scale) of the _rope entry points, checked; None where both are at their defaults (the call
    then goes to the entry point without them)"""
    if rope_table is None and isinstance(attn_scale, (int, float)) and float(attn_scale) == 1.0:
        return None
    if rope_table is not None:
        t = rope_table
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.shape == (64,) and t.is_contiguous()):
            what = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise TypeError(f"rope_table must be a contiguous float32 CUDA tensor of [64] (ops.rope_table), got {what}")
        if t.device != device:
            raise TypeError(f"rope_table lives on {t.device}, q on {device}")
    return (None if rope_table is None else rope_table.data_ptr()), float(attn_scale)


def batch_decode_i4(q: torch.Tensor, kv, layer_idx: int, *, rope_theta: float = 1e4, rope_scale: float = 1.0, append_kv=None, merge=True,
                    rope_table: torch.Tensor = None, attn_scale: float = 1.0, window: int = None):
    """Decode attention over the INT4 paged cache, RoPE fused.  Reference: punica/ops/__init__.py:21-30 ->
    FlashInferBatchDecodeKernel_i4 (rope_theta 1e4, rope_scale 1 hard-coded there).  q fp16 [batch, heads, 128].
    ``append_kv=(k_f32, v_f32)`` (round 6): quant_append_kv_i4 of this step's FP32 k / v projections inside the same launch
    (atom_batch_decode_append_i4) -- same cache contents, same output, one launch fewer.
    ``merge=False`` (only where decode_splits(batch, kv) >= 2): no merge launch -- returns the split partial states float32
    [batch, heads, splits, 130] (a tensor of their own, not the shared workspace) for dense_layer_gemm_i4_merge_q.
    Grouped-query attention: q may hold any multiple G of the cache's heads (query head h reads K/V head h // G); then the GQA op
    (atom_batch_decode_gqa_i4: each K/V tile read once per group, the prefill op's fp16 matrix-core numerics) runs, ``merge=False``
    returns [batch, q heads, decode_splits(batch, kv, q heads), 130], and ``append_kv`` is refused (append with quant_append_kv_i4).
    ``rope_table`` (RoPE scaling: Llama 3.1 "llama3", YaRN): float32 [64] on the device from ``ops.rope_table`` -- the frequency of
    every RoPE pair, read by the launch (a fixed address under graph replay); with it ``rope_theta`` / ``rope_scale`` are ignored.
    ``attn_scale`` multiplies the logits (YaRN: attention_factor ** 2).  Both at their defaults: the entry points and bits of a call
    without them; otherwise the ``_rope`` entry points, for every form above (``append_kv=``, ``merge=False``, grouped-query).
    ``window`` (sliding-window attention): an int W >= 1 -- the query at position p sees keys p - W < j <= p, plain causal attention
    for a sequence no longer than W.  None: exactly the calls above.  With a window atom_batch_decode_gqa_i4_win runs -- the
    grouped-query (matrix-core) op at every head ratio, MHA caches included --, ``merge=False`` takes its splits from
    ``decode_splits(batch, kv, q heads, window=W)``, and ``append_kv`` is refused (the fused append lives in the FP32 decode kernel).
    A rolling cache (utils.RollingKvCacheInt4: it has a ``kv_start`` tensor) takes atom_batch_decode_gqa_i4_ring with the same
    arguments and ``kv.kv_start``: the same positions, masks and angles, read from a page list that starts at ``kv_start[b]``.
    ``window=None`` or a window wider than the cache's is a ``ValueError`` there.  Every other cache makes exactly the calls above."""
    _require_cuda_half(q, "q")
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    batch = q.size(0)
    gqa = q.dim() == 3 and q.size(1) != num_heads
    nq = _qo_heads(q.size(1), num_heads) if gqa else num_heads
    assert q.shape == (batch, nq, head_dim)
    start = _ring_start(kv, _window_arg(window))
    if start is not None:
        if append_kv is not None:
            raise ValueError("append_kv= is not built for sliding-window attention (the fused append lives in the FP32 decode kernel): "
                             "append with quant_append_kv_i4 first")
        _require_cuda(kv.data, kv.param, start)
        assert batch == kv.last_page_offset.numel() == start.numel() and start.dtype == torch.int32 and start.is_contiguous()
        ptrs, dims, max_pages = _kv_args(kv, layer_idx, nq)
        lib = L.lib()
        plan = (batch, nq, num_heads, page_size, max_pages, window)
        ws_bytes = lib.atom_batch_decode_gqa_i4_ring_workspace_bytes(*plan)
        o, ws, ret = _decode_outputs(q, merge, ws_bytes, None if merge else lib.atom_batch_decode_gqa_i4_ring_splits(*plan))
        table, scale = _rope_args(rope_table, attn_scale, q.device) or (None, 1.0)
        st = lib.atom_batch_decode_gqa_i4_ring(L.ptr(o), q.data_ptr(), *ptrs, *dims, float(rope_theta), float(rope_scale), table, scale, window,
                                               start.data_ptr(), max_pages, L.ptr(ws), ws_bytes, L.current_stream(q.device))
        L.check(st, "atom_batch_decode_gqa_i4_ring")
        return ret
    if _window_arg(window) is not None:
        if append_kv is not None:
            raise ValueError("append_kv= is not built for sliding-window attention (the fused append lives in the FP32 decode kernel): "
                             "append with quant_append_kv_i4 first")
        _require_cuda(kv.data, kv.param)
        assert batch == kv.last_page_offset.numel()
        ptrs, dims, max_pages = _kv_args(kv, layer_idx, nq)
        lib = L.lib()
        plan = (batch, nq, num_heads, page_size, max_pages, window)
        ws_bytes = lib.atom_batch_decode_gqa_i4_win_workspace_bytes(*plan)
        o, ws, ret = _decode_outputs(q, merge, ws_bytes, None if merge else lib.atom_batch_decode_gqa_i4_win_splits(*plan))
        table, scale = _rope_args(rope_table, attn_scale, q.device) or (None, 1.0)
        st = lib.atom_batch_decode_gqa_i4_win(L.ptr(o), q.data_ptr(), *ptrs, *dims, float(rope_theta), float(rope_scale), table, scale, window,
                                              max_pages, L.ptr(ws), ws_bytes, L.current_stream(q.device))
        L.check(st, "atom_batch_decode_gqa_i4_win")
        return ret
    if gqa and append_kv is not None:
        raise ValueError("append_kv= is not built for grouped-query attention: append with quant_append_kv_i4 first")
    _require_cuda(kv.data, kv.param)
    assert batch == kv.last_page_offset.numel()
    ptrs, dims, max_pages = _kv_args(kv, layer_idx, nq if gqa else None)
    lib = L.lib()
    name = "atom_batch_decode_gqa_i4" if gqa else "atom_batch_decode_i4"
    rope = _rope_args(rope_table, attn_scale, q.device)
    plan = dims[:1] + dims[3:-1] + (max_pages,)              # (batch, [query heads,] K/V heads, page size, max_pages): what the plan queries take
    ws_bytes = getattr(lib, name + "_workspace_bytes")(*plan)
    o, ws, ret = _decode_outputs(q, merge, ws_bytes, None if merge else getattr(lib, name + "_splits")(*plan))
    new_kv = ()
    if append_kv is not None:                                # (the MHA op only)
        _require_kv_f32(kv, *append_kv)
        name, new_kv = "atom_batch_decode_append_i4", tuple(t.data_ptr() for t in append_kv)
    if rope is not None:                                     # the _rope entries: the grouped-query one serves the MHA op too (G = 1)
        if name == "atom_batch_decode_i4":
            name, dims = "atom_batch_decode_gqa_i4", dims[:3] + (num_heads,) + dims[3:]
        name += "_rope"
    st = getattr(lib, name)(L.ptr(o), q.data_ptr(), *new_kv, *ptrs, *dims, float(rope_theta), float(rope_scale), *(rope or ()), max_pages,
                            L.ptr(ws), ws_bytes, L.current_stream(q.device))
    L.check(st, name)
    return ret


def batch_prefill_i4(q: torch.Tensor, qo_indptr: torch.Tensor, kv, layer_idx: int, *, rope_theta: float = 1e4, rope_scale: float = 1.0,
                     max_q_len: int = None, rope_table: torch.Tensor = None, attn_scale: float = 1.0, window: int = None):
    """Prefill / chunked-prefill attention over the INT4 paged cache, causal, RoPE fused (atom_batch_prefill_i4).  q fp16
    [T, heads, 128] (not yet rotated); qo_indptr int32 [batch + 1] on the device: sequence b's queries are rows
    qo_indptr[b] .. qo_indptr[b+1] and its LAST positions in the cache (already written there, init_kv_i4).  ``max_q_len``: host-side
    bound of every sequence's query count (default T; it sizes the grid).  No host synchronisation: capturable in a graph.  With one
    query per sequence the output is batch_decode_i4's (fp16 matrix-core operands: within rounding of it).
    Grouped-query attention: q may hold any multiple G of the cache's heads (query head h reads K/V head h // G,
    atom_batch_prefill_gqa_i4: each staged K/V tile serves the whole group).
    ``rope_table`` / ``attn_scale``: as in ``batch_decode_i4`` (atom_batch_prefill_gqa_i4_rope; both at their defaults: the call
    without them).
    ``window``: as in ``batch_decode_i4`` (atom_batch_prefill_gqa_i4_win) -- the bound of every query row from that row's own
    position; None: exactly the calls above.  A rolling cache takes atom_batch_prefill_gqa_i4_ring, as in ``batch_decode_i4``; a
    chunk there is at most the cache's ``max_add`` tokens (what ``kv.step(add)`` admits)."""
    _require_cuda_half(q, "q")
    _require_cuda(qo_indptr, kv.data, kv.param)
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    total = q.size(0)
    nq = _qo_heads(q.size(1), num_heads) if q.dim() == 3 else num_heads
    assert q.shape == (total, nq, head_dim) and q.is_contiguous()
    assert qo_indptr.dtype == torch.int32 and qo_indptr.is_contiguous()
    ptrs, dims, max_pages = _kv_args(kv, layer_idx, nq)     # the grouped-query entry: at G = 1 it IS the MHA entry (it forwards)
    batch = dims[0]
    assert qo_indptr.numel() == batch + 1
    max_q = total if max_q_len is None else int(max_q_len)
    lib = L.lib()
    start = _ring_start(kv, _window_arg(window))
    if start is not None:
        _require_cuda(start)
        assert start.numel() == batch and start.dtype == torch.int32 and start.is_contiguous()
        ws_bytes = lib.atom_batch_prefill_gqa_i4_ring_workspace_bytes(total, batch, nq, num_heads, page_size, max_q, max_pages, window)
        ws = _workspace(q.device, ws_bytes) if ws_bytes else None
        o = torch.empty_like(q)
        table, scale = _rope_args(rope_table, attn_scale, q.device) or (None, 1.0)
        st = lib.atom_batch_prefill_gqa_i4_ring(o.data_ptr(), q.data_ptr(), qo_indptr.data_ptr(), total, max_q, *ptrs, *dims, float(rope_theta),
                                                float(rope_scale), table, scale, window, start.data_ptr(), max_pages, L.ptr(ws), ws_bytes,
                                                L.current_stream(q.device))
        L.check(st, "atom_batch_prefill_gqa_i4_ring")
        return o
    if _window_arg(window) is not None:
        ws_bytes = lib.atom_batch_prefill_gqa_i4_win_workspace_bytes(total, batch, nq, num_heads, page_size, max_q, max_pages, window)
        ws = _workspace(q.device, ws_bytes) if ws_bytes else None
        o = torch.empty_like(q)
        table, scale = _rope_args(rope_table, attn_scale, q.device) or (None, 1.0)
        st = lib.atom_batch_prefill_gqa_i4_win(o.data_ptr(), q.data_ptr(), qo_indptr.data_ptr(), total, max_q, *ptrs, *dims, float(rope_theta),
                                               float(rope_scale), table, scale, window, max_pages, L.ptr(ws), ws_bytes,
                                               L.current_stream(q.device))
        L.check(st, "atom_batch_prefill_gqa_i4_win")
        return o
    ws_bytes = lib.atom_batch_prefill_gqa_i4_workspace_bytes(total, batch, nq, num_heads, page_size, max_q, max_pages)
    ws = _workspace(q.device, ws_bytes) if ws_bytes else None
    o = torch.empty_like(q)
    rope = _rope_args(rope_table, attn_scale, q.device)
    fn = lib.atom_batch_prefill_gqa_i4 if rope is None else lib.atom_batch_prefill_gqa_i4_rope
    st = fn(o.data_ptr(), q.data_ptr(), qo_indptr.data_ptr(), total, max_q, *ptrs, *dims, float(rope_theta), float(rope_scale),
            *(rope or ()), max_pages, L.ptr(ws), ws_bytes, L.current_stream(q.device))
    L.check(st, "atom_batch_prefill_i4" if nq == num_heads else "atom_batch_prefill_gqa_i4")
    return o


def kv_fake_quant(x: torch.Tensor, n_bits: int = 4, clip: float = 1.0) -> torch.Tensor:
    """Asymmetric per-head-vector fake quantisation of a [batch, heads, seq, 128] fp16 tensor (any strides over the first
    three dims) -- quantize_attn_k_wrapper / quantize_attn_v_wrapper of the reference (model/quant.py:233-257)."""
    if not x.is_cuda:
        raise L.AtomHipError("kv_fake_quant needs a GPU tensor: no CPU fallback")
    assert x.dtype == torch.float16 and x.dim() == 4 and x.shape[-1] == 128 and x.stride(-1) == 1
    b, h, s, _ = x.shape
    y = torch.empty((b, h, s, 128), dtype=torch.float16, device=x.device)
    st = L.lib().atom_kv_fake_quant_f16(x.data_ptr(), y.data_ptr(), b, h, s, x.stride(0), x.stride(1), x.stride(2),
                                         int(n_bits), float(clip), L.current_stream(x.device))
    L.check(st, "atom_kv_fake_quant_f16")
    return y


def scale_pairs_shared(b_scale: torch.Tensor, n: int) -> bool:
    """True when output channels 2j and 2j+1 share their weight scale in every group (weight_channel_group = 2 -- the only form the
    reference kernel accepts, Dense_layer_gemm_i4_o16.cuh:413-431): the GEMM is then told so (ATOM_B_SCALE_PAIRS) and forms each scale
    product once per pair.  Checked on the values (one device round trip, offline with the weight; never during graph capture)."""
    if n % 2 or torch.cuda.is_current_stream_capturing():
        return False
    s = b_scale.reshape(-1, n)
    return bool((s[:, 0::2] == s[:, 1::2]).all().item())


def _pairs_flag(b_scale: torch.Tensor, n: int) -> bool:
    """scale_pairs_shared() of a weight-scale tensor, remembered ON the tensor object together with its version counter: one device
    round trip per weight (and per in-place rewrite), none for a model's parameters afterwards -- pass the SAME tensor object every
    time (a Parameter, not a fresh ``.data`` view: the tag would die with the view and every call would pay the round trip).  False
    during graph capture for a tensor not seen before (the generic kernels are always right)."""
    tag = getattr(b_scale, "_atom_pairs", None)
    ver = _version_of(b_scale)                # (inference tensors: -1 -- they cannot be written in place)
    if tag is not None and tag[0] == ver:
        return tag[1]
    if torch.cuda.is_current_stream_capturing():
        return False
    v = scale_pairs_shared(b_scale, n)
    try:
        b_scale._atom_pairs = (ver, v)
    except AttributeError:
        pass
    return v


def repack_weight_f6(b4: torch.Tensor, b_scale: torch.Tensor = None) -> torch.Tensor:
    """Packed INT4 weights uint8 [N, K4/2] -> the F6 operand format uint8 [G][f6_rows(N)][104] (atom_repack_weight_f6).
    With the fp16 weight scales `b_scale` [G, N]: atom_repack_weight_f6s -- the returned tensor is a view of a buffer that
    carries the scales as float32 [G][f6_rows(N)] behind the codes (ATOM_B_F6S; dense_layer_gemm_i4_fp16 recognises it by the
    `atom_f6s` attribute and the 256x256 kernel then takes its weight scales from there)."""
    if not b4.is_cuda:
        raise L.AtomHipError("repack_weight_f6 needs a GPU tensor: no CPU fallback")
    n, k4h = b4.shape
    g = k4h // 64
    if b_scale is not None:
        assert b_scale.is_cuda and b_scale.dtype == torch.float16 and b_scale.numel() == g * n
        nbytes = L.lib().atom_f6_weight_bytes(n, k4h * 2 + GROUP_SIZE)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=b4.device)
        st = L.lib().atom_repack_weight_f6s(b4.contiguous().data_ptr(), b_scale.contiguous().data_ptr(), n, k4h * 2 + GROUP_SIZE,
                                             buf.data_ptr(), L.current_stream(b4.device))
        L.check(st, "atom_repack_weight_f6s")
        out = buf[:g * f6_rows(n) * L.F6_PITCH].view(g, f6_rows(n), L.F6_PITCH)
        out.atom_f6s = buf                       # the whole buffer (codes + float32 scales) stays alive with the view
        out.atom_pairs = scale_pairs_shared(b_scale, n)
        return out
    out = torch.empty((g, f6_rows(n), L.F6_PITCH), dtype=torch.uint8, device=b4.device)
    st = L.lib().atom_repack_weight_f6(b4.contiguous().data_ptr(), n, k4h * 2 + GROUP_SIZE, out.data_ptr(),
                                        L.current_stream(b4.device))
    L.check(st, "atom_repack_weight_f6")
    return out


def repack_act_f6(a4: torch.Tensor, a_scale: torch.Tensor, *, scale_layout="ref") -> torch.Tensor:
    """Packed INT4 activations [M, K4/2] + scales -> the F6 activation operand [G][f6_rows(M)][104] (atom_repack_act_f6)."""
    if not a4.is_cuda:
        raise L.AtomHipError("repack_act_f6 needs a GPU tensor: no CPU fallback")
    m, k4h = a4.shape
    out = torch.empty((k4h // 64, f6_rows(m), L.F6_PITCH), dtype=torch.uint8, device=a4.device)
    st = L.lib().atom_repack_act_f6(a4.data_ptr(), a_scale.data_ptr(), m, k4h * 2 + GROUP_SIZE, _LAYOUTS[scale_layout], out.data_ptr(),
                                    L.current_stream(a4.device))
    L.check(st, "atom_repack_act_f6")
    return out


# ----------------------------------------------------------------------------------------------- fused gate / up
def fuse_gate_up_weights(gate, up):
    """(b4 u8 [N, K4/2], b8 i8 [N, 128], sb f16 [G, N], sb8 f16 [N]) of gate_proj and of up_proj -> the fused weight operand of
    gate_up_silu_quant_f6: rows interleaved per 128-feature block and 32-feature quarter (32 gate rows, then the same 32 up rows),
    codes + float32 scales in the F6 format (atom_repack_weight_f6s).  Offline, once per layer.  Returns a dict."""
    b4g, b8g, sbg, sb8g = gate
    b4u, b8u, sbu, sb8u = up
    n = b4g.shape[0]
    assert b4u.shape == b4g.shape and n % GROUP_SIZE == 0 and n >= 2 * GROUP_SIZE
    dev = b4g.device
    q = torch.arange(n, device=dev).view(n // 128, 4, 32)                                   # [block, quarter, 32 features]
    idx = torch.stack([q, q + n], dim=2).reshape(-1)                                        # gate rows, then the same up rows
    b4 = torch.cat([b4g.view(torch.uint8), b4u.view(torch.uint8)], 0).index_select(0, idx).contiguous()
    b8 = torch.cat([b8g, b8u], 0).index_select(0, idx).contiguous()
    g = sbg.numel() // n
    sb = torch.cat([sbg.reshape(g, n), sbu.reshape(g, n)], 1).index_select(1, idx).contiguous()
    sb8 = torch.cat([sb8g.reshape(-1), sb8u.reshape(-1)], 0).index_select(0, idx).contiguous()
    return {"b6s": repack_weight_f6(b4, sb), "b8": b8, "sb8": sb8, "n_inter": n, "k": b4g.shape[1] * 2 + GROUP_SIZE}


def gate_up_silu_quant_f6(a6, a_keeper, a_keeper_scale, fused, *, quant_mode="kernel", clip=1.0, scale_layout="ref",
                          return_dequant=False):
    """quant(silu(x Wg^T) * (x Wu^T)) in one launch, from the F6 activation operand of x straight to the F6 activation operand of
    down_proj: the reference's gate_proj, up_proj and activate_fp16_i4 (punica/models/llama.py:85-87) -- same return tuple as
    activate_fp16_i4(..., wide_codes="f6"), bit-identical to it on the fp16 GEMM outputs."""
    m = a_keeper.size(0)
    n, k = fused["n_inter"], fused["k"]
    assert a6.shape == (k // GROUP_SIZE - 1, f6_rows(m), L.F6_PITCH)
    outs = _alloc_act_outputs(m, n, a6.device, scale_layout, return_dequant, "f6")
    b6s = fused["b6s"]
    st = L.lib().atom_gemm_w4a4_silu_mul_quant_f6(a6.data_ptr(), b6s.atom_f6s.data_ptr(), a_keeper.data_ptr(), fused["b8"].data_ptr(),
                                                  a_keeper_scale.data_ptr(), fused["sb8"].data_ptr(), m, n, k, GROUP_SIZE, GROUP_SIZE,
                                                  _MODES[quant_mode], float(clip),
                                                  _LAYOUTS[scale_layout] | (L.B_SCALE_PAIRS if getattr(b6s, "atom_pairs", False) else 0),
                                                  outs[0].data_ptr(),
                                                  outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), L.ptr(outs[4]),
                                                  L.current_stream(a6.device))
    L.check(st, "atom_gemm_w4a4_silu_mul_quant_f6")
    return _ret(*outs)


# ------------------------------------------------------------------------------------------------ sparse mixture of experts
class MoeRoute:
    """The device tables of atom_moe_route_topk (include/atom_hip.h) for T tokens, E experts and top_k slots per token."""
    __slots__ = ("tokens", "experts", "top_k", "topk_ids", "topk_w", "expert_indptr", "row_token", "slot_row", "tile_expert",
                 "tile_row0", "n_tiles")

    def __init__(self, tokens, experts, top_k, **tables):
        self.tokens, self.experts, self.top_k = int(tokens), int(experts), int(top_k)
        for k, v in tables.items():
            setattr(self, k, v)

    @property
    def rows(self) -> int:
        return self.tokens * self.top_k


def moe_max_tiles(rows: int, experts: int) -> int:
    """Upper bound of the tile count for any routing of ``rows`` routed rows over ``experts`` experts (64-row tiles)."""
    return int(L.lib().atom_moe_max_tiles(int(rows), int(experts)))


def moe_route_topk(logits: torch.Tensor, top_k: int) -> MoeRoute:
    """Router of a sparse MoE block in ONE launch, nothing read back: the top_k experts per token (largest logit first, the lower
    index on equal logits), their renormalised softmax weights (fp16), and the tables the routed GEMM and the combine read -- rows
    grouped by expert in ascending token order.  Reference: model/qMixtralLayer.py:313-317 + the expert mask of :321-341."""
    _require_cuda_half(logits, "logits")
    t, e = logits.shape
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=logits.device)
    mt = moe_max_tiles(t * top_k, e)
    r = MoeRoute(t, e, top_k, topk_ids=i32(t, top_k), topk_w=torch.empty((t, top_k), dtype=torch.float16, device=logits.device),
                 expert_indptr=i32(e + 1), row_token=i32(t * top_k), slot_row=i32(t, top_k), tile_expert=i32(max(mt, 1)),
                 tile_row0=i32(max(mt, 1)), n_tiles=i32(1))
    st = L.lib().atom_moe_route_topk(logits.data_ptr(), t, e, int(top_k), r.topk_ids.data_ptr(), r.topk_w.data_ptr(),
                                     r.expert_indptr.data_ptr(), r.row_token.data_ptr(), r.slot_row.data_ptr(),
                                     r.tile_expert.data_ptr(), r.tile_row0.data_ptr(), r.n_tiles.data_ptr(),
                                     L.current_stream(logits.device))
    L.check(st, "atom_moe_route_topk")
    return r


def moe_gemm_i4(a, a_scale, a_keeper, a_keeper_scale, experts, route: MoeRoute, *, gather: bool, nseg=1, scale_layout="ref"):
    """The routed GEMM: every routed row of ``route`` times ITS expert's weight, one launch for all experts.  ``experts`` = (b4 u8
    [E, N, K4/2], b8 i8 [E, N, 128], sb f16 [E, G, N], sb8 f16 [E, N]) stacked packed weights; ``gather=True``: ``a`` holds one
    quantised row per TOKEN (and so do the scales) and row r reads token route.row_token[r]; ``gather=False``: ``a`` holds the routed
    rows themselves.  Returns ``nseg`` (1 or 2) tensors fp16 [rows, N / nseg] -- gate and up of one launch.  Bit-identical to
    dense_layer_gemm_i4_fp16's tile kernels on each expert's rows."""
    b4, b8, sb, sb8 = experts
    for t in (a, a_scale, a_keeper, a_keeper_scale, b4, b8, sb, sb8):
        if not t.is_cuda:
            raise L.AtomHipError("all GEMM operands must live on the GPU: no CPU fallback")
        if not t.is_contiguous():
            raise ValueError("routed GEMM operands must be contiguous")
    e, n, k4h = b4.shape
    a_rows, rows = a.size(0), route.rows
    k = a.size(1) * 2 + a_keeper.size(1)
    assert e == route.experts and a.size(1) == k4h and nseg in (1, 2) and n % nseg == 0
    assert a_rows == (route.tokens if gather else rows)
    n_seg = n // nseg
    outs = [torch.empty((rows, n_seg), dtype=torch.float16, device=a.device) for _ in range(nseg)]
    st = L.lib().atom_moe_gemm_w4a4_f16(a.data_ptr(), b4.data_ptr(), a_scale.data_ptr(), sb.data_ptr(), a_keeper.data_ptr(), b8.data_ptr(),
                                        a_keeper_scale.data_ptr(), sb8.data_ptr(), route.row_token.data_ptr() if gather else None,
                                        route.expert_indptr.data_ptr(), route.tile_expert.data_ptr(), route.tile_row0.data_ptr(),
                                        route.n_tiles.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if nseg > 1 else None,
                                        a_rows, rows, e, n_seg, nseg, k, GROUP_SIZE, GROUP_SIZE, _LAYOUTS[scale_layout],
                                        L.current_stream(a.device))
    L.check(st, "atom_moe_gemm_w4a4_f16")
    return tuple(outs)


def moe_combine(y: torch.Tensor, route: MoeRoute, residual: torch.Tensor = None) -> torch.Tensor:
    """out[t] = residual[t] + sum over token t's slots, in ascending expert id, of half(y[slot_row[t, k]] * topk_w[t, k]) -- fp16
    adds into a zero accumulator, the residual last (reference qMixtralLayer.py:344-348, :434)."""
    _require_cuda_half(y, "y")
    rows, h = y.shape
    assert rows == route.rows
    if residual is not None:
        _require_cuda_half(residual, "residual")
        assert residual.shape == (route.tokens, h)
    out = torch.empty((route.tokens, h), dtype=torch.float16, device=y.device)
    st = L.lib().atom_moe_combine_f16(y.data_ptr(), route.slot_row.data_ptr(), route.topk_ids.data_ptr(), route.topk_w.data_ptr(),
                                      L.ptr(residual), out.data_ptr(), route.tokens, route.top_k, h, L.current_stream(y.device))
    L.check(st, "atom_moe_combine_f16")
    return out


# ------------------------------------------------------------------------------------------------ multi-adapter LoRA (fp16)
def _lora_tables(y, x, indicies, seg_indptr):
    """(int32 ids, S, seg_indptr) of a LoRA op: one id per row, or one per segment of ``seg_indptr`` (int32 [S + 1], on the device)."""
    _require_cuda_half(y, "y")
    _require_cuda_half(x, "x")
    if not indicies.is_cuda:
        raise L.AtomHipError("indicies must live on the GPU: the LoRA ops have no CPU fallback")
    if indicies.dtype not in (torch.int32, torch.int64) or indicies.dim() != 1:
        raise TypeError(f"indicies must be a 1-d int32 or int64 tensor, got {indicies.dtype} {tuple(indicies.shape)}")
    ids = indicies.contiguous() if indicies.dtype == torch.int32 else indicies.to(torch.int32)   # (a launch, not a host read)
    assert x.dim() == 2 and y.dim() == 2 and x.size(0) == y.size(0)
    if seg_indptr is None:
        assert ids.numel() == x.size(0), "one adapter id per row"
    else:
        assert seg_indptr.is_cuda and seg_indptr.dtype == torch.int32 and seg_indptr.is_contiguous()
        assert seg_indptr.numel() == ids.numel() + 1, "one adapter id per segment"
    return ids, ids.numel()


def bgmv(y: torch.Tensor, x: torch.Tensor, w_T_all: torch.Tensor, indicies: torch.Tensor, layer_idx: int, scale: float, *,
         seg_indptr: torch.Tensor = None):
    """Reference punica/ops/__init__.py:62-91: ``y[i] += scale * x[i] @ w_T_all[indicies[i], layer_idx].T`` in place, FP32 sums and one
    rounding.  y fp16 [B, H2], x fp16 [B, H1], w_T_all fp16 [capacity, L, H2, H1], indicies int64 or int32 [B]; an id of -1 (any id
    outside 0 .. capacity - 1) leaves its rows untouched.  ``seg_indptr`` (int32 [S + 1], device): ``indicies`` holds one id per
    SEGMENT of rows seg_indptr[s] .. seg_indptr[s + 1] - 1 (a prefill request), and rows from seg_indptr[S] on are not written.
    One of H1, H2 is the rank (a multiple of 8 in 8 .. 64), the other a multiple of 64."""
    ids, s = _lora_tables(y, x, indicies, seg_indptr)
    _require_cuda_half(w_T_all, "w_T_all")
    cap, nl, h2, h1 = w_T_all.shape
    assert x.size(1) == h1 and y.size(1) == h2
    st = L.lib().atom_bgmv_f16(y.data_ptr(), x.data_ptr(), w_T_all.data_ptr(), ids.data_ptr(), L.ptr(seg_indptr), x.size(0), s, h1, h2,
                               cap, nl, int(layer_idx), float(scale), L.current_stream(y.device))
    L.check(st, "atom_bgmv_f16")


def add_lora(y: torch.Tensor, x: torch.Tensor, wa_T_all: torch.Tensor, wb_T_all: torch.Tensor, indicies: torch.Tensor, layer_idx: int,
             scale: float, *, seg_indptr: torch.Tensor = None):
    """Reference punica/ops/__init__.py:94-124: ``y[i] += scale * half(x[i] @ wa_T_all[id, layer_idx].T) @ wb_T_all[id, layer_idx].T`` in
    place -- two bgmv passes, the rank-wide intermediate rounded to fp16 between them.  wa_T_all fp16 [capacity, L, r, H1], wb_T_all
    fp16 [capacity, L, H2, r]; H1, H2 multiples of 64, r a multiple of 8 in 8 .. 64; ``indicies`` / ``seg_indptr`` as ``bgmv``."""
    ids, s = _lora_tables(y, x, indicies, seg_indptr)
    _require_cuda_half(wa_T_all, "wa_T_all")
    _require_cuda_half(wb_T_all, "wb_T_all")
    cap, nl, r, h1 = wa_T_all.shape
    h2 = wb_T_all.size(2)
    assert wb_T_all.shape == (cap, nl, h2, r) and x.size(1) == h1 and y.size(1) == h2
    t = torch.empty((x.size(0), r), dtype=torch.float16, device=x.device)
    st = L.lib().atom_add_lora_f16(y.data_ptr(), x.data_ptr(), wa_T_all.data_ptr(), wb_T_all.data_ptr(), ids.data_ptr(),
                                   L.ptr(seg_indptr), t.data_ptr(), x.size(0), s, h1, h2, r, cap, nl, int(layer_idx), float(scale),
                                   L.current_stream(y.device))
    L.check(st, "atom_add_lora_f16")


def kv_quant_u4(k: torch.Tensor):
    """NEW: fp16 k (or v) [T, kv_heads, 128] -> (packed u8 [T, kv_heads, 64], params fp16 [T, kv_heads, 2]) in the form ``init_kv_i4`` /
    ``append_kv_i4`` take: the per-head quantiser of ``quant_append_kv_i4`` applied to ``k.float()``, without a cache."""
    _require_cuda_half(k, "k")
    t, heads, d = k.shape
    packed = torch.empty((t, heads, d // 2), dtype=torch.uint8, device=k.device)
    params = torch.empty((t, heads, 2), dtype=torch.float16, device=k.device)
    st = L.lib().atom_kv_quant_u4_f16(k.data_ptr(), packed.data_ptr(), params.data_ptr(), t, heads, d, L.current_stream(k.device))
    L.check(st, "atom_kv_quant_u4_f16")
    return packed, params


# ------------------------------------------------------------------------------------------------ vocabulary rows
def _row_stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _logits_rows(logits: torch.Tensor, op_has: str, rows: str = "batch"):
    """The ``logits`` argument of sample, logprob, penalize and guide_mask: fp16 [rows, vocab] with contiguous rows on the GPU.
    Returns (rows, vocab, row stride)."""
    if not logits.is_cuda:
        raise L.AtomHipError(f"logits must live on the GPU: {op_has} no CPU fallback")
    if logits.dtype != torch.float16:
        raise TypeError(f"logits must be float16, got {logits.dtype}")
    if logits.dim() != 2 or logits.size(0) < 1 or logits.size(1) < 1 or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise ValueError(f"logits must be [{rows}, vocab] with contiguous rows, got {tuple(logits.shape)} strides {logits.stride()}")
    return logits.size(0), logits.size(1), _row_stride(logits)


def _require_dev(ops_name, name, t, dtype, shape=None):
    """``t`` on the GPU, contiguous, of ``dtype`` (and ``shape``); ``ops_name``: the op family the message names"""
    if not t.is_cuda:
        raise L.AtomHipError(f"{name} must live on the GPU: the {ops_name} ops have no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise TypeError(f"{name} must be a contiguous {dtype} tensor{'' if shape is None else ' of ' + str(list(shape))}, "
                        f"got {t.dtype} {tuple(t.shape)}")


# ------------------------------------------------------------------------------------------------ sampling
_SAMPLE_PARAMS = (("temperature", torch.float32), ("top_k", torch.int32), ("top_p", torch.float32), ("seeds", torch.int64))


def sample(logits: torch.Tensor, temperature: torch.Tensor = None, top_k: torch.Tensor = None, top_p: torch.Tensor = None,
           seeds: torch.Tensor = None, step: torch.Tensor = None, step_offset: int = 0, out: torch.Tensor = None, *,
           rows_per_seq: int = None) -> torch.Tensor:
    """NEW: one token per row of ``logits`` (fp16 [batch, vocab], rows ``stride(0) >= vocab`` apart) under temperature, top-k and
    top-p -- ``atom_sample_f16``, the contract of DESIGN.md 4.13: the token is an exact function of the row's bits, its parameters
    and the draw number ``step[0] + step_offset``; it does not depend on the batch or on timing.  The parameters are DEVICE tensors of
    ``[batch]`` that the launch reads (a captured call follows buffers changed in place): ``temperature`` float32 (<= 0: greedy, the
    first index of the maximum), ``top_k`` int32 (outside 1 .. vocab - 1: off), ``top_p`` float32 (>= 1: off), ``seeds`` int64 (the 64
    bits are the Philox key; uint64 is taken too), ``step`` int64 [1].  None: T = 1, off, off, seed 0, step 0.  Returns int64 [batch]
    (``out`` if given).  One launch; nothing is read back, nothing synchronises.
    ``rows_per_seq`` (the verify rows of speculative decoding, ``atom_sample_rows_f16``): the rows are ``batch / rows_per_seq``
    sequences of that many consecutive rows, ``step`` is int64 ``[batch / rows_per_seq]`` and row r draws number
    ``step[r // rows_per_seq] + r % rows_per_seq + step_offset``; the four parameter tensors stay per ROW."""
    batch, vocab, ld = _logits_rows(logits, "the sampler has")
    given = dict(temperature=temperature, top_k=top_k, top_p=top_p, seeds=seeds)
    for name, dtype in _SAMPLE_PARAMS:
        t = given[name]
        if t is None:
            continue
        ok = t.dtype == dtype or (name == "seeds" and t.dtype == torch.uint64)
        if not (t.is_cuda and ok and t.shape == (batch,) and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous {dtype} tensor of [{batch}] on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if rows_per_seq is not None:
        q = int(rows_per_seq)
        if q < 1 or batch % q:
            raise ValueError(f"rows_per_seq must be positive and divide the {batch} rows, got {rows_per_seq}")
        if step is None or not (step.is_cuda and step.dtype == torch.int64 and step.shape == (batch // q,) and step.is_contiguous()):
            raise TypeError(f"with rows_per_seq={q} step must be a contiguous int64 tensor of [{batch // q}] on the GPU")
    elif step is not None and not (step.is_cuda and step.dtype == torch.int64 and step.numel() == 1):
        raise TypeError("step must be an int64 tensor of one element on the GPU")
    if out is None:
        out = torch.empty(batch, dtype=torch.int64, device=logits.device)
    elif not (out.is_cuda and out.dtype == torch.int64 and out.shape == (batch,) and out.is_contiguous()):
        raise TypeError(f"out must be a contiguous int64 tensor of [{batch}] on the GPU")
    params = (logits.data_ptr(), ld, batch, vocab, L.ptr(temperature), L.ptr(top_k), L.ptr(top_p), L.ptr(seeds), L.ptr(step))
    if rows_per_seq is None:
        st = L.lib().atom_sample_f16(*params, int(step_offset), out.data_ptr(), L.current_stream(logits.device))
        L.check(st, "atom_sample_f16")
    else:
        st = L.lib().atom_sample_rows_f16(*params, int(rows_per_seq), int(step_offset), out.data_ptr(), L.current_stream(logits.device))
        L.check(st, "atom_sample_rows_f16")
    return out


# ------------------------------------------------------------------------------------------------ log-probabilities
LOGPROB_MAX_TOP = 32


def logprob(logits: torch.Tensor, targets: torch.Tensor = None, top_n: int = 0, *, out=None):
    """NEW: per row of ``logits`` (fp16 [rows, vocab], rows ``stride(0) >= vocab`` apart) the log-probability and rank of
    ``targets`` (int64 [rows] on the GPU) and the ``top_n`` (0 .. 32) most probable tokens with their log-probabilities --
    ``atom_logprob_f16``, the contract of DESIGN.md 4.14, on the sampler's arithmetic: the distribution ``ops.sample`` draws from at
    T = 1 without truncation.  Returns ``(logprob, rank, top_ids, top_logprobs)``: float32 [rows], int32 [rows] (0 is the greedy token),
    int64 and float32 [rows, top_n]; None for what was not asked (no ``targets``: the first two; ``top_n = 0``: the last two).  A
    target outside 0 .. vocab - 1 is ignored: log-probability 0, rank -1.  ``out``: a tuple of four preallocated buffers (None where
    nothing is asked) for capture.  One launch; nothing is read back, nothing synchronises."""
    rows, vocab, ld = _logits_rows(logits, "the log-probability op has", rows="rows")
    top_n = int(top_n)
    if not 0 <= top_n <= LOGPROB_MAX_TOP:
        raise ValueError(f"top_n must be 0 .. {LOGPROB_MAX_TOP}, got {top_n}")
    if targets is None and top_n == 0:
        raise ValueError("nothing to do: no targets and top_n = 0")
    if targets is not None and not (targets.is_cuda and targets.dtype == torch.int64 and targets.shape == (rows,) and targets.is_contiguous()):
        raise TypeError(f"targets must be a contiguous int64 tensor of [{rows}] on the GPU, got {targets.dtype} {tuple(targets.shape)} on {targets.device}")
    want = ((torch.float32, (rows,), targets is not None), (torch.int32, (rows,), targets is not None),
            (torch.int64, (rows, top_n), top_n > 0), (torch.float32, (rows, top_n), top_n > 0))
    if out is not None and len(out) != 4:
        raise TypeError("out must be a tuple of four: (logprob, rank, top_ids, top_logprobs)")
    bufs = []
    for i, (dtype, shape, asked) in enumerate(want):
        b = None if out is None else out[i]
        if not asked:
            b = None
        elif b is None:
            b = torch.empty(shape, dtype=dtype, device=logits.device)
        elif not (b.is_cuda and b.dtype == dtype and tuple(b.shape) == shape and b.is_contiguous()):
            raise TypeError(f"out[{i}] must be a contiguous {dtype} tensor of {list(shape)} on the GPU")
        bufs.append(b)
    st = L.lib().atom_logprob_f16(logits.data_ptr(), ld, rows, vocab, L.ptr(targets), L.ptr(bufs[0]), L.ptr(bufs[1]), top_n,
                                  L.ptr(bufs[2]), L.ptr(bufs[3]), L.current_stream(logits.device))
    L.check(st, "atom_logprob_f16")
    return tuple(bufs)


# ------------------------------------------------------------------------------------------------ logit penalties
PENALTY_MAX_BIAS = 512
PENALTY_TILE = 2048            # elements per workgroup of atom_penalize_f16 (csrc/penalize.hip kPenTile)


def penalize(logits: torch.Tensor, state: torch.Tensor = None, fed: torch.Tensor = None, repetition: torch.Tensor = None,
             presence: torch.Tensor = None, frequency: torch.Tensor = None, bias_ids: torch.Tensor = None,
             bias_vals: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """NEW: repetition / presence / frequency penalties and a per-row logit bias on ``logits`` (fp16 [batch, vocab], rows
    ``stride(0) >= vocab`` apart) -- ``atom_penalize_f16``, the contract of DESIGN.md 4.15.  ``state`` int16 [batch, >= vocab] holds one
    word per (sequence, token): the sign bit says the token occurs in the prompt, the low 15 bits count how often it was generated
    (saturating).  With ``fed`` (int64 [batch]) the launch first counts token ``fed[b]`` in ``state[b]`` (a value outside
    0 .. vocab - 1 counts nothing), then penalises.  ``repetition``, ``presence``, ``frequency``: float32 [batch]; ``bias_ids`` int32
    [batch, max_bias] padded with -1 and ``bias_vals`` float32 [batch, max_bias], max_bias <= 512.  All DEVICE tensors that the launch
    reads (a captured call follows buffers changed in place); None: no state, nothing fed, neutral, no bias.  Rows whose parameters
    change nothing and elements that are neither seen nor biased are copied bit for bit.  Returns fp16 [batch, vocab] (``out`` if
    given; ``out`` may be ``logits``).  One launch; nothing is read back, nothing synchronises."""
    batch, vocab, ld = _logits_rows(logits, "the penalty op has")
    for name, t in (("repetition", repetition), ("presence", presence), ("frequency", frequency)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.shape == (batch,) and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous float32 tensor of [{batch}] on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
    state_ld = 0
    if state is not None:
        if not (state.is_cuda and state.dtype == torch.int16 and state.dim() == 2 and state.size(0) == batch and state.size(1) >= vocab
                and (state.size(1) == 1 or state.stride(1) == 1)):
            raise TypeError(f"state must be an int16 tensor of [{batch}, >= {vocab}] with contiguous rows on the GPU")
        state_ld = _row_stride(state)
    if fed is not None:
        if state is None:
            raise ValueError("fed needs state: there is nothing to count into")
        if not (fed.is_cuda and fed.dtype == torch.int64 and fed.shape == (batch,) and fed.is_contiguous()):
            raise TypeError(f"fed must be a contiguous int64 tensor of [{batch}] on the GPU")
    max_bias = 0
    if (bias_ids is None) != (bias_vals is None):
        raise ValueError("bias_ids and bias_vals come together")
    if bias_ids is not None:
        max_bias = bias_ids.size(1) if bias_ids.dim() == 2 else -1
        if not (bias_ids.is_cuda and bias_vals.is_cuda and bias_ids.dtype == torch.int32 and bias_vals.dtype == torch.float32
                and bias_ids.dim() == 2 and bias_ids.size(0) == batch and bias_vals.shape == bias_ids.shape
                and bias_ids.is_contiguous() and bias_vals.is_contiguous()):
            raise TypeError(f"bias_ids int32 and bias_vals float32 must be contiguous [{batch}, max_bias] tensors on the GPU")
        if max_bias > PENALTY_MAX_BIAS:
            raise ValueError(f"at most {PENALTY_MAX_BIAS} bias entries per row, got {max_bias}")
    if out is None:
        out = torch.empty((batch, vocab), dtype=torch.float16, device=logits.device)
    elif not (out.is_cuda and out.dtype == torch.float16 and out.shape == (batch, vocab) and (vocab == 1 or out.stride(1) == 1)):
        raise TypeError(f"out must be a float16 tensor of [{batch}, {vocab}] with contiguous rows on the GPU")
    st = L.lib().atom_penalize_f16(logits.data_ptr(), ld, batch, vocab, L.ptr(state), state_ld, L.ptr(fed),
                                   L.ptr(repetition), L.ptr(presence), L.ptr(frequency), L.ptr(bias_ids) if max_bias else None,
                                   L.ptr(bias_vals) if max_bias else None, max_bias, out.data_ptr(), _row_stride(out),
                                   L.current_stream(logits.device))
    L.check(st, "atom_penalize_f16")
    return out


PENALTY_MAX_ROWS = 9           # the verify rows per sequence atom_penalize_rows_f16 takes (csrc/penalize.hip kPenMaxRows)


def penalize_rows(logits: torch.Tensor, state: torch.Tensor, input_ids: torch.Tensor = None, commit_tokens: torch.Tensor = None,
                  commit_counts: torch.Tensor = None, repetition: torch.Tensor = None, presence: torch.Tensor = None,
                  frequency: torch.Tensor = None, bias_ids: torch.Tensor = None, bias_vals: torch.Tensor = None,
                  out: torch.Tensor = None) -> torch.Tensor:
    """NEW: ``ops.penalize`` for the verify rows of speculative decoding -- ``atom_penalize_rows_f16``, the contract of DESIGN.md 4.20.
    ``logits`` fp16 [batch * rows, vocab] holds ``rows = input_ids.size(1)`` (1 .. 9) consecutive rows per sequence, ``state`` int16
    [batch, >= vocab] one row per SEQUENCE.  The launch first counts the pending tokens ``commit_tokens[b, :commit_counts[b]]`` (int64
    [batch, n] with contiguous rows, int32 [batch]; the count is clamped to 0 .. min(n, 9), a token outside 0 .. vocab - 1 counts nothing)
    into ``state`` -- the tokens the step before emitted -- and then penalises row j of sequence b as ``ops.penalize`` would under
    that state with the drafts ``input_ids[b, 1 .. j]`` (int64 [batch, rows] with contiguous rows) counted as well.  Column 0, the last
    emitted token, is not counted here, and drafts never reach ``state``.  ``repetition``, ``presence``, ``frequency`` float32 [batch] and
    ``bias_ids`` / ``bias_vals`` [batch, max_bias] are per sequence.  All DEVICE tensors that the launch reads (a captured call follows
    buffers changed in place).  ``logits=None`` (then ``out`` and ``input_ids`` are None too) counts the pending tokens and does nothing
    else -- the vocabulary is then ``state.size(1)`` -- and returns None.  Otherwise returns fp16 [batch * rows, vocab] (``out`` if given; ``out`` may be ``logits``).  One launch;
    nothing is read back, nothing synchronises."""
    if state is None or not (state.is_cuda and state.dtype == torch.int16 and state.dim() == 2 and state.size(0) >= 1
                             and (state.size(1) == 1 or state.stride(1) == 1)):
        raise TypeError("state must be an int16 tensor of [batch, >= vocab] with contiguous rows on the GPU")
    batch, state_ld = state.size(0), _row_stride(state)
    rows, vocab, ld, ids_ld = 1, state.size(1), 0, 0
    if logits is None:
        if out is not None or input_ids is not None:
            raise ValueError("logits=None counts the pending tokens alone: out and input_ids must be None too")
        if commit_tokens is None:
            raise ValueError("nothing to do: no logits and no pending tokens")
    else:
        total, vocab, ld = _logits_rows(logits, "the penalty op has", rows="batch * rows")
        if input_ids is None or not (input_ids.is_cuda and input_ids.dtype == torch.int64 and input_ids.dim() == 2
                                     and input_ids.size(0) == batch and (input_ids.size(1) == 1 or input_ids.stride(1) == 1)):
            raise TypeError(f"input_ids must be an int64 tensor of [{batch}, rows] with contiguous rows on the GPU")
        rows, ids_ld = input_ids.size(1), _row_stride(input_ids)
        if not 1 <= rows <= PENALTY_MAX_ROWS or total != batch * rows:
            raise ValueError(f"input_ids must give 1 .. {PENALTY_MAX_ROWS} rows per sequence and logits batch * rows rows, "
                             f"got {tuple(input_ids.shape)} for {total} rows of logits and {batch} rows of state")
        if state.size(1) < vocab:
            raise TypeError(f"state must be an int16 tensor of [{batch}, >= {vocab}] with contiguous rows on the GPU")
    for name, t in (("repetition", repetition), ("presence", presence), ("frequency", frequency)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.shape == (batch,) and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous float32 tensor of [{batch}] on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
    commit_ld = 0
    if (commit_tokens is None) != (commit_counts is None):
        raise ValueError("commit_tokens and commit_counts come together")
    if commit_tokens is not None:
        if not (commit_tokens.is_cuda and commit_tokens.dtype == torch.int64 and commit_tokens.dim() == 2 and commit_tokens.size(0) == batch
                and commit_tokens.size(1) >= 1 and (commit_tokens.size(1) == 1 or commit_tokens.stride(1) == 1)):
            raise TypeError(f"commit_tokens must be an int64 tensor of [{batch}, n >= 1] with contiguous rows on the GPU")
        if not (commit_counts.is_cuda and commit_counts.dtype == torch.int32 and commit_counts.shape == (batch,) and commit_counts.is_contiguous()):
            raise TypeError(f"commit_counts must be a contiguous int32 tensor of [{batch}] on the GPU")
        commit_ld = _row_stride(commit_tokens)
    max_bias = 0
    if (bias_ids is None) != (bias_vals is None):
        raise ValueError("bias_ids and bias_vals come together")
    if bias_ids is not None:
        max_bias = bias_ids.size(1) if bias_ids.dim() == 2 else -1
        if not (bias_ids.is_cuda and bias_vals.is_cuda and bias_ids.dtype == torch.int32 and bias_vals.dtype == torch.float32
                and bias_ids.dim() == 2 and bias_ids.size(0) == batch and bias_vals.shape == bias_ids.shape
                and bias_ids.is_contiguous() and bias_vals.is_contiguous()):
            raise TypeError(f"bias_ids int32 and bias_vals float32 must be contiguous [{batch}, max_bias] tensors on the GPU")
        if max_bias > PENALTY_MAX_BIAS:
            raise ValueError(f"at most {PENALTY_MAX_BIAS} bias entries per row, got {max_bias}")
    if logits is not None:
        if out is None:
            out = torch.empty((batch * rows, vocab), dtype=torch.float16, device=logits.device)
        elif not (out.is_cuda and out.dtype == torch.float16 and out.shape == (batch * rows, vocab) and (vocab == 1 or out.stride(1) == 1)):
            raise TypeError(f"out must be a float16 tensor of [{batch * rows}, {vocab}] with contiguous rows on the GPU")
    st = L.lib().atom_penalize_rows_f16(L.ptr(logits), ld, batch, rows, vocab, state.data_ptr(), state_ld, L.ptr(input_ids), ids_ld,
                                        L.ptr(commit_tokens), commit_ld, L.ptr(commit_counts), L.ptr(repetition), L.ptr(presence),
                                        L.ptr(frequency), L.ptr(bias_ids) if max_bias else None, L.ptr(bias_vals) if max_bias else None,
                                        max_bias, L.ptr(out), 0 if out is None else _row_stride(out), L.current_stream(state.device))
    L.check(st, "atom_penalize_rows_f16")
    return out


# ------------------------------------------------------------------------------------------------ beam search
BEAM_MAX_BEAMS = 16


def beam_select(top_ids: torch.Tensor, top_lp: torch.Tensor, cum: torch.Tensor, finished: torch.Tensor, length: torch.Tensor,
                eos, w_out: int, *, w_in: int = None, out=None):
    """NEW: the selection step of beam search -- ``atom_beam_select``, the contract of DESIGN.md 4.16.  ``top_ids`` int64 / ``top_lp``
    float32 [groups * w_in, C] are ``ops.logprob(..., top_n=C)``'s outputs for the ``w_in`` rows of every prompt group (``w_in=1``
    for the step after the prefill, default ``w_out``; ``w_out`` <= C <= 32); ``cum`` float32, ``finished`` int32 and ``length`` int32
    [groups * w_in] each row's summed log-probability, end flag and token count; ``eos`` the ending token (None or negative: none).
    Returns ``(parent, token, cum, finished, length)`` of the ``w_out`` (1 .. 16) winners per group, [groups * w_out] each: ``parent``
    int32 is the row INSIDE the group.  The winners are the first of (score descending, parent ascending, candidate ascending) with
    score = cum + top_lp in one FP32 addition; a finished row is one frozen candidate.  ``out``: a tuple of five preallocated
    buffers for capture; with ``w_in == w_out`` the last three may be ``cum``, ``finished``, ``length`` themselves.  One launch; nothing
    is read back, nothing synchronises."""
    for t in (top_ids, top_lp, cum, finished, length):
        if not t.is_cuda:
            raise L.AtomHipError("beam_select operands must live on the GPU: no CPU fallback")
    w_out = int(w_out)
    if not 1 <= w_out <= BEAM_MAX_BEAMS:
        raise ValueError(f"w_out must be 1 .. {BEAM_MAX_BEAMS}, got {w_out}")
    if top_ids.dim() != 2 or top_ids.shape != top_lp.shape or top_ids.dtype != torch.int64 or top_lp.dtype != torch.float32:
        raise TypeError("top_ids int64 and top_lp float32 must both be [rows, C]")
    rows, C = top_ids.shape
    if not w_out <= C <= LOGPROB_MAX_TOP:
        raise ValueError(f"C must be w_out .. {LOGPROB_MAX_TOP}, got {C} for w_out {w_out}")
    w_in = w_out if w_in is None else int(w_in)
    if w_in not in (1, w_out) or rows % w_in:
        raise ValueError(f"w_in must be 1 or w_out ({w_out}) and divide the {rows} rows, got {w_in}")
    groups = rows // w_in
    for name, t, dtype in (("cum", cum, torch.float32), ("finished", finished, torch.int32), ("length", length, torch.int32)):
        if not (t.dtype == dtype and t.shape == (rows,) and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous {dtype} tensor of [{rows}]")
    if not (top_ids.is_contiguous() and top_lp.is_contiguous()):
        raise TypeError("top_ids and top_lp must be contiguous")
    want = (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32)
    if out is not None and len(out) != 5:
        raise TypeError("out must be a tuple of five: (parent, token, cum, finished, length)")
    if out is None:
        out = tuple(torch.empty(groups * w_out, dtype=d, device=top_ids.device) for d in want)
    for i, (b, d) in enumerate(zip(out, want)):
        if not (b.is_cuda and b.dtype == d and b.shape == (groups * w_out,) and b.is_contiguous()):
            raise TypeError(f"out[{i}] must be a contiguous {d} tensor of [{groups * w_out}] on the GPU")
    st = L.lib().atom_beam_select(top_ids.data_ptr(), top_lp.data_ptr(), cum.data_ptr(), finished.data_ptr(), length.data_ptr(),
                                  groups, w_in, w_out, C, -1 if eos is None else int(eos), *(b.data_ptr() for b in out),
                                  L.current_stream(top_ids.device))
    L.check(st, "atom_beam_select")
    return tuple(out)


def kv_beam_fork_i4(kv, parent: torch.Tensor):
    """NEW: the cache step of beam search -- row r of a utils.StaticBeamKvCacheInt4 continues the history of row ``parent[r]`` of its
    group (``parent`` int32 [rows], the row inside the group: ``ops.beam_select``'s output).  ``atom_kv_beam_fork_i4``
    shares the parent's full pages by reference and copies its one partial page into the row's spare page; it gathers into
    ``kv.table_out``, and one device-to-device copy on the same stream brings ``kv.page_table`` / ``kv.spare`` up to date, so
    ``ops.kv_step_i4`` keeps reading the one fixed table.  Two stream operations, no host synchronisation, capturable.  A parent outside
    the group keeps its row and sets the cache's status word (read by ``kv.sync_host()``)."""
    tensors = (kv.page_table, kv.table_out, kv.spare, kv.spare_out, kv.row_pages, kv.lengths, kv.state, parent)
    for t in tensors + (kv.data, kv.param):
        if not t.is_cuda:
            raise L.AtomHipError("KV-cache page tables must live on the GPU: no CPU fallback")
    for t in tensors:
        assert t.dtype == torch.int32 and t.is_contiguous()
    batch, cap = kv.page_table.shape
    assert kv.table_out.shape == (batch, cap) and kv.spare.numel() == kv.spare_out.numel() == kv.row_pages.numel() == batch
    assert kv.lengths.numel() == 2 * batch and kv.state.numel() == 4 and parent.numel() == batch and batch % kv.num_beams == 0
    num_layers, num_heads, page_size, head_dim = _kv_dims(kv)
    st = L.lib().atom_kv_beam_fork_i4(kv.data.data_ptr(), kv.param.data_ptr(), kv.page_table.data_ptr(), kv.table_out.data_ptr(),
                                      kv.spare.data_ptr(), kv.spare_out.data_ptr(), kv.row_pages.data_ptr(), kv.lengths.data_ptr(),
                                      kv.state.data_ptr(), parent.data_ptr(), batch, kv.num_beams, cap, kv.data.size(0), num_layers,
                                      num_heads, page_size, head_dim, L.current_stream(kv.page_table.device))
    L.check(st, "atom_kv_beam_fork_i4")
    kv.tables.copy_(kv.tables_out)                           # page_table and spare are views of one buffer: one copy


# ------------------------------------------------------------------------------------------------ speculative decoding
SPEC_MAX_DRAFT = 8
SPEC_MAX_NGRAM = 8


def spec_draft_ngram(hist: torch.Tensor, hist_len: torch.Tensor, out: torch.Tensor, *, ngram_max: int = 3, ngram_min: int = 1):
    """NEW: K draft tokens per sequence by n-gram lookup in the sequence's own history -- ``atom_spec_draft_ngram``, the contract of
    DESIGN.md 4.17.  ``hist`` int32 [batch, hist_cap] holds the prompt and every emitted token, ``hist_len`` int32 [batch] how many;
    ``out`` int64 [batch, K] (1 <= K <= 8) receives the drafts and may be a strided view with contiguous rows -- columns 1 .. K of the
    verify step's ``input_ids``.  The longest of the last ``ngram_max`` .. ``ngram_min`` tokens (1 .. 8) that occurs earlier in the
    history wins, at its most recent occurrence; the drafts are the tokens that followed it, padded with the last token, which is also
    every draft when nothing occurs twice.  Returns ``out``.  One launch; nothing is read back, nothing synchronises."""
    for name, t in (("hist", hist), ("hist_len", hist_len), ("out", out)):
        if not t.is_cuda:
            raise L.AtomHipError(f"{name} must live on the GPU: the speculative-decoding ops have no CPU fallback")
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.size(0) < 1 or hist.size(1) < 1 or not hist.is_contiguous():
        raise TypeError(f"hist must be a contiguous int32 tensor of [batch, hist_cap], got {hist.dtype} {tuple(hist.shape)}")
    batch, hist_cap = hist.shape
    _require_dev("speculative-decoding", "hist_len", hist_len, torch.int32, (batch,))
    if out.dtype != torch.int64 or out.dim() != 2 or out.size(0) != batch or (out.size(1) > 1 and out.stride(1) != 1):
        raise TypeError(f"out must be an int64 tensor of [{batch}, K] with contiguous rows, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    K = out.size(1)
    if not 1 <= K <= SPEC_MAX_DRAFT:
        raise ValueError(f"K (out's columns) must be 1 .. {SPEC_MAX_DRAFT}, got {K}")
    if not 1 <= int(ngram_min) <= int(ngram_max) <= SPEC_MAX_NGRAM:
        raise ValueError(f"n-gram sizes must satisfy 1 <= ngram_min <= ngram_max <= {SPEC_MAX_NGRAM}, got {ngram_min} .. {ngram_max}")
    out_ld = _row_stride(out)
    if out_ld < K:
        raise ValueError(f"out's rows overlap: row stride {out_ld} for {K} columns")
    st = L.lib().atom_spec_draft_ngram(hist.data_ptr(), hist_len.data_ptr(), batch, hist_cap, int(ngram_min), int(ngram_max), K,
                                       out.data_ptr(), out_ld, L.current_stream(hist.device))
    L.check(st, "atom_spec_draft_ngram")
    return out


def spec_accept(targets: torch.Tensor, input_ids: torch.Tensor, n_out: torch.Tensor, budget: torch.Tensor, tokens: torch.Tensor,
                hist: torch.Tensor, hist_len: torch.Tensor, adds: torch.Tensor, draw: torch.Tensor, accepted: torch.Tensor,
                steps: torch.Tensor, done: torch.Tensor):
    """NEW: the accept / commit step of speculative decoding -- ``atom_spec_accept``, the contract of DESIGN.md 4.17.  ``targets`` int64
    [batch, K + 1] are the tokens chosen at the verify rows, ``input_ids`` int64 [batch, K + 1] the last emitted token and the K
    drafts.  Per row the leading drafts that equal their targets are accepted; e = accepted + 1 tokens, cut at ``budget - n_out``
    (int32 [batch] each), are appended to ``tokens`` int64 [batch, max_new] at ``n_out`` and to ``hist`` int32 [batch, hist_cap] at
    ``hist_len``; ``n_out`` and ``hist_len`` grow by e, ``adds`` int32 [batch] receives e (for ``kv_step_rows_i4``), ``input_ids[:, 0]``
    the last emitted token, ``draw`` int64 [batch] the new ``n_out``, ``accepted`` / ``steps`` int32 [batch] count e - 1 and 1, and
    ``done`` int32 [1] says whether every row has reached its budget.  Everything is updated in place by one launch; nothing is read
    back, nothing synchronises."""
    if not targets.is_cuda:
        raise L.AtomHipError("targets must live on the GPU: the speculative-decoding ops have no CPU fallback")
    if targets.dtype != torch.int64 or targets.dim() != 2 or targets.size(0) < 1 or not targets.is_contiguous():
        raise TypeError(f"targets must be a contiguous int64 tensor of [batch, K + 1], got {targets.dtype} {tuple(targets.shape)}")
    batch, Q = targets.shape
    if not 1 <= Q - 1 <= SPEC_MAX_DRAFT:
        raise ValueError(f"K (targets' columns - 1) must be 1 .. {SPEC_MAX_DRAFT}, got {Q - 1}")
    _require_dev("speculative-decoding", "input_ids", input_ids, torch.int64, (batch, Q))
    for name, t in (("tokens", tokens), ("hist", hist)):
        if t.dim() != 2 or t.size(1) < 1:
            raise TypeError(f"{name} must be [batch, n], got {tuple(t.shape)}")
    _require_dev("speculative-decoding", "tokens", tokens, torch.int64, (batch, tokens.size(1)))
    _require_dev("speculative-decoding", "hist", hist, torch.int32, (batch, hist.size(1)))
    for name, t in (("n_out", n_out), ("budget", budget), ("hist_len", hist_len), ("adds", adds), ("accepted", accepted), ("steps", steps)):
        _require_dev("speculative-decoding", name, t, torch.int32, (batch,))
    _require_dev("speculative-decoding", "draw", draw, torch.int64, (batch,))
    _require_dev("speculative-decoding", "done", done, torch.int32, (1,))
    st = L.lib().atom_spec_accept(targets.data_ptr(), input_ids.data_ptr(), n_out.data_ptr(), budget.data_ptr(), tokens.data_ptr(),
                                  hist.data_ptr(), hist_len.data_ptr(), adds.data_ptr(), draw.data_ptr(), accepted.data_ptr(),
                                  steps.data_ptr(), done.data_ptr(), batch, Q - 1, tokens.size(1), hist.size(1),
                                  L.current_stream(targets.device))
    L.check(st, "atom_spec_accept")


# ------------------------------------------------------------------------------------------------ guided decoding
GUIDE_FREE, GUIDE_DEAD = L.GUIDE_FREE, L.GUIDE_DEAD
GUIDE_REJECTED, GUIDE_BAD_STATE = L.GUIDE_REJECTED, L.GUIDE_BAD_STATE
GUIDE_TILE = 2048              # elements per workgroup of atom_guide_mask_f16 (csrc/guide.hip kGuideTile)


def guide_mask(logits: torch.Tensor, state: torch.Tensor, mask: torch.Tensor, out: torch.Tensor = None,
               status: torch.Tensor = None) -> torch.Tensor:
    """NEW: the allowed set of every row's automaton state applied to ``logits`` (fp16 [batch, vocab], rows ``stride(0) >= vocab``
    apart) -- ``atom_guide_mask_f16``, the contract of DESIGN.md 4.18.  ``state`` int32 [batch]: a row of ``mask``, ``GUIDE_FREE`` or
    ``GUIDE_DEAD``; ``mask`` int32 [num_states, >= ceil(vocab / 32)] with contiguous rows, read as 32-bit words: token v is allowed in
    state s iff bit ``v & 31`` of ``mask[s, v >> 5]`` is set.  An allowed element keeps its bits, every other becomes -inf; a FREE or
    DEAD row is copied; any other state outside 0 .. num_states - 1 copies the row and sets ``GUIDE_BAD_STATE`` in ``status`` (int32
    [1]; None: a word of its own that nobody reads).  All DEVICE tensors that the launch reads (a captured call follows buffers
    changed in place).  Returns fp16 [batch, vocab] (``out`` if given; ``out`` may be ``logits``).  One launch; nothing is read back,
    nothing synchronises."""
    batch, vocab, ld = _logits_rows(logits, "the guide ops have")
    _require_dev("guide", "state", state, torch.int32, (batch,))
    if not (mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2 and mask.size(0) >= 1 and 32 * mask.size(1) >= vocab
            and (mask.size(1) == 1 or mask.stride(1) == 1)):
        raise TypeError(f"mask must be an int32 tensor of [num_states, >= {-(-vocab // 32)}] with contiguous rows on the GPU")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=logits.device)
    _require_dev("guide", "status", status, torch.int32, (1,))
    if out is None:
        out = torch.empty((batch, vocab), dtype=torch.float16, device=logits.device)
    elif not (out.is_cuda and out.dtype == torch.float16 and out.shape == (batch, vocab) and (vocab == 1 or out.stride(1) == 1)):
        raise TypeError(f"out must be a float16 tensor of [{batch}, {vocab}] with contiguous rows on the GPU")
    st = L.lib().atom_guide_mask_f16(logits.data_ptr(), ld, batch, vocab, state.data_ptr(), mask.data_ptr(),
                                     _row_stride(mask), mask.size(0), out.data_ptr(), _row_stride(out), status.data_ptr(),
                                     L.current_stream(logits.device))
    L.check(st, "atom_guide_mask_f16")
    return out


def guide_advance(state: torch.Tensor, tokens: torch.Tensor, indptr: torch.Tensor, edge_tok: torch.Tensor, edge_next: torch.Tensor,
                  status: torch.Tensor = None) -> torch.Tensor:
    """NEW: one step of every sequence's automaton -- ``atom_guide_advance``, the contract of DESIGN.md 4.18.  ``state`` int32 [batch]
    is updated in place over ``tokens`` int64 [batch] (compared as int64); the edges are CSR: ``indptr`` int32 [num_states + 1],
    ``edge_tok`` int32 [num_edges] ascending inside a state's range, ``edge_next`` int32 [num_edges].  FREE and DEAD stay; a token
    without an edge makes the state ``GUIDE_DEAD`` and sets ``GUIDE_REJECTED`` in ``status`` (int32 [1]; None: a word of its own that
    nobody reads); a state or a target outside 0 .. num_states - 1 makes it DEAD and sets ``GUIDE_BAD_STATE``.  All DEVICE tensors.
    Returns ``state``.  One launch; nothing is read back, nothing synchronises."""
    if not state.is_cuda:
        raise L.AtomHipError("state must live on the GPU: the guide ops have no CPU fallback")
    if state.dim() != 1 or state.numel() < 1:
        raise ValueError(f"state must be [batch], got {tuple(state.shape)}")
    batch = state.numel()
    _require_dev("guide", "state", state, torch.int32, (batch,))
    _require_dev("guide", "tokens", tokens, torch.int64, (batch,))
    if indptr.dim() != 1 or indptr.numel() < 2 or edge_tok.dim() != 1:
        raise ValueError(f"indptr must be [num_states + 1] and edge_tok [num_edges], got {tuple(indptr.shape)}, {tuple(edge_tok.shape)}")
    _require_dev("guide", "indptr", indptr, torch.int32)
    _require_dev("guide", "edge_tok", edge_tok, torch.int32)
    _require_dev("guide", "edge_next", edge_next, torch.int32, tuple(edge_tok.shape))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=state.device)
    _require_dev("guide", "status", status, torch.int32, (1,))
    num_edges = edge_tok.numel()
    st = L.lib().atom_guide_advance(state.data_ptr(), tokens.data_ptr(), batch, indptr.data_ptr(),
                                    edge_tok.data_ptr() if num_edges else None, edge_next.data_ptr() if num_edges else None,
                                    indptr.numel() - 1, num_edges, status.data_ptr(), L.current_stream(state.device))
    L.check(st, "atom_guide_advance")
    return state


GUIDE_MAX_ROWS = 9             # the verify rows per sequence atom_guide_walk_rows takes (guide_math.h kMaxWalkRows)


def guide_walk_rows(state: torch.Tensor, adds: torch.Tensor, row_state: torch.Tensor, input_ids: torch.Tensor, indptr: torch.Tensor,
                    edge_tok: torch.Tensor, edge_next: torch.Tensor, *, force: bool = True, status: torch.Tensor = None) -> torch.Tensor:
    """NEW: the automaton state behind every verify row of a speculative step -- ``atom_guide_walk_rows``, the contract of DESIGN.md
    4.19.  ``state`` int32 [batch]: the committed state (the one before ``input_ids[:, 0]``), updated in place by the commit of the
    last step: ``adds`` int32 [batch] rows of it were committed (``ops.spec_accept``'s ``adds``), ``row_state`` int32 [batch, Q] held
    its row states and receives this step's: ``row_state[b, j]`` is the state row j's logits are masked with.  ``input_ids`` int64
    [batch, Q] with contiguous rows (a view of a wider buffer is fine): column 0 the last emitted token, the rest the drafts; with
    ``force`` a draft that follows a state with a single edge is overwritten by that edge's token.  A draft without an edge makes the
    rows from it on ``GUIDE_DEAD`` and sets no bit; ``GUIDE_REJECTED`` is set by the commit alone.  ``input_ids=None``: the commit
    alone.  The tables as ``guide_advance``.  All DEVICE tensors.  Returns ``row_state``.  One launch; nothing is read back."""
    if not state.is_cuda:
        raise L.AtomHipError("state must live on the GPU: the guide ops have no CPU fallback")
    if state.dim() != 1 or state.numel() < 1 or row_state.dim() != 2 or not 1 <= row_state.size(1) <= GUIDE_MAX_ROWS:
        raise ValueError(f"state must be [batch] and row_state [batch, 1 .. {GUIDE_MAX_ROWS}], got {tuple(state.shape)}, {tuple(row_state.shape)}")
    batch, Q = state.numel(), row_state.size(1)
    _require_dev("guide", "state", state, torch.int32, (batch,))
    _require_dev("guide", "adds", adds, torch.int32, (batch,))
    _require_dev("guide", "row_state", row_state, torch.int32, (batch, Q))
    ids_ld = Q
    if input_ids is not None:
        if not (input_ids.is_cuda and input_ids.dtype == torch.int64 and tuple(input_ids.shape) == (batch, Q)
                and (Q == 1 or input_ids.stride(1) == 1) and (batch == 1 or input_ids.stride(0) >= Q)):
            raise TypeError(f"input_ids must be an int64 tensor of [{batch}, {Q}] with contiguous rows on the GPU")
        ids_ld = _row_stride(input_ids)
    if indptr.dim() != 1 or indptr.numel() < 2 or edge_tok.dim() != 1:
        raise ValueError(f"indptr must be [num_states + 1] and edge_tok [num_edges], got {tuple(indptr.shape)}, {tuple(edge_tok.shape)}")
    _require_dev("guide", "indptr", indptr, torch.int32)
    _require_dev("guide", "edge_tok", edge_tok, torch.int32)
    _require_dev("guide", "edge_next", edge_next, torch.int32, tuple(edge_tok.shape))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=state.device)
    _require_dev("guide", "status", status, torch.int32, (1,))
    num_edges = edge_tok.numel()
    st = L.lib().atom_guide_walk_rows(state.data_ptr(), adds.data_ptr(), row_state.data_ptr(),
                                      None if input_ids is None else input_ids.data_ptr(), ids_ld, batch, Q, indptr.data_ptr(),
                                      edge_tok.data_ptr() if num_edges else None, edge_next.data_ptr() if num_edges else None,
                                      indptr.numel() - 1, num_edges, 1 if force else 0, status.data_ptr(), L.current_stream(state.device))
    L.check(st, "atom_guide_walk_rows")
    return row_state
