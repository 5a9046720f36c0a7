"""The checker's restatement of the LoRA ops (include/atom_hip.h, atom_bgmv_f16 / atom_add_lora_f16) in float64 on the CPU, and the
EXACT-ARITHMETIC inputs of the core tests: x integers in [-2, 2], A and B in {-1, 0, 1}, y0 integers in [-8, 8], scale a power of
two.  Every partial sum is then an integer far below 2^24, the intermediate t an integer below 2048 and the result a multiple of the
scale below 512 -- all exactly representable wherever the kernel keeps them, so the comparison is bit for bit whatever order the
kernel sums in.  ``add_lora`` asserts that precondition itself (``exact=True``): a changed seed can never turn such a test into a
tolerance test silently."""
import torch


def segments(rows, indices, seg_indptr=None):
    """[(first row, end row, adapter id)] of a call: one row per id, or the segments of ``seg_indptr``"""
    ids = [int(i) for i in indices]
    if seg_indptr is None:
        assert len(ids) == rows
        return [(i, i + 1, a) for i, a in enumerate(ids)]
    ptr = [int(i) for i in seg_indptr]
    assert len(ptr) == len(ids) + 1
    return [(ptr[s], ptr[s + 1], a) for s, a in enumerate(ids)]


def _is_half(t):
    return bool((t == t.half().double()).all())


def bgmv(y, x, w_T_all, indices, layer_idx, scale, seg_indptr=None, exact=False):
    """y fp16 [rows, H2] (not modified), x fp16 [rows, H1], w fp16 [capacity, L, H2, H1] -> fp16 [rows, H2]: rows of segments with an id
    outside 0 .. capacity - 1 and rows behind the last segment are y's, bit for bit"""
    out = y.clone()
    for b, e, a in segments(x.size(0), indices, seg_indptr):
        if 0 <= a < w_T_all.size(0) and e > b:
            r = y[b:e].double() + float(scale) * (x[b:e].double() @ w_T_all[a, layer_idx].double().t())
            assert not exact or _is_half(r), "not an exact-arithmetic case"
            out[b:e] = r.half()
    return out


def add_lora(y, x, wa_T_all, wb_T_all, indices, layer_idx, scale, seg_indptr=None, exact=False, round_t=True):
    """two passes, t rounded to fp16 between them (``round_t=False``: the variant a kernel that keeps t in FP32 would compute)"""
    out = y.clone()
    for b, e, a in segments(x.size(0), indices, seg_indptr):
        if 0 <= a < wa_T_all.size(0) and e > b:
            t = x[b:e].double() @ wa_T_all[a, layer_idx].double().t()
            assert not exact or not round_t or _is_half(t), "t is not exactly representable in fp16"
            if round_t:
                t = t.half().double()
            r = y[b:e].double() + float(scale) * (t @ wb_T_all[a, layer_idx].double().t())
            assert not exact or _is_half(r), "not an exact-arithmetic case"
            out[b:e] = r.half()
    return out


def add_lora_rows(y, x, wa_T_all, wb_T_all, row_ids, layer_idx, scale):
    """the direct per-row, per-element loop (float64 python sums) the helpers above are checked against"""
    out = y.clone()
    for i, a in enumerate(int(v) for v in row_ids):
        if not 0 <= a < wa_T_all.size(0):
            continue
        A, B = wa_T_all[a, layer_idx].double(), wb_T_all[a, layer_idx].double()
        t = [float(torch.tensor(sum(float(x[i, h]) * float(A[j, h]) for h in range(x.size(1)))).half()) for j in range(A.size(0))]
        for n in range(B.size(0)):
            out[i, n] = torch.tensor(float(y[i, n]) + float(scale) * sum(t[j] * float(B[n, j]) for j in range(len(t)))).half()
    return out


def exact_inputs(rows, h1, h2, rank, capacity, layers, seed, guard=0):
    """(y0 [rows + guard, h2], x [rows + guard, h1], wa [capacity, layers, rank, h1], wb [capacity, layers, h2, rank]) fp16 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).half()
    return ri(-8, 8, rows + guard, h2), ri(-2, 2, rows + guard, h1), ri(-1, 1, capacity, layers, rank, h1), ri(-1, 1, capacity, layers, h2, rank)


def bits(t):
    return t.contiguous().view(torch.int16)
