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


LONG_S, LONG_FIRST, LONG_GUARD, LONG_CAP, LONG_LAYERS, LONG_LAYER = 200, 5, 8, 3, 2, 1
LONG_SENTINEL = 0x7BFF                       # fp16 65504 in the guard rows: survives only if they are never written
_LONG_LENS = (0, 1, 2, 3, 5, 15, 16, 17, 33)
_LONG_IDS = (2, 0, -1, 1, 3, 0, 1, -1, 2, 7, 1, 0)          # cyclically, no two neighbours name the same adapter (-1, 3 and 7: none)


def long_table():
    """(seg_indptr [S + 1], ids [S]) of a table longer than the 64 segments the kernels search at a time: S = 200; segments 0 .. 63
    and 128 .. 199 of 0, 1, 2, 3, 5, 15, 16, 17 and 33 rows in turn, 64 .. 127 all empty; the first segment starts at row 5 (and is
    empty itself); ids in no order, with -1 and ids at and above the capacity of 3.  The caller adds LONG_GUARD rows behind
    seg_indptr[S]"""
    lens = [0 if 64 <= s < 128 else _LONG_LENS[s % len(_LONG_LENS)] for s in range(LONG_S)]
    ids = [_LONG_IDS[s % len(_LONG_IDS)] for s in range(LONG_S)]
    ptr = [LONG_FIRST]
    for n in lens:
        ptr.append(ptr[-1] + n)
    assert ptr[-1] >= LONG_S and min(ids) < 0 and max(ids) >= LONG_CAP and sorted(ids) != ids
    assert set(lens[:64]) == set(lens[128:]) == set(_LONG_LENS) and lens[0] == 0
    return ptr, ids


def long_ids_shifted(ids):
    """the ids a search that loses its carried tile count would honour in the third block of 64 segments (128 .. 199): each segment
    there gets its neighbour's adapter"""
    n = LONG_S - 128
    return ids[:128] + [ids[128 + (s + 1) % n] for s in range(n)]


def long_case(rank, h1=320, h2=192):
    """exact inputs on the rows of ``long_table`` + the guard rows: (y, x, wa, wb) of add_lora h1 -> rank -> h2, and (y_s [rows, rank],
    x_e [rows, rank]) to run the two passes alone (shrink: y_s += x wa^T; expand: y += x_e wb^T); guard rows of y and y_s hold
    LONG_SENTINEL"""
    ptr, _ = long_table()
    y, x, wa, wb = exact_inputs(ptr[-1], h1, h2, rank, LONG_CAP, LONG_LAYERS, seed=700 + rank, guard=LONG_GUARD)
    g = torch.Generator().manual_seed(800 + rank)
    y_s = torch.randint(-8, 9, (y.size(0), rank), generator=g).half()
    x_e = torch.randint(-2, 3, (y.size(0), rank), generator=g).half()
    y[ptr[-1]:] = y_s[ptr[-1]:] = torch.tensor([LONG_SENTINEL], dtype=torch.int16).view(torch.float16)
    return y, x, wa, wb, y_s, x_e


def bits(t):
    return t.contiguous().view(torch.int16)
