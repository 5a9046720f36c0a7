"""Planted inputs and mutated references for the activation quantisers (atom_reorder_quant_f16, atom_rmsnorm_reorder_quant_f16,
atom_add_rmsnorm_reorder_quant_f16, atom_silu_mul_quant_f16, the quantisers inside atom_gemm_w4a4_multi_q) and for the u4 head
quantiser (quant_head_u4 and its copies), shared by tests/test_quant_planted_cpu.py, tests/test_gpu_quant_planted.py,
tests/test_gpu_quant.py and tests/test_gpu_kv.py.  numpy only: importable without torch and without a GPU.

Why: on random activations the rounding rule, the lower clamp, the reciprocal's operand and the all-zero-group rule are almost
unobserved -- an exact tie of the FP32 quotient is a 2^-13 event, code -8 is unreachable without a clip, a zero group never occurs.
The rows built here put such values into every group of a row:

  ties        clip 1.0: amax = 7 * 2^e (keeper: 127 * 2^e), every other channel (k + 1/2) * 2^e -- the scale is 2^e exactly in both
              modes, every quotient a true tie.  Any clip: `searched` rows -- for every fp16 amax of one binade the fp16 neighbours
              of every rounding boundary (k + 1/2) * scale are run through the reference and through a mutant, and the groups are
              filled with the values on which the two disagree (so the row moves under that mutant by construction).
  edges       an all-zero row, an all-zero group and an all-zero keeper inside ordinary rows, groups whose largest magnitude is
              negative (code -8 under clip < 1), fp16 max, subnormal halves, -0, a row of 1e-6, one huge value among tiny ones.

The references are the oracle's ops (oracle/atom_oracle.py).  ``mutate=name`` runs the same op with exactly ONE deliberate error
(MUTANTS); ``mutate=None`` IS the oracle's function.  The CPU test shows that every mutant that applies to a case changes at least one
code, scale bit or de-quantised bit of that case's planted rows, i.e. that a kernel with that error could not pass the GPU test,
which compares the kernels with the unmutated oracle bit for bit.

One limit, kernel-flavoured mode: a group whose FP32 scale rounds to a ZERO half (amax below 4 * 2^-24; the keeper: below 64 * 2^-24)
has non-zero codes and a stored scale of 0, and the sign of its de-quantised zeros is not specified (the kernels give +0, the oracle's
code x scale -0 for a negative code).  The subnormal rows keep amax at 16 * 2^-24 (keeper: 256 * 2^-24)."""
import functools

import numpy as np

from oracle import atom_oracle as O

f16, f32 = np.float16, np.float32
GROUP = 128

MUTANTS = ("round_rule", "clamp_low", "clip_on_keeper", "amax_no_abs", "recip_of_stored_scale", "norm_order", "eps", "zero_group",
           "dq_scale")
U4_MUTANTS = ("round_rule", "clamp", "abs_extrema")

# ------------------------------------------------------------------------------------------------ the cases both test files run
MODE_CLIPS = [("kernel", 1.0), ("kernel", 0.9), ("sim", 1.0), ("sim", 0.9)]       # reorder / SiLU planted rows
NORM_MODE_CLIPS = [("kernel", 1.0), ("sim", 0.9)]
EPS = [1e-5, 1e-6]
OTHER_EPS = {1e-5: 1e-6, 1e-6: 1e-5}
TAIL_H = 1024
NORM_HS = [1024, 4096]
# dense_layer_gemm_i4_multi_q: (q_op, N, K, nseg) -- the small shapes of test_quantiser_inside_the_gemm_launch_equals_quantiser_then_gemm
MULTI_Q_CASES = [("reorder", 64, 256, 1), ("rmsnorm", 1408, 640, 2), ("silu_mul", 512, 1408, 1), ("add_rmsnorm", 256, 5120, 3)]
# ... and every op on the other side of MULTI_Q_DOT_K.  One token runs the quantiser inside the dot-product kernel; two tokens run the one
# inside the decode-batch kernel up to K = MULTI_Q_DOT_K and the dot-product kernel's beyond: with these, every op's planted rows reach
# both quantisers at two tokens (the GPU test asserts the route).  The tie rows and the searched rows are built per group and hold at
# any H; the CPU tests keep their hidden sizes (of the random edge rows fewer survive SiLU's division by 32 unchanged at H = 4352).
MULTI_Q_DOT_K = 4096
MULTI_Q_ROUTE_CASES = [("add_rmsnorm", 256, 1024, 1), ("reorder", 64, 4352, 1), ("rmsnorm", 64, 4352, 1), ("silu_mul", 64, 4352, 1)]


def applies(mutant, op, mode, clip, dequant=True):
    """does `mutant` change the arithmetic of this case at all?  op: reorder | rmsnorm | add_rmsnorm | silu_mul"""
    if mutant in ("clamp_low", "clip_on_keeper"):
        return clip < 1.0                                    # code -8 / -128 needs |v * r| > 7.5; the keeper has no clip of its own
    if mutant == "recip_of_stored_scale":
        return mode == "kernel"
    if mutant == "dq_scale":
        return mode == "kernel" and dequant
    if mutant in ("norm_order", "eps"):
        return op in ("rmsnorm", "add_rmsnorm")
    return True


# ------------------------------------------------------------------------------------------------ the oracle's tail with one mutant
def _groups(v, n_bits, clip, mode, mut, keeper):
    """O.quant_groups_sim / O.quant_groups_kernel on [rows, n] with at most one deliberate error.  Returns (codes int8, stored scale
    f16, FP32 scale).  mut:
      round_rule             sim rounds half away from zero, kernel half to even
      clamp_low              lower clamp at -qmax
      clip_on_keeper         the keeper group takes the clip too
      amax_no_abs            the group maximum without abs
      recip_of_stored_scale  kernel: r = 1 / float(half(scale_f))
      zero_group             sim: no 1e-5 clamp of amax (scale 0, 0 / 0); kernel: no guard (0 * inf = NaN -> the lowest code)"""
    qmax = 2 ** (n_bits - 1) - 1
    qmin = -qmax if mut == "clamp_low" else -qmax - 1
    c = clip if (not keeper or mut == "clip_on_keeper") else 1.0
    with np.errstate(all="ignore"):
        if mode == "sim":
            v16 = np.asarray(v, dtype=f16)
            amax = v16.max(axis=-1) if mut == "amax_no_abs" else np.abs(v16).max(axis=-1)
            if mut != "zero_group":
                amax = np.maximum(amax, f16(1e-5))
            if c < 1.0:
                amax = (amax.astype(f32) * f32(c)).astype(f16)
            scale = (amax.astype(f32) / f32(qmax)).astype(f16)
            q = (v16.astype(f32) / scale.astype(f32)[..., None]).astype(f16).astype(f32)
            q = O._round_half_away(q) if mut == "round_rule" else np.rint(q)
            sf = scale.astype(f32)
        elif mode == "kernel":
            v32 = np.asarray(v, dtype=f32)
            amax = (v32.max(axis=-1) if mut == "amax_no_abs" else np.abs(v32).max(axis=-1)).astype(f32)
            if c < 1.0:
                amax = (amax * f32(c)).astype(f32)
            sf = (amax / f32(qmax)).astype(f32)
            rs = sf.astype(f16).astype(f32) if mut == "recip_of_stored_scale" else sf
            r = (f32(1.0) / rs).astype(f32)
            t = (v32 * r[..., None]).astype(f32)
            q = np.rint(t) if mut == "round_rule" else O._round_half_away(t)
            if mut != "zero_group":
                q = np.where(sf[..., None] == 0, f32(0), q)
            scale = sf.astype(f16)
        else:
            raise ValueError(mode)
        q = np.clip(np.where(np.isnan(q), f32(qmin), q), qmin, qmax)
    return q.astype(np.int8), scale, sf


def _tail(y, mode, clip, mut=None):
    """O._quant_row_tail with one mutant; also returns the FP32 scales (s4f, s8f)"""
    M, K = y.shape
    K4 = K - GROUP
    G = K4 // GROUP
    q4, s4, s4f = _groups(y[:, :K4].reshape(M * G, GROUP), 4, clip, mode, mut, False)
    q8, s8, s8f = _groups(y[:, K4:], 8, clip, mode, mut, True)
    return dict(q4=q4.reshape(M, K4), s4=s4.reshape(M, G), q8=q8, s8=s8, s4f=s4f.reshape(M, G), s8f=s8f)


def _check(mutate):
    assert mutate is None or mutate in MUTANTS, mutate
    return mutate


def quant_tail(y16, mode, clip, mutate=None):
    """the shared tail on rows already in channel order (reorder_fp16_i4 without an index)"""
    y = np.asarray(y16, dtype=f16)
    y = y if mode == "sim" else y.astype(f32)
    return O._quant_row_tail(y, mode, clip) if _check(mutate) is None else _tail(y, mode, clip, mutate)


def reorder_quant(x16, idx, mode, clip, mutate=None):
    if idx is None:
        return quant_tail(x16, mode, clip, mutate)
    if _check(mutate) is None:
        return O.reorder_quant(x16, idx, mode, clip)
    return quant_tail(np.asarray(x16, dtype=f16)[:, np.asarray(idx).astype(np.int64)], mode, clip, mutate)


def rmsnorm_reorder_quant(x16, w16, eps, idx, mode, clip, mutate=None):
    """mutants of its own: norm_order (the product x * w * r in the OTHER mode's order and roundings), eps (the other of 1e-5 / 1e-6)"""
    if _check(mutate) is None:
        return O.rmsnorm_reorder_quant(x16, w16, eps, idx, mode, clip)
    if mutate == "eps":
        eps = OTHER_EPS[eps]
    order = {"sim": "kernel", "kernel": "sim"}[mode] if mutate == "norm_order" else mode
    y = O.rmsnorm_f16(x16, w16, eps, order)[:, np.asarray(idx).astype(np.int64)]
    return _tail(y if mode == "sim" else y.astype(f32), mode, clip, mutate)


def silu_mul_quant(a16, b16, mode, clip, mutate=None):
    if _check(mutate) is None:
        return O.silu_mul_quant(a16, b16, mode, clip)
    return _tail(O.silu_mul(a16, b16, mode), mode, clip, mutate)


def dequant(t, mode, mutate=None):
    """the de-quantised tensor (return_dequant): half(code * stored half scale) in both modes = O.act_dequant_sim.
    dq_scale: the kernel-flavoured mode multiplies by the FP32 scale instead"""
    if _check(mutate) != "dq_scale" or mode != "kernel":
        return O.act_dequant_sim(t)
    M, K4 = t["q4"].shape
    with np.errstate(over="ignore"):
        body = (t["q4"].astype(f32).reshape(M, -1, GROUP) * t["s4f"][..., None]).astype(f16).reshape(M, K4)
        return np.concatenate([body, (t["q8"].astype(f32) * t["s8f"][:, None]).astype(f16)], axis=1)


def moved(ref, mut, mode, with_dequant=True):
    """number of codes, scale bits and de-quantised bits in which two results of one op differ"""
    bits = lambda a: np.ascontiguousarray(a, dtype=f16).view(np.uint16)
    n = int((ref["q4"] != mut["q4"]).sum() + (ref["q8"] != mut["q8"]).sum())
    n += int((bits(ref["s4"]) != bits(mut["s4"])).sum() + (bits(ref["s8"]) != bits(mut["s8"])).sum())
    if with_dequant:
        n += int((bits(ref["xq"]) != bits(mut["xq"])).sum())
    return n


def run(op, args, mode, clip, mutate=None):
    """one op + its de-quantised tensor: op reorder (x, idx) | rmsnorm (x, w, eps, idx) | silu_mul (a, b).  (add_rmsnorm is rmsnorm
    on the fp16 sum x + residual.)"""
    if op == "reorder":
        t = reorder_quant(args[0], args[1], mode, clip, mutate)
    elif op == "rmsnorm":
        t = rmsnorm_reorder_quant(args[0], args[1], args[2], args[3], mode, clip, mutate)
    else:
        t = silu_mul_quant(args[0], args[1], mode, clip, mutate)
    t = dict(t)
    t["xq"] = dequant(t, mode, mutate)
    return t


# ------------------------------------------------------------------------------------------------ planted groups
def _rand(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(f16)


@functools.lru_cache(maxsize=None)
def searched_groups(mode, clip, n_bits, mutant, sign):
    """For every fp16 amax a of [1, 2) (times `sign`): the fp16 values within 2 ulps of every rounding boundary (k + 1/2) * scale,
    |v| <= a, run as one group through the reference and through `mutant`; returns [(amax, values on which the codes differ)],
    best first (at most 8).  Groups scale by powers of two (normal range), so one binade of amax stands for all."""
    keeper = n_bits == 8
    qmax = 2 ** (n_bits - 1) - 1
    a = (np.arange(1024, dtype=np.uint16) + np.uint16(0x3C00)).view(f16)                       # 1.0 .. 2 - 2^-10
    s = a.astype(np.float64) * (clip if not keeper else 1.0) / qmax
    k = np.arange(0, qmax + 1, dtype=np.float64) + 0.5
    centre = (s[:, None] * k[None, :]).astype(f16)                                             # [1024, qmax + 1]
    cand = []
    for d in (-2, -1, 0, 1, 2):
        nb = (centre.view(np.uint16).astype(np.int32) + d).astype(np.uint16).view(f16)
        cand += [nb, -nb]
    v = np.concatenate(cand, axis=1)
    v = np.where(np.abs(v) <= a[:, None], v, f16(0))
    grp = np.concatenate([(sign * a)[:, None].astype(f16), v], axis=1)
    g = grp if mode == "sim" else grp.astype(f32)
    q0 = _groups(g, n_bits, clip, mode, None, keeper)[0]
    q1 = _groups(g, n_bits, clip, mode, mutant, keeper)[0]
    diff = q0 != q1
    order = np.argsort(-diff.sum(axis=1), kind="stable")[:8]
    return [(grp[i, 0], np.unique(grp[i][diff[i]])) for i in order if diff[i].any()]


def _fill(amax, vals, e):
    """one 128-channel group: amax once, the values cycled, everything times 2^e"""
    body = np.resize(np.asarray(vals, dtype=f16), GROUP - 1) if len(vals) else np.zeros(GROUP - 1, dtype=f16)
    return (np.concatenate([[amax], body]).astype(f32) * f32(2.0 ** e)).astype(f16)


def searched_rows(mode, clip, H=TAIL_H):
    """one row per value-dependent mutant (round_rule; kernel: recip_of_stored_scale): INT4 groups and keeper filled with the
    values searched_groups found, amax positive and negative in turn, at several binades"""
    G = H // GROUP - 1
    rows = []
    for mutant in ("round_rule",) + (("recip_of_stored_scale",) if mode == "kernel" else ()):
        row = np.zeros(H, dtype=f16)
        for g in range(G + 1):
            hits = searched_groups(mode, clip, 8 if g == G else 4, mutant, 1.0 if g % 2 == 0 else -1.0)
            if hits:
                amax, vals = hits[(g // 2) % len(hits)]
                row[g * GROUP:(g + 1) * GROUP] = _fill(amax, vals, (g % 7) - 3)
        rows.append(row)
    return np.stack(rows)


def tie_rows(H=TAIL_H):
    """true ties in both modes at clip 1.0 (two rows): INT4 group g: amax = +-7 * 2^e, the other channels (k + 1/2) * 2^e, k = -7 .. 6
    (scale 2^e exactly); keeper: +-127 * 2^e and (k + 1/2) * 2^e, k = -128 .. 126.  Row 1 has the signs of the maxima reversed."""
    G = H // GROUP - 1
    rows = np.zeros((2, H), dtype=f16)
    for r in range(2):
        for g in range(G + 1):
            e = (g % 6) - 3 + r
            sgn = 1.0 if (g + r) % 2 == 0 else -1.0
            if g < G:
                k = np.resize(np.arange(-7, 7), GROUP - 1) + 0.5
                top = 7.0
            else:
                k = (np.arange(GROUP - 1) * 2 - 127 + r) + 0.5                   # -126.5 .. 125.5 (row 1: + 1), both parities of floor
                top = 127.0
            rows[r, g * GROUP:(g + 1) * GROUP] = np.concatenate([[sgn * top], k]) * 2.0 ** e
    return rows


def edge_rows(H=TAIL_H, seed=21):
    """the edge rows, in channel order; see ROW_NAMES"""
    G = H // GROUP - 1
    base = lambda i: _rand(H, seed + i, 1.5)
    rows = []
    rows.append(np.zeros(H, dtype=f16))                                          # zero_row
    r = base(1); r[GROUP:2 * GROUP] = 0; rows.append(r)                          # zero_group: one all-zero INT4 group
    r = base(2); r[G * GROUP:] = 0; rows.append(r)                               # zero_keeper
    r = np.abs(base(3)) * f16(0.25)                                              # negative_max: every group's largest magnitude is negative
    r[3::GROUP] = -np.abs(base(4)[3::GROUP]) - f16(2.0); rows.append(r.astype(f16))
    r = base(5); r[7] = 65504.0; r[G * GROUP + 5] = -65504.0; rows.append(r)     # fp16_max (INT4 group 0 and the keeper)
    r = (((np.arange(H) * 7) % 9 - 4) * 4).astype(f32) * f32(2.0 ** -24); r[G * GROUP:] *= 16; rows.append(r.astype(f16))   # subnormal: amax = 16 * 2^-24, keeper 256 * 2^-24
    r = base(6); r[::2] = -0.0; rows.append(r)                                   # negative_zero
    rows.append(np.full(H, 1e-6, dtype=f16))                                     # tiny: a row of 1e-6
    r = (base(7).astype(f32) * f32(1e-4)).astype(f16); r[::GROUP] = 30000.0; r[GROUP::2 * GROUP] = -30000.0; rows.append(r)   # huge_among_tiny
    rows.append((base(8).astype(f32) * f32(1e-3)).astype(f16))                   # small
    rows.append(base(9))                                                         # random
    return np.stack(rows).astype(f16)


EDGE_NAMES = ("zero_row", "zero_group", "zero_keeper", "negative_max", "fp16_max", "subnormal", "negative_zero", "tiny", "huge_among_tiny",
              "small", "random")


def tail_rows(mode, clip, H=TAIL_H):
    """the planted rows of the shared tail for one (mode, clip), fp16 [rows, H] in channel order: ties, searched, edges"""
    return np.concatenate([tie_rows(H), searched_rows(mode, clip, H), edge_rows(H)], axis=0)


def scatter(y, idx):
    """x with x[:, idx] == y: the input of an op that gathers by idx"""
    x = np.empty_like(y)
    x[:, np.asarray(idx).astype(np.int64)] = y
    return x


def perm(H, seed=3):
    return np.random.default_rng(seed).permutation(H).astype(np.int16)


# ------------------------------------------------------------------------------------------------ SiLU: saturated gates
GATE = 32.0                       # a power of two in [17, 48]: silu(32) * b = 32 b exactly, in FP32 and in half


def silu_planted(mode, clip, H=TAIL_H):
    """gate a, up b (fp16 [rows, H]) with silu(a) * b == the planted tail rows where those are 32 x a half (the rest land on
    neighbouring values; the product is exact everywhere): a = 32 (0 on the all-zero groups, so that 0 * b = +-0), b = y / 32.  Then
    three rows of gates drawn from {0} u [17, 48] (1/32 steps) against random b: 22-bit FP32 products in the kernel-flavoured mode."""
    y = tail_rows(mode, clip, H)
    a = np.full(y.shape, GATE, dtype=f16)
    b = (y.astype(f32) / f32(GATE)).astype(f16)
    zero = (y.reshape(len(y), -1, GROUP) == 0).all(axis=-1)                      # all-zero groups: gate 0, up random
    rb = _rand(y.size, 31, 2.0).reshape(y.shape)
    zmask = np.repeat(zero, GROUP, axis=1)
    a[zmask] = 0
    b[zmask] = rb[zmask]
    a2, b2 = silu_random(3, H, seed=33)
    return np.concatenate([a, a2]), np.concatenate([b, b2])


def silu_random(M, H, seed):
    """gates from {0} u [17, 48] in steps of 1/32 (one in eight is 0), up = N(0, 2) with 128 outlier channels: exact products"""
    g = np.random.default_rng(seed)
    a = (g.integers(17 * 32, 48 * 32 + 1, size=(M, H)) / 32.0).astype(f16)
    a[g.random((M, H)) < 0.125] = 0
    b = g.standard_normal((M, H)).astype(f32) * 2
    b[:, g.permutation(H)[:128]] *= 10.0
    return a, b.astype(f16)


def silu_exact(a, b, mode):
    """what silu(a) * b is on saturated gates: a * b, exact in FP32 (kernel) / rounded once to half (sim)"""
    p = a.astype(f32) * b.astype(f32)
    return p if mode == "kernel" else p.astype(f16)


# ------------------------------------------------------------------------------------------------ RMSNorm rows
NORM_NAMES = ("zero_row", "tiny", "fp16_max", "sumsq_2p24", "subnormal", "small", "random", "random2", "ties")


@functools.lru_cache(maxsize=None)
def _norm_base(H, seed=41):
    g = np.random.default_rng(seed + H)
    rows = [np.zeros(H, dtype=f16), np.full(H, 1e-6, dtype=f16)]
    r = _rand(H, seed + 1, 1.5); r[11] = 65504.0; rows.append(r)
    c = int(round((2.0 ** 24 / H) ** 0.5))                                       # 128 at H = 1024, 64 at 4096
    rows.append(((c + g.integers(-1, 2, H)) * g.choice([-1, 1], H)).astype(f16))
    rows.append((g.integers(-1023, 1024, H).astype(f32) * f32(2.0 ** -24)).astype(f16))
    rows.append((_rand(H, seed + 2).astype(f32) * f32(1e-2)).astype(f16))
    rows.append(_rand(H, seed + 3, 2.0))
    r = _rand(H, seed + 4).astype(f32); r[g.permutation(H)[:128]] *= 20.0; rows.append(r.astype(f16))
    rows.append(tie_rows(H)[0])
    w = (1.0 + 0.1 * g.standard_normal(H)).astype(f16)
    return np.stack(rows).astype(f16), w, g.permutation(H).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _norm_searched(H, mode, clip, eps):
    """the kernel-flavoured mode rounds an FP32 quotient, and behind a normalisation no value can be planted: of ~2M random values
    (rows of N(0, 1.5)) keep the two rows on which the round_rule mutant moves the most codes (a tie is a ~1e-5 event per value)"""
    _, w, idx = _norm_base(H)
    x = _rand((2 ** 21 // H) * H, 43 + H, 1.5).reshape(-1, H)
    ref = rmsnorm_reorder_quant(x, w, eps, idx, mode, clip)
    mut = rmsnorm_reorder_quant(x, w, eps, idx, mode, clip, "round_rule")
    n = (ref["q4"] != mut["q4"]).sum(axis=1) + (ref["q8"] != mut["q8"]).sum(axis=1)
    return x[np.argsort(-n, kind="stable")[:2]].copy()


def norm_rows(H, mode="sim", clip=0.9, eps=1e-5):
    """x (fp16 [rows, H]), weight, reorder index for the RMSNorm ops: a zero row, a row of 1e-6, one fp16-max element, a row of
    integers whose squares sum to 2^24 +- (the top of FP32's exact integers: the order of the sum decides the last bit), subnormal
    halves, a small row (variance ~ 1e-4: eps counts), two random rows (one with outlier channels), the clip-1.0 tie row; in the
    kernel-flavoured mode two rows more, searched for ties (_norm_searched)."""
    x, w, idx = _norm_base(H)
    if mode == "kernel":
        x = np.concatenate([x, _norm_searched(H, mode, clip, eps)])
    return x.copy(), w.copy(), idx.copy()


def add_split(s, seed=51):
    """x, residual (fp16) with x + residual == s exactly in half and both finite: residual = half(s / 2) + a small half offset where
    that keeps the sum exact, x = s - residual"""
    s = np.asarray(s, dtype=f16)
    res = (s.astype(f32) * f32(0.5)).astype(f16)
    x = (s.astype(f32) - res.astype(f32)).astype(f16)
    ok = (x.astype(f32) + res.astype(f32)).astype(f16).view(np.uint16) == s.view(np.uint16)
    res = np.where(ok, res, f16(0))
    x = np.where(ok, x, s)
    return x.astype(f16), res.astype(f16)


# ------------------------------------------------------------------------------------------------ the u4 head quantiser
U4_NAMES = ("ties_e-3", "ties_e0", "ties_e2", "ties_mixed_sign", "constant", "constant_zero", "constant_negative", "all_negative",
            "all_positive", "outlier", "subnormal_scale", "random")


def u4_vectors():
    """float32 [n, 128], every value exact in fp16 (so the fp16 and the FP32 entry points see the same numbers):
    lo = 0, hi = 15 * 2^e and (k + 1/2) * 2^e between (scale 2^e: ties); the same around zero (lo = -8 * 2^e); constant vectors (scale
    0); all-negative and all-positive ranges; one outlier; a range of 15 * 2^-20 (the fp16 scale 2^-20 is subnormal); random."""
    g = np.random.default_rng(61)
    k = np.resize(np.arange(15), 126) + 0.5
    rows = []
    for e in (-3, 0, 2):
        rows.append(np.concatenate([[0.0, 15.0], k]) * 2.0 ** e)
    rows.append((np.concatenate([[0.0, 15.0], k]) - 8.0) * 0.5)
    rows += [np.full(128, 0.25), np.zeros(128), np.full(128, -3.5)]
    rows.append(-1.0 - 2.0 * g.random(128))
    rows.append(1.0 + 2.0 * g.random(128))
    r = g.standard_normal(128) * 0.01; r[77] = 100.0; rows.append(r)
    rows.append((np.concatenate([[0.0, 15.0], k]) - 4.0) * 2.0 ** -20)
    rows.append(g.standard_normal(128) * 2)
    v = np.stack(rows).astype(f16)
    g.permuted(v[:4], axis=1, out=v[:4])                                         # the extrema anywhere in the vector
    return v.astype(f32)


def u4_matrix(batch, heads, seed=0):
    """[batch, heads * 128] float32: the planted vectors dealt over (token, head), starting at a different vector per seed"""
    v = u4_vectors()
    i = (np.arange(batch * heads) + seed) % len(v)
    return np.ascontiguousarray(v[i].reshape(batch, heads * 128))


def quant_o4(D32, mutate=None):
    """O.quant_o4 with one mutant: round_rule (half to even), clamp (the code clamped as a SIGNED nibble: 8 .. 15 become 7),
    abs_extrema (extrema of |x|: O.quant_o4's ref_extrema mode)"""
    assert mutate is None or mutate in U4_MUTANTS, mutate
    if mutate is None:
        return O.quant_o4(D32)
    if mutate == "abs_extrema":
        return O.quant_o4(D32, ref_extrema=True)
    D32 = np.asarray(D32, dtype=f32)
    M, N = D32.shape
    g = D32.reshape(M, N // GROUP, GROUP)
    mx, mn = g.max(axis=-1), g.min(axis=-1)
    scale = ((mx - mn) / f32(15)).astype(f32)
    zero = (-mn).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (f32(1.0) / scale).astype(f32)
        t = ((g + zero[..., None]).astype(f32) * r[..., None]).astype(f32)
        q = np.rint(t) if mutate == "round_rule" else O._round_half_away(t)
    q = np.where(scale[..., None] == 0, f32(0), q)
    q = np.clip(q, 0, 7 if mutate == "clamp" else 15).astype(np.int16).reshape(M, N)
    packed = ((q[:, 0::2] & 0xF) | ((q[:, 1::2] & 0xF) << 4)).astype(np.uint8)
    return packed, np.stack([scale.astype(f16), zero.astype(f16)], axis=-1)
