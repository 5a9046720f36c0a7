"""Planted operands for the W4A4 GEMM family and their reference, shared by the CPU tests (tests/test_gemm_planted_cpu.py: every family
meets its exactness bound and tells its wrong rules) and the GPU tests (tests/test_gpu_gemm_planted.py: every route of
tests/gemm_route_cases.py on them, bit for bit).

A family is a function (M, N, K, seed) -> operand dict with the keys of tests/helpers.rand_gemm_operands (codes unpacked, sA [M, G],
sB [G, N]).  The reference is expected(d, entry=..., wrong=None): the definition of include/atom_hip.h,
    D[m, n] = sum_g (A4_g . B4_g^T) sA[m, g] sB[g, n] + (A8 . B8^T) sA8[m] sB8[n],
in float64 on exact integer dot products, rounded ONCE to the output type; wrong= evaluates the same under one named wrong rule.

Exactness.  In the exact families every scale is 0 or a power of two.  Let u be the smallest non-zero scale product; every term
idot * sA * sB is then an integer multiple of u, and margin(d) bounds sum_g |term| / u from above by Cauchy-Schwarz on the codes
actually generated (|a . b| <= |a| |b| per group: tight for the extreme codes).  While that bound is below 2^24 every partial sum of
any subset of the terms, in any order, is an integer below 2^24 in units of u, i.e. an exact FP32 number: every route -- tile kernels,
K groups, eight waves, lane butterflies, split-K -- must give half(float64 sum).  A family narrows its exponent spread, from
min(6, ...) down, until its operands meet the bound (fit()).
"""
import numpy as np
import torch

from tests import gemm_route_cases as _R

G128 = 128
LIMIT = 24.0                                                   # log2 of the FP32 integer range, in units of u

RULES = ("pair_even", "pair_swap", "keeper_neighbour", "group_shift", "clamp_symmetric", "nibble_unsigned", "keeper_unsigned",
         "rtz", "half_away", "flush_scale", "flush_out", "saturate")


def p2(e):
    """2^e as fp16 (e >= -24: subnormals included)"""
    return np.ldexp(1.0, np.asarray(e)).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------- codes
_codes_cache = {}


def rand_codes(M, N, K, seed):
    """uniform int4 / int8 codes of a shape, made once (the families that use random codes share them; one shape is kept)"""
    key = (M, N, K, seed)
    if key not in _codes_cache:
        _codes_cache.clear()
        g = np.random.default_rng(seed)
        K4 = K - G128
        _codes_cache[key] = dict(qa4=g.integers(-8, 8, size=(M, K4), dtype=np.int8), qb4=g.integers(-8, 8, size=(N, K4), dtype=np.int8),
                                 qa8=g.integers(-128, 128, size=(M, 128), dtype=np.int16).astype(np.int8),
                                 qb8=g.integers(-128, 128, size=(N, 128), dtype=np.int16).astype(np.int8))
    return dict(_codes_cache[key])


def _norms(q, width=G128):
    """Euclidean norm of every 128-code group: [rows, groups] float64"""
    x = np.asarray(q).reshape(q.shape[0], -1, width).astype(np.float32)
    return np.sqrt(np.einsum("rgk,rgk->rg", x, x).astype(np.float64))


def unit(d):
    """the smallest non-zero scale product of the operands"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    sA, sB = f(d["sA"]), f(d["sB"])
    best = np.inf
    for g in range(sB.shape[0]):
        a, b = np.abs(sA[:, g]), np.abs(sB[g])
        if (a > 0).any() and (b > 0).any():
            best = min(best, a[a > 0].min() * b[b > 0].min())
    a, b = np.abs(f(d["sA8"])), np.abs(f(d["sB8"]))
    if (a > 0).any() and (b > 0).any():
        best = min(best, a[a > 0].min() * b[b > 0].min())
    return best


def margin(d):
    """log2 of an upper bound of max_{m, n} sum_g |idot_g sA sB| in units of unit(d), from the operands themselves (module docstring)"""
    f = lambda a: np.abs(np.asarray(a, dtype=np.float64))
    na, nb = _norms(d["qa4"]) * f(d["sA"]), _norms(d["qb4"]) * f(d["sB"]).T           # [M, G], [N, G]
    na8, nb8 = _norms(d["qa8"])[:, 0] * f(d["sA8"]), _norms(d["qb8"])[:, 0] * f(d["sB8"])
    top = max((na[i:i + 1024] @ nb.T + np.outer(na8[i:i + 1024], nb8)).max() for i in range(0, na.shape[0], 1024))
    return float(np.log2(max(top / unit(d), 1.0)))


def is_exact(d):
    s = np.concatenate([np.asarray(d[k], dtype=np.float64).reshape(-1) for k in ("sA", "sB", "sA8", "sB8")])
    s = np.abs(s[s != 0])
    return bool((np.frexp(s)[0] == 0.5).all())


def fit(make, G, room=3):
    """the operands of make(spread) at the widest exponent spread, from min(6, 9 - ceil(log2 G) + room) down, that meets the bound
    (room = 0 covers codes at the limit; random codes have room for more, and the bound is checked on what was made)"""
    top = min(6, 9 - int(np.ceil(np.log2(max(G, 1)))) + room)
    for spread in range(max(top, 0), -1, -1):
        d = make(spread)
        if margin(d) < LIMIT:
            d["spread"] = spread
            return d
    raise AssertionError("no exponent spread meets the exactness bound")


def pairs_shared(d):
    return bool((d["sB"][:, 0::2] == d["sB"][:, 1::2]).all())


def unequal_pair_share(d):
    return float((d["sB"][:, 0::2] != d["sB"][:, 1::2]).mean())


# ------------------------------------------------------------------------------------------------------------- families
def _dims(M, N, K):
    assert K % G128 == 0 and K >= 2 * G128 and N % 2 == 0
    return K - G128, (K - G128) // G128


def own_scales(M, N, K, seed, base=-6, free=False):
    """random codes; the weight scales of channels 2j and 2j + 1 differ in EVERY group and pair (exact variant: exponents drawn per
    (g, n) with the odd channel's forced off the even one's; free variant: U(0.005, 0.05) per channel), activation scales drawn per
    (m, g), keeper scales differ between neighbouring channels"""
    K4, G = _dims(M, N, K)
    c = rand_codes(M, N, K, seed)
    g = np.random.default_rng(seed + 1)
    if free:
        u = lambda *s: g.uniform(0.005, 0.05, size=s).astype(np.float16)
        return dict(c, sA=u(M, G), sA8=u(M), sB=u(G, N), sB8=u(N))

    def make(spread):
        r = np.random.default_rng(seed + 2)
        sb = max(1, (spread + 1) // 2)
        sa = max(0, spread - sb)
        even = r.integers(0, sb + 1, size=(G, N // 2))
        odd = (even + 1 + r.integers(0, sb, size=(G, N // 2))) % (sb + 1)             # never the even channel's exponent
        eb = np.stack([even, odd], axis=-1).reshape(G, N)
        k0 = r.integers(0, 2, size=N // 2)
        eb8 = np.stack([k0, 1 - k0], axis=-1).reshape(N)
        return dict(c, sA=p2(base + r.integers(0, sa + 1, size=(M, G))), sA8=p2(base + r.integers(0, 2, size=M)), sB=p2(base + eb),
                    sB8=p2(base + eb8))
    return fit(make, G)


def one_pair_off(M, N, K, seed, where="first"):
    """random codes, weight scales shared by every channel pair except ONE (group, pair): the first of the first group or the last of
    the last group, whose odd channel is a factor 2 off"""
    K4, G = _dims(M, N, K)
    c = rand_codes(M, N, K, seed)

    def make(spread):
        r = np.random.default_rng(seed + 3)
        sb = max(1, (spread + 1) // 2)
        sa = max(0, spread - sb)
        eb = np.repeat(r.integers(0, sb + 1, size=(G, N // 2)), 2, axis=1)
        gi, n = (0, 1) if where == "first" else (G - 1, N - 1)
        eb[gi, n] = eb[gi, n] + 1 if eb[gi, n] < sb else eb[gi, n] - 1
        d = dict(c, sA=p2(-6 + r.integers(0, sa + 1, size=(M, G))), sA8=p2(-6 + r.integers(0, 2, size=M)), sB=p2(-6 + eb),
                 sB8=p2(-6 + np.repeat(r.integers(0, 2, size=N // 2), 2)))
        d["planted"] = (gi, n // 2)
        return d
    return fit(make, G)


def extreme_codes(M, N, K, seed, base=-6):
    """all int4 codes -8 and all keeper codes -128 on both sides; odd activation rows and every second pair of weight rows +7 / +127;
    one all-zero activation row (M >= 3) and one all-zero weight row; power-of-two scales, shared by channel pairs"""
    K4, G = _dims(M, N, K)
    qa4, qb4 = np.full((M, K4), -8, np.int8), np.full((N, K4), -8, np.int8)
    qa8, qb8 = np.full((M, 128), -128, np.int8), np.full((N, 128), -128, np.int8)
    qa4[1::2], qa8[1::2] = 7, 127
    hi = (np.arange(N) // 2) % 2 == 1
    qb4[hi], qb8[hi] = 7, 127
    if M >= 3:
        qa4[M // 2], qa8[M // 2] = 0, 0
    qb4[N - 3], qb8[N - 3] = 0, 0
    c = dict(qa4=qa4, qb4=qb4, qa8=qa8, qb8=qb8)

    def make(spread):
        r = np.random.default_rng(seed + 4)
        sb = (spread + 1) // 2
        sa = spread - sb
        return dict(c, sA=p2(base + r.integers(0, sa + 1, size=(M, G))), sA8=p2(np.full(M, base)),
                    sB=p2(base + np.repeat(r.integers(0, sb + 1, size=(G, N // 2)), 2, axis=1)), sB8=p2(np.full(N, base)))
    return fit(make, G, room=0)                                 # the codes are at the limit


# targets of the planted sums, in units of the scale product: T[m, n] = sign[m] * (P[m] + Q[n])
_TIE_P = (4098, 4102, 6002, 6006, 8186, 8190, 2049, 2051)      # odd multiples of half an ulp (4 below 8192, 2 below 4096) whose lower
_TIE_Q = (0, -1, 1, 4, 3, 5)                                   # neighbour has an even / odd significand; Q moves one unit either side,
_HUGE_P = (4094, 4090, 4095, 4099, 5000, 8190, 4089, 4093)     # and P + 4 onto the tie of the other parity.  x 16: 65504 = 4094 * 16


def _planted_sums(M, N, K, P):
    """codes with T[m, n] = sign[m] (P[m mod 8] + Q[n mod 6]), sign = -1 on rows 8..15 mod 16: a few non-zero codes per row -- up to
    eight 7s in each of the first and last four int4 groups against 1s of the weight, Q[n] in the weight against a 1 of the
    activation, the rest dealt greedily over keeper codes of at most 127 against 1s"""
    K4, G = _dims(M, N, K)
    qa4, qb4 = np.zeros((M, K4), np.int8), np.zeros((N, K4), np.int8)
    qa8, qb8 = np.zeros((M, 128), np.int8), np.zeros((N, 128), np.int8)
    groups = sorted(set(list(range(min(G, 4))) + list(range(max(G - 4, 0), G))))
    sign = np.where((np.arange(M) // 8) % 2 == 1, -1, 1)
    for g in groups:
        qb4[:, g * G128:g * G128 + 8] = 1
    qb4[:, 64] = np.asarray(_TIE_Q)[np.arange(N) % 6]
    qb8[:, :127] = 1
    for m in range(M):
        rest = P[m % 8]
        for g in groups:
            n7 = (m + g) % 8 + 1
            qa4[m, g * G128:g * G128 + n7] = 7 * sign[m]
            rest -= 7 * n7
        qa4[m, 64] = sign[m]
        j = 0
        while rest > 0:
            take = min(127, rest)
            qa8[m, j] = take * sign[m]
            rest -= take
            j += 1
        assert rest == 0 and j <= 127
    T = sign[:, None] * (np.asarray(P)[np.arange(M) % 8][:, None] + np.asarray(_TIE_Q)[np.arange(N) % 6][None, :])
    return dict(qa4=qa4, qb4=qb4, qa8=qa8, qb8=qb8), T


def ties(M, N, K, seed):
    """exact sums on odd multiples of half an fp16 ulp, both parities of the lower neighbour, and one unit either side; the scale of
    a row / a channel pair is one power of two for all its groups and the keeper, so the sum is T 2^e"""
    K4, G = _dims(M, N, K)
    c, T = _planted_sums(M, N, K, _TIE_P)
    ea, eb = -12 + np.arange(M) % 3, -2 + (np.arange(N) // 2) % 2
    d = dict(c, sA=p2(np.repeat(ea[:, None], G, axis=1)), sA8=p2(ea), sB=p2(np.repeat(eb[None, :], G, axis=0)), sB8=p2(eb))
    d["target"] = T.astype(np.float64) * np.ldexp(1.0, ea)[:, None] * np.ldexp(1.0, eb)[None, :]
    d["spread"] = 3
    return d


def huge(M, N, K, seed):
    """planted sums T 2^4 around the fp16 overflow threshold: 65504 exactly, 65520 (the tie that rounds to inf), the values between
    and beyond; activation scales 2^10, weight scales 2^-6"""
    K4, G = _dims(M, N, K)
    c, T = _planted_sums(M, N, K, _HUGE_P)
    d = dict(c, sA=p2(np.full((M, G), 10)), sA8=p2(np.full(M, 10)), sB=p2(np.full((G, N), -6)), sB8=p2(np.full(N, -6)))
    d["target"] = T.astype(np.float64) * 16.0
    d["spread"] = 0
    return d


def tiny_scales(M, N, K, seed, side="act"):
    """random codes; the scales of one side (activation, or weight) are fp16 subnormals 2^-24 .. 2^-15, the other side's 2^-3 ..;
    zero scales on some (m, g) and some (g, channel pair); the last activation row (M >= 2) and channels 0 and 1 have every scale zero"""
    K4, G = _dims(M, N, K)
    c = rand_codes(M, N, K, seed)

    def make(spread):
        r = np.random.default_rng(seed + 5)
        sb = (spread + 1) // 2
        sa = spread - sb
        ea = r.integers(0, sa + 1, size=(M, G)) + (-24 if side == "act" else -3)
        eb = np.repeat(r.integers(0, sb + 1, size=(G, N // 2)), 2, axis=1) + (-3 if side == "act" else -24)
        sA, sB = p2(ea), p2(eb)
        sA8, sB8 = p2(np.full(M, -24 if side == "act" else -3)), p2(np.full(N, -3 if side == "act" else -24))
        mm, gg = np.meshgrid(np.arange(M), np.arange(G), indexing="ij")
        sA[(mm * 7 + gg) % 11 == 5] = 0
        gg, jj = np.meshgrid(np.arange(G), np.arange(N // 2), indexing="ij")
        sB[np.repeat((gg * 5 + jj) % 13 == 3, 2, axis=1)] = 0
        if M >= 2:
            sA[M - 1], sA8[M - 1] = 0, 0
        sB[:, 0:2], sB8[0:2] = 0, 0
        return dict(c, sA=sA, sA8=sA8, sB=sB, sB8=sB8)
    return fit(make, G)


class Family:
    def __init__(self, name, fn, tells, paired, exact=True, sums_only=False, **kw):
        self.name, self.fn, self.tells, self.paired, self.exact, self.sums_only, self.kw = name, fn, tells, paired, exact, sums_only, kw

    def __call__(self, M, N, K, seed=None):
        return self.fn(M, N, K, (M * 1000003 + N * 1009 + K) if seed is None else seed, **self.kw)

    def tells_at(self, G):
        """the rules the family must tell at a shape: with one int4 group there is no neighbouring group's scale row"""
        return tuple(t for t in self.tells if not (t == "group_shift" and G < 2))


_OWN = ("pair_even", "pair_swap", "keeper_neighbour", "group_shift")
FAMILIES = {f.name: f for f in (
    Family("own_scales", own_scales, _OWN, paired=False),
    Family("own_scales_small", own_scales, _OWN, paired=False, base=-10),
    Family("own_scales_free", own_scales, (), paired=False, exact=False, free=True),
    Family("one_pair_off_first", one_pair_off, ("pair_even",), paired=False, where="first"),
    Family("one_pair_off_last", one_pair_off, ("pair_even",), paired=False, where="last"),
    Family("extreme_codes", extreme_codes, ("clamp_symmetric", "nibble_unsigned", "keeper_unsigned"), paired=True),
    Family("extreme_codes_small", extreme_codes, ("clamp_symmetric", "nibble_unsigned", "keeper_unsigned"), paired=True, base=-9),
    Family("ties", ties, ("rtz", "half_away"), paired=True),
    Family("tiny_act", tiny_scales, ("flush_scale", "flush_out"), paired=True, side="act"),
    Family("tiny_weight", tiny_scales, ("flush_scale", "flush_out"), paired=True, side="weight"),
    Family("huge", huge, ("saturate",), paired=True, sums_only=True),
)}


# ------------------------------------------------------------------------------------------------------------- reference
def mutate(d, wrong):
    """the operands as a kernel with one wrong operand rule would read them"""
    d = dict(d)
    G, N = d["sB"].shape
    if wrong == "pair_even":                                   # the odd channel takes the even channel's scale
        d["sB"] = np.repeat(d["sB"][:, 0::2], 2, axis=1)
    elif wrong == "pair_swap":
        d["sB"] = d["sB"].reshape(G, N // 2, 2)[:, :, ::-1].reshape(G, N)
    elif wrong == "keeper_neighbour":                          # sB8[n ^ 1]
        d["sB8"] = d["sB8"].reshape(N // 2, 2)[:, ::-1].reshape(N)
    elif wrong == "group_shift":                               # the scale row of group g + 1 (the last group: of group G - 2)
        row = np.arange(G) + 1
        row[-1] = max(G - 2, 0)
        d["sB"] = d["sB"][row]
    elif wrong == "clamp_symmetric":                           # -8 -> -7, -128 -> -127
        for k, lo in (("qa4", -7), ("qb4", -7), ("qa8", -127), ("qb8", -127)):
            d[k] = np.maximum(d[k], lo)
    elif wrong == "nibble_unsigned":                           # the weight's nibbles read as 0 .. 15
        d["qb4"] = (d["qb4"].astype(np.int16) & 15)
    elif wrong == "keeper_unsigned":                           # the weight's keeper bytes read as 0 .. 255
        d["qb8"] = (d["qb8"].astype(np.int16) & 255)
    elif wrong == "flush_scale":                               # a subnormal fp16 scale read as 0
        for k in ("sA", "sB", "sA8", "sB8"):
            d[k] = np.where(np.abs(d[k].astype(np.float32)) < 2.0 ** -14, np.float16(0), d[k])
    else:
        raise KeyError(wrong)
    return d


_ROUNDINGS = ("rtz", "half_away", "flush_out", "saturate")


def sums(d, device="cpu"):
    """the exact sums of the definition: torch float64 [M, N] on `device` (integer dot products in float64 matrix products, every
    one below 2^53; scale products and their sum in float64 -- exact for operands that meet the bound, far below it)"""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).double()
    qa4, qb4, sA, sB = f(d["qa4"]), f(d["qb4"]), f(d["sA"]), f(d["sB"])
    out = torch.zeros((qa4.shape[0], qb4.shape[0]), dtype=torch.float64, device=device)    # from +0, as every kernel: a zero sum is +0
    out += (f(d["qa8"]) @ f(d["qb8"]).T) * f(d["sA8"])[:, None] * f(d["sB8"])[None, :]
    for g in range(sB.shape[0]):
        sl = slice(g * G128, (g + 1) * G128)
        out += (qa4[:, sl] @ qb4[:, sl].T) * sA[:, g:g + 1] * sB[g:g + 1, :]
    return out


def round_f16(x, mode="rne"):
    """float64 -> fp16 under a named rounding, in float64 arithmetic (independent of the conversion instructions): the quantum of x is
    2^max(e - 10, -24), x / quantum is rounded to an integer by the rule.  rne: nearest, ties to even, >= 65520 -> inf (IEEE).  rtz:
    towards zero (never inf).  half_away: ties away from zero.  flush_out: rne, then subnormal results -> 0.  saturate: rne, inf -> 65504"""
    a = x.abs()
    e = torch.frexp(a)[1].double() - 1                          # a = m 2^e', m in [0.5, 1): floor(log2 a) = e' - 1
    q = torch.pow(torch.full_like(a, 2.0), torch.clamp(e - 10, min=-24))
    n = a / q
    r = {"rtz": torch.floor(n), "half_away": torch.floor(n + 0.5)}.get(mode, torch.round(n))
    y = r * q
    inf = torch.full_like(y, float("inf"))
    if mode == "rtz":
        y = torch.clamp(y, max=65504.0)
    else:
        y = torch.where(y >= 65520.0, inf, y)
    if mode == "flush_out":
        y = torch.where(y < 2.0 ** -14, torch.zeros_like(y), y)
    if mode == "saturate":
        y = torch.clamp(y, max=65504.0)
    return (torch.sign(x) * y).to(torch.float16)               # representable: the conversion is exact


def expected(d, entry="f16", wrong=None, device="cpu", exact=None):
    """What an entry point must return for the operands d: "f16" -> half(sum) as a torch fp16 tensor, "f32" -> the sum as float32.
    wrong: one of RULES.  exact: the sums (sums(d, device)), where the caller has them already."""
    if wrong is not None and wrong not in _ROUNDINGS:
        d, exact = mutate(d, wrong), None
    s = sums(d, device) if exact is None else exact
    s32 = s.float()
    assert torch.equal(s32.double(), s), "a sum is no FP32 number: the operands miss the exactness bound"
    if entry == "f32":
        assert wrong not in _ROUNDINGS
        return s32
    if wrong in _ROUNDINGS:
        return round_f16(s, wrong)
    return s32.to(torch.float16)                                # one rounding: s32 is the exact sum


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def differ(a, b):
    """which elements differ as bit patterns (-0 and +0 differ, a NaN equals itself)"""
    return bits(a) != bits(b)


def take(d, rows, cols):
    """the operands of the sub-problem rows x cols (cols: whole channel pairs keep the pair rules meaningful)"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    return dict(qa4=d["qa4"][rows], qb4=d["qb4"][cols], qa8=d["qa8"][rows], qb8=d["qb8"][cols], sA=d["sA"][rows], sA8=d["sA8"][rows],
                sB=d["sB"][:, cols], sB8=d["sB8"][cols])


def pair_columns(N, limit):
    """at most `limit` columns of N as whole channel pairs, evenly spread, the first and the last pair among them"""
    pairs = np.unique(np.linspace(0, N // 2 - 1, num=min(limit // 2, N // 2)).round().astype(np.int64))
    return np.stack([2 * pairs, 2 * pairs + 1], axis=-1).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- the route cases
# The two 12 x 8192 x 28672 cases run at 512 output channels here: the route queries (atom_gemm_w4a4_packed_order with and without a
# workspace, atom_gemm_w4a4_workspace_bytes, atom_gemm_w4a4_ws_recodes_cached) answer the same for every N from 64 to 8192 at 12 rows
# and this K -- check_route() asserts it for the narrowed case -- and 234 MB of host-generated weight codes per family become 15.
NARROWED = {"long_k_12_rows": 512, "long_k_12_rows_cached": 512}


# Template instances with a channel-pair form that no case of CASES reaches (csrc/gemm_w4a4_v3.hip launch_gemm_v3 default: 256 x 256
# tiles on packed operands, from 1024 such tiles; csrc/gemm_w4a4_mid.hip launch_gemm_f6_mid: the 128 x 64 tile, 257 .. 512 tiles of
# 64 x 64, with float32 and with fp16 weight scales): planted only, no recorded digest.
EXTRA = [
    ("tiles_256x256", "f16", 8192, 8192, 256, dict(order=1)),
    ("f6_mid_128x64", "f16", 257, 4096, 1152, dict(flags=_R.AB_F6 | _R.B_F6S)),
    ("f6_mid_128x64_f16_scales", "f16", 257, 4096, 1152, dict(flags=_R.AB_F6)),
]


def covered_cases():
    """the cases the planted tests run: every case of tests/gemm_route_cases.CASES whose call is taken (status 0) -- 72 of 76 -- and
    EXTRA.  Left out are the four calls that are refused (decode_output_off_16, f32_ / multi_ / multi_q_scales_off_8): they have no
    output.  The three cases that move the weight scales off their 8-byte alignment and are taken run like the others."""
    from tests import gemm_route_cases as C
    return [c[:3] + (NARROWED.get(c[0], c[3]),) + c[4:] for c in C.CASES if "status" not in c[5]] + EXTRA


def case_shape(case):
    """(M, all output channels of the call, K) of a case: the shape its operands are made for"""
    name, entry, M, N, K, o = case
    return M, (2 * N if entry == "gateup" else N * o.get("nseg", 1)), K


_SUM_ENTRIES = ("f16", "f16_ws", "f32", "multi")
ENTRY_FAMILIES = {
    **{e: tuple(f for f in FAMILIES if f != "own_scales_free") for e in _SUM_ENTRIES},
    "o4": ("own_scales", "extreme_codes", "ties"), "o4_ws": ("own_scales", "extreme_codes", "ties"),
    "gateup": ("own_scales", "extreme_codes_small"),         # (scale products 2^-18: SiLU(gate) x up stays inside fp16)
}


def shapes():
    """the distinct operand shapes of the covered cases, in the order of CASES, each with the entry points that use it"""
    out = {}
    for c in covered_cases():
        out.setdefault(case_shape(c), set()).add(c[1])
    return out
