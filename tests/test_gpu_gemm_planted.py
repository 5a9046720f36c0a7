"""The W4A4 GEMM entry points on the planted operands of tests/gemm_planted.py, route by route: every case of tests/gemm_route_cases.py
whose call is taken (72 of 76) and three more for template instances those do not reach (gemm_planted.EXTRA), through that module's
own entry-point plumbing (call()), compared bit for bit -- no tolerance anywhere:

  f16, f16_ws, f32, multi   the exact families against expected(): half(float64 sum), or the sum itself as FP32 (every summation
                            order must give it: tests/test_gemm_planted_cpu.py asserts the bound the argument rests on);
                            the free own_scales family against oracle/atom_oracle.c in the order the route is named for, where the
                            oracle restates it (1, 8, two / four K ranges, the dot-product kernel's lanes), on sampled rows and columns;
  o4, o4_ws                 the oracle's u4 epilogue (quant_o4) of the exact FP32 sums;
  gateup                    the exact gate and up sums, rounded to fp16, through the oracle's SiLU x up quantiser;
  multi_q, merge_q          the activation comes from the in-launch quantiser (scales are no powers of two): the oracle's quantiser, then
                            its GEMM in the order atom_gemm_w4a4_packed_order names, on free own_scales weights and on weight codes at
                            the limit; merge_q on partial states whose merge is exact (equal maxima, denominators 1/2 + 1/2).

Every case runs with its flags as listed and with ATOM_B_SCALE_PAIRS toggled; a call that asserts shared pairs only ever gets families
whose pairs are shared, a call that does not gets the unpaired families as well (own_scales, one_pair_off)."""
import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import c_oracle as CO
from tests import gemm_planted as P
from tests import gemm_route_cases as C
from tests import quant_planted as QP
from tests.helpers import assert_quant_equal, to_device, wide_codes
from tests.test_gpu_gemm_route_digests import GROUPS

pytestmark = pytest.mark.gpu

CASES = P.covered_cases()
RUN_GROUPS = [g for g in GROUPS if any(c[0].startswith(g) for c in CASES)]
NO_FLAGS = ("multi_q", "merge_q")                            # entry points without a scale_layout / flags argument
_made = {}


def made(fam, shape):
    """a family's operands at a shape with what every case of that shape shares: the packed weight and, for an exact family, the
    expected fp16 and FP32 outputs on the device (one shape is kept: cases of a shape are adjacent)"""
    if any(k[1] != shape for k in _made):
        _made.clear()
    if (fam, shape) not in _made:
        d = P.FAMILIES[fam](*shape)
        e = dict(d=d, B4=O.pack_int4(d["qb4"]))
        if P.FAMILIES[fam].exact:
            s = P.sums(d, "cuda")
            e["f16"], e["f32"] = P.expected(d, exact=s), P.expected(d, entry="f32", exact=s)
        _made[(fam, shape)] = e
    return _made[(fam, shape)]


def raw(e, case, flags):
    """the arrays gemm_route_cases.call() takes, from an operand dict"""
    d, o = e["d"], case[5]
    sA, sA8 = np.ascontiguousarray(d["sA"].T), d["sA8"]
    if o.get("layout", C.PLAIN) == C.REF:
        sA, sA8 = O.scales_to_ref_layout(sA), O.scales_to_ref_layout(sA8)
    a4 = wide_codes(d["qa4"]) if flags & C.A_WIDE else O.pack_int4(d["qa4"])
    return dict(A4=a4, B4=e["B4"], A8=d["qa8"], B8=d["qb8"], sA=sA, sA8=sA8, sB=d["sB"], sB8=d["sB8"])


def variants(case):
    """[(flags, family names)]: the listed flags and the same with ATOM_B_SCALE_PAIRS toggled"""
    entry, o = case[1], case[5]
    names = P.ENTRY_FAMILIES[entry]
    listed = o.get("flags", 0)
    out = []
    for i, fl in enumerate((listed, listed ^ C.PAIRS)):
        if fl & C.PAIRS:
            fams = [f for f in names if P.FAMILIES[f].paired]
        elif i == 0:
            fams = list(names)
        else:
            fams = [f for f in names if not P.FAMILIES[f].paired]
        out.append((fl, fams))
    return out


def _count(bad):
    return int(bad.sum().item())


def check_sums(case, dev, e):
    """f16 / f16_ws / f32 / multi: the number of output elements that differ from the exact answer"""
    name, entry, M, N, K, o = case
    if entry in ("f16", "f16_ws"):
        return _count(P.differ(dev.dev("D"), e["f16"]))
    if entry == "f32":
        return _count(P.differ(dev.dev("D"), e["f32"]))
    bad = 0
    for i in range(o["nseg"]):
        cols = slice(i * N, (i + 1) * N)
        if (o.get("f32_mask", 0) >> i) & 1:
            want = e["f32"][:, cols]
        else:
            want = e["f16"][:, cols]
            if i == 0 and o.get("add"):
                want = (want.float() + dev.dev("add").float()).half()               # as torch adds two half tensors
        bad += _count(P.differ(dev.dev(f"out{i}"), want.contiguous()))
    return bad


def check_o4(case, dev, e):
    M, N = case[2], case[3]
    q, sz = O.quant_o4(e["f32"].cpu().numpy())
    return int((dev.get("D4") != q).sum()) + int((dev.get("Dsz").view(np.uint16) != sz.reshape(M, -1).view(np.uint16)).sum())


def gateup_rows(N):
    """rows of the fused gate/up weight [2 N]: per 128-feature block and 32-feature quarter, 32 gate rows then the same 32 up rows"""
    r = np.arange(2 * N)
    return r[(r % 64) < 32], r[(r % 64) >= 32]


def check_gateup(case, dev, e):
    name, entry, M, N, K, o = case
    y = e["f16"].cpu().numpy()
    g, u = gateup_rows(N)
    ref = QP.run("silu_mul", (y[:, g], y[:, u]), "sim" if o["mode"] == 1 else "kernel", o["clip"])
    outs = [dev.dev(k) for k in ("o8", "o6", "s8", "s4", "xq")]
    try:
        assert_quant_equal(outs, ref, M, layout="ref" if o.get("layout", C.PLAIN) == C.REF else "plain", fmt="f6", xq_ref=ref["xq"], what=name)
    except AssertionError as err:
        return str(err)
    return 0


def oracle_order(order):
    return {1: 1, 8: 8, 2: -2, 4: -4, 64: "lanes"}.get(order)


def check_multi_q(case, dev, e, lib):
    """multi_q / merge_q against the oracle's quantiser and its GEMM in the named order"""
    name, entry, M, N, K, o = case
    d = e["d"]
    f16, f32 = np.float16, np.float32
    idx = dev.get("idx") if "idx" in dev.t else None
    bad = 0
    if entry == "merge_q":
        part = dev.get("part")
        x = (part[:, :, 0, :128] + part[:, :, 1, :128]).reshape(M, K)
        assert np.array_equal(x.astype(f16).astype(f32), x)
        t = CO.act_quant(0, x.astype(f16), None, idx, 0, 0.9)
    else:
        q, x = o["q_op"], dev.get("x")
        if q == 1:
            t = CO.act_quant(0, x, None, idx, 0, 0.9)
        elif q == 2:
            t = CO.act_quant(1, x, dev.get("x2"), idx, 0, 0.9, eps=1e-5)
        elif q == 3:
            s = (x.astype(f32) + dev.get("res").astype(f32)).astype(f16)
            bad += int((dev.get("res_out").view(np.uint16) != s.view(np.uint16)).sum())
            t = CO.act_quant(1, s, dev.get("x2"), idx, 0, 0.9, eps=1e-5)
        else:
            t = CO.act_quant(2, x, dev.get("x2"), None, 0, 0.9)
    order = oracle_order(lib.atom_gemm_w4a4_packed_order(M, N, K, 0))
    assert order in (8, "lanes"), name
    want = CO.gemm(O.pack_int4(t["q4"]), e["B4"], t["s4"].T, d["sB"], t["q8"], d["qb8"], t["s8"], d["sB8"], nsplit=order)
    for i in range(o["nseg"]):
        w = want[:, i * N:(i + 1) * N]
        got = dev.get(f"out{i}")
        if (o.get("f32_mask", 0) >> i) & 1:
            with np.errstate(over="ignore"):
                got = got.astype(f16)                                                # D = half(c): the FP32 sums round to the oracle's output
        elif i == 0 and o.get("add"):
            w = (w.astype(f32) + dev.get("add").astype(f32)).astype(f16)
        bad += int((np.ascontiguousarray(got).view(np.uint16) != np.ascontiguousarray(w).view(np.uint16)).sum())
    return bad


def sampled(M, N, seed):
    g = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([[0, M - 1, min(63, M - 1), min(64, M - 1), min(255, M - 1), min(256, M - 1)], g.integers(0, M, 6)]))
    cols = np.unique(np.concatenate([np.arange(0, min(N, 34)), [N - 1, N - 2, N - 33, N - 64], g.integers(0, N, 20)]))
    return rows, cols


def check_free(case, dev, e, lib, flags):
    """free own_scales against the C oracle in the route's named order, on sampled rows and columns; None where the oracle does not
    restate the order (split-K, the staged dot product)"""
    name, entry, M, N, K, o = case
    if entry in ("f16", "f16_ws") and flags & C.AB_F6:
        order = lib.atom_gemm_w4a4_f6_order(M, N, K)
    elif entry in ("f16", "f16_ws") and flags & C.A_WIDE:
        order = 1 if entry == "f16" else None
    elif entry == "f16_ws" or "order" in o:
        order = o.get("order")
    else:
        order = lib.atom_gemm_w4a4_packed_order(M, N, K, 0)
    order = oracle_order(order)
    if order is None:
        return None
    d = e["d"]
    n_all = d["sB"].shape[1]
    rows, cols = sampled(M, n_all, M + n_all + K)
    s = P.take(d, rows, cols)
    want = CO.gemm(O.pack_int4(s["qa4"]), O.pack_int4(s["qb4"]), s["sA"].T, s["sB"], s["qa8"], s["qb8"], s["sA8"], s["sB8"], nsplit=order)
    with np.errstate(over="ignore"):
        if entry in ("f16", "f16_ws", "f32"):
            got = dev.get("D")[np.ix_(rows, cols)].astype(np.float16)                  # f32 entry: D = half(c)
        else:
            got = np.concatenate([dev.get(f"out{i}").astype(np.float16) for i in range(o["nseg"])], axis=1)[np.ix_(rows, cols)]
            if o.get("add"):
                seg0 = cols < N
                add = dev.get("add")[np.ix_(rows, cols[seg0])].astype(np.float32)
                want[:, seg0] = (want[:, seg0].astype(np.float32) + add).astype(np.float16)
    return int((np.ascontiguousarray(got).view(np.uint16) != want.view(np.uint16)).sum())


def run_case(case, lib):
    """every variant and family of one case -> the list of failures"""
    name, entry, M, N, K, o = case
    shape = P.case_shape(case)
    fails = []
    if entry in NO_FLAGS:
        free = made("own_scales_free", shape)
        ext = made("extreme_codes", shape)["d"]
        lim = dict(d=dict(free["d"], qb4=ext["qb4"], qb8=ext["qb8"]), B4=O.pack_int4(ext["qb4"]))
        for fam, e in (("own_scales_free", free), ("own_scales_free+extreme_codes", lim)):
            src = raw(e, case, 0)
            if entry == "merge_q":
                g = np.random.default_rng(K)
                part = np.zeros((M, K // 128, o["splits"], 130), dtype=np.float32)
                part[..., :128] = g.integers(-256, 256, size=part[..., :128].shape) / 256.0
                part[..., 129] = 1.0 / o["splits"]
                src["part"] = part
            st, dev, outs = C.call(case, src=src)
            bad = f"status {st}" if st else check_multi_q(case, dev, e, lib)
            if bad:
                fails.append((name, "no flags", fam, bad))
        return fails
    for flags, fams in variants(case):
        tag = "pairs" if flags & C.PAIRS else "own"
        todo = list(fams) + (["own_scales_free"] if not flags & C.PAIRS and entry in ("f16", "f16_ws", "f32", "multi") else [])
        for fam in todo:
            e = made(fam, shape)
            assert P.pairs_shared(e["d"]) or not flags & C.PAIRS
            st, dev, outs = C.call(case, src=raw(e, case, flags), flags=flags)
            if st:
                bad = f"status {st}"
            elif fam == "own_scales_free":
                bad = check_free(case, dev, e, lib, flags)
            elif entry in ("o4", "o4_ws"):
                bad = check_o4(case, dev, e)
            elif entry == "gateup":
                bad = check_gateup(case, dev, e)
            else:
                bad = check_sums(case, dev, e)
            print(f"{name} [{tag}] {fam}: {'not compared' if bad is None else bad or 'equal'}")
            if bad:
                fails.append((name, tag, fam, bad))
    return fails


@pytest.mark.parametrize("prefix", RUN_GROUPS)
def test_routes_on_planted_operands(prefix):
    from atom_amd import _lib
    cases = [c for c in CASES if c[0].startswith(prefix)]
    assert cases
    fails = []
    for case in cases:
        fails += run_case(case, _lib.lib())
    assert not fails, fails


def test_every_taken_case_is_in_a_group():
    assert sorted(c[0] for c in CASES) == sorted(c[0] for g in RUN_GROUPS for c in CASES if c[0].startswith(g)) and len(CASES) == 72 + len(P.EXTRA)


# ------------------------------------------------------------------------------------------------ host level
def _paired_then_own(M, N, K):
    """(operands with shared pairs, the same with every pair split): the own_scales family and its pair_even reading"""
    own = P.FAMILIES["own_scales"](M, N, K)
    return P.mutate(own, "pair_even"), own


@pytest.mark.parametrize("M,N,K,route", [(513, 4096, 1152, "prefill"), (16, 256, 384, "decode"), (513, 4096, 1152, "f6")])
@pytest.mark.parametrize("how", ["in_place", "data_then_forget"])
def test_scales_rewritten_from_paired_to_unpaired(M, N, K, route, how):
    """A weight-scale tensor rewritten from shared to per-channel values, codes untouched: the next call must give the per-channel
    result -- not the channel-pair kernel, not a cached BF6 weight with the old float32 scales.  In place (the version counter moves),
    and through .data followed by forget_weight_f6 (it does not)."""
    from atom_amd import ops
    paired, own = _paired_then_own(M, N, K)
    assert P.pairs_shared(paired) and not P.pairs_shared(own)
    want_paired, want_own = P.expected(paired, device="cuda"), P.expected(own, device="cuda")
    assert P.differ(want_paired, want_own).any(dim=1).all()
    t = list(to_device(paired, "plain"))
    new = torch.from_numpy(own["sB"]).cuda()

    def gemm():
        if route != "f6":
            return ops.dense_layer_gemm_i4_fp16(*t, scale_layout="plain")
        a6 = ops.repack_act_f6(t[0], t[2], scale_layout="plain")
        return ops.dense_layer_gemm_i4_fp16(a6, ops.repack_weight_f6(t[1], t[3]), *t[2:], scale_layout="plain", a_wide="f6")

    if route == "prefill":
        assert ops.L.lib().atom_gemm_w4a4_ws_recodes_cached(M, N, K) == 1
    assert ops.scale_pairs_shared(t[3], N)
    for _ in range(2):                                           # the second call: the cached weight / the remembered pair tag
        assert not P.differ(gemm(), want_paired).any()
    if how == "in_place":
        t[3].copy_(new)
    else:
        t[3].data.copy_(new)
        ops.forget_weight_f6(t[1], t[3])
    assert not ops.scale_pairs_shared(t[3], N)
    for _ in range(2):
        bad = P.differ(gemm(), want_own)
        assert not bad.any(), f"{_count(bad)} of {bad.numel()} elements are not the per-channel result"


def test_check_scale_pairs_counts_each_planted_pair():
    from atom_amd import ops
    L = ops.L
    M, N, K = 16, 256, 1152
    first, last = P.FAMILIES["one_pair_off_first"](M, N, K), P.FAMILIES["one_pair_off_last"](M, N, K)
    G = K // 128 - 1
    both = first["sB"].copy()
    both[G - 1, N - 1] = both[G - 1, N - 2] * np.float16(2)
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    for sb, want in ((first["sB"], 1), (last["sB"], 1), (both, 2), (P.mutate(first, "pair_even")["sB"], 0),
                     (P.FAMILIES["own_scales"](M, N, K)["sB"], G * N // 2)):
        t = torch.from_numpy(np.ascontiguousarray(sb)).cuda()
        L.check(L.lib().atom_check_scale_pairs(t.data_ptr(), G, N, cnt.data_ptr(), L.current_stream(t.device)), "atom_check_scale_pairs")
        assert int(cnt[0]) == want and ops.scale_pairs_shared(t, N) == (want == 0)
