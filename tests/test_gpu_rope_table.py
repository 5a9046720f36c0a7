"""GPU tests of the table path of the paged INT4 attention ops (``rope_table=``, ``attn_scale=`` of ops.batch_decode_i4 /
ops.batch_prefill_i4: atom_batch_decode_gqa_i4_rope, atom_batch_prefill_gqa_i4_rope, atom_batch_decode_append_i4_rope) against the FP64
reference of tests/rope_table_ref.py, whose angle is 2 pi * position * table[i] with the fp32 table values taken exactly.  On the
needle inputs every way of mishandling the two arguments moves that reference by >= 10 x the bound applied here
(tests/test_rope_table_cpu.py), and so does a wrong position, page, head or key (tests/test_attn_planted_cpu.py).

Bounds: the ops' existing ones per (query row, head), attn_planted.bound -- decode 2e-3 max|ref| + 1e-3, prefill and grouped-query
4e-3 max|ref| + 1e-3.  Long contexts use rope_table_ref.aliased_cache: 131,072 positions over 64 distinct pages."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_planted as A
from tests import rope_table_ref as RT
from tests.helpers import t2n
from tests.test_gpu_attn_planted import _assert_splits, _kv, _run, _shape

pytestmark = pytest.mark.gpu

DECODE = [A.DECODE_CASES[i] for i in (0, 3, 5, 6)]
PREFILL = [A.PREFILL_CASES[i] for i in (1, 2, 4)]


@functools.lru_cache(maxsize=None)
def _table(name):
    """(fp32 table as numpy, attn_scale): the Llama 3.1 table, and a YaRN table with attn_scale 1.3"""
    if name == "llama31":
        return RT.config_table(RT.LLAMA31)
    return RT.config_table(RT.YARN)[0], 1.3


def _dev(table):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).cuda()


def _needle(case, which, prefill):
    shape, P, nkv, G = case
    lens, qo, qo_d, max_q = _shape(case, prefill)
    qo_ref = np.arange(len(lens) + 1) if qo is None else qo
    rel = A.rel_bound(G, prefill)
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 5)
    kv = _kv(c, P)
    _assert_splits(kv, P, nkv, G, qo, max_q)
    table, scale = _table(which)
    ref = RT.ref_prefill(qn, c, qo_ref, table, G=G, attn_scale=scale)
    q, td = torch.from_numpy(qn).cuda(), _dev(table)
    for split in (True, False):
        got = _run(kv, q, qo_d, max_q, split, rope_table=td, attn_scale=scale)
        r = A.error_ratio(got, ref, rel)
        row, head = np.unravel_index(np.argmax(r), r.shape)
        print(f"table needle {A.case_id(case)} prefill={prefill} {which} split={split}: worst error / bound {r.max():.3f} (row {row}, head {head})")
        assert r.max() <= 1.0, (split, int(row), int(head), r.max())


@pytest.mark.parametrize("which", ["llama31", "yarn"])
@pytest.mark.parametrize("case", DECODE, ids=A.case_id)
def test_needle_decode(case, which):
    _needle(case, which, prefill=False)


@pytest.mark.parametrize("which", ["llama31", "yarn"])
@pytest.mark.parametrize("case", PREFILL, ids=A.case_id)
def test_needle_prefill(case, which):
    _needle(case, which, prefill=True)


def _decode_inputs(case, seed=5):
    lens, P, nkv, G = case
    c = A.build_needle(lens, nkv, P, seed=seed)
    qn = A.needle_queries(len(lens), nkv * G, seed)
    return c, qn, _kv(c, P), torch.from_numpy(qn).cuda()


def _new_kv(nkv, B, seed=9):
    """this step's FP32 k / v projections [B, nkv * 128]"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return tuple((torch.randn(B, nkv * 128, generator=g) * 0.5).cuda() for _ in range(2))


def _clone_kv(kv):
    import types
    return types.SimpleNamespace(**{**vars(kv), "data": kv.data.clone(), "param": kv.param.clone()})


def test_defaults_are_the_call_without_the_keywords():
    """rope_table=None, attn_scale=1.0: the entry points, launches and bits of a call that does not name them -- decode, append_kv=,
    merge=False, grouped-query decode and prefill"""
    from atom_amd import ops
    kw = dict(rope_theta=5e5, rope_scale=2.0)
    new = dict(rope_table=None, attn_scale=1.0)
    for case in (A.DECODE_CASES[0], A.DECODE_CASES[2]):
        lens, P, nkv, G = case
        c, qn, kv, q = _decode_inputs(case)
        assert torch.equal(ops.batch_decode_i4(q, kv, A.LAYER, **kw), ops.batch_decode_i4(q, kv, A.LAYER, **kw, **new))
        assert ops.decode_splits(len(lens), kv, nkv * G) >= 2
        assert torch.equal(ops.batch_decode_i4(q, kv, A.LAYER, merge=False, **kw), ops.batch_decode_i4(q, kv, A.LAYER, merge=False, **kw, **new))
        if G == 1:
            k32, v32 = _new_kv(nkv, len(lens))
            a, b = _clone_kv(kv), _clone_kv(kv)
            oa = ops.batch_decode_i4(q, a, A.LAYER, append_kv=(k32, v32), **kw)
            ob = ops.batch_decode_i4(q, b, A.LAYER, append_kv=(k32, v32), **kw, **new)
            assert torch.equal(oa, ob) and torch.equal(a.data, b.data) and torch.equal(a.param, b.param)
            assert not torch.equal(a.data, kv.data)
    for case in (A.PREFILL_CASES[0], A.PREFILL_CASES[1]):
        shape, P, nkv, G = case
        lens, qo, qo_d, max_q = _shape(case, True)
        kv = _kv(A.build_needle(lens, nkv, P, seed=5), P)
        q = torch.from_numpy(A.needle_queries(int(qo[-1]), nkv * G, 5)).cuda()
        assert torch.equal(ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, **kw),
                           ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, **kw, **new))


def test_table_arguments_are_checked():
    from atom_amd import ops
    c, qn, kv, q = _decode_inputs(A.DECODE_CASES[0])
    good = _dev(_table("llama31")[0])
    for bad in (good.cpu(), good.double(), good[:32], torch.cat([good, good])[::2], list(range(64)), np.zeros(64, dtype=np.float32)):
        with pytest.raises(TypeError):
            ops.batch_decode_i4(q, kv, A.LAYER, rope_table=bad)
    qo = torch.arange(len(kv.last_page_offset) + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.batch_prefill_i4(q, qo, kv, A.LAYER, rope_table=good.cpu())


@pytest.mark.parametrize("case", [A.DECODE_CASES[0], A.DECODE_CASES[2], A.PREFILL_CASES[1]], ids=A.case_id)
def test_fp32_table_of_plain_theta(case):
    """The fp32 table of theta = 5e5: within the bound of the FP64 reference of THAT table.  The output is not bit-equal to the theta
    path's -- that one forms its frequencies by v_exp_f32 in the kernel, this one loads correctly rounded ones -- and nothing here
    asks it to be: both are within the bound of their own reference."""
    prefill = isinstance(case[0][0], tuple)
    shape, P, nkv, G = case
    lens, qo, qo_d, max_q = _shape(case, prefill)
    qo_ref = np.arange(len(lens) + 1) if qo is None else qo
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo_ref[-1]), nkv * G, 5)
    table = RT.theta_table(5e5).astype(np.float32)
    ref = RT.ref_prefill(qn, c, qo_ref, table, G=G)
    got = _run(_kv(c, P), torch.from_numpy(qn).cuda(), qo_d, max_q, True, rope_table=_dev(table))
    r = A.error_ratio(got, ref, A.rel_bound(G, prefill))
    print(f"plain-theta table {A.case_id(case)} prefill={prefill}: worst error / bound {r.max():.3f}")
    assert r.max() <= 1.0


@pytest.mark.parametrize("split", [True, False])
def test_fused_append_with_a_table(split):
    """append_kv= with a table and a scale: the cache bytes and the output of quant_append_kv_i4 + decode with them, bit for bit"""
    from atom_amd import ops
    case = A.DECODE_CASES[1]
    lens, P, nkv, G = case
    c, qn, kv, q = _decode_inputs(case)
    if not split:
        kv.max_pages = 0
    table, scale = _table("yarn")
    td = _dev(table)
    k32, v32 = _new_kv(nkv, len(lens))
    a, b = _clone_kv(kv), _clone_kv(kv)
    oa = ops.batch_decode_i4(q, a, A.LAYER, append_kv=(k32, v32), rope_table=td, attn_scale=scale)
    ops.quant_append_kv_i4(b, k32, v32, A.LAYER)
    ob = ops.batch_decode_i4(q, b, A.LAYER, rope_table=td, attn_scale=scale)
    assert torch.equal(a.data, b.data) and torch.equal(a.param, b.param) and not torch.equal(a.data, kv.data)
    assert torch.equal(oa, ob)
    c2 = dict(c, data=t2n(b.data), param=t2n(b.param))
    r = A.error_ratio(t2n(oa), RT.ref_decode(qn, c2, table, attn_scale=scale), A.rel_bound(1, False))
    assert r.max() <= 1.0, r.max()


@pytest.mark.parametrize("case", [A.DECODE_CASES[0], A.DECODE_CASES[2]], ids=A.case_id)
def test_unmerged_partial_states_with_a_table(case):
    """merge=False with a table: the partial states, merged in float64 on the host, are within the bound of the merged output"""
    from atom_amd import ops
    lens, P, nkv, G = case
    c, qn, kv, q = _decode_inputs(case)
    table, scale = _table("yarn")
    td = _dev(table)
    splits = ops.decode_splits(len(lens), kv, nkv * G)
    assert splits >= 2
    part = ops.batch_decode_i4(q, kv, A.LAYER, merge=False, rope_table=td, attn_scale=scale)
    assert part.shape == (len(lens), nkv * G, splits, 130)
    merged = t2n(ops.batch_decode_i4(q, kv, A.LAYER, rope_table=td, attn_scale=scale)).astype(np.float64)
    rel = A.rel_bound(G, False)
    r = A.error_ratio(RT.merge_partials(t2n(part)), merged, rel)
    assert r.max() <= 1.0, r.max()
    assert A.error_ratio(merged, RT.ref_decode(qn, c, table, G=G, attn_scale=scale), rel).max() <= 1.0


# ------------------------------------------------------------------------------------------------ long positions
LONG = (2100, 32768, 131072)


@functools.lru_cache(maxsize=None)
def _long_refs(S, kernel):
    """(cache, queries, qo, G, {path: FP64 reference}) of one long case; path 'table': the Llama 3.1 fp32 table, 'theta': exact
    theta = 5e5 (what rope_theta=5e5 asks for)"""
    c = RT.aliased_cache(S)
    G, rows = {"mha": (1, 1), "g4": (4, 1), "chunk": (4, 8)}[kernel]
    qn = A.needle_queries(rows, 2 * G, 7)
    qo = np.array([0, rows])
    table = _table("llama31")[0]
    refs = {"table": RT.ref_prefill(qn, c, qo, table, G=G), "theta": RT.ref_prefill(qn, c, qo, RT.theta_table(5e5), G=G)}
    return c, qn, qo, G, refs


@pytest.mark.parametrize("kernel", ["mha", "g4", "chunk"])
@pytest.mark.parametrize("S", LONG)
def test_long_positions(S, kernel):
    """Positions up to 131,071 with the Llama 3.1 table: MHA decode, grouped-query decode (G = 4) and an 8-query chunk at the end
    (G = 4), each within the ops' bound.  The same figure of the THETA path (rope_theta = 5e5 against exact theta) is printed beside it
    and not asserted: it describes behaviour this test does not own.
    Measured on an MI355X (worst error / bound; table path | theta path):
        tokens     MHA decode      G = 4 decode    8-query chunk, G = 4
        2,100      0.120 | 0.126   0.190 | 0.248   0.235 | 0.240
        32,768     0.105 | 0.151   0.166 | 0.194   0.208 | 0.319
        131,072    0.070 | 0.397   0.180 | 1.290   0.229 | 0.682"""
    from atom_amd import ops
    c, qn, qo, G, refs = _long_refs(S, kernel)
    kv = _kv(c, 16)
    q = torch.from_numpy(qn).cuda()
    prefill = kernel == "chunk"
    rel = A.rel_bound(G, prefill)
    td = _dev(_table("llama31")[0])

    def run(**rope):
        if prefill:
            return t2n(ops.batch_prefill_i4(q, torch.from_numpy(qo.astype(np.int32)).cuda(), kv, A.LAYER, max_q_len=8, **rope))
        return t2n(ops.batch_decode_i4(q, kv, A.LAYER, **rope))

    r_table = A.error_ratio(run(rope_table=td), refs["table"], rel).max()
    r_theta = A.error_ratio(run(rope_theta=5e5), refs["theta"], rel).max()
    print(f"long positions S={S} {kernel}: worst error / bound -- table path {r_table:.3f}, theta path {r_theta:.3f} (not asserted)")
    assert r_table <= 1.0, (S, kernel, r_table)


def test_table_is_read_at_replay():
    """The prefill op with a table inside a captured graph: the table's CONTENTS change between two replays and the output follows --
    the launch reads the table at run time from its fixed address."""
    from atom_amd import ops
    case = A.PREFILL_CASES[5]
    shape, P, nkv, G = case
    lens, qo, qo_d, max_q = _shape(case, True)
    c = A.build_needle(lens, nkv, P, seed=5)
    qn = A.needle_queries(int(qo[-1]), nkv * G, 5)
    kv, q = _kv(c, P), torch.from_numpy(qn).cuda()
    t1, t2 = _table("llama31")[0], _table("yarn")[0]
    td = _dev(t1)
    ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, rope_table=td)        # (warm-up: the workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = ops.batch_prefill_i4(q, qo_d, kv, A.LAYER, max_q_len=max_q, rope_table=td)
    rel = A.rel_bound(G, True)
    g.replay()
    torch.cuda.synchronize()
    first = t2n(o).copy()
    td.copy_(_dev(t2))
    g.replay()
    torch.cuda.synchronize()
    second = t2n(o).copy()
    ref1, ref2 = RT.ref_prefill(qn, c, qo, t1, G=G), RT.ref_prefill(qn, c, qo, t2, G=G)
    assert A.error_ratio(first, ref1, rel).max() <= 1.0 and A.error_ratio(second, ref2, rel).max() <= 1.0
    assert A.error_ratio(ref2, ref1, rel).max() >= 10.0      # (the two tables are far apart on these inputs)
