"""GPU tests of the sparse mixture-of-experts path (csrc/moe_w4a4.hip, atom_amd/e2e/mixtral.py): the router's tables, the routed GEMM
bit for bit against the C oracle per expert, the combine bit for bit against tests/moe_ref.py, the whole block against the chain of
those, and generation by graph replay against the eager loop."""
import types

import numpy as np
import pytest
import torch

from oracle import atom_oracle as O
from tests import c_oracle, moe_ref
from tests.helpers import rand_gemm_operands, scales_plain, t2n, to_device

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. router
def _check_router(logits, T, E, K, distinct=True, exact_rows=None):
    """ids, tables and n_tiles bit for bit against moe_ref (the lower index of equal logits); the weights bit for bit on
    ``exact_rows`` and within one fp16 ulp elsewhere"""
    from atom_amd import ops
    r = ops.moe_route_topk(logits.to(DEV), K)
    ids_ref, w_ref = moe_ref.route(logits, K)
    if distinct:                                             # (among equal logits torch.topk keeps no rule: not a cross-check there)
        assert torch.equal(torch.topk(logits.float(), K, dim=-1).indices, ids_ref)
    assert torch.equal(r.topk_ids.cpu().long(), ids_ref)
    d = (_bits(r.topk_w).int() - _bits(w_ref).int()).abs()                               # positive halves: the bit patterns are ordered
    ulp = d.max().item()
    print(f"T {T} E {E} top_k {K}: topk_w within {ulp} fp16 ulp of the reference, {int((d != 0).sum())} of {d.numel()} elements differ")
    assert ulp <= 1
    if exact_rows is not None:
        assert len(exact_rows) > 0 and torch.equal(_bits(r.topk_w)[exact_rows], _bits(w_ref)[exact_rows])
    tb = moe_ref.tables(ids_ref, E)
    n = tb["n_tiles"]
    assert r.n_tiles.item() == n and n <= ops.moe_max_tiles(T * K, E) == r.tile_expert.numel()
    assert r.expert_indptr.tolist() == tb["expert_indptr"]
    assert r.row_token.tolist() == tb["row_token"]
    assert r.slot_row.tolist() == tb["slot_row"]
    assert r.tile_expert[:n].tolist() == tb["tile_expert"] and r.tile_row0[:n].tolist() == tb["tile_row0"]


@pytest.mark.parametrize("T,E,K", [(1, 8, 2), (5, 8, 2), (257, 8, 2), (300, 16, 4), (300, 64, 8), (300, 3, 1),
                                   (256, 8, 2), (512, 8, 2), (1025, 8, 2)])              # pass B: one and two full chunks, five chunks
def test_router_tables(T, E, K):
    _check_router(moe_ref.distinct_logits(T, E, 100 + T + E), T, E, K)


@pytest.mark.parametrize("T,E,K", [(600, 8, 2), (600, 2, 2), (600, 3, 1), (600, 16, 4), (600, 64, 8), (600, 5, 5)])
def test_router_on_equal_logits_takes_the_lower_index(T, E, K):
    """planted ties (tests/test_moe_cpu.py: the opposite rule gives other topk_ids on 186 or more of the 600 rows of every case): all
    zeros, +0 / -0, saturated rows, ties across and inside the top_k boundary and for the maximum; E = 2 and top_k = E included"""
    logits, exact_rows = moe_ref.planted_logits(T, E, K, 500 + E + K)
    _check_router(logits, T, E, K, distinct=False, exact_rows=exact_rows)


def test_router_with_empty_experts():
    """every token picks experts 5 and 2: the other six have no row and no tile"""
    T, E, K = 70, 8, 2
    logits = moe_ref.distinct_logits(T, E, 7)
    logits[:, 5], logits[:, 2] = 20.0, 19.0
    _check_router(logits, T, E, K)


def test_router_with_two_experts_fed_by_every_chunk():
    """1000 tokens, all on experts 5 and 2: each gets 1000 rows (16 tiles) that arrive in all four chunks of pass B, so every row
    behind the first chunk depends on the carried base[]"""
    T, E, K = 1000, 8, 2
    logits = moe_ref.distinct_logits(T, E, 8)
    logits[:, 5], logits[:, 2] = 20.0, 19.0
    _check_router(logits, T, E, K)


# ------------------------------------------------------------------------------------------------ 2. routed GEMM
COUNTS = [0, 1, 64, 65, 130, 0]
SENTINEL = 1234.0


def _routed_gemm_case(counts, n_seg, nseg, K, gather, layout, seed):
    """host-built tables for ``counts`` rows per expert; one independent weight set per expert; the outputs against the C oracle on
    each expert's gathered rows, and the rows past R untouched"""
    from atom_amd import _lib as L
    from atom_amd import ops
    E, R, N = len(counts), sum(counts), n_seg * nseg
    a_rows = 150 if gather else R
    d = rand_gemm_operands(a_rows, N, K, seed)
    A4, _, sA, _, A8, _, sA8, _ = to_device(d, layout)
    per = [rand_gemm_operands(1, N, K, seed + 1 + e) for e in range(E)]
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    B4 = f(np.stack([O.pack_int4(p["qb4"]) for p in per]))
    B8 = f(np.stack([p["qb8"] for p in per]))
    sB = f(np.stack([p["sB"] for p in per]))
    sB8 = f(np.stack([p["sB8"] for p in per]))
    row_index = [(r * 7 + 3) % a_rows for r in range(R)] if gather else list(range(R))     # tokens repeat within and across experts
    indptr, te, tr = moe_ref.tables_from_counts(counts)
    mt = ops.moe_max_tiles(R, E)
    assert len(te) <= mt
    pad = mt - len(te)
    t_ri, t_ip = _i32(row_index), _i32(indptr)
    t_te, t_tr, t_nt = _i32(te + [9999] * pad), _i32(tr + [-7] * pad), _i32([len(te)])    # entries past n_tiles: never read
    outs = [torch.full((R + 64, n_seg), SENTINEL, dtype=torch.float16, device=DEV) for _ in range(nseg)]
    st = L.lib().atom_moe_gemm_w4a4_f16(A4.data_ptr(), B4.data_ptr(), sA.data_ptr(), sB.data_ptr(), A8.data_ptr(), B8.data_ptr(),
                                        sA8.data_ptr(), sB8.data_ptr(), t_ri.data_ptr() if gather else None, t_ip.data_ptr(),
                                        t_te.data_ptr(), t_tr.data_ptr(), t_nt.data_ptr(), outs[0].data_ptr(),
                                        outs[1].data_ptr() if nseg > 1 else None, a_rows, R, E, n_seg, nseg, K, 128, 128,
                                        {"ref": 0, "plain": 1}[layout], torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    got = np.concatenate([t2n(o[:R]) for o in outs], axis=1)
    a4p, sA_gm = O.pack_int4(d["qa4"]), np.ascontiguousarray(d["sA"].T)
    for e in range(E):
        lo, hi = indptr[e], indptr[e + 1]
        if hi == lo:
            continue
        src = np.asarray(row_index[lo:hi])
        want = c_oracle.gemm(a4p[src], O.pack_int4(per[e]["qb4"]), sA_gm[:, src], per[e]["sB"], d["qa8"][src], per[e]["qb8"],
                             d["sA8"][src], per[e]["sB8"])
        bad = got[lo:hi].view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), f"expert {e}: {bad.sum()} of {bad.size} outputs differ, first at {np.argwhere(bad)[0]}"
    for o in outs:
        assert (o[R:] == SENTINEL).all(), "rows past R were written"


@pytest.mark.parametrize("layout", ["ref", "plain"])
@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("K", [384, 1408])
@pytest.mark.parametrize("nseg", [1, 2])
def test_routed_gemm_is_the_oracle_per_expert(nseg, K, gather, layout):
    _routed_gemm_case(COUNTS, 128, nseg, K, gather, layout, seed=11 * nseg + K)


def test_routed_gemm_with_the_grid_far_above_the_tile_count():
    """R = 3 over 6 experts: the grid is sized for 3 tiles per feature block, two exist"""
    _routed_gemm_case([0, 2, 0, 0, 1, 0], 128, 2, 384, True, "ref", seed=5)


@pytest.mark.parametrize("layout", ["ref", "plain"])
@pytest.mark.parametrize("K", [256, 768, 896, 1024, 1152])
def test_routed_gemm_ring_at_every_fill(K, layout):
    """G = 1, 5, 6, 7, 8 int4 groups (+ 2 keeper stages) against the ring of 8: the prologue repeats its last stage, fills the ring
    exactly, overfills it by one, and the keeper's two stages wrap around its end"""
    _routed_gemm_case(COUNTS, 128, 2, K, True, layout, seed=3 * K)


@pytest.mark.parametrize("layout", ["ref", "plain"])
@pytest.mark.parametrize("nseg", [1, 2])
def test_routed_gemm_64_feature_segments_one_tile(nseg, layout):
    """n_seg = 64: the weight-scale piece clamps every lane above 31 (nseg 1) or the second feature block's (nseg 2); one expert,
    one tile of 3 rows, so fewer live workgroups than XCDs"""
    _routed_gemm_case([3], 64, nseg, 384, True, layout, seed=17 + nseg)


def test_routed_gemm_64_feature_segments_with_empty_experts():
    _routed_gemm_case([0, 200, 0, 1], 64, 2, 384, True, "ref", seed=23)


def test_routed_gemm_64_experts_of_one_row():
    """R = 64 over 64 experts: 64 tiles, 63 of 64 rows masked in each"""
    _routed_gemm_case([1] * 64, 128, 2, 384, True, "ref", seed=29)


# ------------------------------------------------------------------------------------------------ 3. combine
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [1, 70])
def test_combine_is_the_reference_fp16_arithmetic(T, K, res):
    from atom_amd import ops
    E, H, R = 8, 512, T * K
    g = torch.Generator().manual_seed(31 * T + K)
    ids = torch.rand((T, E), generator=g).argsort(-1)[:, :K]
    # mixed magnitudes: with four slots the fp16 sum depends on the order of the additions
    w = (torch.rand((T, K), generator=g) * 2.0 ** torch.randint(-6, 1, (T, K), generator=g).float()).half()
    y = (torch.randn((R, H), generator=g) * 2.0 ** torch.randint(-4, 7, (R, 1), generator=g).float()).half()
    residual = torch.randn((T, H), generator=g).half() if res else None
    slot_row = torch.randperm(R, generator=g).view(T, K)
    route = ops.MoeRoute(T, E, K, topk_ids=_i32(ids), topk_w=w.to(DEV), slot_row=_i32(slot_row))
    got = ops.moe_combine(y.to(DEV), route, None if residual is None else residual.to(DEV))
    want = moe_ref.combine(y, ids, w, slot_row.tolist(), residual)
    assert torch.equal(_bits(got), _bits(want))
    if K == 4:                                                 # the order matters on these inputs: descending expert id gives other bits
        other = moe_ref.combine(y, E - 1 - ids, w, slot_row.tolist(), residual)
        assert not torch.equal(_bits(other), _bits(want))


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("H", [2056, 4096])
def test_combine_with_more_than_one_block_per_token(H, K, res):
    """H / 8 = 257 and 512 sixteen-byte pieces: two blocks of 256 threads per token, the second with one live thread at H = 2056;
    top_k = 8 (of 64 experts) fills every slot of the kernel's selection"""
    from atom_amd import ops
    T, E, R = 3, (64 if K == 8 else 8), 3 * K
    g = torch.Generator().manual_seed(H + K)
    ids = torch.rand((T, E), generator=g).argsort(-1)[:, :K]
    w = (torch.rand((T, K), generator=g) * 2.0 ** torch.randint(-6, 1, (T, K), generator=g).float()).half()
    y = (torch.randn((R, H), generator=g) * 2.0 ** torch.randint(-4, 7, (R, 1), generator=g).float()).half()
    residual = torch.randn((T, H), generator=g).half() if res else None
    slot_row = torch.randperm(R, generator=g).view(T, K)
    route = ops.MoeRoute(T, E, K, topk_ids=_i32(ids), topk_w=w.to(DEV), slot_row=_i32(slot_row))
    got = ops.moe_combine(y.to(DEV), route, None if residual is None else residual.to(DEV))
    want = moe_ref.combine(y, ids, w, slot_row.tolist(), residual)
    assert torch.equal(_bits(got), _bits(want))
    if K == 8:                                               # descending expert id gives other bits, also in the second block's columns
        other = moe_ref.combine(y, E - 1 - ids, w, slot_row.tolist(), residual)
        assert not torch.equal(_bits(other[:, 2048:]), _bits(want[:, 2048:]))


# ------------------------------------------------------------------------------------------------ 4. the block
H_, F_, E_, K_ = 512, 1408, 8, 2


def _cfg(layers=2, sliding_window=None):
    return types.SimpleNamespace(hidden_size=H_, num_attention_heads=4, num_key_value_heads=2, intermediate_size=F_, rms_norm_eps=1e-5,
                                 rope_theta=1e4, num_hidden_layers=layers, vocab_size=VOCAB, pad_token_id=None, num_local_experts=E_,
                                 num_experts_per_tok=K_, sliding_window=sliding_window)


def _load_moe(moe, g):
    for j in range(moe.num_experts):
        w1, w3 = [(torch.randn(F_, H_, generator=g) * 0.05).half().cuda() for _ in range(2)]
        moe.load_expert_fp16(j, w1, w3, (torch.randn(H_, F_, generator=g) * 0.05).half().cuda())
    moe.gate.weight.data = (torch.randn(E_, H_, generator=g) * 0.1).half().cuda()


@pytest.fixture(scope="module")
def moe_block():
    from atom_amd.e2e import MixtralSparseMoeInt4
    moe = MixtralSparseMoeInt4(_cfg()).cuda()
    _load_moe(moe, torch.Generator().manual_seed(3))
    return moe


@pytest.mark.parametrize("T", [2, 24])
def test_block_equals_the_chain_of_references(moe_block, T):
    from atom_amd import ops
    moe = moe_block
    g = torch.Generator().manual_seed(40 + T)
    x = torch.randn((T, H_), generator=g)
    x[:, -128:] *= 10
    x, gate_in, residual = x.half().cuda(), torch.randn((T, H_), generator=g).half().cuda(), torch.randn((T, H_), generator=g).half().cuda()
    x_q = ops.reorder_fp16_i4(x, None)
    got = moe(x_q, gate_in, residual)
    # 1. routing on the module's own logits
    logits = torch.nn.functional.linear(gate_in, moe.gate.weight).cpu()
    ids, w = moe_ref.route(logits, K_)
    tb = moe_ref.tables(ids, E_)
    indptr, rt = tb["expert_indptr"], np.asarray(tb["row_token"])
    R = T * K_
    # 2. gate / up per expert on the gathered codes
    o8, o4, s8, s4 = x_q
    a4, a8 = t2n(o4).view(np.uint8), t2n(o8)
    sa, sa8 = scales_plain(s4, T, "ref"), scales_plain(s8, T, "ref")
    gu = np.empty((R, 2 * F_), np.float16)
    for e in range(E_):
        src = rt[indptr[e]:indptr[e + 1]]
        if len(src):
            gu[indptr[e]:indptr[e + 1]] = c_oracle.gemm(a4[src], t2n(moe.w13_int4[e]), sa[:, src], t2n(moe.w13_scale_int4[e]), a8[src],
                                                        t2n(moe.w13_int8[e]), sa8[src], t2n(moe.w13_scale_int8[e]))
    # 3. the existing quantiser on those outputs
    gate, up = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (gu[:, :F_], gu[:, F_:])]
    b8, b4, t8, t4 = ops.activate_fp16_i4(gate, up)
    h4, h8, hs, hs8 = t2n(b4).view(np.uint8), t2n(b8), scales_plain(t4, R, "ref"), scales_plain(t8, R, "ref")
    # 4. down per expert
    y = np.empty((R, H_), np.float16)
    for e in range(E_):
        lo, hi = indptr[e], indptr[e + 1]
        if hi > lo:
            y[lo:hi] = c_oracle.gemm(h4[lo:hi], t2n(moe.w2_int4[e]), hs[:, lo:hi], t2n(moe.w2_scale_int4[e]), h8[lo:hi], t2n(moe.w2_int8[e]),
                                     hs8[lo:hi], t2n(moe.w2_scale_int8[e]))
    # 5. combine
    want = moe_ref.combine(torch.from_numpy(y), ids, w, tb["slot_row"], residual.cpu())
    assert torch.equal(_bits(got), _bits(want))


def _chain_of_references(moe, x_q, ids, w, residual):
    """what the block computes from a given routing, reference by reference: the C oracle's GEMM per expert on the gathered codes,
    the project's quantiser on gate / up, the oracle again for down, moe_ref.combine"""
    from atom_amd import ops
    T, K = ids.shape
    E, F, H, R = moe.num_experts, moe.intermediate_size, moe.hidden_size, T * K
    tb = moe_ref.tables(ids, E)
    indptr, rt = tb["expert_indptr"], np.asarray(tb["row_token"])
    o8, o4, s8, s4 = x_q
    a4, a8 = t2n(o4).view(np.uint8), t2n(o8)
    sa, sa8 = scales_plain(s4, T, "ref"), scales_plain(s8, T, "ref")
    gu = np.empty((R, 2 * F), np.float16)
    for e in range(E):
        src = rt[indptr[e]:indptr[e + 1]]
        if len(src):
            gu[indptr[e]:indptr[e + 1]] = c_oracle.gemm(a4[src], t2n(moe.w13_int4[e]), sa[:, src], t2n(moe.w13_scale_int4[e]), a8[src],
                                                        t2n(moe.w13_int8[e]), sa8[src], t2n(moe.w13_scale_int8[e]))
    gate, up = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (gu[:, :F], gu[:, F:])]
    b8, b4, t8, t4 = ops.activate_fp16_i4(gate, up)
    h4, h8, hs, hs8 = t2n(b4).view(np.uint8), t2n(b8), scales_plain(t4, R, "ref"), scales_plain(t8, R, "ref")
    y = np.empty((R, H), np.float16)
    for e in range(E):
        lo, hi = indptr[e], indptr[e + 1]
        if hi > lo:
            y[lo:hi] = c_oracle.gemm(h4[lo:hi], t2n(moe.w2_int4[e]), hs[:, lo:hi], t2n(moe.w2_scale_int4[e]), h8[lo:hi], t2n(moe.w2_int8[e]),
                                     hs8[lo:hi], t2n(moe.w2_scale_int8[e]))
    return moe_ref.combine(torch.from_numpy(y), ids, w, tb["slot_row"], residual.cpu()), tb


def test_block_equals_the_chain_of_references_on_tied_logits():
    """80 tokens whose router logits are exact small integers (gate_in integers in [-2, 2], gate.weight in {-1, 0, 1} with two
    non-zeros per expert: |logit| <= 4 whatever the order of the sum), so that many tokens have equal logits at the top_k boundary;
    expert 6 gets + 9 on a column where gate_in is 1: logit 5 .. 13, chosen by every token -- 80 rows, a full tile and a second one.
    The routing comes from moe_ref.route (the lower index of equal logits); the weights from the router kernel on the same logits,
    after the ids are shown equal and the weights within the router's own 1 ulp, so that this test is about the block alone."""
    from atom_amd import ops
    from atom_amd.e2e import MixtralSparseMoeInt4
    T, ALL = 80, 6
    moe = MixtralSparseMoeInt4(_cfg()).cuda()
    g = torch.Generator().manual_seed(61)
    _load_moe(moe, g)
    gw = torch.zeros((E_, H_))
    for e in range(E_):
        cols = 1 + torch.randperm(H_ - 1, generator=g)[:2]
        gw[e, cols] = (torch.randint(0, 2, (2,), generator=g) * 2 - 1).float()
    gw[ALL, 0] += 9
    moe.gate.weight.data = gw.half().cuda()
    x = torch.randn((T, H_), generator=g)
    x[:, -128:] *= 10
    gate_in = torch.randint(-2, 3, (T, H_), generator=g).float()
    gate_in[:, 0] = 1
    x, gate_in, residual = x.half().cuda(), gate_in.half().cuda(), torch.randn((T, H_), generator=g).half().cuda()
    x_q = ops.reorder_fp16_i4(x, None)
    got = moe(x_q, gate_in, residual)
    logits = torch.nn.functional.linear(gate_in, moe.gate.weight).cpu()
    assert torch.equal(logits.double(), gate_in.cpu().double() @ gw.double().t())      # exact integers
    ids, w_ref = moe_ref.route(logits, K_)
    srt = logits.float().sort(-1, descending=True).values
    ties = int((srt[:, K_ - 1] == srt[:, K_]).sum())
    print(f"{ties} of {T} tokens have equal logits at the top_k boundary")
    assert ties >= 10 and bool((ids == ALL).any(-1).all())
    r = ops.moe_route_topk(logits.cuda(), K_)
    assert torch.equal(r.topk_ids.cpu().long(), ids)
    assert (_bits(r.topk_w).int() - _bits(w_ref).int()).abs().max().item() <= 1
    w = r.topk_w.cpu()
    want, tb = _chain_of_references(moe, x_q, ids, w, residual)
    assert tb["expert_indptr"][ALL + 1] - tb["expert_indptr"][ALL] == T and tb["n_tiles"] >= 3
    assert torch.equal(_bits(got), _bits(want))
    # the tie rule reaches the output: the chain from the opposite rule's routing gives other bits
    ids_hi, w_hi = moe_ref.route(logits, K_, tie="high")
    assert torch.equal(w_hi, w_ref) and not torch.equal(ids_hi, ids)                   # the same weights in the same slots: only ids differ
    other, _ = _chain_of_references(moe, x_q, ids_hi, w, residual)
    assert not torch.equal(_bits(other), _bits(want))


# ------------------------------------------------------------------------------------------------ 5. generation
VOCAB = 1000
PROMPT_LENS = [7, 19, 16, 33, 2]
NEW = 20


def _pool(layers, heads, capacity, block):
    from atom_amd.utils import KvPoolInt4
    pool = KvPoolInt4(layers, heads, 128, capacity, block, DEV)
    pool.buf.zero_()
    pool.param.zero_()
    return pool


def _pages(lens, block, extra=0):
    return sum(-(-(n + extra) // block) for n in lens)


def _model(seed=0):
    from atom_amd.e2e import MixtralForCausalLM
    torch.manual_seed(seed)                                   # embedding, lm_head and the reorder indices come from the global generator
    model = MixtralForCausalLM(_cfg()).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    for mod in model.modules():
        if type(mod).__name__ == "LinearInt4":
            mod.load_fp16_weight((torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05).half().cuda())
        elif type(mod).__name__ == "LlamaRMSNormInt4":
            mod.weight.data = (1 + 0.1 * torch.randn(mod.weight.shape, generator=g)).half().cuda()
        elif type(mod).__name__ == "MixtralSparseMoeInt4":
            _load_moe(mod, g)
    return model


@pytest.fixture(scope="module")
def model():
    return _model()


def _prompts(batch, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS[:batch]]


def _prefill(model, prompts, pool):
    """eager prefill of fresh sequences: (sequences, first tokens [batch], their logits [batch, vocab])"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4, KvCacheInt4
    lens = [len(p) for p in prompts]
    seqs = [KvCacheInt4(pool, n) for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    logits, _ = model(ids, BatchLenInfo(lens, 0, DEV), BatchedKvCacheInt4(seqs), None)
    first = logits[torch.tensor(lens).cumsum(0) - 1]
    return seqs, first.argmax(-1), first


def _eager_decode(model, seqs, ids, steps, cap):
    """the loop a user writes without graph replay: acquire_one on every sequence, a new BatchedKvCacheInt4, one forward, argmax"""
    from atom_amd.utils import BatchLenInfo, BatchedKvCacheInt4
    toks, logs = [], []
    for _ in range(steps):
        for c in seqs:
            c.acquire_one()
        kv = BatchedKvCacheInt4(seqs)
        kv.max_pages = cap
        logits, _ = model(ids, BatchLenInfo([], len(seqs), DEV), None, kv)
        ids = logits.argmax(-1)
        toks.append(ids)
        logs.append(logits)
    return torch.stack(toks), torch.stack(logs)


@pytest.mark.parametrize("batch", [1, 5])
def test_generate_equals_the_eager_loop(model, batch):
    from atom_amd.e2e import generate
    from atom_amd.utils import KvCacheInt4
    prompts = _prompts(batch)
    cap = max(-(-(len(p) + NEW - 1) // 16) for p in prompts)
    capacity = _pages([len(p) for p in prompts], 16, NEW) + 2
    pe = _pool(2, 2, capacity, 16)
    se, first, first_logits = _prefill(model, prompts, pe)
    toks, logs = _eager_decode(model, se, first, NEW - 1, cap)
    want_tokens = torch.cat([first[None], toks]).t().tolist()
    want_logits = torch.cat([first_logits[None], logs])
    print("distinct tokens per run:", [len(set(row)) for row in want_tokens])
    assert torch.isfinite(want_logits.float()).all()

    pg = _pool(2, 2, capacity, 16)
    free = pg.num_free_blocks
    caches = [KvCacheInt4(pg, 0) for _ in prompts]
    got_tokens, got_logits = generate(model, prompts, NEW, pg, caches=caches, return_logits=True)
    assert got_tokens == want_tokens
    assert got_logits.shape == want_logits.shape and torch.equal(got_logits, want_logits)
    assert [c.seqlen for c in caches] == [len(p) + NEW - 1 for p in prompts]
    for c in caches:
        c.release()
    assert pg.num_free_blocks == free


def test_replayed_steps_do_not_synchronise(model):
    from atom_amd.e2e import DecodeGraph
    from atom_amd.utils import StaticBatchedKvCacheInt4
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device="cuda").item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): a synchronising .item() passed under it")
    prompts, steps = _prompts(2), 20
    pool = _pool(2, 2, _pages([len(p) for p in prompts], 16, steps) + 2, 16)
    seqs, first, _ = _prefill(model, prompts, pool)
    skv = StaticBatchedKvCacheInt4(seqs, reserve=steps)
    dg = DecodeGraph(model, skv, steps)
    dg.input_ids.copy_(first)
    dg.step()
    dg.step()                                                # eager warm-up and the capture are allowed to synchronise
    torch.cuda.set_sync_debug_mode("error")
    try:
        while dg.steps_done < steps:
            dg.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    skv.close()
    assert skv.seqlens == [len(p) + steps for p in prompts]


def test_sliding_window_config_is_refused():
    from atom_amd.e2e import MixtralForCausalLM
    with pytest.raises(NotImplementedError):
        MixtralForCausalLM(_cfg(sliding_window=4096))
