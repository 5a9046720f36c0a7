"""CPU-only checks of the LoRA entry points (include/atom_hip.h): the argument validation (it precedes every launch, so no GPU is
needed), the checker's own restatement (tests/lora_ref.py) against a direct per-row loop, and the new symbols."""
import torch

from tests import lora_ref

P = 0x10000          # a non-null, 16-byte aligned address: validation fails before anything reads it


def _lib():
    from atom_amd import _lib as L
    return L, L.lib()


def _bgmv(lib, ptrs=None, rows=32, S=32, H1=4096, H2=16, cap=4, L_=2, layer=1, scale=1.0):
    ptrs = [P, P, P, P, None] if ptrs is None else ptrs
    return lib.atom_bgmv_f16(*ptrs, rows, S, H1, H2, cap, L_, layer, scale, None)


def _add(lib, ptrs=None, rows=32, S=32, H1=4096, H2=1024, rank=16, cap=4, L_=2, layer=1, scale=1.0):
    ptrs = [P, P, P, P, P, None, P] if ptrs is None else ptrs
    return lib.atom_add_lora_f16(*ptrs, rows, S, H1, H2, rank, cap, L_, layer, scale, None)


def _kvq(lib, ptrs=None, T=5, heads=2, dim=128):
    ptrs = [P, P, P] if ptrs is None else ptrs
    return lib.atom_kv_quant_u4_f16(*ptrs, T, heads, dim, None)


def test_new_symbols_resolve():
    L, lib = _lib()
    for name in ("atom_bgmv_f16", "atom_add_lora_f16", "atom_kv_quant_u4_f16"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    from atom_amd import ops
    from atom_amd.e2e import LlamaDecoderLayerWithLora, LlamaForCausalLMWithLora, LlamaModelWithLora  # noqa: F401
    from atom_amd.utils.lora import LlamaLoraManager, LoraManager, LoraWeight  # noqa: F401
    assert callable(ops.bgmv) and callable(ops.add_lora) and callable(ops.kv_quant_u4)


def test_bgmv_rejects_bad_arguments():
    L, lib = _lib()
    for i in range(4):
        assert _bgmv(lib, ptrs=[P] * i + [None] + [P] * (3 - i) + [None]) == L.ERR_INVALID_ARG, i
    assert _bgmv(lib, H1=96) == L.ERR_SHAPE and _bgmv(lib, H1=4096 + 32) == L.ERR_SHAPE
    for r in (4, 72, 12, 0):
        assert _bgmv(lib, H2=r) == L.ERR_SHAPE, r                          # shrink: H2 is the rank
        assert _bgmv(lib, H1=r, H2=4096) == L.ERR_SHAPE, r                 # expand: H1 is the rank
    assert _bgmv(lib, H1=16, H2=96) == L.ERR_SHAPE and _bgmv(lib, H1=4096, H2=4096) == L.ERR_SHAPE
    assert _bgmv(lib, layer=2) == L.ERR_SHAPE and _bgmv(lib, layer=-1) == L.ERR_SHAPE and _bgmv(lib, L_=0, layer=0) == L.ERR_SHAPE
    assert _bgmv(lib, cap=0) == L.ERR_SHAPE and _bgmv(lib, rows=0, S=0) == L.ERR_SHAPE
    assert _bgmv(lib, S=31) == L.ERR_SHAPE                                 # no segment table: one id per row
    seg = [P, P, P, P, P]
    assert _bgmv(lib, ptrs=seg, S=0) == L.ERR_SHAPE and _bgmv(lib, ptrs=seg, S=33) == L.ERR_SHAPE
    for i in range(3):
        assert _bgmv(lib, ptrs=[P] * i + [P + 8] + [P] * (3 - i) + [None]) == L.ERR_ALIGN, i
    assert _bgmv(lib, ptrs=[P, P, P, P + 2, None]) == L.ERR_ALIGN and _bgmv(lib, ptrs=[P, P, P, P, P + 2], S=3) == L.ERR_ALIGN


def test_add_lora_rejects_bad_arguments():
    L, lib = _lib()
    for i in (0, 1, 2, 3, 4, 6):
        ptrs = [P, P, P, P, P, None, P]
        ptrs[i] = None
        assert _add(lib, ptrs=ptrs) == L.ERR_INVALID_ARG, i
    assert _add(lib, H1=96) == L.ERR_SHAPE and _add(lib, H2=96) == L.ERR_SHAPE and _add(lib, H1=0) == L.ERR_SHAPE
    for r in (4, 72, 12, 0):
        assert _add(lib, rank=r) == L.ERR_SHAPE, r
    assert _add(lib, layer=2) == L.ERR_SHAPE and _add(lib, cap=0) == L.ERR_SHAPE
    assert _add(lib, rows=0, S=0) == L.ERR_SHAPE and _add(lib, S=5) == L.ERR_SHAPE
    seg = [P] * 7
    assert _add(lib, ptrs=seg, S=0) == L.ERR_SHAPE and _add(lib, ptrs=seg, S=33) == L.ERR_SHAPE
    for i in (0, 1, 2, 3, 6):
        ptrs = [P, P, P, P, P, None, P]
        ptrs[i] = P + 8
        assert _add(lib, ptrs=ptrs) == L.ERR_ALIGN, i
    assert _add(lib, ptrs=[P, P, P, P, P + 2, None, P]) == L.ERR_ALIGN and _add(lib, ptrs=[P] * 5 + [P + 2, P], S=3) == L.ERR_ALIGN


def test_kv_quant_rejects_bad_arguments():
    L, lib = _lib()
    for i in range(3):
        assert _kvq(lib, ptrs=[P] * i + [None] + [P] * (2 - i)) == L.ERR_INVALID_ARG
    assert _kvq(lib, T=0) == L.ERR_SHAPE and _kvq(lib, heads=0) == L.ERR_SHAPE and _kvq(lib, dim=64) == L.ERR_SHAPE
    assert _kvq(lib, ptrs=[P + 8, P, P]) == L.ERR_ALIGN and _kvq(lib, ptrs=[P, P + 8, P]) == L.ERR_ALIGN
    assert _kvq(lib, ptrs=[P, P, P + 2]) == L.ERR_ALIGN


def test_reference_equals_a_direct_per_row_loop():
    rows, h1, h2, r = 7, 64, 64, 8
    y, x, wa, wb = lora_ref.exact_inputs(rows, h1, h2, r, 3, 2, seed=5)
    ids = [2, -1, 0, 0, 3, 1, 2]                                           # 3: outside the pool, treated as "none"
    want = lora_ref.add_lora_rows(y, x, wa, wb, ids, 1, 0.25)
    got = lora_ref.add_lora(y, x, wa, wb, ids, 1, 0.25, exact=True)
    assert torch.equal(lora_ref.bits(got), lora_ref.bits(want))
    assert torch.equal(lora_ref.bits(got[1]), lora_ref.bits(y[1])) and torch.equal(lora_ref.bits(got[4]), lora_ref.bits(y[4]))
    assert not torch.equal(got[0], y[0])
    # segmented: the same rows grouped -- [0, 1) id 2, [1, 2) none, [2, 4) id 0, an empty one, rows 4 .. 6 behind the table
    seg = lora_ref.add_lora(y, x, wa, wb, [2, -1, 0, 1], 1, 0.25, seg_indptr=[0, 1, 2, 4, 4], exact=True)
    assert torch.equal(lora_ref.bits(seg[:4]), lora_ref.bits(want[:4])) and torch.equal(lora_ref.bits(seg[4:]), lora_ref.bits(y[4:]))
    # add_lora is two bgmv passes
    t = lora_ref.bgmv(torch.zeros(rows, r).half(), x, wa, ids, 1, 1.0, exact=True)
    assert torch.equal(lora_ref.bits(lora_ref.bgmv(y, t, wb, ids, 1, 0.25, exact=True)), lora_ref.bits(want))


def test_exact_inputs_are_exact_at_the_gpu_tests_shapes():
    """the figures the GPU tests rely on: t and the result are fp16 values at the tests' largest shapes"""
    y, x, wa, wb = lora_ref.exact_inputs(82, 320, 192, 24, 3, 2, seed=1)
    lora_ref.add_lora(y, x, wa, wb, [i % 3 for i in range(82)], 1, 0.25, exact=True)
    y, x, wa, wb = lora_ref.exact_inputs(33, 4096, 1024, 64, 2, 1, seed=4)
    lora_ref.add_lora(y, x, wa, wb, [i % 2 for i in range(33)], 0, 0.125, exact=True)
    for rank in (16, 32):                                                  # tests/test_gpu_lora.py::_case at its added ranks
        y, x, wa, wb = lora_ref.exact_inputs(82, 320, 192, rank, 3, 2, seed=10 + rank, guard=8)
        lora_ref.add_lora(y, x, wa, wb, [i % 3 for i in range(90)], 1, 0.25, exact=True)
    for rank in (16, 32, 48, 56):                                          # ... and the operands of its bgmv test, both regimes
        y, x, _, _ = lora_ref.exact_inputs(82, 320, 192, 8, 3, 2, seed=18, guard=8)
        g = torch.Generator().manual_seed(rank)
        w_s, y_s = torch.randint(-1, 2, (3, 2, rank, 320), generator=g).half(), torch.randint(-8, 9, (82, rank), generator=g).half()
        lora_ref.bgmv(y_s, x[:82], w_s, [i % 3 for i in range(82)], 1, 0.25, exact=True)
        w_e, x_e = torch.randint(-1, 2, (3, 2, 192, rank), generator=g).half(), torch.randint(-2, 3, (82, rank), generator=g).half()
        lora_ref.bgmv(y[:82], x_e, w_e, [i % 3 for i in range(82)], 1, 0.25, exact=True)
    ptr, ids = lora_ref.long_table()                                       # the long table: every segment on a real adapter
    for rank in (8, 64):
        y, x, wa, wb, y_s, x_e = lora_ref.long_case(rank)
        every = [s % lora_ref.LONG_CAP for s in range(lora_ref.LONG_S)]
        lora_ref.add_lora(y, x, wa, wb, every, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True)
        lora_ref.bgmv(y_s, x, wa, every, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True)
        lora_ref.bgmv(y, x_e, wb, every, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True)


def test_long_table_meets_the_abi_and_tells_a_lost_tile_count():
    """the table of the GPU test: within the ABI (ascending, inside the rows, rows >= S), more than 64 segments with a whole block
    of 64 empty ones; and shifting the adapters of segments 128 .. 199 by one -- what a search that forgot the tiles of the first
    two blocks would honour -- changes at least one row of EVERY non-empty segment there, for add_lora and for both single passes"""
    ptr, ids = lora_ref.long_table()
    S, rows = lora_ref.LONG_S, ptr[-1]
    assert len(ptr) == S + 1 and len(ids) == S and S > 128 and ptr[0] == lora_ref.LONG_FIRST > 0
    assert all(a <= b for a, b in zip(ptr, ptr[1:])) and rows + lora_ref.LONG_GUARD >= S
    assert ptr[64] == ptr[128] and ptr[64] > ptr[0] and ptr[S] > ptr[128]
    assert -1 in ids and any(a >= lora_ref.LONG_CAP for a in ids) and {0, 1, 2} <= set(ids)
    shifted = lora_ref.long_ids_shifted(ids)
    assert shifted[:128] == ids[:128]
    none = lambda a: not 0 <= a < lora_ref.LONG_CAP
    assert all(a != b and not (none(a) and none(b)) for a, b in zip(ids[128:], shifted[128:]))
    live = [s for s in range(128, S) if ptr[s + 1] > ptr[s]]
    for rank in (8, 64):
        y, x, wa, wb, y_s, x_e = lora_ref.long_case(rank)
        assert y.size(0) == rows + lora_ref.LONG_GUARD
        for what, fn in (("add_lora", lambda i: lora_ref.add_lora(y, x, wa, wb, i, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True)),
                         ("shrink", lambda i: lora_ref.bgmv(y_s, x, wa, i, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True)),
                         ("expand", lambda i: lora_ref.bgmv(y, x_e, wb, i, lora_ref.LONG_LAYER, 0.25, seg_indptr=ptr, exact=True))):
            want, other = fn(ids), fn(shifted)
            told = [s for s in live if not torch.equal(lora_ref.bits(want[ptr[s]:ptr[s + 1]]), lora_ref.bits(other[ptr[s]:ptr[s + 1]]))]
            print(f"rank {rank} {what}: the shifted adapters change {len(told)} of the {len(live)} non-empty segments 128 .. 199")
            assert told == live
            assert torch.equal(lora_ref.bits(want[:ptr[128]]), lora_ref.bits(other[:ptr[128]]))
            assert torch.equal(lora_ref.bits(want[:ptr[0]]), lora_ref.bits((y_s if what == "shrink" else y)[:ptr[0]]))
            assert bool((lora_ref.bits(want[rows:]) == lora_ref.LONG_SENTINEL).all())


def test_pool_folds_alpha_into_b_and_permutes_the_intermediate_channels():
    import types
    from atom_amd.utils.lora import LlamaLoraManager, permute_intermediate
    cfg = types.SimpleNamespace(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)
    mgr = LlamaLoraManager(cfg, capacity=3, lora_rank=8, target_modules=("v_proj", "q_proj", "down_proj"), device="cpu")
    assert mgr.target_modules == ("q_proj", "v_proj", "down_proj") and set(mgr.mgr) == set(mgr.target_modules)
    assert mgr.mgr["v_proj"].wb_T.shape == (3, 2, 128, 8) and mgr.mgr["down_proj"].wa_T.shape == (3, 2, 8, 512)
    w0, w1 = mgr.alloc(), mgr.alloc()
    assert (w0.idx, w1.idx) == (0, 1) and w1.modules["q_proj"].idx == 1
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(8, 256, generator=g), torch.randn(128, 8, generator=g)
    mgr.load(w1, 1, "v_proj", A, B, alpha=16)
    assert torch.equal(mgr.mgr["v_proj"].wa_T[1, 1], A.half()) and torch.equal(mgr.mgr["v_proj"].wb_T[1, 1], (B * 2.0).half())
    assert not mgr.mgr["v_proj"].wb_T[0].any() and not mgr.mgr["v_proj"].wb_T[1, 0].any()
    idx = torch.randperm(512, generator=g)
    Ad, Bd = torch.randn(8, 512, generator=g), torch.randn(256, 8, generator=g)
    A2, B2 = permute_intermediate("down_proj", Ad, Bd, idx)
    act = torch.randn(512, generator=g)
    assert torch.allclose(A2 @ act[idx], Ad @ act, atol=1e-4) and B2 is Bd
    Ag, Bg = torch.randn(8, 256, generator=g), torch.randn(512, 8, generator=g)
    A3, B3 = permute_intermediate("gate_proj", Ag, Bg, idx)
    assert A3 is Ag and torch.equal(B3, Bg[idx])
    mgr.free(w1)
    assert not mgr.mgr["v_proj"].wb_T.any() and mgr.alloc().idx == 1
    try:
        mgr.load(w0, 0, "k_proj", A, B)
        raise AssertionError("an untargeted module was accepted")
    except KeyError:
        pass
