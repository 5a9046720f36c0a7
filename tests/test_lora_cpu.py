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
