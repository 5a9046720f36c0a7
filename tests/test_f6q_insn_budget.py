"""Instruction budget of the headline 256x256 BF6 GEMM instantiation, counted in its device assembly by tools/insn_model.py.

Counts instruction classes only (v_mfma / v_ / ds_ / global_ / s_waitcnt); needs hipcc, skipped without it."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_PER_STEP_BEFORE = 48          # the kernel before the token scales were read in pairs: 8 scale reads per K step, now 4


def _tool():
    spec = importlib.util.spec_from_file_location("insn_model", os.path.join(ROOT, "tools", "insn_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def priced():
    tool = _tool()
    hipcc, _ = tool.makefile_flags()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    return tool.model(tool.build_asm(), G=31, clock_ghz=2.0)


def test_headline_kernel_has_no_spill_and_no_scratch(priced):
    assert priced["spill_or_scratch"] == []
    f = priced["facts"]
    assert f["ScratchSize"] == 0 and f["private_segment_fixed_size"] == 0
    assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0
    assert f["Occupancy"] == 2


def test_main_loop_body_is_within_its_budget(priced):
    loop = priced["static"]["loop"]
    assert loop["mfma"] == 96                                   # three K steps of 32 BF6 MFMA
    assert loop["valu"] <= 588                                  # 6 de-quantisation VALU per MFMA + at most 12 others
    assert loop["lds"] <= 3 * LDS_PER_STEP_BEFORE
    assert priced["per_step"]["lds"] <= LDS_PER_STEP_BEFORE
    assert loop["barrier"] == 3 and loop["vmem"] == 21          # one barrier and seven LDS-DMA groups per step


def test_every_region_has_its_k_steps(priced):
    s = priced["static"]
    assert [s[k]["mfma"] for k in ("prologue", "loop", "tail_ct", "tail_gen", "keeper")] == [96, 96, 64, 32, 64]
    assert priced["dynamic"]["mfma"] == 32 * 31 + 64            # 31 int4 steps + the keeper step at K = 4096
    assert priced["runs"] == {"prologue": 1, "loop": 8, "tail_ct": 1.0, "tail_gen": 2, "keeper": 1}


def test_schedule_matches_the_kernels_loop_structure():
    tool = _tool()
    for G in range(6, 64):
        r = tool.schedule(G)
        assert 3 + 3 * r["loop"] + 2 * r["tail_ct"] + r["tail_gen"] == G and r["tail_gen"] == 2
    with pytest.raises(tool.ModelError):
        tool.schedule(5)
