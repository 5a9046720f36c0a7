"""The W4A4 GEMM entry points give, bit for bit, the outputs recorded before their route decision was folded into one function: one
small case per route (tests/gemm_route_cases.py), sha256 of the raw output bytes (and of the workspace behind them, where the call has
one).  A mismatch means a route, a tile pick or an argument moved; tests/test_gemm_host_tables_cpu.py narrows it down, and
tools/gemm_routes.py under a kernel trace names the kernels (profiles/gemm_routes/)."""
import json
import os

import pytest

from tests import gemm_route_cases as C

GROUPS = ["dot_", "decode_", "mid_int8", "staged_dot", "tiles_", "recode_", "cached_", "splitk_", "long_k_", "short_workspace", "no_workspace_needed",
          "f6_", "wide_", "o4_", "f32_", "multi_dot", "multi_decode", "multi_q_", "multi_scales", "merge_q", "gateup_"]


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "gemm_route_digests.json")) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(recorded):
    names = [c[0] for c in C.CASES]
    assert names == list(recorded) and len(names) == len(set(names)) == 76
    assert all(sum(n.startswith(g) for g in GROUPS) == 1 for n in names), [n for n in names if sum(n.startswith(g) for g in GROUPS) != 1]


def test_cases_take_the_routes_they_are_named_for():
    """CPU: the order, re-coding, workspace and fits queries say of every case what its entry in CASES claims"""
    from atom_amd._lib import lib
    for case in C.CASES:
        C.check_route(lib(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", GROUPS)
def test_outputs_equal_the_recorded_digests(recorded, prefix):
    cases = [c for c in C.CASES if c[0].startswith(prefix)]
    assert cases
    got = C.compute(cases)
    wrong = [n for n in got if got[n] != recorded[n]]
    assert not wrong, wrong
