"""The INT4 paged-KV attention ops give, bit for bit, the outputs recorded before their host paths were folded into one plan and one
launcher per kernel family: one small case per path (tests/attn_digests.py), sha256 of the raw output bytes -- of the partial-state
tensor for merge=False.  A mismatch means a plan or an argument moved; tests/test_attn_host_tables_cpu.py narrows it down."""
import json
import os

import pytest

from tests import attn_digests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "attn_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return attn_digests.compute()


def test_cases_are_the_recorded_ones(computed, recorded):
    assert computed["contexts"] == recorded["contexts"]
    assert list(computed["sha256"]) == list(recorded["sha256"]) and len(recorded["sha256"]) == 23


@pytest.mark.parametrize("prefix", ["decode_unsplit", "decode_split_", "decode_inner", "decode_wgm", "prefill_", "decode_gqa_"])
def test_outputs_equal_the_recorded_digests(computed, recorded, prefix):
    names = [n for n in recorded["sha256"] if n.startswith(prefix)]
    assert names
    wrong = [n for n in names if computed["sha256"].get(n) != recorded["sha256"][n]]
    assert not wrong, wrong
