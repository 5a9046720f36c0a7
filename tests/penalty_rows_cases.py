"""Planted sequences for atom_penalize_rows_f16, shared by tests/test_penalty_rows_cpu.py (each mutant of tests/penalty_rows_ref.py
must be told from the contract by at least one of them) and tests/test_gpu_penalize_rows.py (which runs the kernel on them).  A case is
one sequence: ROWS verify rows of logits (uint16 bits, the background of tests/penalty_cases.py with NaN payloads and signed zeros),
its state words, the step's input ids (column 0, then the drafts), the pending tokens with their count, the three parameters and a
bias list.  The planted elements sit at penalty_cases.SPOTS: both sides of a tile edge, and the partial tail of the last thread."""
import collections

import numpy as np

from tests import penalty_cases, penalty_rows_ref

TILE, VOCAB, SPOTS = penalty_cases.TILE, penalty_cases.VOCAB, penalty_cases.SPOTS
ROWS = 5
Case = collections.namedtuple("Case", "name bits words ids pending count rep pres freq bias_ids bias_vals tells")


def planted():
    rng = np.random.default_rng(20)
    out = []
    vals10 = [2.5, -2.5, 0.75, -0.125, 11.0, -7.0, 3.0, -3.0, 0.33, 5.5]

    def add(name, ids, words=(), pending=(), count=None, rep=1.0, pres=0.0, freq=0.0, bias=(), tells=()):
        """``words``: (spot, word) pairs; bias: (id, value) pairs; every row holds vals10 (each row scaled) at SPOTS"""
        bits = np.stack([penalty_cases.background(rng) for _ in range(ROWS)])
        for j in range(ROWS):
            bits[j, list(SPOTS)] = penalty_cases.half_bits([v * (1.0 + 0.25 * j) for v in vals10])
        state = np.zeros(VOCAB, dtype=np.uint16)
        for s, w in words:
            state[s] = w
        assert len(ids) == ROWS
        out.append(Case(name, bits, state, list(ids), list(pending), len(pending) if count is None else count, rep, pres, freq,
                        [i for i, _ in bias], [v for _, v in bias], tuple(tells)))

    # all drafts equal: row j counts j more, and no row sees the drafts behind it
    add("all_equal", [3, TILE, TILE, TILE, TILE], freq=0.5, pres=0.25, tells=("sees_later_drafts", "drafts_written"))
    # a draft equal to column 0: column 0 was committed by the step that emitted it and is not counted again
    add("draft_equals_col0", [7, 7, 1, 8, 0], words=[(7, 1)], freq=0.5, rep=1.2, tells=("col0_counted",))
    add("col0_alone", [2 * TILE, 1, 1, 8, 8], words=[(2 * TILE, 2)], freq=0.5, tells=("col0_counted",))
    # a draft equal to a pending token: the commit comes first, the draft counts on top of it
    add("draft_equals_pending", [8, TILE - 1, 8, TILE - 1, 0], pending=[TILE - 1, 8], pres=1.0, freq=0.25, tells=("commit_after",))
    add("pending_seen_by_row0", [1, 0, 0, 0, 0], pending=[VOCAB - 1, TILE, 1], rep=1.5, tells=("commit_after",))
    # drafts in two tiles and in the partial tail of the vocabulary's last thread
    add("two_tiles_and_tail", [0, 1, TILE + 1, 2 * TILE, VOCAB - 1], pres=0.5, freq=0.125, rep=1.3, tells=("drafts_written",))
    # drafts and pending tokens outside the vocabulary count nothing (VOCAB + 3 lies inside the padding of the leading dimension)
    add("out_of_range", [0, -1, VOCAB, VOCAB + 3, 2 ** 40], pending=[VOCAB, -5, 3, 2 ** 40 + 8, VOCAB + 3], words=[(0, 1), (8, 2)],
        rep=1.5, freq=0.5)
    # the count saturates at 32767 and keeps the prompt flag
    add("count_32766", [5, 0, 0, 0, 1], words=[(0, 32766)], freq=2.0 ** -10)
    add("count_32767", [5, TILE, TILE - 1, TILE, 1], words=[(TILE, 32767), (TILE - 1, 0xFFFF)], pending=[TILE, TILE - 1], freq=2.0 ** -10,
        rep=1.5)
    # a prompt-flag-only word: the flag is kept, presence and frequency start at the row behind the first draft of it
    add("prompt_flag_only", [2, 1, 1, TILE, 8], words=[(s, 0x8000) for s in SPOTS], rep=1.5, pres=0.5, freq=0.25,
        tells=("sees_later_drafts",))
    # duplicates among the pending tokens count once per occurrence
    add("dup_pending", [0, 1, 7, 7, 1], pending=[8, 8, TILE, 8], freq=0.5, tells=("dup_once",))
    # the count is clamped: a negative one commits nothing, a large one what the row holds
    add("count_negative", [0, 1, 7, 7, 1], pending=[8, TILE], count=-3, freq=0.5, pres=0.25)
    add("count_large", [0, 1, 7, 7, 1], pending=[8, TILE, 8], count=40, freq=0.5, pres=0.25)
    add("count_one_of_three", [0, 1, 7, 7, 1], pending=[8, TILE, 1], count=1, freq=0.5, pres=0.25)
    # a neutral sequence: its rows are copied bit for bit, its state is committed all the same
    add("neutral", [0, 1, TILE, TILE, VOCAB - 1], words=[(1, 3), (TILE, 0x8000)], pending=[TILE, 1, VOCAB - 1])
    # a bias as the only thing that makes the sequence non-neutral; an id equal to a draft, a -inf bias
    add("bias_only", [0, TILE, 1, TILE, 8], pending=[7], bias=[(TILE, -np.inf), (1, 2.0), (2 * TILE, 0.5)])
    add("bias_and_penalties", [0, TILE, 1, TILE, 8], pending=[7, 1], rep=1.25, pres=0.5, freq=0.25,
        bias=[(TILE, -3.0), (1, 2.0), (VOCAB - 1, -np.inf)], tells=("drafts_written",))
    return out


def expected(case, wrong=None):
    return penalty_rows_ref.penalize_rows_seq(case.bits, case.words, case.ids, case.pending, case.count, case.rep, case.pres, case.freq,
                                              case.bias_ids, case.bias_vals, wrong=wrong)
