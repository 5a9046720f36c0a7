"""Planted rows for atom_logprob_f16, shared by tests/test_logprob_cpu.py (each family must tell its rule from the obvious wrong one
of tests/logprob_ref.py) and tests/test_gpu_logprob.py (the kernel against the reference on every one of them)."""
import collections

import numpy as np

from tests.sample_cases import half_bits

Case = collections.namedtuple("Case", "name bits targets top_n tells")     # bits uint16 [rows, vocab], targets one per row

INF, NAN = np.inf, np.nan


def _case(name, row, targets, top_n, tells):
    bits = np.tile(np.asarray(row, dtype=np.uint16), (len(targets), 1))
    return Case(name, bits, [int(t) for t in targets], top_n, tuple(tells))


def planted():
    rng = np.random.default_rng(14)
    out = []
    # ties across the top-n boundary: one 3, six 2s (indices 1, 3, 4, 6, 8, 9); the top-3 takes the 2s at 1 and 3
    row = half_bits([0, 2, 3, 2, 2, 1, 2, -1, 2, 2, 0.5])
    out.append(_case("ties_across_top_n", row, [2, 1, 9, 5], 3, ("tie_high", "rank_counts_all_equals", "rank_one_based", "lp_from_temperature")))
    # the target inside a run of ten equal logits (4 in front of it, 5 behind) under two larger ones
    row = half_bits([1.5] * 3 + [4, 0] + [1.5] * 7 + [7, -2])
    out.append(_case("target_in_a_run", row, [6, 0, 11, 3], 5, ("tie_high", "rank_counts_all_equals", "rank_one_based", "lp_from_temperature")))
    # NaN, +inf, -0, -inf: NaN ranks with -inf, +inf ties with 65504 (lower index first), -0 ties with +0
    row = half_bits([NAN, 65504, INF, -0.0, 0.0, -INF, 1.0, INF, 65500])
    row[0] = 0x7E01
    out.append(_case("special_values", row, [0, 1, 2, 3, 4, 5, 6, 7], 9, ("tie_high", "rank_counts_all_equals", "rank_one_based")))
    row = half_bits([NAN, 3, -0.0, 0.0, -INF, 1.0, -NAN, 2.5, 0])
    out.append(_case("special_values_close", row, [0, 2, 3, 4, 6, 8], 6, ("tie_high", "rank_counts_all_equals", "rank_one_based", "lp_from_temperature")))
    # a -inf target among finite tokens: log-probability -inf, ranked behind every finite token in index order
    row = half_bits([0.5, -INF, 2, -INF, -INF, 1])
    out.append(_case("neg_inf_target", row, [1, 3, 4], 2, ("tie_high", "rank_counts_all_equals", "rank_one_based")))
    # nothing but -inf and NaN: every lp -inf, rank = target, top ids 0, 1, ...
    row = half_bits([-INF] * 9)
    row[4] = 0xFE00
    out.append(_case("all_neg_inf", row, [0, 4, 8], 4, ("tie_high", "rank_counts_all_equals", "rank_one_based")))
    # targets outside the row: ignored
    row = half_bits(rng.normal(0, 2, 50))
    out.append(_case("ignored_targets", row, [-1, -100, 50, 2 ** 62, 49, 0], 2, ("rank_one_based", "lp_from_temperature")))
    # top_n > vocab: the tail holds -1 / -inf
    out.append(_case("top_n_over_vocab", half_bits([1, 3, 3, -INF, 2]), [1, 2, 3], 8, ("tie_high", "rank_counts_all_equals", "rank_one_based")))
    # top_n = 32 over 1000 tokens on a grid of 0.25: ties everywhere, the boundary included
    row = half_bits(np.round(rng.normal(0, 1.5, 1000) * 4) / 4)
    top = np.argsort(-row.view(np.float16).astype(np.float32), kind="stable")
    out.append(_case("top_32", row, [int(top[0]), int(top[31]), int(top[32]), int(top[500]), 999], 32,
                     ("tie_high", "rank_counts_all_equals", "rank_one_based", "lp_from_temperature")))
    return out
