"""Planted rows for the sampler's tests, shared by the CPU tests (which show that each family tells its rule from the obvious wrong
one, tests/sample_ref.py ``wrong=``) and the GPU tests (which run the kernel on them).  A case is one row, its parameters, and the
(seed, step) pairs it is drawn with; the GPU test runs the seeds of a case as the rows of one batch."""
import collections

import numpy as np

from tests import sample_ref

Case = collections.namedtuple("Case", "name bits T k p seeds steps tells")

# steps at which Philox word 0 of seed 5 is a multiple of 2^14 (2^16): with 2^18 (2^16) equal logits the draw's target
# (Z * R) >> 32 = R * 2^26 (R * 2^24) is then exactly a cumulative weight -- a multiple of 2^40 -- so "> target" and ">= target" differ
BOUNDARY_SEED = 5
BOUNDARY_STEPS_2_18 = (245, 10758, 12691)
BOUNDARY_STEPS_2_16 = (66377,)


def half_bits(values):
    with np.errstate(over="ignore"):
        return np.asarray(values, dtype=np.float64).astype(np.float16).view(np.uint16).copy()


def _equal(n, value=1.0):
    return np.full(n, half_bits([value])[0], dtype=np.uint16)


def planted():
    rng = np.random.default_rng(7)
    seeds = list(range(12))
    wide = [3, 2 ** 32 + 9, 2 ** 63 + 12345, 2 ** 64 - 1, 77, 2 ** 40]               # seeds with a non-zero high word among them
    out = []
    add = lambda *a, tells=None: out.append(Case(*a, tells))
    # all logits equal: the token is the draw's rank, ties resolved by index alone
    add("equal4", _equal(4), 1.0, 0, 1.0, seeds, (0, 1), tells="tie_high")
    add("equal64", _equal(64, -2.5), 0.7, 0, 1.0, seeds, (0, 7), tells="tie_high")
    add("equal64_greedy", _equal(64), 0.0, 0, 1.0, [0, 1], (0,), tells="tie_high")
    add("equal65536", _equal(65536), 1.0, 0, 1.0, [BOUNDARY_SEED, 6], BOUNDARY_STEPS_2_16 + (0,), tells="ge_target")
    add("equal2_18", _equal(1 << 18), 1.0, 0, 1.0, [BOUNDARY_SEED, 9], BOUNDARY_STEPS_2_18[:2] + (0, 1, 2), tells="ge_target")
    # ties that straddle the top-k boundary: k = 4 keeps token 0 and the first three of the seven 2.0s
    row = half_bits([3.0, 2.0, 0.5, 2.0, 2.0, 1.0, 2.0, 2.0, -1.0, 2.0, 2.0, 0.0])
    add("ties_at_top_k", row, 1.0, 4, 1.0, seeds, (0, 1, 2), tells="tie_high")
    # ties that straddle the top-p boundary: 0.55 of the mass ends inside the run of 1.5s
    row = half_bits([1.5] * 3 + [4.0] + [1.5] * 9 + [0.0] * 5)
    add("ties_at_top_p", row, 1.0, 0, 0.55, seeds, (0, 1, 2), tells="tie_high")
    # ties inside the drawn key: two large tied groups spread over the row
    row = half_bits(rng.integers(0, 2, 300) * 0.25)
    add("ties_in_drawn_key", row, 1.0, 0, 1.0, seeds, (0, 1), tells="tie_high")
    # top-k and top-p together on a flat-ish row: the order of the two cuts and the sum top-p refers to both matter
    row = half_bits(rng.normal(0.0, 1.0, 200))
    add("k_then_p", row, 1.0, 5, 0.5, seeds, (0, 1, 2, 3), tells="p_before_k")
    add("p_of_kept_sum", row, 1.5, 8, 0.6, seeds, (0, 1, 2, 3), tells="p_full_z")
    # special values: +-0 are one key; NaN is -inf; +inf is 65504; an all -inf and an all-NaN row give token 0
    row = half_bits([0.0, -0.0, -1.0, 0.0, -0.0])
    add("signed_zeros", row, 1.0, 0, 1.0, seeds, (0, 1), tells="tie_high")
    add("signed_zeros_greedy", np.array([0x8000, 0x0000, 0x8000], dtype=np.uint16), 0.0, 0, 1.0, [0], (0,))
    row = half_bits([1.0, 2.0, 0.0, 2.0, -3.0, 1.0, 0.5])
    row[2], row[4] = 0x7E00, 0xFFFF                                                    # NaNs of both signs
    add("nan_is_masked", row, 1.0, 0, 1.0, seeds, (0, 1))
    row = half_bits([65504.0, 1.0, 0.0, 65504.0, 60000.0])
    row[0] = 0x7C00                                                                    # +inf ties with 65504 at index 3
    add("plus_inf", row, 1024.0, 0, 1.0, seeds, (0, 1), tells="tie_high")
    row[1] = 0xFC00
    add("plus_inf_greedy", row, 0.0, 0, 1.0, [0], (0,))
    add("all_minus_inf", np.full(70, 0xFC00, dtype=np.uint16), 1.0, 3, 0.5, [0, 1], (0,))
    add("all_nan", np.full(9, 0x7E00, dtype=np.uint16), 0.0, 0, 1.0, [0, 1], (0,))
    row = np.full(1000, 0xFC00, dtype=np.uint16)
    row[[17, 512, 999]] = half_bits([-5.0, -5.0, -7.0])
    add("mostly_minus_inf", row, 1.0, 900, 0.999, seeds, (0, 1))                       # the kept prefix runs into the -inf tail
    # weights that underflow: x < -40 a little below the maximum at T = 2^-10; far below it at T = 1
    row = half_bits(np.concatenate([[8.0, 7.99, 7.98, 7.97, 7.96], rng.normal(0.0, 2.0, 400)]))
    add("underflow_cold", row, 1e-6, 0, 0.9999, seeds, (0, 1))
    row = half_bits(np.concatenate([rng.normal(100.0, 3.0, 40), rng.normal(0.0, 3.0, 400), rng.normal(74.0, 1.0, 40)]))
    add("underflow", row, 1.0, 0, 1.0, seeds, (0, 1))
    add("underflow_top_k", row, 1.0, 300, 0.99999, seeds, (0,))
    # the second-largest logit one half-ulp below the largest
    row = half_bits(rng.normal(0.0, 1.0, 129))
    row[77], row[5] = 0x4500, 0x44FF
    add("one_ulp_below", row, 1.0, 2, 1.0, seeds, (0, 1))
    add("one_ulp_below_greedy", row, 0.0, 0, 1.0, [0], (0,))
    add("one_ulp_below_hot", row, 1e6, 0, 0.75, wide, (2 ** 32 + 5, 2 ** 62))
    return out


def expected(case, step, wrong=None):
    return [sample_ref.sample_row(case.bits, case.T, case.k, case.p, s, step, wrong=wrong) for s in case.seeds]
