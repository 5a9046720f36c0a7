"""Planted rows for atom_penalize_f16, shared by tests/test_penalty_cpu.py (each family must tell its rule from the obvious wrong
one, tests/penalty_ref.py ``wrong=``) and tests/test_gpu_penalize.py (which runs the kernel on them).  A case is one row of logits
(uint16 bits), its state words, the token fed in (or None), the three parameters and a bias list.  Rows are longer than two tiles of
the kernel, with the planted elements on both sides of a tile edge and in the tail; most elements are unseen and unbiased, and hold
NaN payloads and signed zeros among them, so a kernel that recomputes what it should copy fails every case."""
import collections

import numpy as np

from atom_amd import ops
from tests import penalty_ref

TILE = ops.PENALTY_TILE
VOCAB = 2 * TILE + 5
Case = collections.namedtuple("Case", "name bits words fed rep pres freq bias_ids bias_vals tells")


def half_bits(values):
    with np.errstate(over="ignore"):
        return np.asarray(values, dtype=np.float64).astype(np.float16).view(np.uint16).copy()


def background(rng, vocab=VOCAB):
    """N(0, 3^2) logits with every 97th word a NaN of some payload, a signed zero or an infinity"""
    bits = half_bits(rng.normal(0.0, 3.0, vocab))
    special = (0x7C01, 0xFE00, 0x7DFF, 0x8000, 0x0000, 0xFC00, 0x7C00, 0xFFFF, 0x0001, 0x8001)
    for n, i in enumerate(range(5, vocab, 97)):
        bits[i] = special[n % len(special)]
    return bits


SPOTS = (0, 1, 7, 8, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, VOCAB - 1)


def planted():
    rng = np.random.default_rng(15)
    out = []

    def add(name, values, words, fed=None, rep=1.0, pres=0.0, freq=0.0, bias=(), tells=None, spots=SPOTS):
        """``values`` (floats) and ``words`` are planted at ``spots``; bias: (id, value) pairs"""
        bits, state = background(rng), np.zeros(VOCAB, dtype=np.uint16)
        spots = list(spots)[:len(values)]
        bits[spots] = half_bits(values)
        state[spots] = np.asarray(words, dtype=np.uint16)
        ids, vals = [i for i, _ in bias], [v for _, v in bias]
        out.append(Case(name, bits, state, fed, rep, pres, freq, ids, vals, tells))

    vals10 = [2.5, -2.5, 0.75, -0.125, 11.0, -7.0, 3.0, -3.0, 0.33, 5.5]
    # generated tokens of both signs under a repetition penalty: the positive ones are divided
    add("rep_signs", vals10, [1, 2, 3, 1, 1, 0x8001, 4, 1, 9, 1], rep=1.5, tells="mul_positive")
    # prompt-only tokens: presence and frequency leave them alone, the repetition penalty does not
    add("prompt_only_pres_freq", vals10, [0x8000] * 10, pres=0.5, freq=0.25, tells="pres_freq_on_prompt")
    add("prompt_only_rep", vals10, [0x8000] * 10, rep=2.0, tells="rep_skips_prompt")
    add("prompt_and_generated", vals10, [0x8000, 0x8001, 1, 0x8003, 2, 0x8000, 0, 1, 0x8000, 0x8002], rep=1.25, pres=0.5, freq=0.25,
        tells="pres_freq_on_prompt")
    # the fed token is counted before the row is penalised: a first occurrence is already seen, a later one already one higher
    for spot in (0, TILE - 1, TILE, VOCAB - 1):
        add(f"fed_first_at_{spot}", vals10, [0] * 10, fed=spot, pres=1.0, tells="count_after")
    add("fed_again", vals10, [0, 0, 0, 0, 0, 3, 0, 0, 0, 0], fed=TILE, freq=0.5, rep=1.1, tells="count_after")
    # every line rounds to FP32, only the last to fp16: many seen elements with all four terms
    bits_r = rng.normal(0.0, 4.0, 600)
    spots_r = rng.choice(VOCAB, 600, replace=False).tolist()
    words_r = rng.integers(1, 6, 600).tolist()
    add("fp32_between_lines", bits_r, words_r, rep=1.3, pres=0.37, freq=0.1, bias=[(s, 0.013) for s in spots_r[:200]],
        tells="round_between", spots=spots_r)
    # the bias is added last: after the division / multiplication, not before it
    add("bias_last", [1.0, -1.0, 4.0, -4.0, 0.5, 2.0, -2.0, 8.0, 1.5, 3.0], [1] * 10, rep=2.0,
        bias=[(s, b) for s, b in zip(SPOTS, (-3.0, 3.0, -6.0, 6.0, -1.0, -5.0, 5.0, -9.0, 2.0, -3.5))], tells="bias_first")
    # the count saturates at 32767 and keeps the prompt flag
    add("count_32766", vals10, [32766] + [0] * 9, fed=0, freq=2.0 ** -10)
    add("count_32767", vals10, [32767] + [0] * 9, fed=0, freq=2.0 ** -10, tells="count_wraps")
    add("count_32767_prompt", vals10, [0] * 4 + [0xFFFF] + [0] * 5, fed=TILE - 1, freq=2.0 ** -10, rep=1.5, tells="count_wraps")
    # special values follow IEEE: overflow to inf, a -inf bias, inf - inf, NaN in; -0 stays -0 when only zeros are subtracted
    spec = np.array([60000.0, -60000.0, np.inf, -np.inf, np.nan, -0.0, 0.0, 65504.0, 1e-7, -1e-7])
    add("specials_rep", spec, [1] * 10, rep=0.5)
    add("specials_bias_only", spec, [0] * 10, bias=[(s, b) for s, b in zip(SPOTS, (-np.inf, np.inf, -np.inf, np.inf, 1.0, 0.0, -0.0, 100.0, -1e-7, 0.0))])
    add("specials_freq_inf", spec, [2, 0, 1, 0, 0, 0x8000, 0, 0, 0, 0], freq=np.inf, bias=[(1, 1.0), (TILE, 2.0)])
    add("rep_clamped", vals10, [1] * 10, rep=1e9)
    add("rep_clamped_low", vals10, [1] * 10, rep=1e-9)
    add("rep_off_negative", vals10, [1] * 10, rep=-2.0, pres=0.25)
    add("rep_off_nan", vals10, [1] * 10, rep=np.nan, freq=0.25)
    return out


def expected(case, wrong=None):
    return penalty_ref.penalize_row(case.bits, case.words, case.fed, case.rep, case.pres, case.freq, case.bias_ids, case.bias_vals, wrong=wrong)
