"""The checker's restatement of atom_logprob_f16 (include/atom_hip.h), independent of the kernel's sources: the
canonical logits and the T = 1 weights of tests/sample_ref.py, a stable lexsort for the order, Python ints for the row sum Z, NumPy
float64 log, then float32.  ``wrong=`` swaps ONE rule for the obvious wrong one, for the tests that show a planted family tells the
two apart.  ``lz_step`` moves lz to a float32 neighbour: the only allowance of the contract (the last bit of a double log)."""
import collections

import numpy as np

from tests import sample_ref

WRONG = ("tie_high", "rank_counts_all_equals", "lp_from_temperature", "rank_one_based")
WRONG_TEMPERATURE = 0.5          # what "lp_from_temperature" divides the logits by
NEG_INF = np.float32(-np.inf)
LN2_40 = np.float64(40.0) * np.log(np.float64(2.0))

Row = collections.namedtuple("Row", "logprob rank top_ids top_logprobs z lz")


def log_z(z, lz_step=0):
    lz = np.float32(np.log(np.float64(int(z))) - LN2_40)
    if lz_step:
        lz = np.nextafter(lz, np.float32(np.inf if lz_step > 0 else -np.inf), dtype=np.float32)
    return np.float32(lz)


def logprob_row(bits, target=None, top_n=0, wrong=None, lz_step=0):
    """one row: ``Row(logprob float32, rank int, top_ids int64 [top_n], top_logprobs float32 [top_n], Z int, lz float32)``;
    ``target`` None: logprob and rank are None"""
    assert wrong is None or wrong in WRONG
    l = sample_ref.canonical(bits)
    vocab = l.size
    idx = np.arange(vocab)
    order = np.lexsort((-idx if wrong == "tie_high" else idx, -l))            # l descending, then index
    m = l.max()
    if m == NEG_INF:
        z, lz = 0, np.float32(0.0)
        lp = np.full(vocab, NEG_INF, dtype=np.float32)
    else:
        T = np.float32(WRONG_TEMPERATURE if wrong == "lp_from_temperature" else 1.0)
        z = sum(int(x) for x in sample_ref.weights(l, T).tolist())
        assert (1 << 40) <= z < (1 << 59)
        lz = log_z(z, lz_step)
        with np.errstate(all="ignore"):
            lp = ((l - m).astype(np.float32) - lz).astype(np.float32)
    logprob = rank = None
    if target is not None:
        t = int(target)
        if 0 <= t < vocab:
            logprob = np.float32(lp[t])
            before = l[t + 1:] if wrong == "tie_high" else l[:t]
            rank = int((l > l[t]).sum()) + int((before == l[t]).sum())
            if wrong == "rank_counts_all_equals":
                rank = int((l > l[t]).sum()) + int((l == l[t]).sum()) - 1
            if wrong == "rank_one_based":
                rank += 1
        else:
            logprob, rank = np.float32(0.0), -1
    n = min(top_n, vocab)
    top_ids = np.full(top_n, -1, dtype=np.int64)
    top_lp = np.full(top_n, NEG_INF, dtype=np.float32)
    top_ids[:n] = order[:n]
    top_lp[:n] = lp[order[:n]]
    return Row(logprob, rank, top_ids, top_lp, z, lz)


def logprob(logits, targets=None, top_n=0, wrong=None, lz_step=0):
    """every row of ``logits`` [rows, vocab] (tensor, float16 array or bits): a list of ``Row``"""
    bits = sample_ref.bits_of(logits)
    assert bits.ndim == 2
    if targets is not None and hasattr(targets, "detach"):
        targets = targets.detach().cpu().tolist()
    return [logprob_row(bits[r], None if targets is None else targets[r], top_n, wrong=wrong, lz_step=lz_step)
            for r in range(bits.shape[0])]


def _f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def assert_matches(got, logits, targets=None, top_n=0):
    """``got`` = (logprob, rank, top_ids, top_logprobs) of ops.logprob (tensors or None) against the reference: rank and top_ids
    exactly; logprob and top_logprobs bitwise the reference's with lz, nextafter(lz, +inf) or nextafter(lz, -inf) -- ONE choice for
    the whole row.  Returns how many rows needed a neighbour."""
    bits = sample_ref.bits_of(logits)
    lp, rk, ti, tl = (None if x is None else x.detach().cpu().numpy() for x in got)
    tg = None if targets is None else (targets.detach().cpu().tolist() if hasattr(targets, "detach") else list(targets))
    assert (ti is None) == (top_n == 0) == (tl is None) and (tg is not None or (lp is None and rk is None))
    moved = 0
    for r in range(bits.shape[0]):
        t = None if tg is None else tg[r]
        for step in (0, 1, -1):
            ref = logprob_row(bits[r], t, top_n, lz_step=step)
            if rk is not None:
                assert int(rk[r]) == ref.rank, f"row {r}: rank {int(rk[r])}, expected {ref.rank}"
            if top_n:
                assert ti[r].tolist() == ref.top_ids.tolist(), f"row {r}: top_ids {ti[r].tolist()}, expected {ref.top_ids.tolist()}"
            ok = (lp is None or _f32_bits(lp[r]) == _f32_bits(ref.logprob)) and \
                 (top_n == 0 or np.array_equal(_f32_bits(tl[r]), _f32_bits(ref.top_logprobs)))
            if ok:
                moved += step != 0
                break
        else:
            ref = logprob_row(bits[r], t, top_n)
            raise AssertionError(f"row {r} (target {t}): logprob {None if lp is None else lp[r]!r} top {None if tl is None else tl[r].tolist()}, "
                                 f"expected {ref.logprob!r} {ref.top_logprobs.tolist()} (lz {ref.lz!r}) or with a float32 neighbour of lz")
    return moved
