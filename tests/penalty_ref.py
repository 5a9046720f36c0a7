"""The checker's restatement of atom_penalize_f16 (include/atom_hip.h), independent of the kernel's sources: NumPy
float32 operations (one IEEE rounding each) on the logits' uint16 bits and the state's uint16 words.  ``wrong=`` swaps ONE rule for
the obvious wrong one, for the tests that show a planted family tells the two apart."""
import numpy as np

FLAG, COUNT = 0x8000, 0x7FFF
QNAN = 0x7E00
WRONG = ("mul_positive", "pres_freq_on_prompt", "rep_skips_prompt", "count_after", "round_between", "bias_first", "count_wraps")


def bits_of(x):
    """uint16 array of 16-bit words: a torch half / int16 tensor, a NumPy float16 / int16 array or the words themselves"""
    if hasattr(x, "detach"):
        import torch
        x = x.detach().cpu().contiguous().view(torch.int16).numpy()
    a = np.asarray(x)
    if a.dtype in (np.float16, np.int16):
        a = a.view(np.uint16)
    return a.astype(np.uint16)


def count_up(word, wraps=False):
    word = int(word)
    if wraps:
        return (word + 1) & 0xFFFF
    return word if (word & COUNT) == COUNT else word + 1


def clamp_rep(rep):
    """(on, r): off when not rep > 0, else float32 clamped to [2^-10, 2^10]"""
    rep = np.float32(rep)
    if not rep > 0:
        return False, np.float32(1.0)
    return True, min(max(rep, np.float32(2.0 ** -10)), np.float32(2.0 ** 10))


def to_half_bits(l):
    with np.errstate(all="ignore"):
        h = l.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(l), np.uint16(QNAN), h).astype(np.uint16)


def _add_bias(l, hit):
    """l[i] = l[i] + v for every (i, v), in order (one float32 addition each)"""
    idx = np.array([i for i, _ in hit], dtype=np.int64)
    if len(set(idx.tolist())) == idx.size:
        l[idx] = l[idx] + np.array([v for _, v in hit], dtype=np.float32)
    else:
        for i, v in hit:
            l[i] = l[i] + v


def penalize_row(bits, words=None, fed=None, rep=1.0, pres=0.0, freq=0.0, bias_ids=(), bias_vals=(), wrong=None):
    """one row: (out bits uint16 [vocab], state words uint16 [vocab] after the call, or None without state)"""
    assert wrong is None or wrong in WRONG
    bits = np.asarray(bits, dtype=np.uint16)
    vocab = bits.size
    have_state = words is not None
    words = np.array(words, dtype=np.uint16) if have_state else np.zeros(vocab, dtype=np.uint16)
    assert words.size == vocab and (fed is None or have_state)
    counted = fed is not None and 0 <= int(fed) < vocab
    if counted and wrong != "count_after":
        words[int(fed)] = count_up(words[int(fed)], wraps=wrong == "count_wraps")
    rep_on, r = clamp_rep(rep)
    pres, freq = np.float32(pres), np.float32(freq)
    ids = [int(i) for i in bias_ids]
    neutral = (not rep_on or r == 1) and pres == 0 and freq == 0 and not any(i >= 0 for i in ids)
    if neutral:
        out = bits.copy()
    else:
        with np.errstate(all="ignore"):
            mid = (lambda x: x.astype(np.float16).astype(np.float32)) if wrong == "round_between" else (lambda x: x)
            count = (words & COUNT).astype(np.int64)
            flag = (words >> 15).astype(np.int64)
            seen = words != 0
            biased = np.zeros(vocab, dtype=bool)
            l = bits.view(np.float16).astype(np.float32)
            hit = [(i, np.float32(v)) for i, v in zip(ids, bias_vals) if 0 <= i < vocab]
            biased[[i for i, _ in hit]] = True
            if wrong == "bias_first":
                _add_bias(l, hit)
            if rep_on:
                use = (count > 0) if wrong == "rep_skips_prompt" else seen
                scaled = l * r if wrong == "mul_positive" else np.where(l > 0, l / r, l * r)
                l = mid(np.where(use, scaled, l).astype(np.float32))
            eff = count + flag if wrong == "pres_freq_on_prompt" else count
            t = (freq * eff.astype(np.float32)).astype(np.float32)
            l = mid((l - t).astype(np.float32))
            l = mid(np.where(eff > 0, l - pres, l).astype(np.float32))
            if wrong != "bias_first":
                _add_bias(l, hit)
            assert l.dtype == np.float32
            out = np.where(seen | biased, to_half_bits(l), bits).astype(np.uint16)
    if counted and wrong == "count_after":
        words[int(fed)] = count_up(words[int(fed)])
    return out, (words if have_state else None)


def _per_row(x, batch, default):
    if x is None:
        return [default] * batch
    if hasattr(x, "detach"):
        x = x.detach().cpu().tolist()
    if isinstance(x, (list, tuple, np.ndarray)):
        assert len(x) == batch
        return list(x)
    return [x] * batch


def penalize(logits, state=None, fed=None, rep=None, pres=None, freq=None, bias_ids=None, bias_vals=None, wrong=None):
    """every row of ``logits`` [batch, vocab]: (out uint16 [batch, vocab], state uint16 [batch, vocab] or None).  ``state`` may be wider
    than vocab (its first vocab columns are used); the parameters are scalars, sequences or tensors, None = neutral."""
    bits = bits_of(logits)
    b, vocab = bits.shape
    words = None if state is None else bits_of(state)[:, :vocab]
    F, R, P, Q = (_per_row(x, b, d) for x, d in ((fed, None), (rep, 1.0), (pres, 0.0), (freq, 0.0)))
    if bias_ids is None:
        I, V = [()] * b, [()] * b
    else:
        I = bias_ids.detach().cpu().tolist() if hasattr(bias_ids, "detach") else [list(r) for r in bias_ids]
        V = bias_vals.detach().cpu().tolist() if hasattr(bias_vals, "detach") else [list(r) for r in bias_vals]
    rows = [penalize_row(bits[i], None if words is None else words[i], F[i], R[i], P[i], Q[i], I[i], V[i], wrong=wrong) for i in range(b)]
    out = np.stack([r[0] for r in rows])
    return out, (None if words is None else np.stack([r[1] for r in rows]))
