"""The checker's restatement of atom_sample_f16 (include/atom_hip.h), independent of the kernel's sources: a stable
sort, NumPy float32 for the weight function (one IEEE rounding per operation), uint64 cumulative sums (a row's weights sum below
2^59), Python ints for the 96-bit products, Philox4x32-10 in plain integers.  ``wrong=`` swaps ONE rule for the obvious wrong one, for
the tests that show a planted family tells the two apart."""
import numpy as np

M32 = 0xFFFFFFFF
C = [np.float32(float.fromhex(h)) for h in ("0x1.0p+0", "0x1.62e572p-1", "0x1.ebca2ap-3", "0x1.c9bda2p-5", "0x1.24f70ap-7", "0x1.f099a6p-10")]
LOG2E = np.float32(float.fromhex("0x1.715476p+0"))
WRONG = ("tie_high", "ge_target", "p_before_k", "p_full_z")


def philox4x32_10(counter, key):
    c, k = [int(x) & M32 for x in counter], [int(x) & M32 for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def draw_word(seed, step):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10([step & M32, step >> 32, 0, 0], [seed & M32, seed >> 32])[0]


def bits_of(logits):
    """uint16 array of the fp16 bits: a torch half tensor, a NumPy float16 array or the bits themselves"""
    if hasattr(logits, "detach"):
        import torch
        logits = logits.detach().cpu().contiguous().view(torch.int16).numpy()
    a = np.asarray(logits)
    if a.dtype == np.float16:
        a = a.view(np.uint16)
    return a.astype(np.uint16)


def canonical(bits):
    """step 1: float32 logits, NaN -> -inf, +inf -> 65504, -0 -> +0"""
    l = np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    l = np.where(np.isnan(l), np.float32(-np.inf), l)
    l = np.where(l == np.float32(np.inf), np.float32(65504.0), l)
    return (l + np.float32(0.0)).astype(np.float32)          # -0 + 0 = +0


def clamp_temperature(T):
    """None for a greedy row, else the clamped float32 temperature"""
    T = np.float32(T)
    if not T > 0:
        return None
    return min(max(T, np.float32(2.0 ** -10)), np.float32(2.0 ** 10))


def weights(l, T):
    """step 4: uint64 weights, 2^40 fixed point, of canonical logits under a clamped temperature"""
    with np.errstate(all="ignore"):
        m = l.max()
        r = np.float32(1.0) / np.float32(T)
        x = ((l - m) * r) * LOG2E
        live = x >= np.float32(-40.0)
        xs = np.where(live, x, np.float32(0.0)).astype(np.float32)
        n = np.floor(xs)
        f = xs - n
        q = C[5] * f
        for c in (C[4], C[3], C[2], C[1]):
            q = q + c
            q = q * f
        q = q + C[0]
        assert q.dtype == np.float32 and f.dtype == np.float32
        mant = (q * np.float32(8388608.0)).astype(np.uint64)
        sh = 17 + n.astype(np.int64)
        up, down = np.clip(sh, 0, 63).astype(np.uint64), np.clip(-sh, 0, 63).astype(np.uint64)
        w = np.where(sh >= 0, mant << up, mant >> down)
    return np.where(live, w, np.uint64(0)).astype(np.uint64)


def probabilities(bits, T):
    w = weights(canonical(bits), clamp_temperature(T)).astype(np.float64)
    return w / w.sum()


def top_p_fixed(p):
    p = np.float32(p)
    return int(p * np.float32(4294967296.0)) if p > 0 else 0


def _top_p_cut(cum, p, z):
    """length of the shortest non-empty prefix whose cumulative weight reaches (z * P) >> 32"""
    thr = (int(z) * top_p_fixed(p)) >> 32
    return int(np.searchsorted(cum, np.uint64(thr), side="left")) + 1


def sample_row(bits, T=1.0, k=0, p=1.0, seed=0, step=0, wrong=None, detail=False):
    assert wrong is None or wrong in WRONG
    l = canonical(bits)
    vocab = l.size
    if l.max() == -np.inf:
        return 0
    idx = np.arange(vocab)
    order = np.lexsort((-idx if wrong == "tie_high" else idx, -l))            # l descending, then index
    Tc = clamp_temperature(T)
    if Tc is None:
        return int(order[0])
    w = weights(l, Tc)[order]
    n, p_off = vocab, bool(np.float32(p) >= 1)
    if wrong == "p_before_k" and not p_off:
        cum = np.cumsum(w, dtype=np.uint64)
        n = _top_p_cut(cum, p, cum[-1])
        p_off = True
    if 0 < int(k) < vocab:
        n = min(n, int(k))
    cum = np.cumsum(w[:n], dtype=np.uint64)
    if not p_off:
        z_for_p = int(np.cumsum(w, dtype=np.uint64)[-1]) if wrong == "p_full_z" else int(cum[-1])
        n = min(n, _top_p_cut(cum, p, z_for_p))
        cum = cum[:n]
    z = int(cum[-1])
    target = (z * draw_word(seed, step)) >> 32
    pos = int(np.searchsorted(cum, np.uint64(target), side="left" if wrong == "ge_target" else "right"))
    if detail:
        return int(order[min(pos, n - 1)]), dict(n=n, z=z, target=target, cum=cum, order=order)
    return int(order[min(pos, n - 1)])


def _per_row(x, batch, default):
    if x is None:
        return [default] * batch
    if hasattr(x, "detach"):
        x = x.detach().cpu().tolist()
    if isinstance(x, (list, tuple, np.ndarray)):
        x = list(x)
        assert len(x) == batch
        return x
    return [x] * batch


def sample(logits, temperature=None, top_k=None, top_p=None, seeds=None, step=0, wrong=None):
    """tokens (list of int) of every row of ``logits`` [batch, vocab]; the parameters are scalars, sequences or tensors, None = off"""
    bits = bits_of(logits)
    assert bits.ndim == 2
    b = bits.shape[0]
    T, K, P, S = (_per_row(x, b, d) for x, d in ((temperature, 1.0), (top_k, 0), (top_p, 1.0), (seeds, 0)))
    return [sample_row(bits[i], T[i], K[i], P[i], S[i], step, wrong=wrong) for i in range(b)]
