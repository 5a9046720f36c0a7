"""Torch-CPU restatement of the sparse mixture-of-experts block (checker side only): float softmax over the router logits, the top_k
largest (the lower index of equal ones), renormalise, ``.half()``; rows grouped by expert in ascending token order; every expert output times its fp16 routing weight, added
into an fp16 zero accumulator in expert order; the residual last.  Written from the block's definition, once with the routing tables
the kernels use (``tables`` / ``combine`` / ``block``) and once without any table (``block_direct``)."""
import torch


def distinct_logits(T, E, seed):
    """fp16 [T, E]: per row a random permutation of E distinct multiples of 1/16 (exact in fp16), at least 1/16 apart, shifted per row"""
    g = torch.Generator().manual_seed(seed)
    step = torch.randint(1, 4, (T, 1), generator=g).float() / 16          # 1/16, 1/8 or 3/16 between neighbours
    shift = torch.randint(-32, 33, (T, 1), generator=g).float() / 16
    vals = torch.arange(E).float()[None, :] * step + shift - step * (E // 2)
    perm = torch.rand((T, E), generator=g).argsort(-1)
    out = torch.gather(vals, 1, perm).half()
    assert (out.float().sort(-1).values.diff(dim=-1) >= 1 / 16).all()
    return out


def planted_logits(T, E, K, seed):
    """(fp16 [T, E], exact-weight row indices): rows on which equal logits decide the routing.  Seven kinds of row, eight of each with
    their own positions (rows 0 .. 55, kind = row % 7 in the order below), then T // 8 exact-weight rows; the rest, at least 64, are
    coarse-grid rows: multiples of 1/8 in [-1/4, 1/4].
      zeros      all +0
      signed     +0 / -0 alternating: they compare equal, so the whole row is one tie
      top, low   all 65504, all -65504
      straddle   K - 1 distinct larger values, then min(3, E - K + 1) equal ones (pairwise non-adjacent where E >= 5), the rest
                 smaller: the top_k boundary cuts through the tie.  (E == K has no boundary: an "inside" row stands in.)
      inside     K >= 2: a tie inside the top K and none at its boundary -- K - 2 distinct larger values, two equal ones, the rest
                 smaller; the order inside topk_ids tells the lower index first from the opposite.  (K == 1: a tie for the maximum.)
      maximum    1/4 twice (non-adjacent where E >= 3) over coarse-grid values up to 1/8: lmax is reached twice
      exact      values from {0, -128, -256} with 1 .. K zeros: two selected logits are equal or at least 128 apart, so every exp is
                 exactly 1 or exactly 0 in float (e^-128 is below the smallest float denormal, flushed or not) and each weight is
                 half(1 / m) on the m tied maxima and 0 on the other selected experts"""
    assert 2 <= E <= 64 and 1 <= K <= E
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    coarse = lambda *shape: ri(-2, 2, *shape).float() / 8

    def spread(n):
        """n ascending positions of 0 .. E - 1 in random places, pairwise non-adjacent where E >= 2 n - 1 has the room"""
        if E >= 2 * n - 1:                                    # n - 1 gaps of at least one other position each
            free = E - n - (n - 1)
            cuts = sorted(ri(0, free, n).tolist())            # extra room before each of the n positions
            pos = [cuts[i] + 2 * i for i in range(n)]
            assert all(b - a >= 2 for a, b in zip(pos, pos[1:])) and pos[-1] < E
            return pos
        return torch.randperm(E, generator=g)[:n].sort().values.tolist()

    def place(tied, n_larger, tie_value=1.0):
        """a row with ``tied`` equal values, ``n_larger`` distinct larger ones and the rest distinct and smaller"""
        row = torch.empty(E)
        tie_pos = spread(tied)
        others = [i for i in torch.randperm(E, generator=g).tolist() if i not in tie_pos]
        row[tie_pos] = tie_value
        for j, i in enumerate(others[:n_larger]):
            row[i] = tie_value + 1 + j
        for j, i in enumerate(others[n_larger:]):
            row[i] = tie_value - 1 - j / 8
        return row

    reps, n_exact = 8, T // 8
    out = coarse(T, E)
    exact_rows = []
    r = 0
    for _ in range(reps):
        out[r] = 0.0
        out[r + 1] = torch.where(torch.arange(E) % 2 == 0, 0.0, -0.0)
        out[r + 2], out[r + 3] = 65504.0, -65504.0
        tied = min(3, E - K + 1)
        out[r + 4] = place(tied, K - 1) if tied >= 2 else place(2, K - 2)
        out[r + 5] = place(2, K - 2) if K >= 2 else place(min(3, E), 0)
        out[r + 6] = coarse(E).clamp(max=0.125)
        out[r + 6][spread(2)] = 0.25
        r += 7
    for _ in range(n_exact):
        m = int(ri(1, K, 1))
        row = -128.0 * ri(1, 2, E).float()
        row[torch.randperm(E, generator=g)[:m]] = 0.0
        out[r] = row
        exact_rows.append(r)
        r += 1
    assert r <= T - 64                                       # at least 64 coarse-grid rows
    h = out.half()
    assert torch.equal(h.float(), out)                       # every planted value is an fp16 value
    assert torch.equal(h[1].view(torch.int16)[:2], torch.tensor([0, -32768], dtype=torch.int16))          # the -0 survived
    ex = h[exact_rows].float()
    assert bool(((ex == 0) | (ex == -128) | (ex == -256)).all()) and bool((((ex == 0).sum(-1) >= 1) & ((ex == 0).sum(-1) <= K)).all())
    assert bool((h[r:].float().abs() <= 0.25).all()) and torch.equal(h[r:].float() * 8, (h[r:].float() * 8).round())
    if E > K:                                                # the straddling rows: value K and value K + 1 of the ordered row are equal
        v = h[4:7 * reps:7].float().sort(-1, descending=True).values
        assert bool((v[:, K - 1] == v[:, K]).all()) and (K == 1 or bool((v[:, :K - 1].diff(dim=-1) < 0).all()))
    return h, exact_rows


def _top_ids(l, top_k, tie):
    """the first top_k of a stable descending sort of float logits: of equal values the lower index comes first (``tie="high"``: the
    mutant in which the higher index does, the same sort on the reversed row)"""
    if tie == "low":
        return torch.sort(l, dim=-1, descending=True, stable=True).indices[:, :top_k]
    assert tie == "high"
    return l.shape[-1] - 1 - torch.sort(l.flip(-1), dim=-1, descending=True, stable=True).indices[:, :top_k]


def route(logits, top_k, tie="low"):
    """(ids int64 [T, top_k], w fp16 [T, top_k]): the top_k largest logits first, of equal logits the LOWER expert index first
    (include/atom_hip.h; torch.topk promises no order among equal values and does not keep this one); softmax in float, gathered at
    those experts, renormalised, rounded to half"""
    ids = _top_ids(logits.float(), top_k, tie)
    w = torch.gather(torch.softmax(logits.float(), dim=-1), 1, ids)
    w = w / w.sum(dim=-1, keepdim=True)
    return ids, w.half()


def route_formula(logits, top_k, tie="low"):
    """the same weights by w_k = exp(l_k - l_max) / sum_{j selected} exp(l_j - l_max) in float: the full softmax's denominator cancels"""
    l = logits.float()
    ids = _top_ids(l, top_k, tie)
    top = torch.gather(l, 1, ids)
    ex = torch.exp(top - top[:, :1])
    return ids, (ex / ex.sum(dim=-1, keepdim=True)).half()


def tables_from_counts(counts):
    """(expert_indptr, tile_expert, tile_row0) for the given rows per expert: one tile per started 64 rows, experts in order"""
    indptr = [0]
    for c in counts:
        indptr.append(indptr[-1] + int(c))
    te, tr = [], []
    for e, c in enumerate(counts):
        for r0 in range(0, int(c), 64):
            te.append(e)
            tr.append(indptr[e] + r0)
    return indptr, te, tr


def tables(ids, E):
    """dict of python lists from ids [T, top_k]: expert_indptr [E + 1], row_token [R] (grouped by expert, ascending token),
    slot_row [T][top_k], tile_expert, tile_row0"""
    T, K = ids.shape
    row_token, slot_row, counts = [], [[-1] * K for _ in range(T)], []
    ids = ids.tolist()
    for e in range(E):
        n = 0
        for t in range(T):
            for k in range(K):
                if ids[t][k] == e:
                    slot_row[t][k] = len(row_token)
                    row_token.append(t)
                    n += 1
        counts.append(n)
    indptr, te, tr = tables_from_counts(counts)
    return dict(expert_indptr=indptr, row_token=row_token, slot_row=slot_row, tile_expert=te, tile_row0=tr, n_tiles=len(te))


def hmul(a, b):
    return (a.float() * b.float()).half()


def hadd(a, b):
    return (a.float() + b.float()).half()


def combine(y, ids, w, slot_row, residual=None):
    """y fp16 [R, H] -> fp16 [T, H]: experts in ascending order, each adds half(y[row] * w) of its tokens into the fp16 accumulator"""
    T, K = ids.shape
    acc = torch.zeros((T, y.shape[1]), dtype=torch.float16)
    sr = torch.as_tensor(slot_row, dtype=torch.int64)
    for e in range(int(ids.max()) + 1):
        t, k = torch.nonzero(ids == e, as_tuple=True)
        if t.numel():
            acc[t] = hadd(acc[t], hmul(y[sr[t, k]], w[t, k][:, None]))
    return acc if residual is None else hadd(residual, acc)


def block(x, logits, top_k, E, expert_fn, residual=None):
    """the block through the tables: per expert its rows (ascending token), expert_fn(e, rows) fp16, then ``combine``"""
    ids, w = route(logits, top_k)
    tb = tables(ids, E)
    rt = torch.as_tensor(tb["row_token"], dtype=torch.int64)
    y = torch.empty((rt.numel(), x.shape[1]), dtype=torch.float16)
    for e in range(E):
        lo, hi = tb["expert_indptr"][e], tb["expert_indptr"][e + 1]
        if hi > lo:
            y[lo:hi] = expert_fn(e, x[rt[lo:hi]])
    return combine(y, ids, w, tb["slot_row"], residual)


def block_direct(x, logits, top_k, E, expert_fn, residual=None):
    """the block token by token, no tables: a token's experts in ascending id, out = residual + sum half(expert(x_t) * w)"""
    ids, w = route(logits, top_k)
    out = torch.zeros_like(x)
    for t in range(x.shape[0]):
        acc = torch.zeros(x.shape[1], dtype=torch.float16)
        for e, k in sorted((int(ids[t, k]), k) for k in range(top_k)):
            acc = hadd(acc, hmul(expert_fn(e, x[t:t + 1])[0], w[t, k]))
        out[t] = acc if residual is None else hadd(residual[t], acc)
    return out
