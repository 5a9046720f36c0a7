"""Torch-CPU restatement of the sparse mixture-of-experts block (checker side only): float softmax over the router logits, topk,
renormalise, ``.half()``; rows grouped by expert in ascending token order; every expert output times its fp16 routing weight, added
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


def route(logits, top_k):
    """(ids int64 [T, top_k], w fp16 [T, top_k]): softmax in float, the top_k largest first, renormalised, rounded to half"""
    p = torch.softmax(logits.float(), dim=-1)
    w, ids = torch.topk(p, top_k, dim=-1)
    w = w / w.sum(dim=-1, keepdim=True)
    return ids, w.half()


def route_formula(logits, top_k):
    """the same weights by w_k = exp(l_k - l_max) / sum_{j selected} exp(l_j - l_max) in float: the full softmax's denominator cancels"""
    l = logits.float()
    top, ids = torch.topk(l, top_k, dim=-1)
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
    for e in range(E):
        n = 0
        for t in range(T):
            for k in range(K):
                if int(ids[t, k]) == e:
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
