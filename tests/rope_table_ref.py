"""FP64 reference of the paged INT4 attention ops on their TABLE path (``rope_table=``, ``attn_scale=``: atom_batch_decode_gqa_i4_rope,
atom_batch_prefill_gqa_i4_rope, atom_batch_decode_append_i4_rope), shared by tests/test_rope_table_cpu.py, tests/test_gpu_rope_table.py
and tests/test_gpu_rope_model.py.  numpy only.

The definition is the table itself: pair i (dims i, i + 64) of a vector at position p is rotated by the angle 2 pi * p * table[i], the
table's values (fp32 as the kernels load them, or float64) taken exactly; the logits are <q, k> / sqrt(128) * attn_scale.  Everything
else -- the cache layout, which rows see which keys, grouped-query heads -- is tests/attn_planted.py's, whose builders, queries and
bounds are used by import.  The keys are walked in chunks, so a sequence of 131,072 tokens needs no more memory than one of 8,192."""
import numpy as np

from oracle import atom_oracle as O
from tests import attn_planted as A

D = A.D
TWO_PI = 2.0 * np.pi

LLAMA31 = dict(rope_type="llama3", rope_theta=5e5, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
YARN = dict(rope_type="yarn", rope_theta=1e4, factor=4.0, original_max_position_embeddings=4096)
MUTANTS = ("table_ignored", "rope_scale_on_top", "pair_off_by_one", "attn_scale_ignored", "linear_for_llama3")


def theta_table(theta, rope_scale=1.0):
    """float64 [64]: the theta path's frequencies theta^(-2 i / 128) / rope_scale, in revolutions per position"""
    return theta ** (-np.arange(0, D, 2, dtype=np.float64) / D) / rope_scale / TWO_PI


def table_f32(inv_freq):
    """what ops.rope_table computes: inv_freq (radians per position, float64) / 2 pi, rounded once to fp32"""
    return (np.asarray(inv_freq, dtype=np.float64) / TWO_PI).astype(np.float32)


def config_table(rope_parameters):
    """(fp32 table, attn_scale) of a RoPE-scaling config, through atom_amd.e2e.rope (pure numpy)"""
    from atom_amd.e2e.rope import rope_init
    theta, rope_scale, inv_freq, attention_factor = rope_init(dict(rope_parameters=dict(rope_parameters)))
    assert inv_freq is not None and rope_scale == 1.0
    return table_f32(inv_freq), float(attention_factor) ** 2


def mutant(kind, table, attn_scale, *, theta=5e5, factor=8.0):
    """(table, attn_scale) with ONE deliberate error, as a layer or an op that mishandles the new arguments would compute:
      table_ignored       plain theta frequencies in place of the table
      rope_scale_on_top   the table divided by rope_scale = factor once more
      pair_off_by_one     pair i takes table[i + 1]
      attn_scale_ignored  the logits not scaled
      linear_for_llama3   every pair of plain theta divided by factor (linear scaling)"""
    assert kind in MUTANTS, kind
    t = np.asarray(table, dtype=np.float64)
    if kind == "table_ignored":
        return theta_table(theta), attn_scale
    if kind == "rope_scale_on_top":
        return t / factor, attn_scale
    if kind == "pair_off_by_one":
        return np.concatenate([t[1:], t[-1:]]), attn_scale
    if kind == "attn_scale_ignored":
        return t, 1.0
    return theta_table(theta, factor), attn_scale


def _rotate(x, pos, table):
    """x float64 [..., n, 128] at positions pos [n]: pairs (i, i + 64), angle 2 pi pos table[i]"""
    ang = TWO_PI * np.asarray(pos, dtype=np.float64)[:, None] * np.asarray(table, dtype=np.float64)[None, :]
    c, s = np.cos(ang), np.sin(ang)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)


def ref_prefill(q, c, qo, table, *, G=1, attn_scale=1.0, layer=A.LAYER, seqs=None, chunk=8192):
    """FP64 causal attention over the cache c (a builder's dict of tests/attn_planted.py or aliased_cache): sequence b's queries are
    rows qo[b] .. qo[b + 1] at its last positions, query head h reads K/V head h // G.  q f16 [T, nkv * G, 128] -> float64 of the same
    shape.  ``seqs``: these sequences only (the other rows stay 0)."""
    data, param, indptr, indices, lpo = c["data"], c["param"], c["indptr"], c["indices"], c["lpo"]
    qn = np.asarray(q).astype(np.float64)
    T, Nq, _ = qn.shape
    nkv, P = data.shape[3], data.shape[4]
    assert Nq == nkv * G and len(table) == D // 2
    out = np.zeros((T, Nq, D))
    for b in (range(len(lpo)) if seqs is None else seqs):
        S = O.kv_seq_len(indptr, lpo, P, b)
        r0, r1 = int(qo[b]), int(qo[b + 1])
        n = r1 - r0
        if n == 0 or S <= 0:
            continue
        pos = np.arange(S - n, S)
        pages = np.asarray(indices[int(indptr[b]):int(indptr[b + 1])], dtype=np.int64)
        qf = _rotate(qn[r0:r1].transpose(1, 0, 2), pos, table)                     # [heads, rows, D]
        for hk in range(nkv):
            hs = list(range(hk * G, hk * G + G))
            qh = qf[hs].reshape(G * n, D)
            rpos = np.tile(pos, G)                                                 # position of each (head, row)
            scores = np.full((G * n, S), -np.inf)
            for j0 in range(0, S, chunk):
                j = np.arange(j0, min(j0 + chunk, S))
                kf = O._dequant_u4_rows(data[pages[j // P], layer, 0, hk, j % P], param[pages[j // P], layer, 0, hk, j % P])
                s = qh @ _rotate(kf, j, table).T * (attn_scale / np.sqrt(D))
                scores[:, j0:j0 + len(j)] = np.where(j[None, :] <= rpos[:, None], s, -np.inf)
            pr = np.exp(scores - scores.max(axis=1, keepdims=True))
            pr /= pr.sum(axis=1, keepdims=True)
            o = np.zeros((G * n, D))
            for j0 in range(0, S, chunk):
                j = np.arange(j0, min(j0 + chunk, S))
                vf = O._dequant_u4_rows(data[pages[j // P], layer, 1, hk, j % P], param[pages[j // P], layer, 1, hk, j % P])
                o += pr[:, j0:j0 + len(j)] @ vf
            out[r0:r1, hs] = o.reshape(G, n, D).transpose(1, 0, 2)
    return out


def ref_decode(q, c, table, **kw):
    """one query per sequence at its last position.  q f16 [B, nkv * G, 128]"""
    return ref_prefill(q, c, np.arange(len(c["lpo"]) + 1), table, **kw)


def aliased_cache(S, distinct=64, *, nkv=2, P=16, seed=11):
    """ONE sequence of S tokens whose page list cycles over ``distinct`` needle pages (tests/attn_planted.build_needle): the cache of a
    131,072-token context is half a megabyte, every position still has its own RoPE angle, and the softmax stays peaked."""
    c = A.build_needle([distinct * P], nkv, P, seed)
    npages = -(-S // P)
    own = c["indices"][:distinct]
    c["indices"] = np.tile(own, -(-npages // distinct))[:npages].astype(np.int32)
    c["indptr"] = np.array([0, npages], dtype=np.int32)
    c["lpo"] = np.array([S - (npages - 1) * P], dtype=np.int32)
    c["seqlens"] = [S]
    return c


def merge_partials(part):
    """the ops' un-merged partial states float [rows, heads, splits, 130] (128 un-normalised values, running maximum in base 2,
    denominator) merged in float64: [rows, heads, 128]"""
    p = np.asarray(part, dtype=np.float64)
    o, m, d = p[..., :D], p[..., D], p[..., D + 1]
    M = m.max(axis=-1, keepdims=True)
    w = np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(M), M, 0.0)), 0.0)
    den = (d * w).sum(axis=-1)
    return (o * w[..., None]).sum(axis=-2) / np.where(den > 0, den, 1.0)[..., None]
