"""Host restatement of speculative decoding's integer rules (include/atom_hip.h; atom_amd/csrc/spec_math.h): the n-gram
drafter in two forms -- the rule as the header words it, and the one-maximum form the kernel computes, function for function -- the
accept / commit step, the page-table step with per-sequence counts, and a host speculative loop over any ``next_token(history)``.
numpy and plain Python only."""
import numpy as np

KV_STEP_OVERFLOW, KV_STEP_BAD_LENGTH = 1, 2


# ------------------------------------------------------------------------------------------------ the drafter
def draft_rule(hist, length, K, ngram_max, ngram_min, hist_cap=None):
    """the rule of atom_spec_draft_ngram, step by step: K drafts of one row (a list)"""
    hist_cap = len(hist) if hist_cap is None else hist_cap
    if length <= 0 or length > hist_cap:
        return [0] * K
    h = [int(t) for t in hist[:length]]
    for n in range(ngram_max, ngram_min - 1, -1):           # 1. n from ngram_max down, skipping len <= n
        if length <= n:
            continue
        starts = [s for s in range(0, length - n) if h[s:s + n] == h[length - n:]]     # 2. 0 <= s, s + n <= len - 1
        if starts:
            s = max(starts)                                  # 3. the most recent; 4. the first n with a match wins
            return [h[s + n + j] if s + n + j < length else h[-1] for j in range(K)]   # 5.
    return [h[-1]] * K                                       # 6.


def clamp_len(length, hist_cap):
    return 0 if (length <= 0 or length > hist_cap) else length


def match_len(hist, suffix, e, nmax):
    lim = min(nmax, e + 1)
    m = 0
    while m < lim and hist[e - m] == suffix[m]:
        m += 1
    return m


def draft_word(m, e, ngram_min):
    return (m << 32) | e if m >= ngram_min else 0


def draft_token(hist, length, w, j):
    if w == 0:
        return hist[length - 1]
    at = (w & 0xFFFFFFFF) + 1 + j
    return hist[at] if at < length else hist[length - 1]


def draft_words(hist, length, K, ngram_max, ngram_min, hist_cap=None):
    """the kernel's form (spec_math.h): the maximum of word(match length, end) over the ends 0 .. len - 2"""
    hist_cap = len(hist) if hist_cap is None else hist_cap
    length = clamp_len(length, hist_cap)
    if length == 0:
        return [0] * K
    h = [int(t) for t in hist[:length]]
    suffix = [h[length - 1 - t] if t < length else 0 for t in range(8)]
    best = 0
    for e in range(length - 1):
        if h[e] == suffix[0]:
            best = max(best, draft_word(match_len(h, suffix, e, ngram_max), e, ngram_min))
    return [draft_token(h, length, best, j) for j in range(K)]


def draft(hist, hist_len, K, ngram_max, ngram_min):
    """a batch: hist [batch, hist_cap], hist_len [batch] -> int64 [batch, K]"""
    hist = np.asarray(hist)
    return np.array([draft_rule(row.tolist(), int(n), K, ngram_max, ngram_min, hist.shape[1]) for row, n in zip(hist, hist_len)],
                    dtype=np.int64).reshape(len(hist), K)


# ------------------------------------------------------------------------------------------------ accept / commit
def accept_count(drafts, targets, K):
    a = 0
    while a < K and int(drafts[a]) == int(targets[a]):
        a += 1
    return a


def emit_count(a, budget, n_out):
    return max(min(a + 1, int(budget) - int(n_out)), 0)


def accept(targets, input_ids, n_out, budget, tokens, hist, hist_len, adds, draw, accepted, steps):
    """atom_spec_accept on copies: returns a dict of every output buffer and ``done``"""
    targets = np.asarray(targets)
    o = dict(input_ids=np.array(input_ids), n_out=np.array(n_out), tokens=np.array(tokens), hist=np.array(hist),
             hist_len=np.array(hist_len), adds=np.array(adds), draw=np.array(draw), accepted=np.array(accepted), steps=np.array(steps))
    batch, Q = targets.shape
    K, max_new, hist_cap = Q - 1, o["tokens"].shape[1], o["hist"].shape[1]
    done = 1
    for b in range(batch):
        no, hl = int(o["n_out"][b]), int(o["hist_len"][b])
        e = emit_count(accept_count(o["input_ids"][b, 1:], targets[b], K), budget[b], no)
        for i in range(e):
            if 0 <= no + i < max_new:
                o["tokens"][b, no + i] = targets[b, i]
            if 0 <= hl + i < hist_cap:
                o["hist"][b, hl + i] = targets[b, i]
        o["adds"][b] = e
        if e > 0:
            o["n_out"][b] = no + e
            o["hist_len"][b] = hl + e
            o["input_ids"][b, 0] = targets[b, e - 1]
            o["draw"][b] = no + e
            o["accepted"][b] += e - 1
            o["steps"][b] += 1
        done &= int(no + e >= int(budget[b]))
    o["done"] = np.array([done], dtype=np.int32)
    return o


# ------------------------------------------------------------------------------------------------ the page-table step
class StepRows:
    """atom_kv_step_rows_i4 on the host: committed lengths, and after every ``step`` the lengths the tables cover (``tab``), ``indptr``
    and ``last_page_offset``; ``status`` collects the bits"""

    def __init__(self, lens, row_pages, page_size):
        self.lens, self.row_pages, self.P, self.status = [int(n) for n in lens], [int(r) for r in row_pages], int(page_size), 0
        self.tab = list(self.lens)

    def step(self, adds, lookahead):
        tab = []
        for b, (n, add) in enumerate(zip(self.lens, adds)):
            maxlen, add = self.row_pages[b] * self.P, int(add)
            if add < 0:
                add, self.status = 0, self.status | KV_STEP_BAD_LENGTH
            if add + lookahead > maxlen - n:
                self.status |= KV_STEP_OVERFLOW
                tab.append(n)
            else:
                self.lens[b] = n + add
                tab.append(n + add + lookahead)
        self.tab = tab
        return self

    @property
    def indptr(self):
        return [0] + np.cumsum([-(-n // self.P) for n in self.tab]).tolist()

    @property
    def last_page_offset(self):
        return [(n - 1) % self.P + 1 if n > 0 else 0 for n in self.tab]


# ------------------------------------------------------------------------------------------------ the loop
def plain_loop(next_token, prompt, budget):
    """one token per step: ``budget`` new tokens"""
    h = list(prompt)
    for _ in range(budget):
        h.append(next_token(h))
    return h[len(prompt):]


def spec_loop(next_token, prompt, budget, K, propose):
    """speculative decoding of one sequence over ``next_token(history)``: the first token comes from the prompt alone, then every step
    verifies ``propose(history, n_out)`` (K drafts).  Returns (new tokens, accepted, steps, accept counts per step)."""
    h = list(prompt)
    h.append(next_token(h))
    n_out, accepted, steps, counts = 1, 0, 0, []
    while n_out < budget:
        drafts = [int(t) for t in propose(h, n_out)]
        assert len(drafts) == K
        targets = [next_token(h + drafts[:j]) for j in range(K + 1)]        # the verify forward: row j sees the last token and j drafts
        a = accept_count(drafts, targets, K)
        e = emit_count(a, budget, n_out)
        h += targets[:e]
        n_out, accepted, steps = n_out + e, accepted + e - 1, steps + 1
        counts.append(a)
    return h[len(prompt):], accepted, steps, counts
