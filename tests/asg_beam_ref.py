"""The ASG beam search of include/speechless_hip.h (sl_asg_beam_search) restated in numpy float32, prefixes as
tuples (TEST INFRASTRUCTURE ONLY).  Its scorer is restated over the tables export_scorer_tables returns -- trie_child,
trie_min and trie_word read directly, the n-grams from a dict of the non-empty table slots -- so it works on the very
float32 values the device reads, and it calls nothing of the code under test."""
import numpy as np

F = np.float32
NEG_INF = F("-inf")


class TableScorer:
    """expand / expand_end of the CTC decoder's scorer (csrc/beam_shared.h: expand, step_into_child,
    expand_end_delta) in float32, one rounded operation per line.  state = (lm, score, trie node, history tuple, history length)."""

    def __init__(self, tables):
        self.child, self.mu, self.word = tables["trie_child"], tables["trie_min"], tables["trie_word"]
        self.order = int(tables["order"])
        p, ids = tables["params"], tables["ids"]
        self.oov, self.lw, self.wc, self.vwc = F(p[0]), F(p[1]), F(p[2]), F(p[3])
        self.bos, self.eos, self.space = int(ids[0]), int(ids[1]), int(ids[2])
        self.n_nodes = self.word.shape[0]
        rows = tables["ngrams"]
        rows = rows[rows[:, 0] != 0]
        values = rows[:, 6:8].copy().view(np.float32)
        self.grams = {tuple(int(w) for w in r[:6]): (F(v[0]), F(v[1])) for r, v in zip(rows, values)}

    def initial(self):
        return (F(0), F(0), 0, (0, 0, 0, 0, self.bos), 1)

    def _key(self, n, words):
        w = [0] * (6 - len(words)) + list(words)
        w[0] |= n << 29
        return tuple(w)

    def ngram_score(self, hist, hlen, word):
        clen = min(hlen, self.order - 1)
        backoff = F(0)
        while True:
            ctx = list(hist[5 - clen:]) if clen else []
            hit = self.grams.get(self._key(clen + 1, ctx + [word]))
            if hit is not None:
                return F(backoff + hit[0])
            if clen == 0:
                return F(backoff + self.oov)
            hit = self.grams.get(self._key(clen, ctx))
            if hit is not None:
                backoff = F(backoff + hit[1])
            clen -= 1

    def _advance(self, hist, hlen, word):
        return tuple(hist[1:]) + (word,), min(hlen + 1, self.order - 1)

    def _word(self, node):
        return int(self.word[node]) if 0 <= node < self.n_nodes else 0

    def expand(self, state, c):
        """-> (state, delta)"""
        lm, score, node, hist, hlen = state
        if c == self.space:
            word = self._word(node)
            d = self.ngram_score(hist, hlen, word)
            v = lm
            if word != 0:
                v = F(v + self.vwc)
            v = F(v + self.wc)
            new = F(v + d)
            hist, hlen = self._advance(hist, hlen, word)
            return (new, new, 0, hist, hlen), F(new - score)
        inside = 0 <= node < self.n_nodes
        mu = F(self.mu[node, c]) if inside else self.oov
        new = F(mu + lm)
        return (lm, new, int(self.child[node, c]) if inside else -1, hist, hlen), F(new - score)

    def expand_end(self, state):
        """-> delta"""
        lm, score, node, hist, hlen = state
        d = F(0)
        if node != 0:
            word = self._word(node)
            d = F(d + self.ngram_score(hist, hlen, word))
            hist, hlen = self._advance(hist, hlen, word)
        d = F(d + self.ngram_score(hist, hlen, self.eos))
        return F(F(lm + d) - score)


def written_characters(j, last, k):
    """the characters grapheme j writes behind last grapheme `last` (None: absent)"""
    if j < k - 2:
        return [j]
    if last is None or last >= k - 2:
        return []
    return [last] * (1 if j == k - 2 else 2)


class _Terms:
    """per prefix, memoised: for every grapheme j the scorer deltas of the characters it writes behind the prefix's last
    grapheme (d1, d2, their count n) and the state behind them"""

    def __init__(self, scorer, k):
        self.scorer, self.k, self.memo = scorer, k, {}

    def of(self, prefix, state):
        hit = self.memo.get(prefix)
        if hit is None:
            k = self.k
            last = prefix[-1] if prefix else None
            d = np.zeros((2, k), dtype=np.float32)
            n = np.zeros((k,), dtype=np.int32)
            states = []
            for j in range(k):
                st = state
                if j != last:
                    for c in written_characters(j, last, k):
                        st, d[n[j], j] = self.scorer.expand(st, c)
                        n[j] += 1
                states.append(st)
            hit = self.memo[prefix] = (d, n, states)
        return hit


def asg_beam_search(logq, trans, init, length, beam_width, scorer=None):
    """One utterance.  logq (T', K), trans (K, K), init (K,): float32.  Returns (graphemes, score, merges, returns): the
    number of merged candidate pairs (both finite) and of prefixes that entered the beam after having left it.  The K
    candidates of a hypothesis are float32 vectors: every element goes through the definition's operations, each rounded."""
    logq, trans, init = (np.ascontiguousarray(x, dtype=np.float32) for x in (logq, trans, init))
    k = logq.shape[1]
    T = max(0, min(int(length), logq.shape[0]))
    terms = _Terms(scorer, k) if scorer else None
    beam = []  # (prefix, score, state)
    seen, merges, returns = set(), 0, 0
    for t in range(T):
        cands = {}  # prefix -> (score, i, j, state)
        sources = [((), None, scorer.initial() if scorer else None)] if t == 0 else beam
        for i, (prefix, s, state) in enumerate(sources):
            last = prefix[-1] if prefix else None
            if t == 0:
                a = init + logq[0]
            else:
                a = s + trans[last]
                a = a + logq[t]
            states = None
            if scorer:
                d, n, states = terms.of(prefix, state)
                a = np.where(n >= 1, scorer.lw * d[0] + a, a)
                a = np.where(n >= 2, scorer.lw * d[1] + a, a)
            assert a.dtype == np.float32
            for j in range(k):
                new_prefix = prefix if j == last else prefix + (j,)
                other = cands.get(new_prefix)
                if other is not None:
                    if a[j] > NEG_INF and other[0] > NEG_INF:
                        merges += 1
                    if (-other[0], other[1], other[2]) < (-a[j], i, j):
                        continue
                cands[new_prefix] = (a[j], i, j, states[j] if states else None)
        ranked = sorted((v for v in cands.items() if v[1][0] > NEG_INF), key=lambda v: (-v[1][0], v[1][1], v[1][2]))
        old = {p for p, _, _ in beam}
        beam = [(p, a, state) for p, (a, _, _, state) in ranked[:beam_width]]
        for p, _, _ in beam:
            if p not in old and p in seen:
                returns += 1
            seen.add(p)
    best, best_total = None, NEG_INF
    for prefix, a, state in beam:
        total = F(F(scorer.lw * scorer.expand_end(state)) + a) if scorer else a
        if best is None or total > best_total:
            best, best_total = prefix, total
    return (list(best) if best is not None else []), F(best_total), merges, returns


def asg_beam_search_batch(logq, trans, init, lengths, beam_width, scorer=None):
    """-> (list of grapheme lists, scores float32 (B,), total merges, total returning prefixes)"""
    results = [asg_beam_search(logq[b], trans, init, lengths[b], beam_width, scorer) for b in range(len(lengths))]
    return ([r[0] for r in results], np.array([r[1] for r in results], dtype=np.float32),
            sum(r[2] for r in results), sum(r[3] for r in results))
