"""The GPU beam search's reformulation (ctc_beam.hip), restated in numpy float32 and checked on the CPU against the
host decoder sl_host_ctc_beam_search (TensorFlow's sequential CTCBeamSearchDecoder + the KenLM-style scorer):
  * the kernel's per-frame procedure: rank sort of the slots, the first loop from the parents' old probabilities, the
    child loop that only walks children above the running bottom (or children that are branches of the frame), stops
    at the first branch at or below the bottom, evicts the first minimum in slot order, and canonical prefix ids from
    a (parent, label) map;
  * the flat scorer tables of sl_host_scorer_export (trie, n-gram hash table) against the host model and trie."""
import math
from pathlib import Path

import numpy as np
import pytest

TOY = Path(__file__).resolve().parent / "golden" / "toy_kenlm"
ALPHABET = list("acehost ")
f32 = np.float32
NEG = f32(-np.inf)


def softmax_rows(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- flat scorer tables
M32 = 0xFFFFFFFF


def ngram_hash(w6):
    h = 0x811C9DC5
    for w in w6:
        h = ((h ^ int(w)) * 0x01000193) & M32
        h ^= h >> 15
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


class FlatLm:
    """The device's view of the scorer: sl_host_scorer_export's arrays, queried as ctc_beam.hip queries them."""

    def __init__(self, tables):
        self.t = tables
        self.order = tables["order"]
        self.oov, self.lm_weight, self.wcw, self.vwcw = (f32(v) for v in tables["params"])
        self.bos, self.eos, self.space = (int(v) for v in tables["ids"])
        self.slots = tables["ngrams"].shape[0]

    def find(self, ids):
        n = len(ids)
        w6 = [0] * (6 - n) + [int(i) for i in ids]
        w6[0] |= n << 29
        i = ngram_hash(w6) & (self.slots - 1)
        while True:
            e = self.t["ngrams"][i]
            if e[0] == 0:
                return None
            if list(map(int, e[:6])) == w6:
                return e[6:8].view(np.float32)
            i = (i + 1) & (self.slots - 1)

    def score(self, hist, word):
        ctx = list(hist[max(0, len(hist) - (self.order - 1)):]) if self.order > 1 else []
        backoff = f32(0)
        while True:
            hit = self.find(ctx + [word])
            if hit is not None:
                return f32(backoff + hit[0])
            if not ctx:
                return f32(backoff + self.oov)
            bo = self.find(ctx)
            if bo is not None:
                backoff = f32(backoff + bo[1])
            ctx = ctx[1:]

    def advance(self, hist, word):
        out = list(hist) + [word]
        return out[max(0, len(out) - (self.order - 1)):] if self.order > 1 else []

    def word(self, node):
        return int(self.t["trie_word"][node]) if node >= 0 else 0

    def child(self, node, label):
        return int(self.t["trie_child"][node, label]) if node >= 0 else -1

    def min_unigram(self, node, label):
        return f32(self.t["trie_min"][node, label]) if node >= 0 else self.oov


# ---------------------------------------------------------------------------------------------- the kernel, restated
def lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    hi, lo = (a, b) if a > b else (b, a)
    return f32(hi + f32(math.log1p(float(f32(math.exp(float(f32(lo - hi))))))))


def normalise(p, eps):
    x = [f32(math.log(float(v))) if v > 0 else NEG for v in (p.astype(np.float32) + f32(eps))]
    mx = NEG
    for v in x:
        mx = v if mx < v else mx
    s = f32(0)
    for v in x:
        s = f32(s + f32(math.exp(float(f32(v - mx)))))
    norm = f32(mx + f32(math.log(float(s))))
    return [f32(v - norm) for v in x]


class Entry:
    __slots__ = ("node", "pnode", "label", "nt", "nb", "nl", "lm", "score", "delta", "trie", "hist", "cache")


def fill_cache(e, lm, n_labels):
    e.cache = [None] * n_labels
    for m in range(n_labels):
        if m == lm.space:
            w = lm.word(e.trie)
            v = e.lm
            if w != 0:
                v = f32(v + lm.vwcw)
            v = f32(v + lm.wcw)
            e.cache[m] = f32(v + lm.score(e.hist, w))
        else:
            e.cache[m] = f32(lm.min_unigram(e.trie, m) + e.lm)


def batched_beam_search(probs, beam_width, merge, lm=None, eps=1e-8, stats=None):
    """One utterance, (T, k) probabilities; blank = k - 1.  Returns (labels, log_prob).  stats: a dict whose "returns" counts
    the new beam entries that the map already knew (prefixes that had left the beam)."""
    t_len, k = probs.shape
    blank, n_labels = k - 1, k - 1
    arena = [-1]
    ids = {}  # (parent node, label) -> node: the kernel's per-utterance hash map
    root = Entry()
    root.node, root.pnode, root.label = 0, -1, -1
    root.nt, root.nb, root.nl = f32(0), f32(0), NEG
    root.lm = root.score = root.delta = f32(0)
    root.trie, root.hist = 0, [lm.bos] if lm else []
    if lm:
        fill_cache(root, lm, n_labels)
    slots = [root]
    for t in range(t_len):
        inp = normalise(probs[t], eps)
        n = len(slots)
        tot = [e.nt for e in slots]
        rank = [sum(1 for q in range(n) if tot[q] > tot[s] or (tot[q] == tot[s] and q < s)) for s in range(n)]
        br = [None] * n
        for s in range(n):
            br[rank[s]] = slots[s]
        ot, ob, onl = [e.nt for e in br], [e.nb for e in br], [e.nl for e in br]
        pos = {e.node: p for p, e in enumerate(br)}
        ppos = [pos.get(e.pnode, -1) if e.pnode >= 0 else -1 for e in br]

        def first(p, active):
            e = br[p]
            nl = onl[p]
            if e.pnode >= 0:
                q = ppos[p]
                if active(p, q):
                    prev = ob[q] if merge and e.label == br[q].label else ot[q]
                    nl = lse(nl, f32(f32(lm.lm_weight * e.delta) + prev) if lm else prev)
                nl = f32(nl + inp[e.label])
            nb = f32(ot[p] + inp[blank])
            e.nl, e.nb, e.nt = nl, nb, lse(nb, nl)

        for p in range(n):  # every branch from the parents' OLD totals
            first(p, lambda p, q: q >= 0 and ot[q] != NEG)
        if any(q >= 0 and q < p and ((br[q].nt == NEG) != (ot[q] == NEG)) for p, q in enumerate(ppos)):
            for p in range(n):  # the host's order (only with -inf inputs)
                first(p, lambda p, q: q >= 0 and (br[q].nt if q < p else ot[q]) != NEG)
        cbt = {(ppos[j], br[j].label): j for j in range(n) if ppos[j] >= 0}
        slot_src = list(range(n))
        slot_tot = [e.nt for e in br]
        bslot = list(range(n))
        reset = [False] * n
        size = n

        def bottom():
            s = min(range(size), key=lambda s: (slot_tot[s], s))
            return s, slot_tot[s]

        full = size == beam_width
        bs, bv = bottom() if full else (0, NEG)
        for i in range(n):
            if reset[i] or not ot[i] > NEG:
                continue
            if full and not ot[i] > bv:
                break
            e = br[i]
            cv, cj = {}, {}
            for ind in range(k):
                if ind == blank:
                    continue
                prev = ob[i] if merge and ind == e.label else ot[i]
                x = f32(f32(lm.lm_weight * f32(e.cache[ind] - e.score)) + prev) if lm else prev
                cv[ind] = f32(inp[ind] + x)
                cj[ind] = cbt.get((i, ind), -1)
            for ind in [ind for ind in cv if cj[ind] >= 0 or not full or cv[ind] > bv]:
                j, v = cj[ind], cv[ind]
                if j >= 0 and bslot[j] >= 0 and slot_tot[bslot[j]] != NEG:
                    continue
                if v > NEG and (size < beam_width or v > bv):
                    if size == beam_width:
                        s = bs
                        if slot_src[s] >= 0:
                            bslot[slot_src[s]] = -1
                    else:
                        s = size
                        size += 1
                        slot_src.append(None)
                        slot_tot.append(None)
                    slot_src[s] = -1 - (i * 64 + ind)
                    slot_tot[s] = v
                    full = size == beam_width
                    if full:
                        bs, bv = bottom()
                elif j >= 0:
                    reset[j] = True
        new_slots = []
        for s in range(size):
            src = slot_src[s]
            if src >= 0:
                new_slots.append(br[src])
                continue
            i, ind = divmod(-1 - src, 64)
            par = br[i]
            c = Entry()
            key = (par.node, ind)
            if stats is not None:
                stats["returns"] += key in ids
            if key not in ids:
                ids[key] = len(arena)
                arena.append(key)
            c.node, c.pnode, c.label = ids[key], par.node, ind
            c.nt = c.nl = slot_tot[s]
            c.nb = NEG
            if lm:
                if ind == lm.space:
                    c.hist = lm.advance(par.hist, lm.word(par.trie))
                    c.lm = c.score = par.cache[ind]
                    c.trie = 0
                else:
                    c.hist, c.lm, c.score = par.hist, par.lm, par.cache[ind]
                    c.trie = lm.child(par.trie, ind)
                c.delta = f32(c.score - par.score)
                fill_cache(c, lm, n_labels)
            new_slots.append(c)
        slots = new_slots
    best, best_total = None, None
    for e in slots:
        total = e.nt
        if lm:
            d, hist = f32(0), e.hist
            if e.trie != 0:
                w = lm.word(e.trie)
                d = f32(d + lm.score(hist, w))
                hist = lm.advance(hist, w)
            d = f32(d + lm.score(hist, lm.eos))
            total = f32(total + f32(lm.lm_weight * f32(f32(e.lm + d) - e.score)))
        if best is None or total > best_total:
            best, best_total = e, total
    labels, prev, node = [], -1, best.node
    while node > 0:
        pnode, lab = arena[node]
        if not merge or lab != prev:
            labels.append(lab)
        prev, node = lab, pnode
    return labels[::-1], float(best_total)


# ---------------------------------------------------------------------------------------------- tests
def host_decoder(alphabet, lm, **kw):
    from speechless_amd.decoder import CtcBeamSearchDecoder
    return CtcBeamSearchDecoder(alphabet, lm, threads=4, **kw)


def flat_lm(decoder):
    from speechless_amd.decoder import export_scorer_tables
    return FlatLm(export_scorer_tables(decoder._scorer))


def check(alphabet, lm, probs_batch, lengths, beam_width, merge, weights=(.8, 0., 2.3)):
    dec = host_decoder(alphabet, lm, beam_width=beam_width, merge_repeated=merge, kenlm_weight=weights[0],
                       word_count_weight=weights[1], valid_word_count_weight=weights[2])
    flat = flat_lm(dec) if lm is not None else None
    want, want_lp = dec.decode(probs_batch, lengths)
    for b in range(len(lengths)):
        got, got_lp = batched_beam_search(probs_batch[b, :lengths[b]], beam_width, merge, flat)
        assert got == want[b], (b, got, want[b])
        assert abs(got_lp - float(want_lp[b])) <= 1e-4 * max(1.0, abs(float(want_lp[b]))), (b, got_lp, want_lp[b])


@pytest.fixture(scope="module")
def toy_lm():
    from speechless_amd.decoder import NGramLanguageModel
    return NGramLanguageModel(TOY / "lm.arpa")


@pytest.fixture(scope="module")
def generated_lm(tmp_path_factory):
    from speechless_amd.decoder import NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    path = tmp_path_factory.mktemp("lm") / "lm.arpa"
    write_synthetic_arpa(path, ALPHABET, 300, order=4, seed=3)
    lm = NGramLanguageModel(path)
    lm.arpa_path = path
    return lm


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("beam_width", [1, 8, 100, 128])
def test_restatement_plain(beam_width, merge):
    rng = np.random.RandomState(beam_width + merge)
    probs = softmax_rows(rng.randn(3, 14, len(ALPHABET) + 1) * 2.0)
    check(ALPHABET, None, probs, [14, 9, 1], beam_width, merge)


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("beam_width", [1, 8, 100, 128])
def test_restatement_toy_lm(toy_lm, beam_width, merge):
    rng = np.random.RandomState(7 * beam_width + merge)
    probs = softmax_rows(rng.randn(2, 14, len(ALPHABET) + 1) * 2.5)
    for weights in ((.8, 0., 2.3), (1.5, 1.0, 0.0)):
        check(ALPHABET, toy_lm, probs, [14, 6], beam_width, merge, weights)


@pytest.mark.parametrize("beam_width", [8, 100])
def test_restatement_generated_lm(generated_lm, beam_width):
    rng = np.random.RandomState(beam_width)
    probs = softmax_rows(rng.randn(2, 12, len(ALPHABET) + 1) * 2.5)
    check(ALPHABET, generated_lm, probs, [12, 12], beam_width, False)


def test_restatement_uniform_frames_and_empty_input(toy_lm):
    probs = np.full((2, 8, len(ALPHABET) + 1), 1.0 / (len(ALPHABET) + 1), dtype=np.float32)
    for lm in (None, toy_lm):
        for beam_width in (1, 8):
            check(ALPHABET, lm, probs, [8, 0], beam_width, False)


def test_flat_ngram_table_scores_as_the_host_model(generated_lm, toy_lm):
    """Sentence scores (sl_host_lm_score_sentence = sum of NGramModel::score) from the flat table: vocabulary words,
    out-of-vocabulary words, back-off chains of every length."""
    from speechless_amd.synthetic_lm import synthetic_words
    for lm, words in ((toy_lm, ["the", "cat", "sat", "a", "at", "cot"]),
                      (generated_lm, synthetic_words(ALPHABET, 300, 3))):
        flat = flat_lm(host_decoder(ALPHABET, lm))
        vocab_id = {}
        rng = np.random.RandomState(1)
        for _ in range(60):
            sentence = [words[rng.randint(len(words))] if rng.rand() < 0.85 else "zz" for _ in range(rng.randint(0, 7))]
            hist, total = [flat.bos], 0.0
            for w in sentence:
                wid = vocab_id.setdefault(w, word_id(flat, w))
                total += float(flat.score(hist, wid))
                hist = flat.advance(hist, wid)
            total += float(flat.score(hist, flat.eos))
            assert abs(total - lm.score(" ".join(sentence))) < 1e-9 * max(1.0, abs(total)), sentence


def word_id(flat, word):
    node = 0
    for ch in word:
        if ch not in ALPHABET[:-1]:
            return 0
        node = flat.child(node, ALPHABET.index(ch))
    return flat.word(node)


def test_flat_trie_answers_as_the_host_trie(generated_lm):
    """min_unigram of every prefix of every vocabulary word and of random strings: the minimum unigram of the words
    under the prefix (the host's trie), or the <unk> unigram once the prefix is off the trie."""
    from speechless_amd.synthetic_lm import synthetic_words
    flat = flat_lm(host_decoder(ALPHABET, generated_lm))
    words = synthetic_words(ALPHABET, 300, 3)
    unigram = {}
    for line in open(generated_lm.arpa_path, encoding="utf8"):
        parts = line.split()
        if len(parts) >= 2 and parts[1] in words and len(parts) == 3 and parts[1] not in unigram:
            unigram[parts[1]] = f32(float(parts[0]))
    rng = np.random.RandomState(0)
    probes = [w[:i] for w in words for i in range(1, len(w) + 1)]
    probes += ["".join(rng.choice(ALPHABET[:-1], size=rng.randint(1, 6))) for _ in range(300)]
    for p in probes:
        under = [unigram[w] for w in words if w.startswith(p)]
        node, score = 0, None
        for ch in p:
            score = flat.min_unigram(node, ALPHABET.index(ch))
            node = flat.child(node, ALPHABET.index(ch))
        want = min(under) if under else flat.oov
        assert score == want, (p, score, want)
        assert (node >= 0) == bool(under), p  # off the trie exactly when no word continues the prefix
        assert (flat.word(node) != 0) == (p in words), p


def test_export_rejects_duplicate_characters(toy_lm):
    from speechless_amd.decoder import export_scorer_tables
    dec = host_decoder(list("acehost") + [" "], toy_lm)
    export_scorer_tables(dec._scorer)
    dup = host_decoder(list("aacehost "), toy_lm)
    with pytest.raises(ValueError):
        export_scorer_tables(dup._scorer)
