"""Synthetic ARPA n-gram models for the beam-search tests and tools/beam_time.py: random words over an alphabet, random
log10 probabilities and back-offs, n-grams of every order up to `order` (some with <s>, </s> and <unk>)."""
import numpy as np


def synthetic_words(alphabet, n_words, seed=0, max_len=8):
    letters = [c for c in alphabet if c != " "]
    rng = np.random.RandomState(seed)
    words, seen = [], set()
    while len(words) < n_words:
        w = "".join(rng.choice(letters, size=rng.randint(1, max_len + 1)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words


def write_synthetic_arpa(path, alphabet, n_words, order=3, seed=0, grams_per_order=None):
    """Writes an ARPA model of `order` over n_words random words; returns the word list."""
    rng = np.random.RandomState(seed + 1)
    words = synthetic_words(alphabet, n_words, seed)
    vocab = ["<unk>", "<s>", "</s>"] + words
    sections = {1: [("{:.4f}".format(-99.0 if w == "<s>" else -rng.uniform(1.0, 6.0)), (w,),
                     "{:.4f}".format(-rng.uniform(0.05, 1.0))) for w in vocab]}
    n = grams_per_order or n_words
    for o in range(2, order + 1):
        grams = set()
        while len(grams) < n:
            g = [vocab[1] if rng.rand() < 0.1 else words[rng.randint(len(words))]]
            g += [words[rng.randint(len(words))] for _ in range(o - 2)]
            g.append("</s>" if rng.rand() < 0.05 else words[rng.randint(len(words))])
            grams.add(tuple(g))
        sections[o] = [("{:.4f}".format(-rng.uniform(0.1, 3.0)), g,
                        "{:.4f}".format(-rng.uniform(0.05, 1.0)) if o < order else None) for g in sorted(grams)]
    with open(path, "w", encoding="utf8") as f:
        f.write("\\data\\\n")
        for o in range(1, order + 1):
            f.write("ngram {}={}\n".format(o, len(sections[o])))
        for o in range(1, order + 1):
            f.write("\n\\{}-grams:\n".format(o))
            for p, g, bo in sections[o]:
                f.write("{}\t{}".format(p, " ".join(g)) + ("\t{}\n".format(bo) if bo is not None else "\n"))
        f.write("\n\\end\\\n")
    return words
