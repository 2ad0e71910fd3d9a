"""Label codec at the boundary of the hot path (host logic).

Mirrors the interface of the reference's speechless/grapheme_enconding.py (sic): `CtcGraphemeEncoding` with
`encode`, `encode_label_batch`, `decode_graphemes`, `decode_grapheme_batch`, `decode_prediction_batch`
(grapheme_enconding.py:8-61,121-137).  Behaviour pinned by the reference's own tests
(speechless/test/test_grapheme_encoding.py:9-31) via tests/golden/codec_golden.json.

`AsgGraphemeEncoding` has the semantics of the ASG half of the reference file (grapheme_enconding.py:64-118; its known
answers, test/test_grapheme_encoding.py:34-50, are reproduced in tests/test_asg.py): no blank, two extra graphemes that
stand for "the previous letter once more" and "twice more".  The reference's ASG loss raises NotImplementedError
(net.py:396-399), so there no model can use it; here Wav2Letter(criterion="asg") does (csrc/asg.hip).
"""
import numpy as np

english_frequent_characters = list("abcdefghijklmnopqrstuvwxyz '")  # english_corpus.py:19 (28 characters)
german_frequent_characters = english_frequent_characters + list("äöüß")  # german_corpus.py:14 (32 characters)


class CtcGraphemeEncoding:
    def __init__(self, allowed_characters):
        self.allowed_characters = list(allowed_characters)
        self.allowed_character_count = len(self.allowed_characters)
        self.grapheme_set_size = self.allowed_character_count + 1
        self.ctc_blank = self.grapheme_set_size - 1  # blank is the LAST index (tf.nn.ctc_loss convention)
        self.graphemes_by_character = {c: i for i, c in enumerate(self.allowed_characters)}
        # code point -> index table for the vectorised batch encoder (-1 = not allowed)
        self._table = np.full(max(ord(c) for c in self.allowed_characters) + 1, -1, dtype=np.int32)
        for c, i in self.graphemes_by_character.items():
            self._table[ord(c)] = i

    def encode_character(self, label_char):
        index = self.graphemes_by_character.get(label_char)
        if index is None:
            raise ValueError("Unexpected char: '{}'".format(label_char))
        return index

    def encode(self, label):
        return [self.encode_character(c) for c in label]

    def encode_label_batch(self, labels):
        """int32 (B, Lmax), padded with -1 (never read: the CTC op is told the true lengths)."""
        width = max(len(label) for label in labels)
        batch = np.full((len(labels), width), -1, dtype=np.int32)
        for row, label in zip(batch, labels):
            if not label:
                continue
            codes = np.frombuffer(label.encode("utf-32-le"), dtype=np.uint32)  # one table lookup per label, not per char
            known = codes < self._table.size
            indices = self._table[np.where(known, codes, 0)]
            if not known.all() or (indices < 0).any():
                bad = int(np.argmax(~known | (indices < 0)))
                raise ValueError("Unexpected char: '{}'".format(label[bad]))
            row[:len(label)] = indices
        return batch

    def decode_grapheme(self, grapheme, previous_grapheme=None):
        if 0 <= grapheme < self.allowed_character_count:
            return self.allowed_characters[grapheme]
        if grapheme == self.ctc_blank:
            return ""
        raise ValueError("Unexpected grapheme: '{}'".format(grapheme))

    def decode_graphemes(self, graphemes, merge_repeated=True):
        out = []
        previous = None
        for g in graphemes:
            g = int(g)
            if not (merge_repeated and g == previous):
                out.append(self.decode_grapheme(g))
            previous = g
        return "".join(out)

    def decode_grapheme_batch(self, grapheme_batch, prediction_lengths, merge_repeated=True):
        return [self.decode_graphemes(list(grapheme_batch[i])[:int(prediction_lengths[i])],
                                      merge_repeated=merge_repeated)
                for i in range(len(grapheme_batch))]

    def decode_prediction_batch(self, prediction_batch, prediction_lengths):
        """prediction_batch: (B, T', K) probabilities -> greedy strings (argmax, first max wins)."""
        return self.decode_grapheme_batch(np.argmax(prediction_batch, 2), prediction_lengths)


class AsgGraphemeEncoding(CtcGraphemeEncoding):
    """No blank; a letter repeated two / three times in a row is written as the letter followed by `asg_twice` /
    `asg_thrice` (the last two indices), so that no two adjacent graphemes of an encoded label are equal.  Four in a row
    cannot be written: ValueError."""

    def __init__(self, allowed_characters):
        super().__init__(allowed_characters)
        self.grapheme_set_size = self.allowed_character_count + 2
        self.ctc_blank = None  # there is none
        self.asg_twice = self.grapheme_set_size - 2
        self.asg_thrice = self.grapheme_set_size - 1

    def _compress_runs(self, indices):
        """int array of letter indices -> the same with every run of 2 / 3 equal letters as (letter, twice / thrice)"""
        indices = np.asarray(indices, dtype=np.int32)
        if indices.size == 0:
            return indices
        starts = np.concatenate([[0], np.flatnonzero(np.diff(indices)) + 1])
        lengths = np.diff(np.concatenate([starts, [indices.size]]))
        if lengths.max() > 3:
            raise ValueError("{}-fold repetition found, ASG only supports up to 3-fold.".format(int(lengths.max())))
        marks = np.array([-1, -1, self.asg_twice, self.asg_thrice], dtype=np.int32)[lengths]
        pairs = np.stack([indices[starts], marks], axis=1).ravel()
        return pairs[pairs >= 0]

    def encode(self, label):
        return [int(g) for g in self._compress_runs(super().encode(label))]

    def encode_label_batch(self, labels):
        """int32 (B, Lmax) of ENCODED labels, padded with -1: a row's length is its count of entries >= 0."""
        rows = [self._compress_runs(row[:len(label)]) for row, label in zip(super().encode_label_batch(labels), labels)]
        batch = np.full((len(rows), max(len(r) for r in rows)), -1, dtype=np.int32)
        for out, r in zip(batch, rows):
            out[:len(r)] = r
        return batch

    def decode_grapheme(self, grapheme, previous_grapheme=None):
        if 0 <= grapheme < self.allowed_character_count:
            return self.allowed_characters[grapheme]
        if grapheme not in (self.asg_twice, self.asg_thrice):
            raise ValueError("Unexpected grapheme: '{}'".format(grapheme))
        # a repeat mark with no letter in front of it (a net's raw output can hold one) stands for nothing; the reference
        # says so for asg_thrice (grapheme_enconding.py:113-114) and fails with a TypeError / IndexError for asg_twice
        if previous_grapheme is None or not 0 <= previous_grapheme < self.allowed_character_count:
            return ""
        return self.allowed_characters[previous_grapheme] * (1 if grapheme == self.asg_twice else 2)

    def decode_graphemes(self, graphemes, merge_repeated=True):
        out = []
        previous = None
        for g in graphemes:
            g = int(g)
            if merge_repeated and g == previous:
                continue
            out.append(self.decode_grapheme(g, previous_grapheme=previous))
            previous = g
        return "".join(out)
