"""Host side of the letter / word error counts: the Levenshtein distance the reference takes from the `editdistance` package
(speechless/net.py:31-37), the word rule of sl_edit_distance (include/speechless_hip.h) restated on index lists, and the
packing of index lists for the kernel.  The device side is csrc/edit_distance.hip, reached through Engine.error_counts /
Engine.edit_distance_batch."""
import numpy as np


def edit_distance(a, b):
    """Levenshtein distance between two sequences (the reference uses the `editdistance` package, net.py:31-37)."""
    a, b = list(a), list(b)
    if len(a) < len(b):
        a, b = b, a
    previous = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        current = [i]
        for j, y in enumerate(b, 1):
            current.append(min(previous[j] + 1, current[j - 1] + 1, previous[j - 1] + (x != y)))
        previous = current
    return previous[-1]


def space_index_of(allowed_characters):
    """Position of " " in the alphabet, -1 if it has none: the `space` of sl_edit_distance.  Raises ValueError when the
    alphabet holds another character that str.split() treats as a separator -- the kernel knows one separator only."""
    for character in allowed_characters:
        if character != " " and character.isspace():
            raise ValueError("error_count_device='gpu' splits words at ' ' only, but allowed_characters holds the whitespace "
                             "character {!r}: str.split() would split there, too".format(character))
    return list(allowed_characters).index(" ") if " " in allowed_characters else -1


def word_spans(indices, space_index):
    """(start, length) of every word of an index list: a word is a maximal run of indices != space_index -- what
    str.split() yields for an alphabet whose only whitespace character sits at space_index.  space_index < 0: no
    separator, a non-empty list is one word."""
    spans, start = [], None
    for position, index in enumerate(indices):
        if space_index >= 0 and index == space_index:
            if start is not None:
                spans.append((start, position - start))
                start = None
        elif start is None:
            start = position
    if start is not None:
        spans.append((start, len(indices) - start))
    return spans


def host_counts(expected_rows, predicted_rows, space_index):
    """What sl_edit_distance computes, on the host: (letter errors, word errors) as int32 (B,) arrays."""
    def words(row):
        return [tuple(row[s:s + n]) for s, n in word_spans(row, space_index)]
    letters = [edit_distance(e, p) for e, p in zip(expected_rows, predicted_rows)]
    word_errors = [edit_distance(words(list(e)), words(list(p))) for e, p in zip(expected_rows, predicted_rows)]
    return np.array(letters, dtype=np.int32), np.array(word_errors, dtype=np.int32)


def pack_rows(rows, pad=-1):
    """Index lists as ((B, max(longest, 1)) int32 array padded with `pad`, (B,) int32 lengths)."""
    lengths = np.array([len(r) for r in rows], dtype=np.int32)
    packed = np.full((len(rows), max(int(lengths.max()) if len(rows) else 0, 1)), pad, dtype=np.int32)
    for row, indices in zip(packed, rows):
        row[:len(indices)] = indices
    return packed, lengths
