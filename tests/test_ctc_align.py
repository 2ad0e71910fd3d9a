"""CTC forced alignment without a GPU: the float32 restatement of sl_ctc_align (include/speechless_hip.h) against brute-force
enumeration of every CTC path, PositionalLabel, and the conversion of a lattice path into character / word frame ranges."""
import itertools

import numpy as np
import pytest


def viterbi(logq, label, t_b, blank, dtype=np.float32):
    """sl_ctc_align for one utterance, restated in numpy: same recursion, tie rule, end-state rule and edge cases; in float32
    (dtype) every step is an exact max and one rounded add, as on the GPU.  logq: (T', K).  Returns (score, path (T',))."""
    logq = np.asarray(logq, dtype=dtype)
    label = [int(c) for c in label]
    n = len(label)
    s_count = 2 * n + 1
    path = np.full((logq.shape[0],), -1, dtype=np.int32)
    reps = sum(1 for i in range(1, n) if label[i] == label[i - 1])
    if t_b == 0:
        return (dtype(0) if n == 0 else dtype(-np.inf)), path
    if t_b < n + reps:
        return dtype(-np.inf), path
    ext = np.full((s_count,), blank, dtype=np.int64)
    ext[1::2] = label
    skip = np.zeros((s_count,), dtype=bool)
    for s in range(3, s_count, 2):
        skip[s] = ext[s] != ext[s - 2]
    minus_inf = dtype(-np.inf)
    d = np.full((s_count,), minus_inf, dtype=dtype)
    d[0] = logq[0, blank]
    if s_count > 1:
        d[1] = logq[0, ext[1]]
    back = np.zeros((t_b, s_count), dtype=np.int8)
    for t in range(1, t_b):
        p1 = np.full((s_count,), minus_inf, dtype=dtype)
        p1[1:] = d[:-1]
        p2 = np.full((s_count,), minus_inf, dtype=dtype)
        p2[2:] = d[:-2]
        p2[~skip] = minus_inf
        best = d.copy()
        bp = np.zeros((s_count,), dtype=np.int8)
        m = p1 > best           # strict: on a tie the earlier candidate (stay) keeps it
        best[m] = p1[m]
        bp[m] = 1
        m = p2 > best
        best[m] = p2[m]
        bp[m] = 2
        d = (best + logq[t, ext]).astype(dtype)
        back[t] = bp
    end = s_count - 2 if s_count >= 2 and d[s_count - 2] > d[s_count - 1] else s_count - 1
    s = end
    for t in range(t_b - 1, -1, -1):
        path[t] = s
        if t > 0:
            s -= int(back[t, s])
    return d[end], path


def collapse(states, label, blank):
    """the label sequence a lattice state path spells (merge repeats of the same state, drop blanks)"""
    out, prev = [], -1
    for s in states:
        if s != prev and s % 2 == 1:
            out.append(label[(s - 1) // 2])
        prev = s
    return out


def path_score64(logq, label, states, blank):
    lq = np.asarray(logq, dtype=np.float64)
    return float(sum(lq[t, blank if s % 2 == 0 else label[(s - 1) // 2]] for t, s in enumerate(states)))


def symbols_to_states(symbols, label, blank):
    """the unique lattice state path of a frame symbol sequence that collapses to label"""
    states, pos, prev = [], -1, blank
    for c in symbols:
        if c == blank:
            states.append(2 * (pos + 1))
        else:
            if not (c == prev and states and states[-1] % 2 == 1):
                pos += 1
            states.append(2 * pos + 1)
        prev = c
    return states


def brute_force(logq, label, t_b, k):
    """every symbol sequence of t_b frames that collapses to label, scored in float64: (best, second best, best states)"""
    blank = k - 1
    lq = np.asarray(logq, dtype=np.float64)
    scores = []
    for seq in itertools.product(range(k), repeat=t_b):
        out, prev = [], None
        for c in seq:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if out == list(label):
            scores.append((sum(lq[t, c] for t, c in enumerate(seq)), seq))
    if not scores:
        return -np.inf, -np.inf, None
    scores.sort(key=lambda x: -x[0])
    second = scores[1][0] if len(scores) > 1 else -np.inf
    return scores[0][0], second, symbols_to_states(scores[0][1], label, blank)


def log_softmax32(x):
    x = np.asarray(x, dtype=np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def test_restatement_matches_brute_force_enumeration():
    rng = np.random.RandomState(0)
    cases = 0
    for k in (2, 3, 4):
        for t_b in range(0, 8 if k < 4 else 7):
            for _ in range(6 if k < 4 else 3):
                n = int(rng.randint(0, 4))
                label = [int(c) for c in rng.randint(0, k - 1, size=n)]
                if rng.rand() < 0.3 and n >= 2:
                    label[1] = label[0]  # a repeat: needs a blank between
                t_pad = t_b + int(rng.randint(0, 3))
                logq = log_softmax32(rng.randn(max(t_pad, 1), k) * rng.choice([0.1, 1.0, 5.0]))
                score, path = viterbi(logq, label, t_b, k - 1)
                best, second, states = brute_force(logq[:t_b], label, t_b, k)
                assert np.all(path[t_b:] == -1)
                if best == -np.inf:
                    assert score == -np.inf and np.all(path == -1), (label, t_b)
                    continue
                if t_b == 0:
                    assert score == 0 and label == []
                    continue
                assert abs(float(score) - best) <= 1e-5 * max(1.0, abs(best)), (label, t_b, score, best)
                assert collapse(path[:t_b], label, k - 1) == label
                if best - second > 1e-4:
                    assert list(path[:t_b]) == states, (label, t_b, list(path[:t_b]), states)
                cases += 1
    assert cases > 40


def test_restatement_edge_cases():
    logq = log_softmax32(np.random.RandomState(1).randn(6, 4))
    # L = 0: every frame blank, the score the blank column's sum
    score, path = viterbi(logq, [], 5, 3)
    assert list(path) == [0, 0, 0, 0, 0, -1] and score == np.float32(np.sum(logq[:5, 3], dtype=np.float32))
    # T = 0: score 0 for the empty label, -inf otherwise
    assert viterbi(logq, [], 0, 3)[0] == 0 and viterbi(logq, [1], 0, 3)[0] == -np.inf
    # repeats need a blank between: [1, 1] in 2 frames is infeasible, in 3 it is blank-separated
    assert viterbi(logq, [1, 1], 2, 3)[0] == -np.inf
    assert list(viterbi(logq, [1, 1], 3, 3)[1][:3]) == [1, 2, 3]


def test_tie_rule_on_constant_rows():
    """Every path scores the same: stay beats s-1 beats s-2, S-1 beats S-2 at the end."""
    logq = np.full((4, 3), np.float32(np.log(1 / 3)), dtype=np.float32)
    _, path = viterbi(logq, [0, 1], 4, 2)
    assert list(path) == [1, 3, 4, 4]


def test_positional_label():
    from speechless_amd import PositionalLabel
    pl = PositionalLabel([("hello", (0.5, 1.25)), ("world", (1.5, 2.0))])
    assert pl.labels == ["hello", "world"] and pl.label == "hello world"
    assert pl.serialize() == "hello|0.5|1.25\nworld|1.5|2.0"
    back = PositionalLabel.deserialize(pl.serialize())
    assert back.labeled_sections == pl.labeled_sections and back.label == pl.label
    samples = PositionalLabel([("a", (8000, 16000))]).convert_range_to_seconds(16000)
    assert samples.labeled_sections == [("a", (0.5, 1.0))]
    assert pl.with_corrected_labels(str.upper).label == "HELLO WORLD"
    with pytest.raises(ValueError, match="Sections must be specified"):
        PositionalLabel([])
    with pytest.raises(ValueError, match="Range must be specified"):
        PositionalLabel([("a", (0, 1)), ("b", None)])


def test_alignment_frame_ranges():
    from speechless_amd import CtcAlignment
    # "ab  c": leading blanks, a one-frame character, a run of two spaces, trailing blanks and frames past T
    label = "ab  c"
    # states: a=1 b=3 ' '=5 ' '=7 c=9; blanks even
    path = [0, 0, 1, 1, 3, 4, 5, 6, 7, 7, 8, 9, 9, 10, -1, -1]
    a = CtcAlignment.from_path(label, -12.5, path)
    assert list(a.frame_label_positions) == [-1, -1, 0, 0, 1, -1, 2, -1, 3, 3, -1, 4, 4, -1, -1, -1]
    assert a.character_frames == [(2, 4), (4, 5), (6, 7), (8, 10), (11, 13)]
    assert a.word_frames == [("ab", (2, 5)), ("c", (11, 13))]
    pl = a.positional_label(0.02)
    assert pl.labels == ["ab", "c"]
    assert np.allclose([r for _, r in pl.labeled_sections], [(0.04, 0.1), (0.22, 0.26)])
    # infeasible: no ranges, no positional label
    bad = CtcAlignment.from_path("abc", -np.inf, [-1] * 4)
    assert bad.character_frames == [] and bad.word_frames == [] and bad.positional_label(0.02) is None
    # only spaces: characters but no words
    spaces = CtcAlignment.from_path("  ", -1.0, [1, 2, 3])
    assert spaces.character_frames == [(0, 1), (2, 3)] and spaces.positional_label(0.02) is None


def test_alignment_symbols_are_exported():
    from speechless_amd import _lib
    assert "sl_ctc_align" in _lib.SIGNATURES and "sl_ctc_align_workspace_bytes" in _lib.SIGNATURES
