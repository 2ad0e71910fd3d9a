"""ASG forced alignment without a GPU: the float32 restatement of sl_asg_align (include/speechless_hip.h) against a brute
force over every monotone alignment, its tie rule and infeasible cases, and alignment.AsgAlignment's frame ranges."""
import itertools

import numpy as np
import pytest

F32 = np.float32
NEG_INF = F32(-np.inf)


def asg_align_reference(logq, trans, init, labels, label_len, input_len):
    """sl_asg_align for one utterance in numpy float32 scalars, the operations in the header's order.  logq (t_out, k)
    emissions as they are, trans (k, k) [from][to], init (k,), labels any int sequence of at least label_len entries.
    Returns (score float32, path int32 (t_out,): the state per frame, -1 past T_b or everywhere when infeasible)."""
    logq, trans, init = (np.asarray(x, dtype=F32) for x in (logq, trans, init))
    t_out, k = logq.shape
    L = min(max(int(label_len), 0), len(labels))
    T = min(max(int(input_len), 0), t_out)
    path = np.full(t_out, -1, dtype=np.int32)
    if L == 0 or T == 0 or L > T:
        return NEG_INF, path
    lab = [min(max(int(c), 0), k - 1) for c in labels[:L]]
    delta = [NEG_INF] * L
    delta[0] = init[lab[0]] + logq[0, lab[0]]
    moved = np.zeros((T, L), dtype=bool)
    for t in range(1, T):
        new = list(delta)  # (states above t are -inf and stay so)
        for s in range(min(t, L - 1), -1, -1):
            best = delta[s] + trans[lab[s], lab[s]]
            if s >= 1:
                move = delta[s - 1] + trans[lab[s - 1], lab[s]]
                if move > best:
                    best = move
                    moved[t, s] = True
            new[s] = best + logq[t, lab[s]]
        delta = new
    score = delta[L - 1]
    if score == NEG_INF:
        return NEG_INF, path
    s = L - 1
    for t in range(T - 1, -1, -1):
        path[t] = s
        if moved[t, s]:
            s -= 1
    return score, path


def random_inputs(rng, t_out, k, batch=None):
    """logq = a log-softmax of normals, trans / init of order 1 (float32)"""
    z = rng.randn(*((t_out, k) if batch is None else (batch, t_out, k)))
    z = z - z.max(-1, keepdims=True)
    logq = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(F32)
    return logq, rng.uniform(-1, 1, size=(k, k)).astype(F32), rng.uniform(-1, 1, size=k).astype(F32)


def monotone_paths(t_n, n_states):
    """every alignment of n_states states over t_n frames: state 0 first, n_states - 1 last, steps of 0 or 1"""
    for steps in itertools.product((0, 1), repeat=t_n - 1):
        if sum(steps) == n_states - 1:
            yield np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)


def path_score32(logq, trans, init, lab, states):
    """a path's score in float32, in frame order, as (acc + g) + e"""
    acc = init[lab[0]] + logq[0, lab[0]]
    for t in range(1, len(states)):
        acc = (acc + trans[lab[states[t - 1]], lab[states[t]]]) + logq[t, lab[states[t]]]
    return acc


@pytest.mark.parametrize("k", [2, 3, 4])
def test_restatement_equals_the_maximum_over_every_alignment_bit_for_bit(k):
    """Rounding is monotone, so the DP over rounded sums and the enumeration of rounded path scores agree exactly."""
    rng = np.random.RandomState(40 + k)
    unique = 0
    for t_n in range(1, 8):
        for n in range(1, t_n + 1):
            logq, trans, init = random_inputs(rng, t_n + 1, k)  # (one frame past T_b: the path ends in -1)
            lab = [int(c) for c in rng.randint(0, k, size=n)]
            score, path = asg_align_reference(logq, trans, init, lab + [k + 3], n, t_n)
            scored = [(path_score32(logq, trans, init, lab, p), p) for p in monotone_paths(t_n, n)]
            best = max(s for s, _ in scored)
            assert F32(score).tobytes() == F32(best).tobytes(), (t_n, lab)
            maximal = [p for s, p in scored if s == best]
            assert any(np.array_equal(path[:t_n], p) for p in maximal) and path[t_n] == -1, (t_n, lab, path)
            unique += len(maximal) == 1
    assert unique > 0  # (where one path alone is maximal, the membership above says the path IS that one; equal letters tie)


def test_tie_rule_stays_as_long_as_it_can():
    """All-zero emissions and scores: every path scores 0, stay wins every tie in the forward pass, so the backtrace from
    L - 1 never steps down while it still can stay -- the label's states are entered as EARLY as possible."""
    zeros = np.zeros((5, 3), dtype=F32)
    score, path = asg_align_reference(zeros, np.zeros((3, 3)), np.zeros(3), [0, 1, 2], 3, 5)
    # delta_t(s) = 0 for s <= t, -inf above: a move is taken only where stay is -inf, i.e. into state s at frame t = s
    assert score == 0 and list(path) == [0, 1, 2, 2, 2]


def test_infeasible_utterances_score_minus_infinity_and_have_no_path():
    rng = np.random.RandomState(5)
    logq, trans, init = random_inputs(rng, 6, 4)
    closed = init.copy()
    closed[2] = NEG_INF
    for lab, n, t_b, g0 in (([1, 2], 0, 6, init), ([1, 2], 2, 0, init), ([1, 2, 3, 0, 1], 5, 4, init), ([2, 1], 2, 6, closed)):
        score, path = asg_align_reference(logq, trans, g0, lab, n, t_b)
        assert score == NEG_INF and (path == -1).all()
    score, path = asg_align_reference(logq, trans, closed, [1, 2], 2, 6)  # (the closed letter is not the first: feasible)
    assert np.isfinite(score) and path[0] == 0 and path[5] == 1


# ---------------------------------------------------------------------------------------------------- AsgAlignment
def make_alignment(label, runs, score=-3.5, t_out=None):
    """`runs`: frames per encoded grapheme, in order -> AsgAlignment over the path they spell"""
    from speechless_amd.alignment import AsgAlignment
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding, english_frequent_characters
    enc = AsgGraphemeEncoding(english_frequent_characters)
    encoded = enc.encode(label)
    assert len(runs) == len(encoded)
    path = np.concatenate([np.full(n, i, dtype=np.int32) for i, n in enumerate(runs)] + [np.zeros(0, dtype=np.int32)])
    path = np.concatenate([path, np.full((t_out or len(path)) - len(path), -1, dtype=np.int32)])
    return AsgAlignment.from_path(label, encoded, enc.asg_twice, enc.asg_thrice, score, path), enc, encoded


def test_asg_alignment_ranges_of_hello():
    a, enc, encoded = make_alignment("hello", [2, 1, 3, 1, 4], t_out=13)  # h e l <twice> o
    assert encoded[3] == enc.asg_twice and a.feasible and a.encoded_label == encoded
    assert a.grapheme_frames == [(0, 2), (2, 3), (3, 6), (6, 7), (7, 11)]
    assert a.character_frames == [(0, 2), (2, 3), (3, 6), (6, 7), (7, 11)]  # the second l takes the mark's range
    assert a.word_frames == [("hello", (0, 11))]
    pl = a.positional_label(0.02)
    assert pl.labels == ["hello"] and pl.labeled_sections[0][1] == (0 * 0.02, 11 * 0.02)


def test_asg_alignment_shares_the_thrice_marks_range():
    a, enc, encoded = make_alignment("aaa b", [3, 2, 1, 5])  # a <thrice> ' ' b
    assert encoded == [0, enc.asg_thrice, enc.encode_character(" "), 1]
    assert a.grapheme_frames == [(0, 3), (3, 5), (5, 6), (6, 11)]
    assert a.character_frames == [(0, 3), (3, 5), (3, 5), (5, 6), (6, 11)]
    assert a.word_frames == [("aaa", (0, 5)), ("b", (6, 11))]
    pl = a.positional_label(0.5)
    assert pl.labeled_sections == [("aaa", (0.0, 2.5)), ("b", (3.0, 5.5))]


def test_asg_alignment_of_one_letter_and_of_a_sentence():
    a, _, _ = make_alignment("a", [7], t_out=9)
    assert a.grapheme_frames == a.character_frames == [(0, 7)] and a.word_frames == [("a", (0, 7))]
    label = "she wasn't three"  # ... t h r e <twice>
    runs = [1, 2, 1, 1, 2, 1, 1, 3, 1, 1, 1, 1, 2, 1, 2, 4]
    a, enc, encoded = make_alignment(label, runs)
    assert len(encoded) == len(label) and encoded[-1] == enc.asg_twice
    bounds = np.concatenate([[0], np.cumsum(runs)])
    assert a.grapheme_frames == [(int(lo), int(hi)) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert a.character_frames == a.grapheme_frames  # no thrice mark: one range per character
    assert a.grapheme_frames[0][0] == 0 and a.grapheme_frames[-1][1] == sum(runs)
    assert all(x[1] == y[0] and x[0] < x[1] for x, y in zip(a.grapheme_frames[:-1], a.grapheme_frames[1:]))
    assert a.word_frames == [("she", (0, 4)), ("wasn't", (5, 14)), ("three", (15, 25))]
    pl = a.positional_label(0.01)
    assert pl.label == label
    for (_, (start, end)), (_, (first, last)) in zip(pl.labeled_sections, a.word_frames):
        assert start == first * 0.01 and end == last * 0.01


def test_infeasible_asg_alignment_has_no_ranges():
    from speechless_amd.alignment import AsgAlignment
    a, _, _ = make_alignment("hello", [0, 0, 0, 0, 0], score=-np.inf, t_out=4)
    assert not a.feasible and (a.frame_grapheme_positions == -1).all()
    assert a.grapheme_frames == [] and a.character_frames == [] and a.word_frames == []
    assert a.positional_label(0.02) is None
    with pytest.raises(ValueError, match="in one run"):  # a feasible score over a path that skips a grapheme
        AsgAlignment("ab", [0, 1], -1.0, [0, 0, 0])
    with pytest.raises(ValueError, match="repeat marks"):
        AsgAlignment.from_path("aab", [0, 5, 1], 28, 29, -1.0, [0, 1, 2])
