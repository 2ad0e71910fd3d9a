"""CTC segment posteriors without a GPU: the float64 restatement of sl_ctc_segment_scores (tests/ctc_segment_ref.py) against the sum
over all frame labelings, its edge rules, the host-side refusals of the entry point and of the engine's segment check, and the host
data model (word_spans, cut_section_spans, WordConfidence, ScoredAlignment)."""
import itertools

import numpy as np
import pytest

from ctc_segment_ref import brute_force_scores, forward_score, segment_scores

K = 3  # two letters and the blank


def _logq(rng, t, k=K, scale=1.5):
    lg = scale * rng.randn(t, k)
    return lg - np.log(np.exp(lg).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("t", [1, 2, 3, 4, 5, 6])
def test_restatement_equals_the_sum_over_all_frame_labelings(t):
    """every label of 0 to 3 letters over two letters -- those with a repeated letter among them -- at T <= 6, k = 3"""
    rng = np.random.RandomState(t)
    logq = _logq(rng, t)
    brute = brute_force_scores(logq, K)
    labels = [s for n in range(4) for s in itertools.product(range(K - 1), repeat=n)]
    assert (0, 0) in labels and (1, 1, 0) in labels and () in labels
    for label in labels:
        got = forward_score(logq, list(label), K)
        want = brute.get(label, -np.inf)
        if want == -np.inf:
            assert got == -np.inf, (label, got)
        else:
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (label, got, want)
    # nothing else has any mass at T <= 3: the strings of up to 3 letters are all a labeling of 3 frames can say
    if t <= 3:
        assert set(brute) <= set(labels)


@pytest.mark.parametrize("t", [2, 5, 9])
def test_scores_of_short_strings_behave_as_probabilities(t):
    """each string's score is at most 1, the strings of up to 2 letters together too, and the remainder is what the longer
    strings hold: nothing at T = 2, where no labeling says more than two letters"""
    rng = np.random.RandomState(10 + t)
    k = 4
    logq = _logq(rng, t, k)
    strings = [s for n in range(3) for s in itertools.product(range(k - 1), repeat=n)]
    p = np.array([np.exp(forward_score(logq, list(s), k)) for s in strings])
    assert np.all(p <= 1.0 + 1e-12) and np.all(p >= 0.0)
    remainder = 1.0 - p.sum()
    assert remainder >= -1e-12
    if t == 2:
        assert abs(remainder) <= 1e-12
    else:
        assert remainder > 1e-6


def test_edge_rules_of_the_restatement():
    rng = np.random.RandomState(5)
    k, t_out = 5, 12
    logq = np.stack([_logq(rng, t_out, k), _logq(rng, t_out, k)]).astype(np.float32)
    labels = np.array([[0, 1, 1, 2, 3, 0], [2, 2, 2, 9, -4, 1]], dtype=np.int32)
    input_len = [10, 40]
    blank0 = logq[0, :, k - 1].astype(np.float64)

    def score(*segment, seg_l_max=6):
        return segment_scores(logq, labels, input_len, [segment], seg_l_max)[0]
    # L = 0: the sum of the blank's logq over the frames; L = 0 and T = 0: 0
    assert score(0, 2, 7, 3, 3) == pytest.approx(blank0[2:7].sum(), abs=1e-12)
    assert score(0, 4, 4, 0, 0) == 0.0
    assert score(0, 4, 4, 0, 2) == -np.inf  # letters and no frame
    # the frame range is clamped into [0, min(input_len, t_out)]: frames 10, 11 of utterance 0 do not count, nor do frames < 0
    assert score(0, 6, 12, 0, 0) == pytest.approx(blank0[6:10].sum(), abs=1e-12)
    assert score(0, -3, 2, 0, 0) == pytest.approx(blank0[0:2].sum(), abs=1e-12)
    assert score(0, 10, 12, 0, 0) == 0.0 and score(0, 11, 12, 0, 1) == -np.inf
    assert score(1, 0, 40, 0, 0) == pytest.approx(logq[1, :, k - 1].astype(np.float64).sum(), abs=1e-12)  # input_len > t_out
    # T smaller than L + the number of adjacent equal letters: -inf; one frame more: finite
    assert score(0, 0, 3, 0, 3) == -np.inf and np.isfinite(score(0, 0, 4, 0, 3))
    assert score(1, 0, 4, 0, 3) == -np.inf and np.isfinite(score(1, 0, 5, 0, 3))
    # the label range is clamped into [0, l_max] and its length to seg_l_max
    assert score(0, 0, 10, 4, 99) == score(0, 0, 10, 4, 6)
    assert score(0, 0, 10, 0, 6, seg_l_max=2) == score(0, 0, 10, 0, 2)
    assert score(0, 0, 10, 5, 2) == score(0, 0, 10, 0, 0)  # end before begin: no letters
    # label values are clamped into [0, k) as clamp_label does: 9 reads column k - 1, -4 column 0
    assert score(1, 0, 8, 3, 5) == forward_score(logq[1, :8], [k - 1, 0], k)
    # b outside [0, batch)
    assert score(-1, 0, 5, 0, 1) == -np.inf and score(2, 0, 5, 0, 1) == -np.inf
    # a whole utterance is minus its CTC loss: the sum over every label is 1 at T = 1
    one = np.array([np.exp(forward_score(logq[0, :1], s, k)) for s in [[]] + [[c] for c in range(k - 1)]])
    assert one.sum() == pytest.approx(1.0, abs=1e-6)  # (logq is float32)


def test_entry_point_host_side_checks(hip_lib):
    """Without a GPU: no workspace is asked for, and bad arguments are refused before any launch with the output untouched."""
    size = hip_lib.raw("sl_ctc_segment_scores_workspace_bytes")
    assert all(size(n, l) == 0 for n in (1, 300, 100000) for l in (0, 63, 64, 511))
    score = hip_lib.raw("sl_ctc_segment_scores")
    out = np.full((8,), 123.0, dtype=np.float32)
    buf = np.zeros((64,), dtype=np.int32).ctypes.data  # a valid host address: nothing may be launched on it
    ok = [buf, buf, buf, buf, out.ctypes.data]
    assert score(*ok, 1, 10, 29, 100, 4, 512, None, 0, None) == -2 and "seg_l_max = 512" in hip_lib.last_error()
    assert score(*ok, 1, 10, 29, 100, 4, -1, None, 0, None) == -2 and "seg_l_max = -1" in hip_lib.last_error()
    assert score(*ok, 1, 10, 65, 100, 4, 10, None, 0, None) == -2 and "k = 65" in hip_lib.last_error()
    assert score(*ok, 1, 10, 1, 100, 4, 10, None, 0, None) == -2 and "k = 1" in hip_lib.last_error()
    assert score(*ok, 1, 10, 29, 100, 0, 10, None, 0, None) == -2 and "n_segments >= 1" in hip_lib.last_error()
    for i, name in enumerate(("logq", "labels", "input_len", "segments", "log_posterior")):
        args = list(ok)
        args[i] = None
        assert score(*args, 1, 10, 29, 100, 4, 10, None, 0, None) == -1
        assert name + " is a null pointer" in hip_lib.last_error()
    assert score(*ok, 0, 10, 29, 100, 4, 10, None, 0, None) == -1
    assert score(*ok, 1, 0, 29, 100, 4, 10, None, 0, None) == -1
    assert np.all(out == 123.0)


def test_segment_check_names_the_first_bad_row():
    from speechless_amd.engine_decode import check_segments
    good = [(0, 0, 5, 0, 2), (2, 3, 3, 4, 4), (1, 0, 100000, 0, 511)]
    seg = check_segments(good, 3)
    assert seg.dtype == np.int32 and seg.shape == (3, 5) and seg.flags["C_CONTIGUOUS"]
    for bad in ((3, 0, 5, 0, 2), (-1, 0, 5, 0, 2), (0, -1, 5, 0, 2), (0, 6, 5, 0, 2), (0, 0, 5, -1, 2), (0, 0, 5, 3, 2),
                (0, 0, 5, 0, 512)):
        with pytest.raises(ValueError, match=r"segment 2 = \[" + str(bad[0])):
            check_segments(good[:2] + [bad] + [bad], 3)
    for shape in ([], [(0, 0, 5, 0)], np.zeros((2, 5), dtype=np.float32), np.zeros((0, 5), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"\(N, 5\)"):
            check_segments(shape, 3)


def test_segment_symbols_are_exported():
    from speechless_amd import _lib
    assert "sl_ctc_segment_scores" in _lib.SIGNATURES and "sl_ctc_segment_scores_workspace_bytes" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------- host data model
class _Aligned:
    def __init__(self, word_frames, label=None):
        self.word_frames = word_frames
        self.label = " ".join(w for w, _ in word_frames) if label is None else label


def test_word_spans():
    from speechless_amd import CtcAlignment, word_spans
    assert word_spans("") == [] and word_spans("   ") == []
    assert word_spans("ab") == [(0, 2)]
    assert word_spans("ab c") == [(0, 2), (3, 4)]
    label = "  ab  c   def "
    spans = word_spans(label)
    assert [label[i:j] for i, j in spans] == label.split() == ["ab", "c", "def"]
    # the same walk as the alignment's word_frames
    a = CtcAlignment.from_path("ab  c", -1.0, [0, 0, 1, 1, 3, 4, 5, 6, 7, 7, 8, 9, 9, 10, -1, -1])
    assert [a.label[i:j] for i, j in word_spans(a.label)] == [w for w, _ in a.word_frames]


def test_cut_section_spans_equals_cut_sections():
    """the cases of tests/test_longform.py::test_cut_sections: the same texts and frame ranges, and spans that index the label"""
    from speechless_amd import CtcAlignment, cut_section_spans, cut_sections
    words = [("a", (10, 20)), ("bb", (24, 40)), ("c", (45, 50)), ("dd", (60, 90)), ("e", (95, 100))]
    for max_frames in (40, 39, 5, 1000):
        aligned = _Aligned(words)
        got = cut_section_spans(aligned, max_frames)
        assert [(text, frames) for text, frames, _ in got] == cut_sections(aligned, max_frames)
        assert [aligned.label[i:j] for _, _, (i, j) in got] == [text for text, _, _ in got]
    assert cut_section_spans(_Aligned(words), 40) == [("a bb c", (10, 55), (0, 6)), ("dd e", (55, 100), (7, 11))]
    assert cut_section_spans(_Aligned([("long", (3, 500))]), 10) == [("long", (3, 500), (0, 4))]
    # double spaces: the span runs from the first word's first character to the last word's last and keeps the label's spacing
    a = CtcAlignment.from_path("ab  c", -1.0, [0, 0, 1, 1, 3, 4, 5, 6, 7, 7, 8, 9, 9, 10, -1, -1])
    assert cut_section_spans(a, 4) == [("ab", (2, 8), (0, 2)), ("c", (8, 13), (4, 5))]
    assert cut_section_spans(a, 11) == [("ab c", (2, 13), (0, 5))] and a.label[0:5] == "ab  c"
    for max_frames in (4, 11):
        assert [(t, f) for t, f, _ in cut_section_spans(a, max_frames)] == cut_sections(a, max_frames)
    assert cut_section_spans(CtcAlignment.from_path("abc", -np.inf, [-1] * 4), 100) == []


def test_scored_alignment_from_a_hand_made_path():
    from speechless_amd import CtcAlignment, ScoredAlignment, WordConfidence
    a = CtcAlignment.from_path("ab  c", -1.0, [0, 0, 1, 1, 3, 4, 5, 6, 7, 7, 8, 9, 9, 10, -1, -1])
    scored = ScoredAlignment(a, np.array([-0.5, -2.0], dtype=np.float32), np.float32(-3.25))
    assert scored.alignment is a and scored.label == "ab  c" and scored.log_posterior == -3.25
    assert [(w.word, w.first, w.end, w.log_posterior) for w in scored.words] == [("ab", 2, 5, -0.5), ("c", 11, 13, -2.0)]
    assert all(isinstance(w, WordConfidence) for w in scored.words)
    assert scored.words[0].confidence == pytest.approx(np.exp(-0.5)) and 0.0 < scored.words[1].confidence < 1.0
    assert WordConfidence("x", 0, 1, -np.inf).confidence == 0.0 and WordConfidence("x", 0, 1, 0.0).confidence == 1.0
    with pytest.raises(ValueError, match="1 word scores for the 2 words"):
        ScoredAlignment(a, [-0.5], -3.25)
    # infeasible: no words, -inf
    none = ScoredAlignment(CtcAlignment.from_path("abc", -np.inf, [-1] * 4), [], -np.inf)
    assert none.words == [] and none.log_posterior == -np.inf
