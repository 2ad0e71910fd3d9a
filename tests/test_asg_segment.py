"""ASG segment posteriors without a GPU: the float64 restatement of sl_asg_segment_scores (tests/asg_segment_ref.py) against the
sum over all k^T frame labelings and against minus the ASG loss of tests/test_asg.py, its edge rules, the entry point's host-side
refusals, and the host data model (grapheme_spans, cut_section_grapheme_spans, encode_transcripts)."""
import itertools

import numpy as np
import pytest

from asg_segment_ref import brute_force_scores, forward_score, segment_scores
from test_asg import EPS, asg_reference


def _strings(k, t_n):
    """every string over k graphemes without adjacent equal ones, of 1 .. t_n graphemes"""
    return [s for n in range(1, t_n + 1) for s in itertools.product(range(k), repeat=n)
            if all(a != b for a, b in zip(s, s[1:]))]


@pytest.mark.parametrize("k,t_n", [(2, 1), (2, 4), (2, 6), (3, 1), (3, 3), (3, 6)])
def test_restatement_equals_the_sum_over_all_labelings(k, t_n):
    rng = np.random.RandomState(10 * k + t_n)
    e = rng.randn(t_n, k) * 2.0
    g = rng.randn(k, k) * 1.5
    g0 = rng.randn(k)
    for start in (g0, g[1]):  # g0, and a previous grapheme: the row of transitions out of it
        brute = brute_force_scores(e, g, start)
        assert sum(np.exp(v) for v in brute.values()) == pytest.approx(1.0, abs=1e-12)
        strings = _strings(k, t_n)
        assert set(brute) == set(strings)
        for s in strings:
            assert forward_score(e, g, start, list(s)) == pytest.approx(brute[s], abs=1e-12)
    # the same through segment_scores: a segment in mid-label starts from the transitions out of the grapheme before it
    labels = np.array([[1, 0, 1][:max(2, min(3, t_n + 1))]], dtype=np.int32)
    logq = e[None].astype(np.float32)
    got = segment_scores(logq, g, g0, labels, [t_n], [(0, 0, t_n, 1, 2), (0, 0, t_n, 0, 1)], 4)
    e32 = logq[0].astype(np.float64)
    assert got[0] == pytest.approx(brute_force_scores(e32, g, g[1])[(0,)], abs=1e-12)
    assert got[1] == pytest.approx(brute_force_scores(e32, g, g0)[(1,)], abs=1e-12)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_whole_label_over_all_frames_is_minus_the_asg_loss(seed):
    rng = np.random.RandomState(seed)
    k, t_n = 7, 23
    label = [int(c) for c in rng.randint(0, k, size=6)]
    label[3] = label[2]  # adjacent equal graphemes need no special rule
    p = rng.dirichlet(np.ones(k) * 0.3, size=t_n)
    g = rng.randn(k, k)
    g0 = rng.randn(k)
    loss = asg_reference(p, g, g0, label)[0]
    e = np.log(p + EPS)
    labels = np.array([label], dtype=np.int64)
    for logq in (e, e + rng.uniform(-50, 50, size=(t_n, 1))):  # a per-frame constant cancels in N - Z
        got = segment_scores(logq[None], g, g0, labels, [t_n], [(0, 0, t_n, 0, len(label))], 16)[0]
        assert got == pytest.approx(-loss, abs=1e-9)


def test_edge_rules_and_clamps():
    rng = np.random.RandomState(5)
    k, t_out, l_max = 5, 12, 6
    logq = rng.randn(2, t_out, k).astype(np.float32)
    trans = rng.randn(k, k).astype(np.float32)
    init = rng.randn(k).astype(np.float32)
    labels = np.array([[0, 1, 2, 3, 4, 1], [4, 9, -3, 2, 2, 0]], dtype=np.int32)  # (9 and -3: clamped to 4 and 0)
    input_len = [10, 12]

    def score(*seg, seg_l_max=6):
        return segment_scores(logq, trans, init, labels, input_len, [seg], seg_l_max)[0]

    assert score(0, 3, 3, 2, 2) == 0.0                 # L = 0 and T = 0
    assert score(0, 3, 8, 2, 2) == -np.inf             # L = 0 and T > 0: without a blank no path says nothing
    assert score(0, 3, 3, 0, 2) == -np.inf             # T = 0 and L > 0
    assert score(0, 0, 3, 0, 4) == -np.inf             # T < L
    assert np.isfinite(score(0, 0, 4, 0, 4))           # T = L: the one path
    assert score(-1, 0, 5, 0, 1) == -np.inf and score(2, 0, 5, 0, 1) == -np.inf  # b outside [0, batch)
    # both ranges beyond their ends are clamped: to T_b (not t_out) and to l_max
    assert score(0, -4, 99, -2, 99) == score(0, 0, 10, 0, 6)
    assert score(0, 10, 12, 0, 0) == 0.0               # frames past input_len are clamped away
    assert score(0, 8, 5, 3, 1) == 0.0                 # negative ranges: T = 0 and L = 0
    # seg_l_max cuts the span
    assert score(0, 0, 10, 1, 6, seg_l_max=2) == score(0, 0, 10, 1, 3)
    # label values are clamped into [0, k)
    clamped = labels.copy()
    clamped[1, 1], clamped[1, 2] = 4, 0
    assert score(1, 0, 12, 0, 6) == segment_scores(logq, trans, init, clamped, input_len, [(1, 0, 12, 0, 6)], 6)[0]
    assert score(1, 2, 9, 2, 4) == segment_scores(logq, trans, init, clamped, input_len, [(1, 2, 9, 2, 4)], 6)[0]  # p = 9 -> 4
    # a mid-label segment starts from the transitions out of the grapheme before it
    assert score(0, 2, 9, 2, 4) == forward_score(logq[0, 2:9], trans, trans[1], [2, 3])
    assert score(0, 2, 9, 0, 2) == forward_score(logq[0, 2:9], trans, init, [0, 1])


def test_minus_infinity_scores_close_paths_without_a_nan():
    rng = np.random.RandomState(6)
    k, t_n = 4, 9
    logq = rng.randn(1, t_n, k).astype(np.float32)
    trans = rng.randn(k, k).astype(np.float32)
    init = rng.randn(k).astype(np.float32)
    labels = np.array([[0, 1, 2]], dtype=np.int32)
    seg = [(0, 0, t_n, 0, 3), (0, 1, t_n, 1, 3)]
    open_ = segment_scores(logq, trans, init, labels, [t_n], seg, 3)
    assert np.all(np.isfinite(open_))
    on_path = trans.copy()
    on_path[1, 2] = -np.inf  # the move 1 -> 2 is on both segments' paths
    assert np.all(segment_scores(logq, on_path, init, labels, [t_n], seg, 3) == -np.inf)
    elsewhere = trans.copy()
    elsewhere[3, 0] = elsewhere[2, 1] = -np.inf  # not on the label's path: Z shrinks, N stays
    got = segment_scores(logq, elsewhere, init, labels, [t_n], seg, 3)
    assert np.all(np.isfinite(got)) and np.all(got > open_)
    closed_start = init.copy()
    closed_start[0] = -np.inf
    assert segment_scores(logq, trans, closed_start, labels, [t_n], seg[:1], 3)[0] == -np.inf
    # everything closed: Z = -inf and N = -inf give -inf, not NaN
    got = segment_scores(logq, np.full((k, k), -np.inf), np.full(k, -np.inf), labels, [t_n], seg, 3)
    assert np.all(got == -np.inf)
    # a frame whose emissions are all -inf
    dead = logq.copy()
    dead[0, 4] = -np.inf
    assert np.all(segment_scores(dead, trans, init, labels, [t_n], seg, 3) == -np.inf)


def test_entry_point_host_side_checks(hip_lib):
    """Without a GPU: no workspace is asked for, and bad arguments are refused before any launch with the output untouched."""
    size = hip_lib.raw("sl_asg_segment_scores_workspace_bytes")
    assert all(size(n, l, k) == 0 for n in (1, 300, 100000) for l in (0, 64, 65, 511) for k in (2, 31, 64))
    score = hip_lib.raw("sl_asg_segment_scores")
    out = np.full((8,), 123.0, dtype=np.float32)
    buf = np.zeros((64,), dtype=np.int32).ctypes.data  # a valid host address: nothing may be launched on it
    ok = [buf, buf, buf, buf, buf, buf, out.ctypes.data]
    assert score(*ok, 1, 10, 31, 100, 4, 512, None, 0, None) == -2 and "seg_l_max = 512" in hip_lib.last_error()
    assert score(*ok, 1, 10, 31, 100, 4, -1, None, 0, None) == -2 and "seg_l_max = -1" in hip_lib.last_error()
    assert score(*ok, 1, 10, 65, 100, 4, 10, None, 0, None) == -2 and "k = 65" in hip_lib.last_error()
    assert score(*ok, 1, 10, 1, 100, 4, 10, None, 0, None) == -2 and "k = 1" in hip_lib.last_error()
    assert score(*ok, 1, 10, 31, 100, 0, 10, None, 0, None) == -2 and "n_segments >= 1" in hip_lib.last_error()
    for i, name in enumerate(("logq", "trans", "init", "labels", "input_len", "segments", "log_posterior")):
        args = list(ok)
        args[i] = None
        assert score(*args, 1, 10, 31, 100, 4, 10, None, 0, None) == -1
        assert name + " is a null pointer" in hip_lib.last_error()
    assert score(*ok, 0, 10, 31, 100, 4, 10, None, 0, None) == -1
    assert score(*ok, 1, 0, 31, 100, 4, 10, None, 0, None) == -1
    assert score(*ok, 1, 10, 31, -1, 4, 10, None, 0, None) == -1
    # the order of sl_ctc_segment_scores: unsupported shapes before invalid arguments
    assert score(None, None, None, None, None, None, None, 0, 0, 65, -1, 0, 512, None, 0, None) == -2
    assert np.all(out == 123.0)


def test_segment_check_takes_the_kind():
    from speechless_amd import longform
    from speechless_amd.engine_decode import check_segments
    assert longform.ASG_SEGMENT_MAX_LABEL == 511
    good = [(0, 0, 5, 0, 2), (1, 0, 100000, 0, 511)]
    assert np.array_equal(check_segments(good, 2, "asg"), check_segments(good, 2))
    with pytest.raises(ValueError, match=r"segment 1 = \[0, 0, 5, 0, 512\].*511 graphemes \(sl_asg_segment_scores\)"):
        check_segments(good[:1] + [(0, 0, 5, 0, 512)], 2, "asg")
    with pytest.raises(ValueError, match=r"segment 0 = \[2, .*511 letters \(sl_ctc_segment_scores\)"):
        check_segments([(2, 0, 5, 0, 2)], 2)


def test_segment_symbols_are_exported():
    from ctypes import c_int, c_size_t
    from speechless_amd import _lib
    assert _lib.SIGNATURES["sl_asg_segment_scores_workspace_bytes"] == (c_size_t, [c_int, c_int, c_int])
    # sl_ctc_segment_scores' arguments with trans and init behind logq
    ctc = _lib.SIGNATURES["sl_ctc_segment_scores"]
    assert _lib.SIGNATURES["sl_asg_segment_scores"] == (ctc[0], ctc[1][:1] + ctc[1][:2] + ctc[1][1:])


# ---------------------------------------------------------------------------------------------- host data model
class _Aligned:
    def __init__(self, label, word_frames):
        self.label = label
        self.word_frames = word_frames


def test_grapheme_spans():
    from speechless_amd import english_frequent_characters, grapheme_spans, word_spans
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
    enc = AsgGraphemeEncoding(english_frequent_characters)
    label = "hello  all beee"  # runs of two (ll, the double space, ll) and of three (eee)
    encoded = enc.encode(label)
    # h e l 2 o _ 2 a l 2 _ b e 3
    assert len(encoded) == 14 and encoded[3] == encoded[6] == encoded[9] == enc.asg_twice and encoded[13] == enc.asg_thrice
    chars = word_spans(label)
    assert chars == [(0, 5), (7, 10), (11, 15)]
    spans = grapheme_spans(label, chars)
    assert spans == [(0, 5), (7, 10), (11, 14)]
    for (i, j), (begin, end) in zip(chars, spans):  # a word's span is the encoding of the word alone
        assert encoded[begin:end] == enc.encode(label[i:j])
    assert grapheme_spans(label, [(0, 15), (0, 0), (15, 15), (5, 7), (0, 10)]) == [(0, 14), (0, 0), (14, 14), (5, 7), (0, 10)]
    for bad in ((0, 3), (3, 5), (0, 6), (6, 10), (11, 13), (11, 14)):  # inside ll, the double space and eee
        with pytest.raises(ValueError, match="splits the run"):
            grapheme_spans(label, [(0, 5), bad])
    with pytest.raises(ValueError, match="outside"):
        grapheme_spans(label, [(0, 16)])
    assert grapheme_spans("", []) == [] and grapheme_spans("ab", [(0, 2)]) == [(0, 2)]


def test_cut_section_grapheme_spans_equals_cut_sections():
    from speechless_amd import cut_section_grapheme_spans, cut_section_spans, cut_sections, english_frequent_characters
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
    enc = AsgGraphemeEncoding(english_frequent_characters)
    label = "hello  all beee zoo"
    words = [("hello", (2, 20)), ("all", (24, 40)), ("beee", (45, 50)), ("zoo", (60, 90))]
    encoded = enc.encode(label)
    for max_frames in (40, 30, 5, 1000):
        aligned = _Aligned(label, words)
        got = cut_section_grapheme_spans(aligned, max_frames)
        assert [(text, frames) for text, frames, _ in got] == cut_sections(aligned, max_frames)
        for (text, _, (begin, end)), (_, _, (i, j)) in zip(got, cut_section_spans(aligned, max_frames)):
            assert encoded[begin:end] == enc.encode(label[i:j]) and label[i:j].split() == text.split()
    assert cut_section_grapheme_spans(_Aligned(label, words), 40) == [
        ("hello all", (2, 42), (0, 10)), ("beee", (42, 55), (11, 14)), ("zoo", (55, 90), (15, 18))]
    assert cut_section_grapheme_spans(_Aligned(label, []), 40) == []


def test_a_transcript_that_cannot_be_encoded_gets_none():
    """a decode can stack repeat marks: l, thrice, l says "llll", which no encoded label can say"""
    from speechless_amd import english_frequent_characters
    from speechless_amd.alignment import encode_transcripts
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
    enc = AsgGraphemeEncoding(english_frequent_characters)
    a, l = enc.encode("a")[0], enc.encode("l")[0]
    decoded = [[a, l, enc.asg_thrice, l], [a, l, enc.asg_twice, a], [], [l, enc.asg_twice, enc.asg_twice]]
    transcripts = [enc.decode_graphemes(d, merge_repeated=False) for d in decoded]
    assert transcripts == ["allll", "alla", "", "ll"]
    with pytest.raises(ValueError, match="4-fold"):
        enc.encode(transcripts[0])
    assert encode_transcripts(enc, transcripts) == [None, [a, l, enc.asg_twice, a], [], [l, enc.asg_twice]]


def test_scored_alignment_over_an_asg_alignment():
    from speechless_amd import AsgAlignment, ScoredAlignment, english_frequent_characters
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
    enc = AsgGraphemeEncoding(english_frequent_characters)
    label = "all be"
    encoded = enc.encode(label)  # a l 2 _ b e
    path = [0, 0, 1, 2, 2, 3, 4, 5, 5, -1]
    a = AsgAlignment.from_path(label, encoded, enc.asg_twice, enc.asg_thrice, -4.0, path)
    scored = ScoredAlignment(a, [-0.25, -1.0], -2.5)
    assert [(w.word, w.first, w.end, w.log_posterior) for w in scored.words] == [("all", 0, 5, -0.25), ("be", 6, 9, -1.0)]
    assert scored.label == label and scored.alignment is a and scored.log_posterior == -2.5
