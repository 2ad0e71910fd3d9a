"""ASG alignment of long recordings without a GPU: the vectorised restatement (tests/asg_align_long_ref.py) returns the bytes of
the scalar one of tests/test_asg_align.py; alignment.AsgAlignment finds its frame ranges in one linear pass, with the checks and
errors of the per-grapheme search it replaces; alignment.cut_sections cuts an AsgAlignment; longform names the limit."""
import time

import numpy as np
import pytest

from asg_align_long_ref import asg_align_long_reference
from test_asg_align import F32, NEG_INF, asg_align_reference, make_alignment, random_inputs


def same_bytes(a, b):
    return F32(a[0]).tobytes() == F32(b[0]).tobytes() and a[1].dtype == b[1].dtype == np.int32 and \
        a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("k", [2, 3, 30])
def test_vectorised_restatement_returns_the_scalar_ones_bytes(k):
    rng = np.random.RandomState(70 + k)
    finite = infeasible = 0
    for case in range(60):
        t_out = int(rng.randint(1, 61))
        width = int(rng.randint(1, 41))
        logq, trans, init = random_inputs(rng, t_out, k)
        if case % 3 == 1:  # -inf scores: some close every path, some only a few
            trans[rng.rand(k, k) < 0.15] = NEG_INF
            init[rng.rand(k) < 0.2] = NEG_INF
        labels = [int(c) for c in rng.randint(-2, k + 2, size=width)]  # (values outside [0, k) are clamped)
        label_len = int(rng.randint(-1, width + 4))  # clamped to [0, width]
        input_len = int(rng.randint(-1, t_out + 4))  # clamped to [0, t_out]
        if case % 4 == 0:
            label_len, input_len = min(width, t_out), t_out  # feasible, and the diagonal where width >= t_out
        want = asg_align_reference(logq, trans, init, labels, label_len, input_len)
        got = asg_align_long_reference(logq, trans, init, labels, label_len, input_len)
        assert same_bytes(got, want), (case, t_out, width, label_len, input_len)
        assert not np.isnan(got[0])
        finite += bool(np.isfinite(got[0]))
        infeasible += got[0] == NEG_INF
    assert finite >= 10 and infeasible >= 10  # (a condition on the seeds: both kinds are there)


def test_vectorised_restatement_on_the_named_infeasible_rows_and_ties():
    rng = np.random.RandomState(5)
    logq, trans, init = random_inputs(rng, 6, 4)
    closed = init.copy()
    closed[2] = NEG_INF
    for lab, n, t_b, g0 in (([1, 2], 0, 6, init), ([1, 2], 2, 0, init), ([1, 2, 3, 0, 1], 5, 4, init), ([2, 1], 2, 6, closed),
                            ([1, 2], 2, 6, closed), ([1, 2], 9, 60, init)):
        assert same_bytes(asg_align_long_reference(logq, trans, g0, lab, n, t_b), asg_align_reference(logq, trans, g0, lab, n, t_b))
    zeros = np.zeros((5, 3), dtype=F32)
    score, path = asg_align_long_reference(zeros, np.zeros((3, 3)), np.zeros(3), [0, 1, 2], 3, 5)
    assert score == 0 and list(path) == [0, 1, 2, 2, 2]  # a tie stays: states are entered as early as possible


def test_vectorised_restatement_is_fast_enough_for_the_longest_label():
    """8191 states over 8300 frames: a GPU test restates several such rows, so one has to stay near a second."""
    rng = np.random.RandomState(8)
    logq, trans, init = random_inputs(rng, 8300, 30)
    labels = rng.randint(0, 30, size=8191)
    start = time.perf_counter()
    score, path = asg_align_long_reference(logq, trans, init, labels, 8191, 8300)
    elapsed = time.perf_counter() - start
    assert np.isfinite(score) and path[0] == 0 and path[-1] == 8190 and np.all(np.diff(path) >= 0) and np.all(np.diff(path) <= 1)
    assert elapsed < 20, elapsed  # (measured well under 2 s; the scalar restatement needs minutes)


# ------------------------------------------------------------------------------------------------------------ AsgAlignment
def grapheme_frames_by_search(positions, n):
    """the per-grapheme search the linear pass replaces (one flatnonzero per grapheme): ranges, or the index that fails"""
    ranges, end = [], 0
    for i in range(n):
        frames = np.flatnonzero(positions == i)
        if frames.size == 0 or frames[0] != end or frames[-1] + 1 - frames[0] != frames.size:
            return i
        end = int(frames[-1]) + 1
        ranges.append((int(frames[0]), end))
    return ranges


def test_linear_pass_equals_the_search_on_restated_paths():
    from speechless_amd.alignment import AsgAlignment
    rng = np.random.RandomState(12)
    letters = "abcdefghij"
    checked = 0
    for _ in range(40):
        t_out = int(rng.randint(2, 61))
        n = int(rng.randint(1, min(t_out, 40) + 1))
        label = "".join(letters[(i * 3 + int(rng.randint(0, 2))) % 10] for i in range(n))
        label = "".join(c for i, c in enumerate(label) if i == 0 or c != label[i - 1])  # no runs: one grapheme per character
        n = len(label)
        logq, trans, init = random_inputs(rng, t_out, 30)
        t_b = int(rng.randint(n, t_out + 1))
        encoded = [letters.index(c) for c in label]
        score, path = asg_align_long_reference(logq, trans, init, encoded, n, t_b)
        a = AsgAlignment(label, encoded, score, path)
        want = grapheme_frames_by_search(path, n)
        assert a.feasible and a.grapheme_frames == want and a.character_frames == want
        assert a.grapheme_frames[0][0] == 0 and a.grapheme_frames[-1][1] == t_b
        checked += 1
    assert checked == 40


def test_linear_pass_raises_where_the_search_fails():
    from speechless_amd.alignment import AsgAlignment
    malformed = [("ab", [0, 0, 0]),        # grapheme 1 never reached
                 ("ab", [1, 1, 1]),        # grapheme 0 missing
                 ("ab", [-1, 0, 1]),       # grapheme 0 does not start at frame 0
                 ("ab", [0, 1, 0]),        # grapheme 0 in two runs
                 ("abc", [0, 2, 1]),       # out of order
                 ("abc", [0, 1, -1, 2]),   # a hole before grapheme 2
                 ("abc", [0, 1, 2, 1]),    # grapheme 1 comes back
                 ("ab", [])]               # no frames at all
    for label, path in malformed:
        encoded = ["abc".index(c) for c in label]
        failing = grapheme_frames_by_search(np.asarray(path, dtype=np.int32), len(label))
        assert isinstance(failing, int)
        with pytest.raises(ValueError, match="does not pass grapheme {} of {!r} in one run behind grapheme {}".format(
                failing, label, failing - 1)):
            AsgAlignment(label, encoded, -1.0, path)
    # values that name no grapheme are passed over, as the search passes them over
    a = AsgAlignment("ab", [0, 1], -1.0, [0, 0, 1, -1, 7, -1])
    assert a.grapheme_frames == [(0, 2), (2, 3)] == grapheme_frames_by_search(np.asarray([0, 0, 1, -1, 7, -1]), 2)


def test_linear_pass_is_linear_at_the_longest_label(monkeypatch):
    """8191 graphemes over 30 000 frames: the per-grapheme search made one numpy pass over the path per grapheme (8191 x 30 000
    positions); the linear pass makes a fixed number of them, whatever the label's length."""
    from speechless_amd import alignment
    from speechless_amd.alignment import AsgAlignment
    n, t_b = 8191, 30000
    rng = np.random.RandomState(3)
    runs = np.ones(n, dtype=np.int64)
    np.add.at(runs, rng.randint(0, n, size=t_b - n), 1)
    path = np.concatenate([np.repeat(np.arange(n, dtype=np.int32), runs), np.full(9, -1, dtype=np.int32)])
    label = "".join("ab c"[i % 4] for i in range(n))
    passes = []
    original = np.flatnonzero

    def counted(x):
        passes.append(np.size(x))
        return original(x)
    monkeypatch.setattr(alignment.np, "flatnonzero", counted)
    a = AsgAlignment(label, [0] * n, -5.0, path)
    monkeypatch.undo()
    assert len(passes) <= 2 and sum(passes) <= 2 * path.size, len(passes)
    bounds = np.concatenate([[0], np.cumsum(runs)])
    assert a.grapheme_frames == [(int(lo), int(hi)) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert len(a.word_frames) == len(label.split())


def test_cut_sections_cuts_an_asg_alignment():
    from speechless_amd.alignment import cut_sections
    label = "aa bee sees three"  # runs of two: the encoded label is as long as the label, with repeat marks
    runs = [2, 1, 3, 1, 2, 1, 4, 1, 1, 2, 1, 5, 2, 1, 1, 1, 3]
    a, enc, encoded = make_alignment(label, runs, t_out=sum(runs) + 4)
    assert encoded.count(enc.asg_twice) == 4 and len(encoded) == len(runs)
    assert a.word_frames == [("aa", (0, 3)), ("bee", (6, 10)), ("sees", (14, 19)), ("three", (24, 32))]
    assert cut_sections(a, 100) == [(label, (0, 32))]
    assert cut_sections(a, 10) == [("aa bee", (0, 12)), ("sees", (12, 21)), ("three", (21, 32))]
    assert cut_sections(a, 3) == [("aa", (0, 4)), ("bee", (4, 12)), ("sees", (12, 21)), ("three", (21, 32))]
    infeasible, _, _ = make_alignment("aa b", [0, 0, 0, 0], score=-np.inf, t_out=3)
    assert cut_sections(infeasible, 10) == []


def test_longform_names_the_asg_limit():
    from speechless_amd import longform
    assert longform.ASG_ALIGN_MAX_LABEL == 8191
