"""CTC phrase search without a GPU: the float32 restatement of sl_ctc_spot (tests/ctc_spot_ref.py) against the brute force over all
frame labelings, hand-derived tie cases, the properties of the hit picking, a planted phrase, and the entry point's refusals on
the host."""
import numpy as np
import pytest

from ctc_spot_ref import brute_force_scores, ctc_spot, pick_hits, spot_frames

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED, SL_ERR_WORKSPACE_TOO_SMALL = -1, -2, -3


def _log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def _one_hot_logq(symbols, k):
    """logq that is exactly 0 at each frame's symbol and -inf elsewhere"""
    logq = np.full((len(symbols), k), -np.inf, dtype=np.float32)
    logq[np.arange(len(symbols)), symbols] = 0.0
    return logq


def _brute_cases():
    rng = np.random.RandomState(2024)
    cases = []
    for i in range(72):
        k = 2 + i % 2
        t = 1 + (i // 2) % 6
        n = 1 + (i // 12) % 3
        phrase = [int(c) for c in rng.randint(0, k - 1, size=n)]
        if i % 5 == 0 and n >= 2:
            phrase[1] = phrase[0]  # a repeated letter (always, at k = 2)
        scale = (0.01, 1.0, 8.0)[i % 3]
        cases.append((k, t, phrase, _log_softmax(scale * rng.randn(t + 1, k)), t if i % 4 else t + 1))
    return cases


def test_restatement_equals_the_brute_force_bit_for_bit():
    mismatches, finite = 0, 0
    for k, t, phrase, logq, t_b in _brute_cases():
        score, begin = spot_frames(logq, phrase, t_b)
        brute = brute_force_scores(logq, phrase, t_b)
        mismatches += int((score.view(np.uint32) != brute.view(np.uint32)).sum())
        finite += int(np.isfinite(brute).sum())
        assert np.all(score[t_b:] == -np.inf) and np.all(begin[t_b:] == -1)
        assert np.all((begin >= 0) == np.isfinite(score))
        # the begin tag is a begin of that score: the best labeling of exactly the frames begin .. t scores the same
        for end in np.flatnonzero(np.isfinite(score)):
            b = int(begin[end])
            assert 0 <= b <= end
            assert brute_force_scores(logq[b:end + 1], phrase, end + 1 - b)[-1] == score[end]
    assert mismatches == 0 and finite > 100


def test_one_hot_ties_a_blank_run_does_not_extend_the_begin_and_a_first_letter_run_does():
    k, a, b, blank = 3, 0, 1, 2
    # blank blank a b: the span starts on the letter frame 2 (there is no leading blank state)
    score, begin = spot_frames(_one_hot_logq([blank, blank, a, b], k), [a, b], 4)
    assert score.tolist() == [-np.inf, -np.inf, -np.inf, 0.0] and begin.tolist() == [-1, -1, -1, 2]
    # a a a b: staying in the first letter ties with a fresh start from the filler at 0 == 0, and the earlier candidate -- stay --
    # keeps it, so the begin is the first frame of the run
    score, begin = spot_frames(_one_hot_logq([a, a, a, b], k), [a, b], 4)
    assert score.tolist() == [-np.inf, -np.inf, -np.inf, 0.0] and begin.tolist() == [-1, -1, -1, 0]
    # one letter: every frame of the run ends an occurrence that began at the run's first frame
    score, begin = spot_frames(_one_hot_logq([blank, a, a, blank, a], k), [a], 5)
    assert score.tolist() == [-np.inf, 0.0, 0.0, -np.inf, 0.0] and begin.tolist() == [-1, 1, 1, -1, 4]
    # a blank a says "aa" and "a a" alike; without the blank the repeated letter cannot be said
    score, begin = spot_frames(_one_hot_logq([a, blank, a], k), [a, a], 3)
    assert score.tolist() == [-np.inf, -np.inf, 0.0] and begin.tolist() == [-1, -1, 0]
    score, _ = spot_frames(_one_hot_logq([a, a, a], k), [a, a], 3)
    assert np.all(score == -np.inf)
    # the inner blank between DIFFERENT letters is optional, and a trailing blank frame ends nothing
    score, begin = spot_frames(_one_hot_logq([a, blank, blank, b, blank], k), [a, b], 5)
    assert score.tolist() == [-np.inf, -np.inf, -np.inf, 0.0, -np.inf] and begin.tolist() == [-1, -1, -1, 0, -1]
    # frames at and beyond t_b, an empty phrase, and letters clamped into [0, k) (the skip rule compares them as given)
    score, begin = spot_frames(_one_hot_logq([a, b, a, b], k), [a, b], 2)
    assert score.tolist() == [-np.inf, 0.0, -np.inf, -np.inf] and begin.tolist() == [-1, 0, -1, -1]
    assert np.all(spot_frames(_one_hot_logq([a, b], k), [], 2)[0] == -np.inf)
    score, begin = spot_frames(_one_hot_logq([a, a], k), [-5, -7], 2)  # both read column 0, and differ: no blank needed
    assert score.tolist() == [-np.inf, 0.0] and begin.tolist() == [-1, 0]


def _check_picking(score, begin, threshold, max_hits):
    hits, hit_score, n = pick_hits(score, begin, threshold, max_hits)
    assert np.all(hits[n:] == -1) and np.all(hit_score[n:] == -np.inf)
    spans = [tuple(h) for h in hits[:n]]
    for i, (first, end) in enumerate(spans):
        assert 0 <= first < end <= len(score) and begin[end - 1] == first and score[end - 1] == hit_score[i]
        assert hit_score[i] >= threshold and np.isfinite(hit_score[i])
        for other_first, other_end in spans[:i]:
            assert end <= other_first or other_end <= first
    assert np.all(np.diff(hit_score[:n]) <= 0)
    if n < max_hits:  # nothing above the threshold is left that no hit overlaps
        for u in range(len(score)):
            if score[u] > -np.inf and score[u] >= threshold:
                assert any(begin[u] < end and first <= u for first, end in spans), u
    return spans


def test_picking_properties_on_random_frames():
    rng = np.random.RandomState(7)
    for case in range(40):
        k = 3 + case % 3
        t = 20 + 7 * case
        phrase = [int(c) for c in rng.randint(0, k - 1, size=1 + case % 4)]
        logq = _log_softmax((1.0 + case % 5) * rng.randn(t, k))
        score, begin = spot_frames(logq, phrase, t)
        finite = np.sort(score[np.isfinite(score)])
        for threshold in (-np.inf, float(finite[len(finite) // 2]), float(finite[-1]), 1.0):
            for max_hits in (1, 3, 64):
                spans = _check_picking(score, begin, threshold, max_hits)
                assert (len(spans) == 0) == (threshold == 1.0)
    # equal scores: the smallest frame first
    hits, hit_score, n = pick_hits(np.array([-1.0, -0.5, -0.5, -0.5], dtype=np.float32), np.array([0, 1, 2, 3]), -np.inf, 8)
    assert n == 4 and hits[:4].tolist() == [[1, 2], [2, 3], [3, 4], [0, 1]]


def test_a_planted_phrase_is_found_at_both_places():
    rng = np.random.RandomState(11)
    k, t = 29, 120
    phrase = [7, 4, 11, 11, 14]  # h e l l o
    logits = rng.randn(t, k).astype(np.float64)
    logits[:, k - 1] += 6.0
    spans = []
    for start in (17, 80):
        frame = start
        for c in phrase:  # one frame per letter and a blank frame behind it (every further frame of a span costs score)
            logits[frame, k - 1] -= 6.0
            logits[frame, c] += 12.0
            frame += 2
        spans.append((start, frame - 1))
    logq = _log_softmax(logits)
    _, _, hits, hit_score, n_hits = ctc_spot(logq[None], [t], np.array([phrase + [0, 0]]), [5], [0], [-np.inf], 4)
    assert n_hits[0] >= 2 and sorted(map(tuple, hits[0, :2])) == spans
    print("planted", hit_score[0, :2], "others", hit_score[0, 2:])
    # nine frames at their most likely symbol, which stands 6 or more above 28 standard normal logits; elsewhere every letter
    # of the phrase stands against a blank that is 6 above it on average
    assert np.all(hit_score[0, :2] > -1.0) and np.all(hit_score[0, 2:] < -10.0)
    _, _, hits, _, n_hits = ctc_spot(logq[None], [t], np.array([phrase + [0, 0]]), [5], [0], [-5.0], 4)
    assert n_hits[0] == 2 and sorted(map(tuple, hits[0, :2])) == spans and np.all(hits[0, 2:] == -1)
    # a query of an utterance that is not there, and one without letters, find nothing
    _, _, _, _, n_hits = ctc_spot(logq[None], [t], np.array([phrase, phrase, phrase]), [5, 5, 0], [1, -1, 0], [-np.inf] * 3, 4)
    assert n_hits.tolist() == [0, 0, 0]


def spot_refusals(hip_lib):
    """every refusal of sl_ctc_spot, on host pointers: nothing may be launched, and the outputs stay as they were"""
    size = hip_lib.raw("sl_ctc_spot_workspace_bytes")
    assert size(1, 1, 1) == 8 and size(660, 500, 12) == 660 * 500 * 8 and size(1024, 30000, 511) == 1024 * 30000 * 8
    assert all(size(*bad) == 0 for bad in ((0, 10, 5), (3, 0, 5), (3, 10, 0), (3, 10, 512), (-1, 10, 5)))
    assert all(size(n, t, q) <= size(n + 1, t, q) and size(n, t, q) <= size(n, t + 1, q) and size(n, t, q) <= size(n, t, q + 1)
               for n in (1, 7) for t in (1, 500) for q in (1, 63, 510))
    spot = hip_lib.raw("sl_ctc_spot")
    out = np.full((64,), 123, dtype=np.int32)
    buf = np.zeros((64,), dtype=np.int32).ctypes.data  # a valid host address: nothing may be launched on it
    ok = [buf] * 6 + [out.ctypes.data] * 3 + [None, None]
    names = ("logq", "input_len", "queries", "query_len", "query_utt", "min_score", "hits", "hit_score", "n_hits")
    ws = size(2, 10, 5)

    def call(args=ok, batch=1, t_out=10, k=29, n_queries=2, q_max=5, max_hits=4, workspace=buf, nbytes=ws):
        return spot(*args, batch, t_out, k, n_queries, q_max, max_hits, workspace, nbytes, None)

    for bad, text in ((dict(k=65), "k = 65"), (dict(k=1), "k = 1"), (dict(q_max=512), "q_max = 512"), (dict(q_max=0), "q_max = 0"),
                      (dict(max_hits=65), "max_hits = 65"), (dict(max_hits=0), "max_hits = 0"),
                      (dict(n_queries=0), "n_queries >= 1")):
        assert call(**bad) == SL_ERR_UNSUPPORTED and text in hip_lib.last_error()
    for i, name in enumerate(names):
        args = list(ok)
        args[i] = None
        assert call(args) == SL_ERR_INVALID_ARGUMENT and name + " is a null pointer" in hip_lib.last_error()
    assert call(batch=0) == SL_ERR_INVALID_ARGUMENT and call(t_out=0) == SL_ERR_INVALID_ARGUMENT
    assert call(nbytes=ws - 1) == SL_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in hip_lib.last_error()
    assert call(workspace=None) == SL_ERR_WORKSPACE_TOO_SMALL
    # unsupported shapes come before invalid arguments
    assert spot(*([None] * 11), 0, 0, 65, 2, 5, 4, None, 0, None) == SL_ERR_UNSUPPORTED
    assert np.all(out == 123)


def test_entry_point_host_side_checks(hip_lib):
    spot_refusals(hip_lib)


def test_query_check_names_the_first_bad_query():
    from speechless_amd.engine_decode import check_queries
    good = dict(queries=np.zeros((3, 4), dtype=np.int64), lengths=[4, 1, 2], utterances=[0, 1, 1], min_scores=[-np.inf, -2.0, 0.0],
                max_hits=4, batch=2, n_labels=28)
    queries, lengths, utterances, thresholds, max_hits = check_queries(**good)
    assert queries.dtype == lengths.dtype == utterances.dtype == np.int32 and thresholds.dtype == np.float32
    assert queries.shape == (3, 4) and queries.flags["C_CONTIGUOUS"] and max_hits == 4
    for bad, text in ((dict(lengths=[4, 0, 2]), "query 1: length 0"), (dict(lengths=[4, 1, 5]), "query 2: length 5"),
                      (dict(utterances=[0, 2, 1]), "query 1: .*utterance 2"), (dict(utterances=[-1, 1, 1]), "query 0: .*utterance -1"),
                      (dict(min_scores=[0.0, 0.0, np.nan]), "query 2: .*threshold nan"), (dict(max_hits=0), "max_hits = 0"),
                      (dict(max_hits=65), "max_hits = 65"), (dict(lengths=[4, 1]), "N lengths"),
                      (dict(queries=np.zeros((3, 512), dtype=np.int32)), "at most 511"),
                      (dict(queries=np.zeros((3, 4), dtype=np.float32)), r"\(N, Qmax\)"),
                      (dict(queries=np.zeros((0, 4), dtype=np.int32)), r"\(N, Qmax\)"),
                      (dict(queries=np.full((3, 4), 28)), r"query 0 holds an index outside \[0, 28\)")):
        with pytest.raises(ValueError, match=text):
            check_queries(**dict(good, **bad))
    # what lies behind a query's length is not looked at
    padded = np.full((3, 4), -1)
    padded[0], padded[1, 0], padded[2, :2] = 5, 6, 7
    assert check_queries(**dict(good, queries=padded))[0].tolist() == padded.tolist()


def test_phrase_hit():
    from speechless_amd import PhraseHit
    hit = PhraseHit("abc", 3, 9, -1.5, np.log(0.25))
    assert (hit.phrase, hit.first, hit.end, hit.log_probability) == ("abc", 3, 9, -1.5)
    assert hit.confidence() == pytest.approx(0.25) and hit.seconds(0.5) == (1.5, 4.5)
    assert hit == PhraseHit("abc", 3, 9, -1.5, np.log(0.25)) and hit != PhraseHit("abc", 3, 10, -1.5, np.log(0.25))
    plain = PhraseHit("abc", 3, 9, -1.5)
    assert np.isnan(plain.log_posterior) and np.isnan(plain.confidence()) and plain == PhraseHit("abc", 3, 9, -1.5)
    assert "abc" in repr(hit)


def test_spot_symbols_are_exported():
    from speechless_amd import _lib
    assert "sl_ctc_spot" in _lib.SIGNATURES and "sl_ctc_spot_workspace_bytes" in _lib.SIGNATURES
