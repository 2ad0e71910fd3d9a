"""sl_ctc_spot on the GPU: every output identical to the float32 restatement (tests/ctc_spot_ref.py) at both ends of every
instantiation's range, the hit picking at its edges, a cross-check against sl_ctc_align, its refusals, and end to end through
Engine and Wav2Letter.  Zero tolerance throughout the kernel's tests: the header defines the result bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest

from ctc_spot_ref import ctc_spot
from test_ctc_spot import spot_refusals
from test_gpu_ctc_segment import _label, _repeats

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
from fuzz_ctc import regime_logits  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 77
KINDS = ("learnt", "sharp", "uniform", "collapse", "one_hot")  # ("wrong" draws from the k - 2 other letters: none at k = 2)
# states per lane of ctc_spot_kernel<NJ> -> the q_max it serves (csrc/ctc_spot.hip: states_per_lane)
INSTANTIATIONS = {2: (1, 63), 4: (64, 127), 8: (128, 255), 16: (256, 511)}
PHRASE_LENGTHS = [1, 2, 63, 64, 127, 128, 255, 256, 511]


def gpu_logq(hip_lib, logits, eps=1e-8):
    """sl_softmax_logq of (B, T, K) logits -> logq numpy"""
    import torch
    b, t, k = logits.shape
    lg = torch.tensor(logits, dtype=torch.float32, device="cuda:0")
    probs = torch.zeros_like(lg)
    logq = torch.zeros_like(lg)
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return logq.cpu().numpy()


def one_hot_logq(rng, label, t, k):
    """frames that say the label somewhere with logq EXACTLY 0 at one symbol per frame -- runs of a letter, runs of blanks -- and
    -inf or -20 at the others: scores tie at 0 over whole runs, and states fall back to -inf"""
    seq = []
    for j, c in enumerate(label):
        if j and c == label[j - 1]:
            seq.append(k - 1)
        seq.append(int(c))
    symbols = np.full((t,), k - 1, dtype=np.int64)
    slack = max(t - len(seq) - 3, 0)  # frames to spend on longer runs and further blanks: the label fits where t allows it
    pos = int(rng.randint(0, 3)) if t >= len(seq) + 3 else 0
    for sym in seq:
        run = 1 + (int(rng.randint(0, 2)) if slack > 0 else 0)
        symbols[pos:pos + run] = sym
        gap = int(rng.randint(0, 2)) if slack >= run and sym != k - 1 else 0
        pos += run + gap
        slack -= run - 1 + gap
    logq = np.where(rng.rand(t, k) < 0.5, -np.inf, -20.0).astype(np.float32)
    logq[np.arange(t), symbols] = 0.0
    return logq


def run_spot_kernel(hip_lib, logq, input_len, queries, query_len, query_utt, min_score, max_hits, frames=True):
    """sl_ctc_spot on a (B, T, K) logq.  Every output has one query's worth of spare room behind it that starts from SENTINEL
    and is checked here.  Returns (frame_score, frame_begin, hits, hit_score, n_hits) numpy, the first two None without
    frames."""
    import torch
    dev = "cuda:0"
    b, t, k = logq.shape
    queries = np.ascontiguousarray(queries, dtype=np.int32)
    n, q_max = queries.shape
    lq = torch.tensor(logq, dtype=torch.float32, device=dev)
    il = torch.tensor(np.asarray(input_len), dtype=torch.int32, device=dev)
    qs = torch.tensor(queries, dtype=torch.int32, device=dev)
    ql = torch.tensor(np.asarray(query_len), dtype=torch.int32, device=dev)
    qu = torch.tensor(np.asarray(query_utt), dtype=torch.int32, device=dev)
    ms = torch.tensor(np.asarray(min_score, dtype=np.float32), dtype=torch.float32, device=dev)
    hits = torch.full((n + 1, max_hits, 2), SENTINEL, dtype=torch.int32, device=dev)
    hit_score = torch.full((n + 1, max_hits), float(SENTINEL), dtype=torch.float32, device=dev)
    n_hits = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev)
    frame_score = torch.full((n + 1, t), float(SENTINEL), dtype=torch.float32, device=dev)
    frame_begin = torch.full((n + 1, t), SENTINEL, dtype=torch.int32, device=dev)
    need = hip_lib.raw("sl_ctc_spot_workspace_bytes")(n, t, q_max)
    assert need == n * t * 8
    ws = torch.empty((need + 64,), dtype=torch.uint8, device=dev)
    ws[need:] = SENTINEL
    hip_lib.call("sl_ctc_spot", lq.data_ptr(), il.data_ptr(), qs.data_ptr(), ql.data_ptr(), qu.data_ptr(), ms.data_ptr(),
                 hits.data_ptr(), hit_score.data_ptr(), n_hits.data_ptr(), frame_score.data_ptr() if frames else None,
                 frame_begin.data_ptr() if frames else None, b, t, k, n, q_max, max_hits, ws.data_ptr(), need,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (frame_score, frame_begin, hits, hit_score, n_hits)]
    assert all(np.all(x[n:] == SENTINEL) for x in out) and torch.all(ws[need:] == SENTINEL).item()
    if not frames:
        assert np.all(out[0] == SENTINEL) and np.all(out[1] == SENTINEL)
    return [None if i < 2 and not frames else x[:n] for i, x in enumerate(out)]


def check_against_restatement(logq, input_len, queries, query_len, query_utt, min_score, max_hits, got, what=""):
    """zero tolerance: the bits of both float outputs and every integer"""
    ref = ctc_spot(logq, input_len, queries, query_len, query_utt, min_score, max_hits)
    names = ("frame_score", "frame_begin", "hits", "hit_score", "n_hits")
    for name, g, r in zip(names, got, ref):
        if g is None:
            continue
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name, g.shape, r.shape, g.dtype, r.dtype)
        same = g.view(np.uint32) == r.view(np.uint32) if g.dtype == np.float32 else g == r
        assert np.all(same), (what, name, np.argwhere(~same)[:5], g[~same][:5], r[~same][:5])
    print("spot {}: {} queries, {} hits, {} finite frames".format(what, len(ref[4]), int(ref[4].sum()),
                                                                  int(np.isfinite(ref[0]).sum())))
    return ref


def _instantiation_case(hip_lib, rng, n, k, nj):
    """Utterances whose labels have n letters with input_len 1, L + repeats - 1 (infeasible), L + repeats, 15, 16, 17, 33, 200, one
    above t_out and one below 0; per utterance its label as a query, and a few more"""
    labels = [_label(rng, n, k, nj) for _ in range(10)]
    input_len = [1, n + _repeats(labels[1]) - 1, n + _repeats(labels[2]), 15, 16, 17, 33, 200, 100000, -3]
    t_out = max(max(input_len[:8]) + 3, n + _repeats(labels[8]) + 9)
    logq = np.zeros((len(labels), t_out, k), dtype=np.float32)
    soft = []
    for b, label in enumerate(labels):
        kind = KINDS[(n + b + k) % len(KINDS)]
        if kind == "one_hot":
            logq[b] = one_hot_logq(rng, label, t_out, k)
        else:
            soft.append(b)
            logq[b] = regime_logits(rng, label, t_out, k, kind)
    logq[soft] = gpu_logq(hip_lib, logq[soft])
    queries, query_len, query_utt, min_score = [], [], [], []
    for b, label in enumerate(labels):
        queries.append(label)
        query_len.append(n if b % 2 else n + 5)  # (beyond q_max: clamped)
        query_utt.append(b)
        min_score.append(-np.inf if b % 3 else -1.5 * n)
    for b, count in ((3, 1), (4, min(n, 3)), (5, min(n, 2)), (6, min(n, 9)), (7, 1), (7, min(n, 3)), (8, min(n, 9)), (8, n // 2), (3, 0), (-1, n), (len(labels), n), (8, -2)):
        start = int(rng.randint(0, n - max(count, 0) + 1))
        part = labels[b % len(labels)][start:start + max(count, 0)]
        queries.append(part + [int(c) for c in rng.randint(0, k, size=n - len(part))])  # (anything behind the phrase)
        query_len.append(count)
        query_utt.append(b)
        min_score.append(-np.inf)
    return logq, input_len, np.array(queries, dtype=np.int32).reshape(len(queries), n), query_len, query_utt, min_score


def test_case_table_covers_the_dispatcher():
    bounds = sorted(v for lo_hi in INSTANTIATIONS.values() for v in lo_hi)
    assert bounds == [1, 63, 64, 127, 128, 255, 256, 511] and set(bounds) <= set(PHRASE_LENGTHS)
    assert all(2 * hi <= 64 * nj for nj, (_, hi) in INSTANTIATIONS.items())  # the filler and 2L - 1 states


@pytest.mark.parametrize("k", [2, 29, 64])
@pytest.mark.parametrize("n", PHRASE_LENGTHS)
def test_spot_at_every_instantiation(hip_lib, n, k):
    nj = next(nj for nj, (lo, hi) in INSTANTIATIONS.items() if lo <= n <= hi)
    rng = np.random.RandomState(1000 * n + k)
    case = _instantiation_case(hip_lib, rng, n, k, nj)
    got = run_spot_kernel(hip_lib, *case, 5)
    ref = check_against_restatement(*case, 5, got, "NJ={} L={} k={}".format(nj, n, k))
    frame_score, _, _, _, n_hits = ref
    assert np.all(frame_score[0, 1:] == -np.inf) and np.all(frame_score[1] == -np.inf) and np.all(frame_score[9] == -np.inf)
    assert np.isfinite(frame_score[8]).any() and n_hits[8] >= 1  # (input_len above t_out: the whole row)
    assert np.all(n_hits[-4:] == 0)  # no letters, utterances that are not there


def test_thresholds_and_max_hits(hip_lib):
    """thresholds that admit none, some and all of the frames, max_hits of 1 and of more than the hits that exist, null per-frame
    outputs, several queries per utterance and utterances of different lengths"""
    rng = np.random.RandomState(5)
    k, t_out = 29, 200
    phrases = [[int(c) for c in rng.randint(0, k - 1, size=m)] for m in (1, 2, 3, 5)]
    input_len = [200, 171, 64]
    logits = np.stack([regime_logits(rng, phrases[3] * 6, t_out, k, kind) for kind in ("learnt", "sharp", "uniform")])
    logq = gpu_logq(hip_lib, logits.astype(np.float32))
    queries = np.zeros((len(phrases) * 3, 5), dtype=np.int32)
    query_len, query_utt = [], []
    for i, (b, phrase) in enumerate((b, p) for b in range(3) for p in phrases):
        queries[i, :len(phrase)] = phrase
        query_len.append(len(phrase))
        query_utt.append(b)
    n = len(query_len)
    everything = [-np.inf] * n
    frame_score = ctc_spot(logq, input_len, queries, query_len, query_utt, everything, 1)[0]
    some = [float(np.median(row[np.isfinite(row)])) for row in frame_score]
    exists = 0
    for what, min_score in (("all", everything), ("some", some), ("none", [1.0] * n), ("the best", frame_score.max(axis=1))):
        for max_hits in (1, 64):
            case = (logq, input_len, queries, query_len, query_utt, min_score, max_hits)
            got = run_spot_kernel(hip_lib, *case)
            ref = check_against_restatement(*case, got, "{} max_hits={}".format(what, max_hits))
            without = run_spot_kernel(hip_lib, *case, frames=False)
            check_against_restatement(*case, without, "{} max_hits={} without frames".format(what, max_hits))
            n_hits = ref[4]
            if what == "none":
                assert np.all(n_hits == 0)
            elif max_hits == 1:
                assert np.all(n_hits == 1)
            else:
                assert np.all(n_hits >= 1)
                exists += int((n_hits < 64).sum())
    assert exists > 0  # more slots than hits


def test_every_hit_scores_what_the_aligner_scores_on_its_frames(hip_lib):
    """sl_ctc_align of the phrase over a copy of each hit's frames returns the hit's score bit for bit: the aligner's leading
    and trailing blank can only lower a left-to-right fp32 sum (rounded addition is monotonic)"""
    import torch
    rng = np.random.RandomState(9)
    k, t_out, batch = 29, 160, 4
    phrases = [_label(rng, m, k, 2) for m in (1, 2, 4, 7, 12)]
    input_len = [160, 150, 97, 33]
    kinds = ("learnt", "sharp", "uniform", "learnt")
    logits = np.stack([regime_logits(rng, sum(phrases, []) * 2, t_out, k, kind) for kind in kinds]).astype(np.float32)
    logq = gpu_logq(hip_lib, logits)
    queries = np.zeros((batch * len(phrases), 12), dtype=np.int32)
    query_len, query_utt = [], []
    for i, (b, phrase) in enumerate((b, p) for b in range(batch) for p in phrases):
        queries[i, :len(phrase)] = phrase
        query_len.append(len(phrase))
        query_utt.append(b)
    case = (logq, input_len, queries, query_len, query_utt, [-np.inf] * len(query_len), 6)
    got = run_spot_kernel(hip_lib, *case)
    check_against_restatement(*case, got, "random batch")
    _, _, hits, hit_score, n_hits = got
    spans = [(q, int(first), int(end), hit_score[q, h]) for q in range(len(query_len)) for h, (first, end) in
             enumerate(hits[q, :n_hits[q]])]
    assert len(spans) > 60
    frames = max(end - first for _, first, end, _ in spans)
    cut = np.zeros((len(spans), frames, k), dtype=np.float32)
    labels = np.zeros((len(spans), 12), dtype=np.int32)
    for i, (q, first, end, _) in enumerate(spans):
        cut[i, :end - first] = logq[query_utt[q], first:end]
        labels[i] = queries[q]
    dev = "cuda:0"
    lq, lab = torch.tensor(cut, device=dev), torch.tensor(labels, device=dev)
    ll = torch.tensor([query_len[q] for q, _, _, _ in spans], dtype=torch.int32, device=dev)
    il = torch.tensor([end - first for _, first, end, _ in spans], dtype=torch.int32, device=dev)
    path = torch.zeros((len(spans), frames), dtype=torch.int32, device=dev)
    score = torch.zeros((len(spans),), dtype=torch.float32, device=dev)
    need = hip_lib.raw("sl_ctc_align_workspace_bytes")(len(spans), frames, 12)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_ctc_align", lq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(),
                 len(spans), frames, k, 12, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    aligned = score.cpu().numpy()
    expected = np.array([s for _, _, _, s in spans], dtype=np.float32)
    different = np.flatnonzero(aligned.view(np.uint32) != expected.view(np.uint32))
    print("aligner against hits: {} hits, {} differ".format(len(spans), len(different)), aligned[different], expected[different])
    assert len(different) == 0


def test_refusals_on_host_pointers(hip_lib):
    spot_refusals(hip_lib)


# ---------------------------------------------------------------------------------------------- Engine and Wav2Letter
PHRASES = ["she", "a", "quiet zoo", "see"]


def _net():
    from test_gpu_longform import _net as longform_net
    return longform_net("f16x3")


def _check_hits(found, phrases, hits, scores, counts, posteriors=None):
    """one example's PhraseHit lists against rows of Engine.ctc_spot (and of a direct ctc_segment_scores call)"""
    assert len(found) == len(phrases)
    total = 0
    for p, (phrase, row) in enumerate(zip(phrases, found)):
        assert len(row) == counts[p]
        for h, hit in enumerate(row):
            assert (hit.phrase, hit.first, hit.end) == (phrase, hits[p, h, 0], hits[p, h, 1])
            assert np.float32(hit.log_probability) == scores[p, h]
            frames = hit.end - hit.first
            assert hit.seconds(0.02) == (hit.first * 0.02, hit.end * 0.02)
            if posteriors is None:
                assert np.isnan(hit.log_posterior) and np.isnan(hit.confidence())
            else:
                assert np.float32(hit.log_posterior) == posteriors[total]
                # the sum over all paths of the frames holds the best one
                assert hit.log_posterior >= hit.log_probability - 1e-6 * (frames + abs(hit.log_probability))
                assert 0.0 <= hit.confidence() <= 1.0 + 1e-6 * frames
            total += 1
    return total


def test_find_phrases_batch_end_to_end():
    from test_gpu_ctc_segment import _batch
    net = _net()
    engine = net.eval_engine
    rng = np.random.RandomState(21)
    batch = _batch(rng, 3, 301)
    found = net.find_phrases_batch(batch, PHRASES, max_hits=4)
    assert len(found) == 3
    encoded = net.grapheme_encoding.encode_label_batch(PHRASES)
    lengths = [len(p) for p in PHRASES]
    count = len(PHRASES)
    frames = [x.z_normalized_transposed_spectrogram().shape[0] // net.input_to_prediction_length_ratio for x in batch]
    hits, scores, counts = engine.ctc_spot(np.tile(encoded, (3, 1)), lengths * 3, np.repeat(np.arange(3), count),
                                           [-np.inf] * (3 * count), 4, frames)
    assert counts.min() >= 1  # random weights: every phrase has some finite reading
    logq = engine.cur.logq.cpu().numpy()
    restated = ctc_spot(logq, frames, np.tile(encoded, (3, 1)), lengths * 3, np.repeat(np.arange(3), count), [-np.inf] * 12, 4)
    assert np.array_equal(hits, restated[2]) and np.array_equal(scores, restated[3]) and np.array_equal(counts, restated[4])
    starts = np.concatenate([[0], np.cumsum(lengths)])
    label_batch = np.tile(np.concatenate([encoded[p, :n] for p, n in enumerate(lengths)]), (3, 1))
    for b in range(3):
        rows = slice(b * count, (b + 1) * count)
        segments = [(b, hits[q, h, 0], hits[q, h, 1], starts[q % count], starts[q % count + 1])
                    for q in range(b * count, (b + 1) * count) for h in range(counts[q])]
        posteriors = engine.ctc_segment_scores(label_batch, np.array(segments, dtype=np.int64))
        assert _check_hits(found[b], PHRASES, hits[rows], scores[rows], counts[rows], posteriors) == len(segments)
    # without confidence: the same hits, no posterior; a threshold per letter drops what lies below it times the length
    plain = net.find_phrases_batch(batch, PHRASES, max_hits=4, with_confidence=False)
    for b in range(3):
        rows = slice(b * count, (b + 1) * count)
        _check_hits(plain[b], PHRASES, hits[rows], scores[rows], counts[rows])
    per_letter = float(np.median([hit.log_probability / len(hit.phrase) for rows in found for row in rows for hit in row]))
    kept = net.find_phrases_batch(batch, PHRASES, max_hits=4, min_log_probability_per_letter=per_letter, with_confidence=False)
    for rows, all_rows in zip(kept, found):
        for phrase, row, all_row in zip(PHRASES, rows, all_rows):
            bound = np.float32(per_letter) * np.int32(len(phrase))
            assert all(np.float32(hit.log_probability) >= bound for hit in row)
            assert [(h.first, h.end) for h in row] == [(h.first, h.end) for h in all_row
                                                      if np.float32(h.log_probability) >= bound][:len(row)]
    assert 0 < sum(len(row) for rows in kept for row in rows) < sum(len(row) for rows in found for row in rows)


def test_find_phrases_in_recording_matches_the_single_pass():
    from speechless_amd.net import LabeledSpectrogram
    from test_gpu_longform import WINDOW, _Example, _recording
    net = _net()
    x = _recording(1400, seed=7)  # three windows of 512, and short enough for one forward pass
    single = net.find_phrases_batch([LabeledSpectrogram(id="r", label="", spectrogram=x)], PHRASES, max_hits=6)[0]
    windows = net.find_phrases_in_recording(_Example(x, ""), PHRASES, max_hits=6, window_input_frames=WINDOW)
    assert len(windows) == len(PHRASES) and sum(len(row) for row in windows) > len(PHRASES)
    for row, expected in zip(windows, single):
        assert [(h.phrase, h.first, h.end, h.log_probability) for h in row] == \
            [(h.phrase, h.first, h.end, h.log_probability) for h in expected]
        for hit, other in zip(row, expected):
            assert abs(hit.log_posterior - other.log_posterior) <= 2e-6 * (hit.end - hit.first + abs(other.log_posterior))
    # the engine's checks name the first bad query
    engine = net.eval_engine
    with pytest.raises(ValueError, match="query 1: length 0"):
        engine.ctc_spot(np.zeros((2, 3), dtype=np.int32), [3, 0], [0, 0], [-np.inf] * 2, 4)
    with pytest.raises(ValueError, match="query 0: .*utterance 5"):
        engine.ctc_spot(np.zeros((1, 3), dtype=np.int32), [3], [5], [-np.inf], 4)
    with pytest.raises(ValueError, match=r"query 0 holds an index outside \[0, 28\)"):
        engine.ctc_spot(np.full((1, 3), 28, dtype=np.int32), [3], [0], [-np.inf], 4)
    with pytest.raises(ValueError, match="max_hits = 65"):
        engine.ctc_spot(np.zeros((1, 3), dtype=np.int32), [3], [0], [-np.inf], 65)
    with pytest.raises(ValueError, match="at most 511"):
        engine.ctc_spot(np.zeros((1, 512), dtype=np.int32), [3], [0], [-np.inf], 4)


def test_find_phrases_refusals():
    from speechless_amd import Wav2Letter, english_frequent_characters
    from test_gpu_longform import LAYER_SIZES, _Example, _recording
    x = _recording(300)
    asg = Wav2Letter(128, english_frequent_characters, seed=1, layer_sizes=LAYER_SIZES, criterion="asg")
    for call in (lambda: asg.find_phrases_batch([_Example(x, "abc")], ["abc"]),
                 lambda: asg.find_phrases_in_recording(_Example(x, "abc"), ["abc"]),
                 lambda: asg.engine.ctc_spot(np.zeros((1, 3), dtype=np.int32), [3], [0], [-np.inf], 4)):
        with pytest.raises(ValueError, match="criterion='asg'"):
            call()
    net = _net()
    for call in (net.find_phrases_batch, net.find_phrases_in_recording):
        example = _Example(x, "abc")
        with pytest.raises(ValueError, match="empty phrase"):
            call([example] if call == net.find_phrases_batch else example, ["abc", ""])
        with pytest.raises(ValueError, match="512 letters.*at most 511"):
            call([example] if call == net.find_phrases_batch else example, ["a" * 512])
        with pytest.raises(ValueError, match="Unexpected char"):
            call([example] if call == net.find_phrases_batch else example, ["abc", "a#c"])
    wave = Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, seed=1, layer_sizes=LAYER_SIZES)
    with pytest.raises(ValueError, match="use_raw_wave_input=True is not supported .*out of scope"):
        wave.find_phrases_in_recording(_Example(x[:, :1], "abc"), ["abc"])
