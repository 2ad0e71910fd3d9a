"""sl_ctc_segment_scores on the GPU: against the float64 restatement (tests/ctc_segment_ref.py) at both ends of every
instantiation's range, against minus the CTC loss, its refusals, and end to end through Engine and Wav2Letter.

Tolerance against the restatement: 1e-6 * (frames + |reference|) nats per segment.  A log-sum-exp step passes on at most the
largest error of its inputs (its derivatives are weights that sum to 1) and adds the error of the fp32 exp2 / log2 of a sum in
[1, 3], which is below 1e-6; the lattice values themselves are doubles.  The second term covers the float32 result (2^-24 = 6e-8
relative).  -inf must match exactly.  Every comparison prints its worst |error| / bound before it asserts."""
import sys
from pathlib import Path

import numpy as np
import pytest

from ctc_segment_ref import forward_score, segment_frames, segment_scores

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
from fuzz_ctc import regime_logits  # noqa: E402

pytestmark = pytest.mark.gpu

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED = -1, -2
SENTINEL = 123.0
KINDS = ("learnt", "sharp", "uniform", "collapse")  # ("wrong" draws from the k - 2 other letters: none at k = 2)
# states per lane of ctc_segment_kernel<NJ> -> the seg_l_max it serves (csrc/ctc_segment.hip: states_per_lane)
INSTANTIATIONS = {2: (0, 63), 4: (64, 127), 8: (128, 255), 16: (256, 511)}


def run_segment_kernel(hip_lib, logits, labels, input_len, segments, seg_l_max, eps=1e-8, spare=3):
    """logq from sl_softmax_logq, then sl_ctc_segment_scores into an output of n + spare floats that start from SENTINEL.
    Returns (logq numpy, the n results numpy); the spare entries are checked here."""
    import torch
    b, t, k = logits.shape
    dev = "cuda:0"
    labels = np.asarray(labels, dtype=np.int32)
    assert labels.ndim == 2 and labels.shape[0] == b
    segments = np.ascontiguousarray(segments, dtype=np.int32).reshape(-1, 5)
    n = segments.shape[0]
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.zeros((b, t, k), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    lab = torch.tensor(labels if labels.size else np.zeros((b, 1), dtype=np.int32), dtype=torch.int32, device=dev)
    il = torch.tensor(np.asarray(input_len), dtype=torch.int32, device=dev)
    sg = torch.tensor(segments, dtype=torch.int32, device=dev)
    out = torch.full((n + spare,), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    need = hip_lib.raw("sl_ctc_segment_scores_workspace_bytes")(n, seg_l_max)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_ctc_segment_scores", logq.data_ptr(), lab.data_ptr(), il.data_ptr(), sg.data_ptr(), out.data_ptr(), b, t, k,
                 labels.shape[1], n, seg_l_max, ws.data_ptr(), need, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    return logq.cpu().numpy(), got[:n]


def check_against_restatement(logq, labels, input_len, segments, seg_l_max, got, what=""):
    """the module's tolerance, segment by segment; returns the worst |error| / bound"""
    labels = np.asarray(labels)
    ref = segment_scores(logq, labels, input_len, segments, seg_l_max)
    frames = segment_frames(segments, input_len, logq.shape[1], labels.shape[1], seg_l_max, logq.shape[0])
    finite = np.isfinite(ref)
    assert np.array_equal(got[~finite], ref[~finite].astype(np.float32)), (what, got[~finite], ref[~finite])
    assert np.all(np.isfinite(got[finite]))
    bound = 1e-6 * (frames[finite] + np.abs(ref[finite]))
    zero = bound == 0  # (T = 0 and L = 0: exactly 0)
    assert np.all(got[finite][zero] == 0.0)
    ratio = np.abs(got[finite][~zero].astype(np.float64) - ref[finite][~zero]) / bound[~zero]
    worst = float(ratio.max()) if ratio.size else 0.0
    print("segment scores {}: {} segments ({} -inf), worst |error| / bound {:.3e}, most negative score {:.1f}".format(
        what, len(ref), int((~finite).sum()), worst, float(ref[finite].min()) if finite.any() else 0.0))
    assert worst <= 1.0, (what, worst)
    return worst


def _repeats(label):
    return sum(1 for i in range(1, len(label)) if label[i] == label[i - 1])


def _label(rng, n, k, nj):
    """n random letters, with adjacent equal letters across and inside lane boundaries (a lane holds nj / 2 letters)"""
    label = [int(c) for c in rng.randint(0, k - 1, size=n)]
    per_lane = max(nj // 2, 1)
    for p in range(per_lane, n, 3 * per_lane):  # the first letter of a lane equals the last of the lane below
        label[p] = label[p - 1]
    for p in range(2 * per_lane + 1, n, 5 * per_lane):  # and a pair just behind a boundary
        label[p] = label[p - 1]
    return label


def _instantiation_case(rng, seg_l_max, k, nj):
    """B = 3 utterances whose labels have seg_l_max letters, T_b = L + repeats + slack for slack 0 / 1 / 17, t_out 3 frames
    more; the segments of the issue's list, all in one launch"""
    n = seg_l_max
    labels_list = [_label(rng, n, k, nj) for _ in range(3)]
    input_len = [n + _repeats(l) + slack for l, slack in zip(labels_list, (0, 1, 17))]
    t_out = max(input_len) + 3
    logits = np.zeros((3, t_out, k), dtype=np.float32)
    for b in range(3):
        kind = KINDS[(seg_l_max + b + k) % len(KINDS)]
        logits[b] = regime_logits(rng, labels_list[b], t_out, k, kind)
    labels = np.array(labels_list, dtype=np.int32).reshape(3, n)
    segments = [(-1, 0, 5, 0, min(n, 1)), (3, 0, 5, 0, min(n, 1))]  # b out of range
    for b in range(3):
        tb, lab = input_len[b], labels_list[b]
        segments += [
            (b, 0, tb, 0, n),                      # the whole utterance: frame 0 and the last frame
            (b, 0, t_out + 5, 0, n + 100),         # both ranges beyond their ends: clamped to the same
            (b, tb, t_out, 0, min(n, 3)),          # frames past input_len: clamped away
            (b, min(3, tb), min(20, tb), 1, 1),    # L = 0: the blanks' sum
            (b, 2, 2, 0, 0),                       # L = 0 and T = 0
        ]
        if n >= 1:
            segments.append((b, 0, n + _repeats(lab) - 1, 0, n))  # one frame short: infeasible
        # parts of the label over parts of the frames, neither begin nor length a multiple of 16
        for begin, count, first, spare in ((n // 3, n // 2, 5, 7), (1, min(n - 1, 9), 3, 2), (n - min(n, 5), min(n, 5), 1, 21)):
            if count < 1 or begin < 0:
                continue
            part = lab[begin:begin + count]
            end = min(first + len(part) + _repeats(part) + spare, tb)
            segments.append((b, first, end, begin, begin + count))  # (infeasible where the frames run out: -inf on both sides)
            segments.append((b, tb - (end - first), tb, begin, begin + count))  # the same up against the last frame
    return logits, labels, input_len, np.array(segments, dtype=np.int64)


def test_case_table_covers_the_dispatcher():
    bounds = sorted(v for lo_hi in INSTANTIATIONS.values() for v in lo_hi)
    assert bounds == [0, 63, 64, 127, 128, 255, 256, 511]
    assert all(2 * hi + 1 <= 64 * nj < 2 * (2 * hi + 1) + 2 for nj, (_, hi) in INSTANTIATIONS.items())


@pytest.mark.parametrize("k", [2, 29, 64])
@pytest.mark.parametrize("bound", [0, 1], ids=["lower", "upper"])
@pytest.mark.parametrize("nj", sorted(INSTANTIATIONS))
def test_segment_scores_at_every_instantiation(hip_lib, nj, bound, k):
    seg_l_max = INSTANTIATIONS[nj][bound]
    rng = np.random.RandomState(1000 * nj + 10 * k + bound)
    logits, labels, input_len, segments = _instantiation_case(rng, seg_l_max, k, nj)
    logq, got = run_segment_kernel(hip_lib, logits, labels, input_len, segments, seg_l_max)
    ref = segment_scores(logq, labels, input_len, segments, seg_l_max)
    assert np.isfinite(ref[2]) and ref[0] == ref[1] == -np.inf  # (the whole first utterance is feasible; b out of range)
    check_against_restatement(logq, labels, input_len, segments, seg_l_max, got, "NJ={} seg_l_max={} k={}".format(nj, seg_l_max, k))
    assert got[2] == got[3]  # the clamped ranges are the whole utterance


def test_three_hundred_one_word_segments_in_one_launch(hip_lib):
    """words of 1 .. 9 letters anywhere in three utterances, the smallest instantiation, several launches' worth of waves"""
    rng = np.random.RandomState(300)
    k, t_out, l_max = 29, 237, 150
    labels = rng.randint(0, k - 1, size=(3, l_max)).astype(np.int32)
    labels[:, 10::7] = labels[:, 9::7][:, :labels[:, 10::7].shape[1]]  # adjacent equal letters here and there
    input_len = [237, 200, 101]
    logits = np.stack([regime_logits(rng, list(labels[b]), t_out, k, kind) for b, kind in enumerate(("learnt", "sharp", "uniform"))])
    segments = []
    for _ in range(300):
        b = int(rng.randint(0, 3))
        letters = int(rng.randint(1, 10))
        l0 = int(rng.randint(0, l_max - letters + 1))
        f0 = int(rng.randint(0, input_len[b] - 2))
        segments.append((b, f0, min(f0 + letters + int(rng.randint(0, 40)), t_out), l0, l0 + letters))
    segments = np.array(segments, dtype=np.int64)
    logq, got = run_segment_kernel(hip_lib, logits.astype(np.float32), labels, input_len, segments, 9)
    assert np.isfinite(got).sum() > 200
    check_against_restatement(logq, labels, input_len, segments, 9, got, "300 words")
    # a seg_l_max below a segment's span cuts the span: the same launch at seg_l_max = 4
    logq, got = run_segment_kernel(hip_lib, logits.astype(np.float32), labels, input_len, segments, 4)
    check_against_restatement(logq, labels, input_len, segments, 4, got, "300 words cut to 4 letters")


def test_long_segment_far_into_a_recording(hip_lib):
    """2000 frames and 300 letters in one segment that starts at frame 1003 of 3100: the score is far below what fp32 lattice
    values could hold to the bound"""
    rng = np.random.RandomState(2000)
    k, t_out, n = 29, 3100, 300
    label = _label(rng, n, k, 16)
    labels = np.array([label + [0] * 11], dtype=np.int32)
    logits = (6.0 * rng.randn(1, t_out, k)).astype(np.float32)
    segments = np.array([(0, 1003, 3003, 0, n), (0, 1003, 3003, 5, 11 + n)], dtype=np.int64)
    logq, got = run_segment_kernel(hip_lib, logits, labels, [t_out], segments, n + 6)
    assert got[0] < -5000
    check_against_restatement(logq, labels, [t_out], segments, n + 6, got, "2000 frames x 300 letters")


@pytest.mark.parametrize("k", [29, 64])
def test_whole_utterance_equals_minus_the_ctc_loss(hip_lib, k):
    """one segment per utterance that covers all of it against sl_ctc_loss_grad on the same batch: the loss's own relative 1e-5"""
    from test_gpu_ctc_long import run_kernel
    import torch
    rng = np.random.RandomState(k)
    lengths = [0, 1, 40, 100, 255, 300]
    input_len = [30, 2, 90, 257, 600, 640]
    t_out, l_max = 640, 300
    labels = np.zeros((len(lengths), l_max), dtype=np.int32)
    logits = np.zeros((len(lengths), t_out, k), dtype=np.float32)
    for b, n in enumerate(lengths):
        labels[b, :n] = _label(rng, n, k, 16)
        logits[b] = regime_logits(rng, list(labels[b, :n]), t_out, k, KINDS[b % len(KINDS)])
    _, loss, _ = run_kernel(hip_lib, logits, labels, lengths, input_len)
    torch.cuda.synchronize()
    segments = np.array([(b, 0, input_len[b], 0, n) for b, n in enumerate(lengths)], dtype=np.int64)
    logq, got = run_segment_kernel(hip_lib, logits, labels, input_len, segments, l_max)
    check_against_restatement(logq, labels, input_len, segments, l_max, got, "whole utterances, k = {}".format(k))
    print("minus loss", -loss, "segment posterior", got)
    assert np.all(np.isfinite(loss)) and np.all(np.abs(got + loss) <= 1e-5 * np.abs(loss))


def test_refusals_leave_the_output_untouched(hip_lib):
    import torch
    dev = "cuda:0"
    k, t, l_max, n = 29, 20, 8, 4
    logq = torch.zeros((2, t, k), dtype=torch.float32, device=dev)
    lab = torch.zeros((2, l_max), dtype=torch.int32, device=dev)
    il = torch.full((2,), t, dtype=torch.int32, device=dev)
    sg = torch.tensor([[0, 0, 10, 0, 3]] * n, dtype=torch.int32, device=dev)
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.empty((16,), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    score = hip_lib.raw("sl_ctc_segment_scores")
    ptrs = [x.data_ptr() for x in (logq, lab, il, sg, out)]
    assert score(*ptrs, 2, t, k, l_max, n, 512, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED
    assert "seg_l_max = 512" in hip_lib.last_error() and "511" in hip_lib.last_error()
    assert score(*ptrs, 2, t, 65, l_max, n, 8, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED and "k = 65" in hip_lib.last_error()
    assert score(*ptrs, 2, t, k, l_max, 0, 8, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED
    for i, name in enumerate(("logq", "labels", "input_len", "segments", "log_posterior")):
        args = list(ptrs)
        args[i] = None
        assert score(*args, 2, t, k, l_max, n, 8, ws.data_ptr(), 16, st) == SL_ERR_INVALID_ARGUMENT
        assert name + " is a null pointer" in hip_lib.last_error()
    # the workspace: the entry point asks for none at any shape (a segment's lattice lives in registers), so there is no size
    # below the one asked for; a null workspace of 0 bytes is taken
    need = hip_lib.raw("sl_ctc_segment_scores_workspace_bytes")(n, 8)
    assert need == 0
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL).item()
    assert score(*ptrs, 2, t, k, l_max, n, 8, None, 0, st) == 0
    torch.cuda.synchronize()
    ref = segment_scores(np.zeros((2, t, k)), np.zeros((2, l_max), dtype=np.int32), [t, t], [(0, 0, 10, 0, 3)] * n, 8)
    assert np.all(np.abs(out.cpu().numpy() - ref) <= 1e-6 * (10 + np.abs(ref)))


# ---------------------------------------------------------------------------------------------- Engine and Wav2Letter
def _net():
    from test_gpu_longform import _net as longform_net
    return longform_net("f16x3")


def _batch(rng, n, frames):
    from speechless_amd.net import LabeledSpectrogram
    words = ("she", "was", "abc", "a", "zoo", "quiet")
    return [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(words, size=rng.randint(1, 6))),
                               spectrogram=rng.randn(frames - 20 * i, 128).astype(np.float32)) for i in range(n)]


def _check_scored(net, scored, logq, frames, tolerance_factor=1.0):
    """a ScoredAlignment against the restatement applied to logq (T', K) and the alignment it holds"""
    from speechless_amd import word_spans
    label = scored.label
    encoded = [int(c) for c in net.grapheme_encoding.encode_label_batch([label])[0]] if label else []
    k = logq.shape[1]
    assert [w.word for w in scored.words] == label.split() == [w for w, _ in scored.alignment.word_frames]
    for w, (_, (first, end)), (begin, stop) in zip(scored.words, scored.alignment.word_frames, word_spans(label)):
        assert (w.first, w.end) == (first, end) and label[begin:stop] == w.word
        ref = forward_score(logq[first:end], encoded[begin:stop], k)
        assert abs(w.log_posterior - ref) <= tolerance_factor * 1e-6 * (end - first + abs(ref)), (w, ref)
        assert 0.0 <= w.confidence <= 1.0
    ref = forward_score(logq[:frames], encoded, k)
    if np.isfinite(scored.log_posterior) or np.isfinite(ref):
        assert abs(scored.log_posterior - ref) <= tolerance_factor * 1e-6 * (frames + abs(ref))
    return ref


def test_word_confidence_batch_end_to_end():
    net = _net()
    rng = np.random.RandomState(12)
    batch = _batch(rng, 3, 301)
    scored = net.word_confidence_batch(batch)
    logq = net.eval_engine.cur.logq.cpu().numpy()
    alignments = net.alignment_batch(batch)
    losses = [r.loss for r in net.test_and_predict_batch(batch).results]
    assert len(scored) == 3
    for b, (s, a, x, loss) in enumerate(zip(scored, alignments, batch, losses)):
        frames = x.z_normalized_transposed_spectrogram().shape[0] // net.input_to_prediction_length_ratio
        assert s.label == x.label and s.alignment.word_frames == a.word_frames and len(s.words) == len(x.label.split()) > 0
        assert s.alignment.log_probability == a.log_probability
        _check_scored(net, s, logq[b], frames)
        assert abs(s.log_posterior + loss) <= 1e-5 * abs(loss)
        assert s.log_posterior >= s.alignment.log_probability  # the sum over all paths holds the best one


def test_predict_with_confidence_returns_the_transcripts_of_predict():
    net = _net()
    rng = np.random.RandomState(13)
    batch = _batch(rng, 3, 260)
    spectrograms = [x.z_normalized_transposed_spectrogram() for x in batch]
    scored = net.predict_with_confidence_batch(spectrograms)
    logq = net.eval_engine.cur.logq.cpu().numpy()
    assert [s.label for s in scored] == net.predict_batch_greedily(spectrograms)
    for b, (s, x) in enumerate(zip(scored, spectrograms)):
        _check_scored(net, s, logq[b], x.shape[0] // net.input_to_prediction_length_ratio)
        assert np.isfinite(s.log_posterior)  # the greedy path itself says the greedy transcript
    one = net.predict_with_confidence(batch[0])
    assert one.label == net.predict(batch[0]) == scored[0].label
    assert [w.word for w in one.words] == one.label.split()


def test_confidence_of_recording_matches_the_batch_and_tiles_like_cut_sections():
    from speechless_amd import cut_sections
    from test_gpu_longform import WINDOW, _Example, _recording
    net = _net()
    rng = np.random.RandomState(14)
    label = " ".join(rng.choice(["she", "was", "abc", "a", "zoo", "quiet", "morning"], size=40))
    x = _recording(1400, seed=5)  # three windows of 512, and short enough for one forward pass
    example = _Example(x, label)
    from speechless_amd.net import LabeledSpectrogram
    single = net.word_confidence_batch([LabeledSpectrogram(id="r", label=label, spectrogram=x)])[0]
    scored, sections = net.confidence_of_recording(example, max_section_frames=120, window_input_frames=WINDOW)
    assert scored.alignment.word_frames == single.alignment.word_frames and len(scored.words) == 40
    for w, v in zip(scored.words, single.words):
        assert (w.word, w.first, w.end) == (v.word, v.first, v.end)
        assert abs(w.log_posterior - v.log_posterior) <= 2e-6 * (w.end - w.first + abs(v.log_posterior))
    assert abs(scored.log_posterior - single.log_posterior) <= 2e-6 * (700 + abs(single.log_posterior))
    assert [(text, frames) for text, frames, _ in sections] == cut_sections(scored.alignment, 120) and len(sections) > 3
    assert all(b[1][0] == a[1][1] for a, b in zip(sections, sections[1:]))
    assert all(np.isfinite(score) and score < 0 for _, _, score in sections)
    # without max_section_frames: the words alone
    scored2, none = net.confidence_of_recording(example, window_input_frames=WINDOW)
    assert none == [] and [w.log_posterior for w in scored2.words] == [w.log_posterior for w in scored.words]
    # a section of more than 511 letters names the argument to lower
    long_label = " ".join(["ab"] * 230)  # 689 letters over 700 frames
    with pytest.raises(ValueError, match="max_section_frames"):
        net.confidence_of_recording(_Example(x, long_label), max_section_frames=100000, window_input_frames=WINDOW)
    scored3, _ = net.confidence_of_recording(_Example(x, long_label), window_input_frames=WINDOW)
    assert len(scored3.words) == 230 and np.isnan(scored3.log_posterior)  # (the whole label is beyond a segment's 511 letters)


def test_a_wrong_word_scores_lower_than_the_right_one():
    """Hand-built peaked emissions that say "the cat sat": over the frames of "cat", the letters "cat" score near 1 and the
    letters of a wrong word far lower, and so do the whole labels.
    Margins: every frame gives its peak class the logq `peak` = -log(1 + 28 e^-12) and every other class peak - 12.  The right
    letters have the path along the peaks: score >= T * peak.  A path of the wrong letters spends a frame on each of d, o and g,
    none of which is ever the peak class: P <= C(T, 3) e^-36 (choose the three frames; the other frames' factors sum to at most
    1), which is below e^-25 at T = 59 and below e^-29 at T = 15."""
    import torch
    from math import comb, log, log1p, exp
    net = _net()
    engine = net.eval_engine
    enc = net.grapheme_encoding
    k, strength = 29, 12.0
    right, wrong = "the cat sat", "the dog sat"
    codes = [int(c) for c in enc.encode_label_batch([right])[0]]
    frames_per_letter, gap = 3, 2
    t_out = len(codes) * (frames_per_letter + gap) + 4
    logits = np.zeros((1, t_out, k), dtype=np.float32)
    logits[:, :, k - 1] = strength
    starts = []
    for i, c in enumerate(codes):
        t0 = 2 + i * (frames_per_letter + gap)
        starts.append(t0)
        logits[0, t0:t0 + frames_per_letter, k - 1] = 0.0
        logits[0, t0:t0 + frames_per_letter, c] = strength
    logq = torch.log_softmax(torch.tensor(np.repeat(logits, 2, axis=0), device=engine.device), dim=2)
    labels = enc.encode_label_batch([right, wrong])
    first, end = starts[4] - 1, starts[6] + frames_per_letter + 1  # the frames of "cat"
    segments = [(0, first, end, 4, 7), (1, first, end, 4, 7), (0, 0, t_out, 0, 11), (1, 0, t_out, 0, 11)]
    cat, dog, whole_right, whole_wrong = engine.ctc_segment_scores_long(logq, labels, [t_out, t_out], np.array(segments))
    peak = -log1p((k - 1) * exp(-strength))
    assert (end - first, t_out) == (15, 59)
    assert 15 * peak - 1e-4 <= cat <= 0 and dog <= log(comb(15, 3)) - 3 * strength + 1e-4 and dog < cat - 20
    assert 59 * peak - 1e-4 <= whole_right <= 0 and whole_wrong <= log(comb(59, 3)) - 3 * strength + 1e-4
    assert whole_wrong < whole_right - 20
    ref = segment_scores(logq.cpu().numpy(), labels, [t_out, t_out], segments, 11)
    assert np.all(np.abs(np.array([cat, dog, whole_right, whole_wrong]) - ref) <= 1e-6 * (t_out + np.abs(ref)))
    # the engine's checks: the first bad row is named, labels a segment covers must be letters
    with pytest.raises(ValueError, match=r"segment 1 = \[2, "):
        engine.ctc_segment_scores_long(logq, labels, [t_out, t_out], np.array([segments[0], (2, 0, 5, 0, 1)]))
    with pytest.raises(ValueError, match="outside"):
        engine.ctc_segment_scores_long(logq, np.full((2, 11), 28), [t_out, t_out], np.array(segments))
    with pytest.raises(ValueError, match="logq must be"):
        engine.ctc_segment_scores_long(logq[0], labels, [t_out], np.array(segments[:1]))


def test_asg_and_raw_wave_nets_are_refused():
    from speechless_amd import Wav2Letter, english_frequent_characters
    from test_gpu_longform import LAYER_SIZES, _Example, _recording
    x = _recording(300)
    asg = Wav2Letter(128, english_frequent_characters, seed=1, layer_sizes=LAYER_SIZES, criterion="asg")
    for call in (lambda: asg.confidence_of_recording(_Example(x, "abc")), lambda: asg.predict_with_confidence_batch([x]),
                 lambda: asg.word_confidence_batch([_Example(x, "abc")]),
                 lambda: asg.engine.ctc_segment_scores(np.zeros((1, 3), dtype=np.int32), np.array([(0, 0, 5, 0, 1)]))):
        with pytest.raises(ValueError, match="criterion='asg'"):
            call()
    wave = Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, seed=1, layer_sizes=LAYER_SIZES)
    with pytest.raises(ValueError, match="use_raw_wave_input=True is not supported .*out of scope"):
        wave.confidence_of_recording(_Example(x[:, :1], "abc"))
