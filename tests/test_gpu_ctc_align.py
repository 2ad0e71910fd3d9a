"""CTC forced alignment on the GPU: sl_ctc_align bit-identical to the float32 restatement (tests/test_ctc_align.py) on the fuzz
regimes of tools/fuzz_ctc.py, the tie rule, peaked distributions, and the Wav2Letter API on every evaluation arithmetic."""
import sys
from pathlib import Path

import numpy as np
import pytest

from test_ctc_align import collapse, path_score64, symbols_to_states, viterbi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def run_align_kernel(hip_lib, logits, labels_list, input_len, eps=1e-8, l_max=None):
    """logq from sl_softmax_logq, then sl_ctc_align.  Returns (logq, paths, scores) as numpy."""
    import torch
    b, t, k = logits.shape
    dev = "cuda:0"
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, l_max), dtype=np.int32)
    for i, l in enumerate(labels_list):
        labels[i, :len(l)] = l
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.zeros((b, t, k), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor([len(l) for l in labels_list], dtype=torch.int32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    path = torch.full((b, t), 7, dtype=torch.int32, device=dev)
    score = torch.zeros((b,), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    need = hip_lib.raw("sl_ctc_align_workspace_bytes")(b, t, l_max)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_ctc_align", logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(),
                 score.data_ptr(), b, t, k, l_max, ws.data_ptr(), need, st)
    torch.cuda.synchronize()
    return logq.cpu().numpy(), path.cpu().numpy(), score.cpu().numpy()


def check_against_restatement(logq, labels_list, input_len, paths, scores, k, full=True):
    for i, label in enumerate(labels_list):
        t_b = min(max(int(input_len[i]), 0), logq.shape[1])
        ref_score, ref_path = viterbi(logq[i], label, t_b, k - 1)
        assert np.array_equal(paths[i], ref_path), (i, len(label), t_b, np.flatnonzero(paths[i] != ref_path)[:5])
        assert np.float32(scores[i]).tobytes() == np.float32(ref_score).tobytes(), (i, scores[i], ref_score)
        if full and ref_score != -np.inf and t_b > 0:
            assert collapse(paths[i][:t_b], label, k - 1) == list(label)
            best64, _ = viterbi(logq[i], label, t_b, k - 1, dtype=np.float64)
            got64 = path_score64(logq[i], label, paths[i][:t_b], k - 1)
            assert abs(got64 - best64) <= 1e-5 * abs(best64), (i, got64, best64)


def fuzz_case(rng, k, t, b, l_hi, kinds, tight=False):
    sys.path.insert(0, str(ROOT / "tools"))
    from fuzz_ctc import regime_logits
    input_len = [int(rng.randint(max(2, t // 2), t + 1)) for _ in range(b)]
    if tight:
        lab_len = [int(min(l_hi, rng.randint(int(0.6 * il), il + 1))) for il in input_len]
    else:
        lab_len = [int(rng.randint(0, min(l_hi, il) + 1)) for il in input_len]
    labels_list = [[int(c) for c in rng.randint(0, k - 1, size=n)] for n in lab_len]
    logits = np.zeros((b, t, k), dtype=np.float32)
    for i in range(b):
        a, c = rng.choice(kinds), rng.choice(kinds)
        la = regime_logits(rng, labels_list[i], input_len[i], k, a)
        if tight or rng.rand() < 0.4:
            h = input_len[i] // 2
            la[h:] = regime_logits(rng, labels_list[i], input_len[i], k, c)[h:]
        logits[i, :input_len[i]] = la
    return logits, labels_list, input_len


FUZZ_KINDS = ("uniform", "sharp", "collapse", "learnt", "wrong")
# (t_out, rows, longest label, tight) of the fuzz cases, in the order in which one seeded stream draws them; also run through
# sl_ctc_align_long by test_gpu_ctc_align_long.py
FUZZ_SHAPES = [(300, 6, 100, False), (300, 4, 255, True), (1000, 4, 250, False), (4000, 3, 511, False), (4000, 2, 120, False)]


@pytest.mark.parametrize("k", [29, 64])
def test_align_kernel_bit_exact_on_fuzz_regimes(hip_lib, k):
    """Backpointers in LDS (300 / 1000 frames) and in HBM (4000 frames), 4 / 8 / 16 states per lane, all five regimes,
    tight labels, and rows that cannot be aligned (too many labels, repeats without room for the blank, T = 0)."""
    rng = np.random.RandomState(11 + k)
    for t, b, l_hi, tight in FUZZ_SHAPES:
        logits, labels_list, input_len = fuzz_case(rng, k, t, b, l_hi, FUZZ_KINDS, tight)
        logq, paths, scores = run_align_kernel(hip_lib, logits, labels_list, input_len)
        check_against_restatement(logq, labels_list, input_len, paths, scores, k)
    # infeasible rows next to feasible ones; empty labels; T = 0; input lengths beyond t_out (clamped)
    t = 40
    labels_list = [[1] * 30, list(range(20)) * 2, [], [], [3, 4], [5, 5, 5]]
    input_len = [40, 39, 17, 0, 0, 60]
    logits = rng.randn(len(labels_list), t, k).astype(np.float32)
    logq, paths, scores = run_align_kernel(hip_lib, logits, labels_list, input_len)
    assert scores[0] == -np.inf and np.all(paths[0] == -1)       # 30 repeats need 59 frames
    assert scores[1] == -np.inf and np.all(paths[1] == -1)       # 40 labels in 39 frames
    assert np.all(paths[2][:17] == 0) and np.all(paths[2][17:] == -1)
    assert scores[3] == 0 and np.all(paths[3] == -1)
    assert scores[4] == -np.inf and np.all(paths[4] == -1)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k)


def lds_limit(query, rows, l_max, beyond=20000):
    """(the largest t_out whose backpointer rows stay in LDS, the smallest whose rows go to the workspace in HBM) for `rows`
    utterances at this l_max, from a workspace query (sl_ctc_align's or sl_asg_align's), which is monotonic in t_out"""
    lo, hi = 1, beyond
    assert query(rows, lo, l_max) == 0 and query(rows, hi, l_max) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if query(rows, mid, l_max) == 0 else (lo, mid)
    return lo, hi


@pytest.mark.parametrize("in_hbm", [False, True])
@pytest.mark.parametrize("l_max,nj", [(127, 4), (128, 8), (255, 8), (256, 16), (511, 16)])
def test_every_kernel_instantiation_on_either_side_of_the_lds_limit(hip_lib, l_max, nj, in_hbm):
    """All six ctc_align_kernel<NJ, BP_LDS>, chosen by the l_max ARGUMENT (4 / 8 / 16 states per lane on either side of where
    the count changes, and the longest label) and by t_out: a few hundred frames with the backpointers in LDS, and the first
    t_out at which they leave it (2481 / 1233 / 609 frames: 39 / 20 / 10 backtrace windows, the last one partial).  Three rows:
    the longest label over all frames, a label with zero slack (T = L + repeats), and a short row; two regimes per row."""
    sys.path.insert(0, str(ROOT / "tools"))
    from fuzz_ctc import regime_logits
    query = hip_lib.raw("sl_ctc_align_workspace_bytes")
    last_lds, first_hbm = lds_limit(query, 3, l_max)
    assert query(3, first_hbm, l_max) == 3 * first_hbm * 16 * nj  # (rows of 16 * NJ bytes: the instantiation meant)
    k = 64 if in_hbm else 29
    t = first_hbm if in_hbm else min(last_lds, max(300, l_max + l_max // 8 + 30))
    assert (query(3, t, l_max) > 0) == in_hbm
    rng = np.random.RandomState(1000 * l_max + in_hbm)
    labels_list = [[int(c) for c in rng.randint(0, k - 1, size=n)] for n in (l_max, min(l_max, t // 2), l_max // 3)]
    tight = labels_list[1]
    input_len = [t, len(tight) + sum(a == b for a, b in zip(tight, tight[1:])), t // 3 + 5]
    logits = np.zeros((3, t, k), dtype=np.float32)
    for i, (label, t_b) in enumerate(zip(labels_list, input_len)):
        first, second = rng.choice(FUZZ_KINDS, size=2, replace=False)
        logits[i, :t_b] = regime_logits(rng, label, t_b, k, first)
        logits[i, t_b // 2:t_b] = regime_logits(rng, label, t_b, k, second)[t_b // 2:]
    logq, paths, scores = run_align_kernel(hip_lib, logits, labels_list, input_len, l_max=l_max)
    assert np.isfinite(scores).all()  # (every row can be aligned, the second one only just)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k)


def test_align_kernel_tie_rule_on_constant_rows(hip_lib):
    k, t = 3, 4
    logits = np.zeros((2, t, k), dtype=np.float32)
    logq, paths, scores = run_align_kernel(hip_lib, logits, [[0, 1], [0, 0]], [4, 4])
    assert list(paths[0]) == [1, 3, 4, 4]
    check_against_restatement(logq, [[0, 1], [0, 0]], [4, 4], paths, scores, k)
    # longer constant rows with 29 classes: the restatement's rule, bit for bit
    rng = np.random.RandomState(4)
    labels_list = [[int(c) for c in rng.randint(0, 28, size=n)] for n in (0, 1, 37, 120)]
    logits = np.zeros((4, 500, 29), dtype=np.float32)
    logq, paths, scores = run_align_kernel(hip_lib, logits, labels_list, [500, 333, 500, 260])
    check_against_restatement(logq, labels_list, [500, 333, 500, 260], paths, scores, 29)


def test_align_kernel_follows_a_peaked_argmax_path(hip_lib):
    """Where every frame's argmax already spells the label, the alignment IS that argmax path, frame for frame."""
    rng = np.random.RandomState(8)
    k, t, b = 29, 600, 4
    logits = rng.randn(b, t, k).astype(np.float32)
    labels_list, want = [], []
    for i in range(b):
        n = int(rng.randint(20, 120))
        label = [int(c) for c in rng.randint(0, k - 1, size=n)]
        seq = []
        for j, c in enumerate(label):
            if j and c == label[j - 1]:
                seq.append(k - 1)
            seq.append(c)
        cuts = 2 * np.sort(rng.choice(np.arange(1, t // 2), size=len(seq), replace=False))  # (two frames apart at least)
        bounds = np.concatenate([[0], cuts, [t]])
        symbols = np.full((t,), k - 1)
        for j, sym in enumerate(seq):  # symbol j on [bounds[j+1] - run, bounds[j+1]); blanks elsewhere
            run = int(rng.randint(1, 4))
            lo = max(bounds[j] + 1 if j else 0, bounds[j + 1] - run)
            symbols[lo:bounds[j + 1]] = sym
        logits[i, np.arange(t), symbols] += 25.0
        labels_list.append(label)
        want.append(symbols_to_states(list(symbols), label, k - 1))
    logq, paths, scores = run_align_kernel(hip_lib, logits, labels_list, [t] * b)
    for i in range(b):
        assert list(paths[i]) == want[i]
    check_against_restatement(logq, labels_list, [t] * b, paths, scores, k)


def _spectrogram_batch(rng, n, frames, features, words=("she", "was", "abc", "a", "zoo")):
    from speechless_amd.net import LabeledSpectrogram
    return [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(list(words), size=rng.randint(1, 4))),
                               spectrogram=rng.randn(int(rng.randint(*frames)), features).astype(np.float32))
            for i in range(n)]


def _check_net_alignments(net, batch):
    alignments = net.alignment_batch(batch)
    ev = net.eval_engine
    logq = ev.cur.logq.cpu().numpy()
    enc = net.grapheme_encoding
    k = enc.grapheme_set_size
    ratio = net.input_to_prediction_length_ratio
    for x, a, lq in zip(batch, alignments, logq):
        label = [int(c) for c in enc.encode_label_batch([x.label])[0]]
        t_b = x.z_normalized_transposed_spectrogram().shape[0] // ratio
        ref_score, ref_path = viterbi(lq, label, t_b, k - 1)
        assert np.float32(a.log_probability).tobytes() == np.float32(ref_score).tobytes()
        ref_pos = np.where(ref_path % 2 == 1, (ref_path - 1) // 2, -1)
        assert np.array_equal(a.frame_label_positions, ref_pos)
        assert a.label == x.label and len(a.character_frames) == len(x.label)
        for i, (first, end) in enumerate(a.character_frames):
            assert np.all(a.frame_label_positions[first:end] == i)
            assert np.sum(a.frame_label_positions == i) == end - first
        assert [w for w, _ in a.word_frames] == x.label.split()
    return alignments


def test_wav2letter_alignment_batch_on_every_evaluation_path():
    """The reference signature (f16x3 evaluation engine), compute_dtype="f32", and a raw-wave net (bf16x3): paths and scores
    bit-identical to the restatement applied to the engine's own logq; the forward-only evaluation engine gets no gradient
    buffers."""
    from speechless_amd import Wav2Letter, english_frequent_characters
    rng = np.random.RandomState(5)
    batch = _spectrogram_batch(rng, 3, (150, 260), 128)
    net = Wav2Letter(128, english_frequent_characters, seed=3)
    assert net.eval_dtype == "f16x3" and net.eval_engine is not net.engine
    _check_net_alignments(net, batch)
    assert all(g is None for g in net.eval_engine.cur.g)
    net32 = Wav2Letter(128, english_frequent_characters, seed=3, compute_dtype="f32")
    _check_net_alignments(net32, batch)
    wave = Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, seed=5,
                      layer_sizes=dict(out_filter_count=256))
    assert wave.eval_dtype == "bf16x3"
    wave_batch = _spectrogram_batch(rng, 2, (9000, 12000), 1)
    _check_net_alignments(wave, wave_batch)
    # seconds: 1 / sample_rate per input step on a raw-wave net, but only with a sample rate to go by
    with pytest.raises(ValueError, match="seconds_per_input_step"):
        wave.positional_label_batch(wave_batch)
    labels = wave.positional_label_batch(wave_batch, seconds_per_input_step=1 / 16000)
    assert all(l is None or l.label == " ".join(x.label.split()) for l, x in zip(labels, wave_batch))


def test_positional_label_batch_on_labeled_examples():
    from speechless_amd import Wav2Letter, english_frequent_characters
    from speechless_amd.spectrogram import LabeledExample
    rng = np.random.RandomState(6)
    audio = [0.1 * rng.randn(int(rng.randint(20000, 32000))).astype(np.float32) for _ in range(2)]
    batch = [LabeledExample(lambda a=a: a, sample_rate=16000, id="e{}".format(i), label=lab, hop_length=128)
             for i, (a, lab) in enumerate(zip(audio, ["she was", "a zoo  abc"]))]
    net = Wav2Letter(128, english_frequent_characters, seed=2)
    alignments = net.alignment_batch(batch)
    labels = net.positional_label_batch(batch)
    step = net.input_to_prediction_length_ratio * 128 / 16000
    for a, pl in zip(alignments, labels):
        assert pl is not None and pl.labels == [w for w, _ in a.word_frames]
        for (_, (s, e)), (_, (first, end)) in zip(pl.labeled_sections, a.word_frames):
            assert np.isclose(s, first * step, rtol=1e-12) and np.isclose(e, end * step, rtol=1e-12)
