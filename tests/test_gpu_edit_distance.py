"""Letter and word error counts on the GPU (csrc/edit_distance.hip, Engine.error_counts / edit_distance_batch,
Wav2Letter(error_count_device="gpu")) against speechless_amd.net.edit_distance applied to the decoded strings and to their
.split().  Exact integer equality everywhere: there is no tolerance."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOY = Path(__file__).resolve().parent / "golden" / "toy_kenlm"
K = 29
SPACE = 27
CHARACTERS = list("abcdefghijklmnopqrstuvwxyz'") + [" "]  # index 27 is the separator, 28 the CTC blank
NO_SPACE_CHARACTERS = list("abcdefghijklmnopqrstuvwxyz'") + ["_"]
SMALL = dict(main_filter_count=20, out_filter_count=40, inner_count=1)
UNTOUCHED = 77


def host_counts(a_row, b_row, space=SPACE):
    """(letter errors, word errors, words of a) the way ExpectationVsPrediction counts them: on strings"""
    from speechless_amd.net import edit_distance
    characters = CHARACTERS if space == SPACE else NO_SPACE_CHARACTERS
    assert space in (SPACE, -1)
    a, b = ("".join(characters[i] for i in row) for row in (a_row, b_row))
    return edit_distance(a, b), edit_distance(a.split(), b.split()), len(a.split())


def launch(hip_lib, pairs, space=SPACE, a_max=None, b_max=None, extra_stride=3, lengths=None):
    """sl_edit_distance on the (a, b) index-list pairs; rows a_max + extra_stride apart, everything beyond a row's length
    POISONED: -1 and values >= K in turn.  lengths: device lengths other than the true ones.  Returns int32 (3, B)."""
    import torch
    n = len(pairs)
    a_max = max(len(a) for a, _ in pairs) if a_max is None else a_max
    b_max = max(len(b) for _, b in pairs) if b_max is None else b_max
    sides = []
    for side, width in ((0, a_max + extra_stride), (1, b_max + extra_stride)):
        rows = np.where(np.arange(n * width).reshape(n, width) % 2 == 0, -1, K + 5).astype(np.int32)
        for row, pair in zip(rows, pairs):
            row[:len(pair[side])] = pair[side]
        sides.append(torch.tensor(rows, device="cuda"))
    true_lengths = ([len(a) for a, _ in pairs], [len(b) for _, b in pairs])
    a_len, b_len = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (lengths or true_lengths))
    out = torch.full((3, n), UNTOUCHED, dtype=torch.int32, device="cuda")
    a, b = sides
    hip_lib.call("sl_edit_distance", a.data_ptr(), a_len.data_ptr(), a.stride(0), b.data_ptr(), b_len.data_ptr(), b.stride(0),
                 n, a_max, b_max, space, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def check(hip_lib, pairs, space=SPACE, **kw):
    got = launch(hip_lib, pairs, space, **kw)
    want = np.array([host_counts(a, b, space) for a, b in pairs], dtype=np.int32).T
    assert got.tolist() == want.tolist(), (pairs, got.tolist(), want.tolist())
    return want


def random_row(rng, n, separator_probability=0.2):
    return [SPACE if rng.rand() < separator_probability else int(rng.randint(0, 27)) for _ in range(n)]


def encode(text):
    return [CHARACTERS.index(c) for c in text]


# ------------------------------------------------------------------------------------------ letters
def test_empty_and_identical_rows(hip_lib):
    row = encode("the quick brown fox")
    for pair in (([], []), ([], row), (row, []), (row, row)):
        check(hip_lib, [pair])
    check(hip_lib, [([], []), ([], row), (row, []), (row, row)])


@pytest.mark.parametrize("position", ["first", "middle", "last"])
def test_single_edits(hip_lib, position):
    base = encode("she had your dark suit in greasy wash water")
    at = {"first": 0, "middle": len(base) // 2, "last": len(base) - 1}[position]
    substituted = base[:at] + [(base[at] + 1) % 26] + base[at + 1:]
    inserted = base[:at + (position == "last")] + [25] + base[at + (position == "last"):]
    deleted = base[:at] + base[at + 1:]
    want = check(hip_lib, [(base, substituted), (base, inserted), (base, deleted), (inserted, base), (deleted, base)])
    assert want[0].tolist() == [1] * 5


@pytest.mark.parametrize("a_length,b_length", [(a, b) for a in (63, 64, 65) for b in (63, 64, 65)] +
                         [(127, 129), (1, 200), (200, 1), (200, 500),
                          # 256 | 257: four | sixteen columns per lane; 1024: the longest supported expected row
                          (256, 70), (257, 70), (1024, 40)])
def test_lengths_around_lane_and_word_boundaries(hip_lib, a_length, b_length):
    """each case its own launch, so that a_max = a_length picks the kernel variant (1 / 4 / 16 columns per lane)"""
    rng = np.random.RandomState(1000 * a_length + b_length)
    a = random_row(rng, a_length)
    b = random_row(rng, b_length)
    n = min(a_length, b_length)
    b[:n:2] = a[:n:2]  # related rows: matches all along the diagonal, not a distance of max(a, b)
    check(hip_lib, [(a, b)])


def test_poisoned_padding_and_wide_strides(hip_lib):
    rng = np.random.RandomState(7)
    pairs = [(random_row(rng, int(rng.randint(0, 30))), random_row(rng, int(rng.randint(0, 50)))) for _ in range(5)]
    check(hip_lib, pairs, extra_stride=37)            # rows much further apart than the maxima
    check(hip_lib, pairs, a_max=64, b_max=128)        # maxima beyond every row: the poison lies below them, too


# ------------------------------------------------------------------------------------------ words
WORD_CASES = [
    ("  the cat", "the cat"), ("the cat  ", "the cat"), ("the  cat", "the cat"), (" the   cat ", "a the cat"),
    ("    ", "the cat"), ("the cat", "   "), ("   ", " "), ("thecat", "the cat"), ("thecat", "thecat"), ("thecat", "thecut"),
    ("there then", "thera thew"),             # words equal except for their last index
    ("the then them", "then the the them"),   # words that are prefixes of one another
    ("a a a a", "a a a"), ("a a a", "a a a a"), (" ".join(["ab"] * 40), " ".join(["ab"] * 33 + ["abc"] * 4)),
    ("ab", "ab ab ab ab ab ab ab"), ("x", " "), ("", "a b"),
]


def test_word_rule(hip_lib):
    pairs = [(encode(a), encode(b)) for a, b in WORD_CASES]
    want = check(hip_lib, pairs)
    assert want[2].tolist() == [len(a.split()) for a, _ in WORD_CASES]
    for pair in pairs[:6]:
        check(hip_lib, [pair])


def test_without_separator(hip_lib):
    """space = -1: every non-empty row is one word -- index 27 is a letter like any other"""
    pairs = [(encode(a), encode(b)) for a, b in WORD_CASES]
    want = check(hip_lib, pairs, space=-1)
    assert want[2].tolist() == [1 if a else 0 for a, _ in WORD_CASES]


def test_word_count_pointer_may_be_null(hip_lib):
    import torch
    a, b = (torch.tensor([encode(t)], dtype=torch.int32, device="cuda") for t in ("a bc d", "a bd"))
    a_len, b_len = (torch.tensor([t.shape[1]], dtype=torch.int32, device="cuda") for t in (a, b))
    out = torch.zeros((2,), dtype=torch.int32, device="cuda")
    hip_lib.call("sl_edit_distance", a.data_ptr(), a_len.data_ptr(), 6, b.data_ptr(), b_len.data_ptr(), 4, 1, 6, 4, SPACE,
                 out[0:].data_ptr(), out[1:].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert out.tolist() == list(host_counts(encode("a bc d"), encode("a bd"))[:2])


# ------------------------------------------------------------------------------------------ batch shape
def test_batch_of_one_and_of_thirty_three(hip_lib):
    rng = np.random.RandomState(33)
    pairs = [(random_row(rng, int(rng.randint(0, 41))), random_row(rng, int(rng.randint(0, 91)))) for _ in range(33)]
    assert len({(len(a), len(b)) for a, b in pairs}) == 33  # every row a different length pair
    want = np.array([host_counts(a, b) for a, b in pairs])
    words_a = want[:, 2]
    words_b = np.array([host_counts(b, b)[2] for _, b in pairs])
    # drawn on the CPU: without these the batch shows little
    assert (words_a == 0).any() and (words_b == 0).any() and max(words_a.max(), words_b.max()) >= 10
    check(hip_lib, pairs)
    check(hip_lib, pairs[:1])


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(hip_lib):
    """What the host can see is refused with a negative code and a message before any launch: a maximum above the row stride
    (a length up to it would leave its row), shapes beyond the kernel's limits."""
    from speechless_amd._lib import HipLibraryError
    pair = (encode("the cat"), encode("the hat"))
    with pytest.raises(HipLibraryError, match=r"status -1: sl_edit_distance: a_max = 20 .* above the row stride 10"):
        launch(hip_lib, [pair], a_max=20, b_max=20, extra_stride=-10)
    with pytest.raises(HipLibraryError, match=r"status -1: .*null pointer"):
        hip_lib.call("sl_edit_distance", None, None, 1, None, None, 1, 1, 1, 1, SPACE, None, None, None, None)
    assert hip_lib.raw("sl_edit_distance_supported")(1024, 4000) == 1
    assert hip_lib.raw("sl_edit_distance_supported")(1025, 10) == 0
    assert hip_lib.raw("sl_edit_distance_supported")(200, 8000) == 0
    with pytest.raises(HipLibraryError, match=r"status -2: sl_edit_distance: a_max = 1025.*unsupported"):
        launch(hip_lib, [pair], a_max=1025)
    assert hip_lib.raw("sl_edit_distance")(None, None, 1, None, None, 1, 0, 1, 1, SPACE, None, None, None, None) == -1
    assert "batch > 0" in hip_lib.last_error()


def test_length_outside_its_row_is_reported_per_utterance(hip_lib):
    """The lengths are in HBM and the call does not synchronise: a row with a length outside [0, max] reads nothing and
    reports -1; its neighbours are counted.  Engine.edit_distance_batch / error_counts turn the -1 into a ValueError."""
    pairs = [(encode("the cat"), encode("the hat")), (encode("a b"), encode("a")), (encode("abc"), encode("abd"))]
    got = launch(hip_lib, pairs, lengths=([7, 8, 3], [7, 1, -1]))
    assert got[:, 0].tolist() == [1, 1, 2]
    assert got[:, 1].tolist() == [-1, -1, -1] and got[:, 2].tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------------ engine
def spectrogram_batch(seed, lengths, labels):
    from speechless_amd.net import LabeledSpectrogram
    rng = np.random.RandomState(seed)
    return [LabeledSpectrogram("u{}".format(i), label, rng.randn(n, 128).astype(np.float32))
            for i, (n, label) in enumerate(zip(lengths, labels))]


LENGTHS = [70, 91, 64, 120, 83, 102]
LABELS = ["c c cm qc", "the cat sat", "", " cocoa  q ", "m", "c co c c m oq cqcqcqc c mocuoceqm and more"]


def test_engine_error_counts_and_launch_list():
    from speechless_amd import Wav2Letter, english_frequent_characters, launch_list
    from speechless_amd.net import edit_distance
    net = Wav2Letter(128, english_frequent_characters, seed=5, layer_sizes=SMALL, compute_dtype="f32")
    batch = spectrogram_batch(5, LENGTHS, LABELS)
    inputs = net._input_dictionary_for_loss_net(batch)
    names = Wav2Letter.InputNames
    eng = net.eval_engine
    space = list(english_frequent_characters).index(" ")
    eng.forward(inputs[names.input_batch])
    eng.set_labels(inputs[names.label_batch], inputs[names.label_lengths], inputs[names.prediction_lengths])
    decoded, _ = eng.greedy_decode()
    predicted = [net.grapheme_encoding.decode_graphemes(d, merge_repeated=False) for d in decoded]
    assert sum(bool(p) for p in predicted) >= 3 and any(" " in p for p in predicted)
    want_letters = [edit_distance(x.label, p) for x, p in zip(batch, predicted)]
    want_words = [edit_distance(x.label.split(), p.split()) for x, p in zip(batch, predicted)]
    buf = eng.cur
    got = []
    assert eng._run_recorded(buf, "error counts", lambda: got.append(eng.error_counts(space))) is False
    letters, words = got[0]
    assert letters.dtype == np.int32 and letters.shape == (6,) and words.dtype == np.int32 and words.shape == (6,)
    assert letters.tolist() == want_letters and words.tolist() == want_words
    assert ("sl_edit_distance", "edit_distance") in launch_list.entry_points(buf.launch_lists["error counts"])
    # the host-resident twin makes the same launch on uploaded rows
    expected = [[list(english_frequent_characters).index(c) for c in x.label] for x in batch]
    letters, words = eng.edit_distance_batch(expected, decoded, space)
    assert letters.tolist() == want_letters and words.tolist() == want_words
    # a batch of another size than the buffer set's, and one beyond the kernel's limits (counted on the host)
    letters, words = eng.edit_distance_batch(expected[:2], decoded[:2], space)
    assert letters.tolist() == want_letters[:2] and words.tolist() == want_words[:2]
    long_row = [i % 26 for i in range(1030)]
    letters, words = eng.edit_distance_batch([long_row], [long_row[:-3]], space)
    assert letters.tolist() == [3] and words.tolist() == [1]
    with pytest.raises(ValueError):
        eng.edit_distance_batch(expected, decoded[:2], space)


def compare_devices(labels, **kw):
    from speechless_amd import Wav2Letter
    results = {}
    for device in ("host", "gpu"):
        net = Wav2Letter(128, error_count_device=device, layer_sizes=SMALL, compute_dtype="f32", **kw)
        results[device] = net.test_and_predict_batch(spectrogram_batch(5, LENGTHS, labels))
    gpu, host = results["gpu"], results["host"]
    assert len(gpu.results) == len(host.results) == 6
    for g, h in zip(gpu.results, host.results):
        assert vars(g) == vars(h)
        assert (type(g.letter_error_count), type(g.word_error_count)) == (int, int)
        assert str(g) == str(h)
        assert (g.letter_error_rate, g.word_error_rate) == (h.letter_error_rate, h.word_error_rate)
    assert gpu.summary_line() == host.summary_line() and str(gpu) == str(host)
    return host.results


def test_wav2letter_gpu_error_counts_equal_the_host_ones():
    from speechless_amd import english_frequent_characters
    labels = [label if label.strip() else "q c" for label in LABELS]  # (rates divide by the expected counts)
    results = compare_devices(labels, allowed_characters=english_frequent_characters, seed=5)
    predicted = [r.predicted for r in results]
    # not vacuous (seed 5 confirmed with the CPU port, oracle/w2l_torch_cpu.py: six noisy strings of c, q, m, o and spaces)
    assert sum(bool(p) for p in predicted) >= 3 and any(" " in p for p in predicted)
    assert any(r.letter_error_count for r in results) and any(r.word_error_count for r in results)


@pytest.mark.parametrize("beam_search_device", ["host", "gpu"])
def test_wav2letter_gpu_error_counts_behind_the_beam_search(beam_search_device):
    labels = ["the cat", "a cat the cat", "cats", "the  hat ", "at a host", "he"]
    compare_devices(labels, allowed_characters=list("acehost "), kenlm_directory=TOY, seed=5,
                    beam_search_device=beam_search_device)
