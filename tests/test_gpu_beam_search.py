"""The GPU beam search (ctc_beam.hip, GpuCtcBeamSearchDecoder) against the host decoder it restates
(csrc_host/beam_search.cpp): identical label sequences, |d log_prob| <= 1e-4 * max(1, |log_prob|)."""
import math
from pathlib import Path

import numpy as np
import pytest

TOY = Path(__file__).resolve().parent / "golden" / "toy_kenlm"
ALPHABET = list("acehost ")
ENGLISH = list("abcdefghijklmnopqrstuvwxyz' ")


def softmax_rows(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def assert_same(host, gpu, probs, lengths):
    want, want_lp = host.decode(probs, lengths)
    got, got_lp = gpu.decode(probs, lengths)
    for i in range(len(want)):
        assert got[i] == want[i], (i, got[i], want[i])
        assert abs(float(got_lp[i]) - float(want_lp[i])) <= 1e-4 * max(1.0, abs(float(want_lp[i]))), \
            (i, got_lp[i], want_lp[i])
    return got


def decoders(alphabet, lm=None, **kw):
    from speechless_amd.decoder import CtcBeamSearchDecoder, GpuCtcBeamSearchDecoder
    return CtcBeamSearchDecoder(alphabet, lm, threads=16, **kw), GpuCtcBeamSearchDecoder(alphabet, lm, **kw)


@pytest.fixture(scope="module")
def toy_lm():
    from speechless_amd.decoder import NGramLanguageModel
    return NGramLanguageModel(TOY / "lm.arpa")


@pytest.fixture(scope="module")
def order4_lm(tmp_path_factory):
    from speechless_amd.decoder import NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    path = tmp_path_factory.mktemp("lm4") / "lm.arpa"
    write_synthetic_arpa(path, ENGLISH, 5000, order=4, seed=7)
    return NGramLanguageModel(path)


@pytest.mark.gpu
def test_reference_known_answer():
    logits = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    probs = softmax_rows(logits)[None]
    for merge, want in ((True, [0]), (False, [0, 0])):
        host, gpu = decoders(["A"], beam_width=1, merge_repeated=merge, epsilon=0.0)
        assert assert_same(host, gpu, probs, [5]) == [want]


@pytest.mark.gpu
@pytest.mark.parametrize("beam_width", [1, 8, 64, 100, 128])
@pytest.mark.parametrize("weights", [None, (.8, 0., 2.3), (1.5, 1.0, 0.0)])
def test_plain_and_toy_language_model(toy_lm, beam_width, weights):
    rng = np.random.RandomState(beam_width)
    probs = softmax_rows(rng.randn(6, 60, len(ALPHABET) + 1) * 2.5)
    lengths = [60, 1, 33, 0, 59, 12]
    for merge in (False, True):
        if weights is None:
            host, gpu = decoders(ALPHABET, beam_width=beam_width, merge_repeated=merge)
        else:
            host, gpu = decoders(ALPHABET, toy_lm, beam_width=beam_width, merge_repeated=merge, kenlm_weight=weights[0],
                                 word_count_weight=weights[1], valid_word_count_weight=weights[2])
        assert_same(host, gpu, probs, lengths)


@pytest.mark.gpu
@pytest.mark.parametrize("t_max, beam_width, seeds", [(5, 2, (12, 0, 49)), (8, 3, (0, 0, 10))])
def test_smallest_node_table(toy_lm, tmp_path, t_max, beam_width, seeds):
    """11 / 25 nodes at most: hash maps of 32 / 64 slots (the floor is 16), whose probe chains wrap, with prefixes that leave
    the beam and return (the seeds were chosen for that on the CPU restatement of the kernel, test_beam_search_batched.py, which
    counts them; asserted below); a row of one frame and a row of none beside them: the root alone, and the backtrace of a
    one-node arena.  k = 5 without a model and with a 12-word bigram model over the same four characters; the toy model at its
    own alphabet (k = 9, the smallest that spells its words: for a word it cannot spell the HOST scorer leaves trie nodes at a
    minimum of FLT_MAX behind, and is no reference then)."""
    from test_beam_search_batched import batched_beam_search, flat_lm
    from speechless_amd.decoder import NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    small = list("cat ")
    write_synthetic_arpa(tmp_path / "lm.arpa", small, 12, order=2, seed=3)
    lengths = [t_max, 1, 0, t_max - 1, t_max]
    models = ((small, None), (small, NGramLanguageModel(tmp_path / "lm.arpa")), (ALPHABET, toy_lm))
    for seed, (alphabet, lm) in zip(seeds, models):
        probs = softmax_rows(np.random.RandomState(seed).randn(5, t_max, len(alphabet) + 1) * 2.5)
        for merge in (False, True):
            host, gpu = decoders(alphabet, lm, beam_width=beam_width, merge_repeated=merge)
            got = assert_same(host, gpu, probs, lengths)
            assert len(got[1]) <= 1 and got[2] == []
            stats = {"returns": 0}
            for b, length in enumerate(lengths):
                restated, _ = batched_beam_search(probs[b, :length], beam_width, merge, flat_lm(host) if lm else None,
                                                  stats=stats)
                assert restated == got[b]
            assert stats["returns"] >= 1, (seed, merge)


@pytest.mark.gpu
def test_generated_order4_language_model_batch(order4_lm):
    rng = np.random.RandomState(3)
    b, t = 32, 500
    probs = softmax_rows(rng.randn(b, t, len(ENGLISH) + 1) * 3.0)
    lengths = [(0, 1, 17, 500)[i % 4] for i in range(b)]
    host, gpu = decoders(ENGLISH, order4_lm, beam_width=100)
    assert_same(host, gpu, probs, lengths)
    long = softmax_rows(rng.randn(1, 4000, len(ENGLISH) + 1) * 3.0)
    assert_same(host, gpu, long, [4000])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [29, 64])
def test_class_counts(k):
    alphabet = [chr(ord("a") + i) if i < 26 else chr(0x100 + i) for i in range(k - 2)] + [" "]
    rng = np.random.RandomState(k)
    probs = softmax_rows(rng.randn(4, 120, k) * 2.0)
    for merge in (False, True):
        host, gpu = decoders(alphabet, beam_width=100, merge_repeated=merge)
        assert_same(host, gpu, probs, [120, 77, 5, 120])


@pytest.mark.gpu
def test_uniform_frames_break_ties_as_the_host_does(toy_lm):
    probs = np.full((2, 20, len(ALPHABET) + 1), 1.0 / (len(ALPHABET) + 1), dtype=np.float32)
    for lm in (None, toy_lm):
        for beam_width in (1, 8, 100):
            for merge in (False, True):
                host, gpu = decoders(ALPHABET, lm, beam_width=beam_width, merge_repeated=merge)
                assert_same(host, gpu, probs, [20, 7])


@pytest.mark.gpu
def test_language_model_changes_the_transcription_on_the_gpu(toy_lm):
    from test_beam_search import _acoustics
    probs = _acoustics("the cot", ALPHABET, t_per_char=1, confusions={5: ("a", 0.45)}, seed=4)
    host, gpu = decoders(ALPHABET, toy_lm, beam_width=32)
    got = assert_same(host, gpu, probs[None], [len(probs)])
    assert "".join(ALPHABET[i] for i in got[0]) == "the cat"


@pytest.mark.gpu
def test_numpy_and_device_tensor_inputs_agree(toy_lm):
    import torch
    rng = np.random.RandomState(11)
    probs = softmax_rows(rng.randn(5, 40, len(ALPHABET) + 1) * 2.0)
    _, gpu = decoders(ALPHABET, toy_lm, beam_width=16)
    a, lp_a = gpu.decode(probs, [40, 3, 20, 0, 39])
    b, lp_b = gpu.decode(torch.from_numpy(probs).cuda(), torch.tensor([40, 3, 20, 0, 39], dtype=torch.int32).cuda())
    assert a == b and np.array_equal(lp_a, lp_b)


@pytest.mark.gpu
def test_limits_raise_a_named_value_error(tmp_path):
    from speechless_amd.decoder import BeamSearchLimitError, GpuCtcBeamSearchDecoder, NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    with pytest.raises(BeamSearchLimitError):
        GpuCtcBeamSearchDecoder([chr(0x100 + i) for i in range(64)])  # 65 classes
    with pytest.raises(BeamSearchLimitError):
        GpuCtcBeamSearchDecoder(ALPHABET, beam_width=129)
    with pytest.raises(BeamSearchLimitError):
        GpuCtcBeamSearchDecoder(ALPHABET, beam_width=0)
    write_synthetic_arpa(tmp_path / "lm.arpa", ALPHABET, 50, order=7, grams_per_order=5)
    with pytest.raises(BeamSearchLimitError):
        GpuCtcBeamSearchDecoder(ALPHABET, NGramLanguageModel(tmp_path / "lm.arpa"))
    assert issubclass(BeamSearchLimitError, ValueError)


@pytest.mark.gpu
def test_wav2letter_gpu_beam_search_predicts_what_the_host_does():
    from speechless_amd import Wav2Letter
    from speechless_amd.net import LabeledSpectrogram
    small = dict(main_filter_count=20, out_filter_count=40, inner_count=1)
    rng = np.random.RandomState(2)
    batch = [LabeledSpectrogram("u{}".format(i), "the cat", rng.randn(90 + 10 * i, 128)) for i in range(3)]
    results = {}
    for device in ("host", "gpu"):
        net = Wav2Letter(128, ALPHABET, kenlm_directory=TOY, seed=5, layer_sizes=small, compute_dtype="f32",
                         beam_search_device=device)
        results[device] = net.test_and_predict_batch(batch).results
    assert [r.predicted for r in results["gpu"]] == [r.predicted for r in results["host"]]
    assert all(math.isclose(g.loss, h.loss, rel_tol=1e-6) for g, h in zip(results["gpu"], results["host"]))
    with pytest.raises(ValueError):
        Wav2Letter(128, ALPHABET, kenlm_directory=TOY, layer_sizes=small, beam_search_device="tpu")
