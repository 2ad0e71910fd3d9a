"""The ASG beam search on the GPU (asg_beam.hip, GpuAsgBeamSearchDecoder) against its float32 restatement
(tests/asg_beam_ref.py) with ZERO tolerance: the same grapheme lists and bit-equal scores."""
from pathlib import Path

import numpy as np
import pytest

from asg_beam_ref import asg_beam_search_batch
from test_asg_beam import exported_scorer

pytestmark = pytest.mark.gpu

TOY = Path(__file__).resolve().parent / "golden" / "toy_kenlm"
ALPHABET = list("acehost ")
ENGLISH = list("abcdefghijklmnopqrstuvwxyz' ")
SMALL = dict(main_filter_count=20, out_filter_count=40, inner_count=1)  # the toy stack of the other GPU tests
SEED = 6  # at beam widths <= 8 these inputs hold merges and returning prefixes (asserted below from the restatement)


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


def random_case(seed, b, t, k):
    rng = np.random.RandomState(seed)
    return ((rng.randn(b, t, k) * 2).astype(np.float32), rng.uniform(-2, 2, size=(k, k)).astype(np.float32),
            rng.uniform(-2, 2, size=k).astype(np.float32))


def assert_bits(characters, lm, weights, beam_width, logq, trans, init, lengths):
    """decode on the GPU and by the restatement: equal lists, bit-equal scores; returns the restatement's result"""
    from speechless_amd.decoder import GpuAsgBeamSearchDecoder
    kw = {} if weights is None or lm is None else dict(kenlm_weight=weights[0], word_count_weight=weights[1],
                                                     valid_word_count_weight=weights[2])
    gpu = GpuAsgBeamSearchDecoder(characters, lm, beam_width=beam_width, **kw)
    scorer = exported_scorer(characters, lm, **({"weights": weights} if weights else {})) if lm is not None else None
    got, got_score = gpu.decode(logq, trans, init, lengths)
    want, want_score, merges, returns = asg_beam_search_batch(logq, trans, init, lengths, beam_width, scorer)
    for i in range(len(want)):
        assert got[i] == want[i], (i, got[i], want[i])
    assert got_score.dtype == np.float32 and got_score.tobytes() == want_score.tobytes(), (got_score, want_score)
    return want, want_score, merges, returns


@pytest.mark.parametrize("beam_width", [1, 2, 8, 64, 128])
@pytest.mark.parametrize("weights", [None, (.8, 0., 2.3), (1.5, 1.0, 0.0)])
def test_restatement_parity_plain_and_toy_language_model(toy_lm, beam_width, weights):
    logq, trans, init = random_case(SEED, 6, 60, len(ALPHABET) + 2)
    lengths = [60, 1, 33, 0, 59, 12]
    _, _, merges, returns = assert_bits(ALPHABET, toy_lm if weights else None, weights, beam_width, logq, trans, init,
                                        lengths)
    if 2 <= beam_width <= 8:  # both rules of the definition are exercised (a beam of one holds no parent and child)
        assert merges >= 1 and returns >= 1, (merges, returns)


@pytest.mark.parametrize("t_max, beam_width, seed", [(5, 2, 5), (8, 3, 6)])
def test_smallest_node_table_with_returning_prefixes(toy_lm, t_max, beam_width, seed):
    """k = 5 and 11 / 25 nodes at most: hash maps of 32 / 64 slots (the floor is 16), whose probe chains wrap, with prefixes
    that leave the beam and return (the seeds were chosen on the restatement for that, with and without the model); a row of
    one frame and a row of none beside them: the root alone, and the backtrace of a one-node arena."""
    characters = list("at ")
    logq, trans, init = random_case(seed, 5, t_max, len(characters) + 2)
    for lm in (None, toy_lm):
        want, _, merges, returns = assert_bits(characters, lm, None, beam_width, logq, trans, init,
                                               [t_max, 1, 0, t_max - 1, t_max])
        assert merges >= 1 and returns >= 1, (merges, returns)
        assert len(want[1]) == 1 and want[2] == []


@pytest.mark.parametrize("k", [30, 64])
def test_class_counts_with_an_order_4_model(order4_lm, k):
    logq, trans, init = random_case(3, 2, 40, k)
    # (k = 64: the English characters and 34 more letters that no word of the model uses)
    characters = ENGLISH + [chr(0x100 + i) for i in range(k - 30)]
    assert_bits(characters, order4_lm, None, 100, logq, trans, init, [40, 37])


@pytest.mark.parametrize("beam_width", [3, 128])
def test_ties_are_broken_by_the_order_rules_alone(beam_width):
    k = 10
    logq = np.full((2, 12, k), -np.log(k), dtype=np.float32)
    trans, init = np.zeros((k, k), dtype=np.float32), np.zeros((k,), dtype=np.float32)
    want, _, _, _ = assert_bits(ALPHABET, None, None, beam_width, logq, trans, init, [12, 5])
    assert want == [[0], [0]]


def test_minus_infinity_scores(toy_lm):
    k = len(ALPHABET) + 2
    logq, trans, init = random_case(9, 3, 20, k)
    trans[3, :] = -np.inf
    trans[:, 6] = -np.inf
    for lm in (None, toy_lm):
        assert_bits(ALPHABET, lm, None, 8, logq, trans, init, [20, 7, 1])
    dead = np.full((k,), -np.inf, dtype=np.float32)
    want, want_score, _, _ = assert_bits(ALPHABET, toy_lm, None, 8, logq, trans, dead, [20, 7, 1])
    assert want == [[], [], []] and np.isneginf(want_score).all()


def test_an_exhaustive_beam_is_the_viterbi_decode(hip_lib):
    from test_gpu_asg import run_viterbi_kernel
    from speechless_amd.decoder import GpuAsgBeamSearchDecoder
    logq, trans, init = random_case(21, 8, 3, 5)
    lengths = [3, 3, 3, 2, 3, 1, 3, 3]
    got, score = GpuAsgBeamSearchDecoder(list("at "), beam_width=128).decode(logq, trans, init, lengths)
    paths, vit_score, _ = run_viterbi_kernel(hip_lib, logq, trans, init, lengths)
    assert score.tobytes() == vit_score.tobytes()
    for i, row in enumerate(paths):
        row = row[row >= 0]
        assert got[i] == [int(g) for g in row[np.concatenate([[True], row[1:] != row[:-1]])]]


def test_repeat_marks_reach_the_transcript(toy_lm):
    from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
    enc = AsgGraphemeEncoding(ALPHABET)
    graphemes = enc.encode("coo taaat")  # a doubled and a tripled letter: c o <2> ' ' t a <3> t
    assert enc.asg_twice in graphemes and enc.asg_thrice in graphemes
    k = enc.grapheme_set_size
    rng = np.random.RandomState(4)
    logq = rng.randn(1, 3 * len(graphemes), k).astype(np.float32)
    for t in range(logq.shape[1]):
        logq[0, t, graphemes[t // 3]] += 12.0
    trans, init = np.zeros((k, k), dtype=np.float32), np.zeros((k,), dtype=np.float32)
    for lm in (None, toy_lm):
        want, _, _, _ = assert_bits(ALPHABET, lm, None, 16, logq, trans, init, [logq.shape[1]])
        assert want == [graphemes]
        assert enc.decode_graphemes(want[0], merge_repeated=False) == "coo taaat"


def test_numpy_and_device_tensor_inputs_agree(toy_lm):
    import torch
    from speechless_amd.decoder import GpuAsgBeamSearchDecoder
    logq, trans, init = random_case(2, 3, 25, len(ALPHABET) + 2)
    lengths = np.array([25, 11, 19])
    gpu = GpuAsgBeamSearchDecoder(ALPHABET, toy_lm, beam_width=16)
    a, a_score = gpu.decode(logq, trans, init, lengths)
    dev = [torch.from_numpy(x).cuda() for x in (logq, trans, init, lengths)]
    b, b_score = gpu.decode(*dev)
    assert a == b and a_score.tobytes() == b_score.tobytes()


def test_limits_raise_a_named_value_error(hip_lib):
    from speechless_amd.decoder import BeamSearchLimitError, GpuAsgBeamSearchDecoder
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder(ALPHABET, beam_width=129)
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder([chr(0x100 + i) for i in range(63)])
    assert hip_lib.raw("sl_asg_beam_search_workspace_bytes")(1, 6, 65, 8) == 0
    assert hip_lib.raw("sl_asg_beam_search_workspace_bytes")(1, 6, 10, 129) == 0
    assert hip_lib.raw("sl_asg_beam_search_workspace_bytes")(1, 1 << 18, 10, 128) == 0
    gpu = GpuAsgBeamSearchDecoder(ALPHABET, beam_width=128)
    with pytest.raises(BeamSearchLimitError):  # t_out * beam_width beyond the 25-bit node ids: a 0 workspace size
        gpu.decode(np.zeros((1, 1 << 18, 10), dtype=np.float32), np.zeros((10, 10)), np.zeros(10), [4])
    with pytest.raises(ValueError):
        gpu.decode(np.zeros((1, 4, 9), dtype=np.float32), np.zeros((9, 9)), np.zeros(9), [4])


def test_wav2letter_asg_decodes_with_the_language_model():
    from speechless_amd import Wav2Letter
    from speechless_amd.net import LabeledSpectrogram
    rng = np.random.RandomState(2)
    batch = [LabeledSpectrogram("u{}".format(i), "the cat", rng.randn(90 + 10 * i, 128)) for i in range(2)]
    scores = np.random.RandomState(6)
    trans, init = scores.uniform(-1, 1, size=(10, 10)), scores.uniform(-1, 1, size=10)
    predicted = {}
    for directory in (TOY, None):
        net = Wav2Letter(128, ALPHABET, criterion="asg", kenlm_directory=directory, seed=5, layer_sizes=SMALL,
                         compute_dtype="f32", beam_search_device="gpu")
        net.engine.set_asg_scores(trans, init)
        predicted[directory] = [r.predicted for r in net.test_and_predict_batch(batch).results]
        engine = net.eval_engine
        logq, lengths = engine.cur.logq.cpu().numpy(), engine.cur.input_len.cpu().numpy()
        state = engine.get_asg_state()
        enc = net.grapheme_encoding
        if directory is not None:
            scorer = exported_scorer(ALPHABET, net._beam_decoder.language_model)
            want, _, _, _ = asg_beam_search_batch(logq, state["trans"], state["init"], lengths,
                                                  net._beam_decoder.beam_width, scorer)
            assert predicted[directory] == [enc.decode_graphemes(w, merge_repeated=False) for w in want]
        else:
            assert net._beam_decoder is None
            viterbi, _ = engine.asg_viterbi()
            assert predicted[directory] == [enc.decode_graphemes(w, merge_repeated=False) for w in viterbi]
