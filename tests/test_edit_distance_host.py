"""Host side of the GPU error counts (no GPU needed): ExpectationVsPrediction with given counts, the error_count_device
keyword's validation, and the helpers of speechless_amd/error_counts.py against str.split() and net.edit_distance."""
import numpy as np
import pytest

SMALL = dict(main_filter_count=20, out_filter_count=40, inner_count=1)


def test_expectation_vs_prediction_reports_given_counts():
    from speechless_amd.net import ExpectationVsPrediction, ExpectationsVsPredictions
    given = ExpectationVsPrediction("the cat sat", "the hat", 1.5, letter_error_count=40, word_error_count=6)
    assert (given.letter_error_count, given.word_error_count) == (40, 6)  # stored as they are, right or wrong
    assert given.expected_letter_count == 11 and given.expected_words == ["the", "cat", "sat"]
    assert given.expected_word_count == 3 and given.letter_error_rate == 40 / 11 and given.word_error_rate == 2.0
    assert "Errors: 40 letters (364%), 6 words (200%), loss: 1.50." in str(given)
    assert ExpectationsVsPredictions([given]).average_word_error_count == 6
    # a given zero is a count, not a request to compute one
    zero = ExpectationVsPrediction("the cat", "a dog", 0.0, letter_error_count=0, word_error_count=0)
    assert (zero.letter_error_count, zero.word_error_count) == (0, 0)
    one = ExpectationVsPrediction("the cat", "a dog", 0.0, letter_error_count=3)
    assert (one.letter_error_count, one.word_error_count) == (3, 2)


def test_expectation_vs_prediction_without_counts_is_unchanged():
    from speechless_amd.net import ExpectationVsPrediction, edit_distance
    r = ExpectationVsPrediction("the cat sat", "the hat", 1.5)
    assert r.letter_error_count == edit_distance("the cat sat", "the hat") == 5
    assert r.word_error_count == edit_distance(["the", "cat", "sat"], ["the", "hat"]) == 2
    assert str(r) == 'Expected:  "the cat sat"\nPredicted: "the hat"\nErrors: 5 letters (45%), 2 words (67%), loss: 1.50.'
    positional = ExpectationVsPrediction("a", "b", 2.0)
    keyword = ExpectationVsPrediction(predicted="b", expected="a", loss=2.0)
    assert vars(positional) == vars(keyword)


def test_error_count_device_validation():
    """both messages come before any engine is built: no GPU needed"""
    from speechless_amd import Wav2Letter, english_frequent_characters
    with pytest.raises(ValueError, match="error_count_device must be 'host' or 'gpu', not 'tpu'"):
        Wav2Letter(128, english_frequent_characters, layer_sizes=SMALL, error_count_device="tpu")
    with pytest.raises(ValueError, match=r"allowed_characters holds the whitespace character '\\t'"):
        Wav2Letter(128, list("ab \t"), layer_sizes=SMALL, error_count_device="gpu")
    with pytest.raises(ValueError, match=r"whitespace character '\\xa0'"):
        Wav2Letter(128, list("ab\xa0"), layer_sizes=SMALL, error_count_device="gpu")


def test_space_index_of():
    from speechless_amd import english_frequent_characters, german_frequent_characters
    from speechless_amd.error_counts import space_index_of
    assert space_index_of(english_frequent_characters) == list(english_frequent_characters).index(" ")
    assert space_index_of(german_frequent_characters) == list(german_frequent_characters).index(" ")
    assert space_index_of("abc") == -1 and space_index_of(" ab") == 0
    with pytest.raises(ValueError, match="'\\\\n'"):
        space_index_of("ab \n")


def test_word_spans_against_str_split():
    from speechless_amd.error_counts import host_counts, word_spans
    from speechless_amd.net import edit_distance
    alphabet = "ab "
    rng = np.random.RandomState(11)
    texts = ["", " ", "  ", "a", " a", "a ", "a  b", "ab", "  ab  ba "]
    texts += ["".join(alphabet[i] for i in rng.randint(0, 3, size=rng.randint(0, 25))) for _ in range(300)]
    rows = [[alphabet.index(c) for c in text] for text in texts]
    for text, row in zip(texts, rows):
        spans = word_spans(row, 2)
        assert [text[s:s + n] for s, n in spans] == text.split()
        assert all(n > 0 for _, n in spans)
        assert word_spans(row, -1) == ([(0, len(row))] if row else [])
    others = rows[1:] + rows[:1]
    letters, words = host_counts(rows, others, 2)
    assert letters.dtype == np.int32 and words.dtype == np.int32
    assert letters.tolist() == [edit_distance(a, b) for a, b in zip(texts, texts[1:] + texts[:1])]
    assert words.tolist() == [edit_distance(a.split(), b.split()) for a, b in zip(texts, texts[1:] + texts[:1])]


def test_pack_rows():
    from speechless_amd.error_counts import pack_rows
    packed, lengths = pack_rows([[1, 2, 3], [], [4]])
    assert packed.dtype == np.int32 and packed.tolist() == [[1, 2, 3], [-1, -1, -1], [4, -1, -1]]
    assert lengths.dtype == np.int32 and lengths.tolist() == [3, 0, 1]
    packed, lengths = pack_rows([[], []])
    assert packed.shape == (2, 1) and lengths.tolist() == [0, 0]  # (a row is never narrower than one entry)
