"""engine_decode.check_label_batch on the host: what the four forced aligners and Engine.set_labels ask of a label batch,
for both criteria.  No GPU, no library: the function takes arrays and returns arrays.  The fragments matched here are the
ones the GPU tests of the aligners match on."""
import numpy as np
import pytest

from speechless_amd.engine_decode import check_label_batch

K = 30
KINDS = {"ctc": dict(n_labels=K - 1, blank=K - 1), "asg": dict(n_labels=K, blank=None)}


def check(kind, labels, lengths, batch, **kw):
    rule = KINDS[kind]
    return check_label_batch(labels, lengths, batch, rule["n_labels"], blank=rule["blank"], **kw)


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_accepted_batches_come_back_as_int32(kind):
    labels = [[3, 7, 7, 0], [5, 99, -1, -1]]  # (padding may hold anything)
    for lengths in ([4, 1], np.array([[4], [1]]), np.array([4, 1], dtype=np.int64)):
        got, got_len = check(kind, labels, lengths, 2)
        assert got.dtype == np.int32 and got.shape == (2, 4) and np.array_equal(got, labels)
        assert got_len.dtype == np.int32 and got_len.tolist() == [4, 1]
    # an empty label beside a full one, and a batch of no columns at all
    check(kind, labels, [0, 1], 2)
    got, got_len = check(kind, np.zeros((2, 0), dtype=np.int32), [0, 0], 2)
    assert got.shape == (2, 0) and got_len.tolist() == [0, 0]


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_shapes_and_lengths_are_refused(kind):
    labels = np.zeros((2, 4), dtype=np.int32)
    for bad_labels, bad_lengths in ((np.zeros((3, 4), dtype=np.int32), [1, 1]), (np.zeros(4, dtype=np.int32), [1, 1]),
                                    (labels, [1, 1, 1]), (labels, [1])):
        with pytest.raises(ValueError, match=r"label batch must be \(B, Lmax\) with B lengths$"):
            check(kind, bad_labels, bad_lengths, 2)
    with pytest.raises(ValueError, match=r"label length -1 of utterance 1 outside \[0, 4\]"):
        check(kind, labels, [4, -1], 2)
    with pytest.raises(ValueError, match=r"label length 5 of utterance 0 outside \[0, 4\]"):
        check(kind, labels, [5, 1], 2)


def test_the_blank_is_no_label_under_ctc_and_the_last_class_is_one_under_asg():
    labels = np.array([[0, 1], [2, K - 1]], dtype=np.int32)
    with pytest.raises(ValueError, match=r"label 1 holds an index outside \[0, 29\) \(blank is 29\)$"):
        check("ctc", labels, [2, 2], 2)
    check("ctc", labels, [2, 1], 2)  # (beyond the length it is padding)
    check("asg", labels, [2, 2], 2)
    labels[0, 1] = K
    with pytest.raises(ValueError, match=r"label 0 holds an index outside \[0, 30\)$") as error:
        check("asg", labels, [2, 2], 2)
    assert "blank is" not in str(error.value)
    labels[0, 1] = -1
    for kind in KINDS:
        with pytest.raises(ValueError, match="label 0 holds an index outside"):
            check(kind, labels, [2, 1], 2)


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_long_aligners_state_their_width_limit_and_count_three_lengths(kind):
    text = "labels of {} letters: forced alignment takes at most {} (an entry point)"
    in_len = np.array([9, 9], dtype=np.int32)
    check(kind, np.zeros((2, 6), dtype=np.int32), [6, 2], 2, in_len=in_len, max_letters=6, too_long_text=text)
    with pytest.raises(ValueError, match=r"labels of 7 letters: forced alignment takes at most 6 \(an entry point\)"):
        check(kind, np.zeros((2, 7), dtype=np.int32), [1, 1], 2, in_len=in_len, max_letters=6, too_long_text=text)
    # the width is refused before any row is looked at, the shapes before the width
    with pytest.raises(ValueError, match="at most 6"):
        check(kind, np.full((2, 7), -5, dtype=np.int32), [9, 9], 2, in_len=in_len, max_letters=6, too_long_text=text)
    for bad_in_len, lengths in ((np.array([9], dtype=np.int32), [1, 1]), (in_len, [1, 1, 1])):
        with pytest.raises(ValueError, match="label batch must be .* with B label lengths and B prediction lengths"):
            check(kind, np.zeros((2, 7), dtype=np.int32), lengths, 2, in_len=bad_in_len, max_letters=6, too_long_text=text)


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_set_labels_mode_checks_the_indices_and_not_the_lengths(kind):
    labels = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    # a length beyond the width takes the whole row, and nobody counts the lengths: Engine.set_labels has always been so
    got, got_len = check(kind, labels, [7, 3, 1], 2, check_lengths=False)
    assert np.array_equal(got, labels) and got_len.tolist() == [7, 3, 1]
    with pytest.raises(ValueError, match="outside"):
        check(kind, labels, [7, 3], 2)
    # the rows it does look at are held to the same rule, with the same text
    labels[1, 2] = K
    with pytest.raises(ValueError, match=r"label 1 holds an index outside \[0, (29\) \(blank is 29\)|30\))$"):
        check(kind, labels, [7, 3], 2, check_lengths=False)
