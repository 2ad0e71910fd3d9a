"""Long recordings under criterion="asg" on the GPU: Wav2Letter.asg_align_recording / asg_positional_label_of_recording /
predict_recording end to end on the small net of tests/test_gpu_longform.py, on the reference signature (f16x3 evaluation
engine) and on compute_dtype="f32" -- against sl_asg_align on one forward() of the same recording, and against the float32
restatements on the very logq forward_long stitched."""
import numpy as np
import pytest

from asg_align_long_ref import asg_align_long_reference
from test_asg import asg_viterbi
from test_gpu_longform import LAYER_SIZES, WEIGHT_SEED, WINDOW, _Example, _recording, _spy_on_forward_long

pytestmark = pytest.mark.gpu

F32 = np.float32
WORDS = ["she", "was", "abc", "a", "zoo", "quiet", "morning", "all", "feet"]  # (runs of two: repeat marks in the encoded label)
_nets = {}


def _net(kind):
    """one ASG net per arithmetic for the whole module: fixed glorot weights, scores of order 1"""
    from oracle import w2l_oracle as o
    from speechless_amd import Wav2Letter, english_frequent_characters
    if kind not in _nets:
        net = Wav2Letter(128, english_frequent_characters, seed=3, layer_sizes=LAYER_SIZES, criterion="asg",
                         **({} if kind == "f16x3" else {"compute_dtype": kind}))
        assert net.eval_dtype == kind and net.grapheme_encoding.grapheme_set_size == 30
        net.predictive_net.set_weights(Wav2Letter._glorot_uniform(o.layer_specs(128, 30, **LAYER_SIZES), WEIGHT_SEED))
        rng = np.random.RandomState(17)
        net.engine.set_asg_scores(rng.uniform(-1, 1, size=(30, 30)), rng.uniform(-1, 1, size=30))
        _nets[kind] = net
    return _nets[kind]


def _label(rng, enc, graphemes):
    """words until one more would take the ENCODED label beyond `graphemes` graphemes"""
    words = []
    while True:
        word = str(rng.choice(WORDS))
        if len(enc.encode(" ".join(words + [word]))) > graphemes:
            return " ".join(words)
        words.append(word)


def _spied(net, call):
    """call() with Engine.forward_long watched: (its result, the logq tensors forward_long returned as numpy (T', K))"""
    engine = net.eval_engine
    seen = []
    original = _spy_on_forward_long(engine, seen)
    try:
        out = call()
    finally:
        engine.forward_long = original
    return out, [logq.cpu().numpy()[0] for _, logq in seen]


@pytest.mark.parametrize("frames", [1999, 2000])
@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_asg_align_recording_equals_the_one_pass_alignment_and_the_restatement(kind, frames):
    net = _net(kind)
    enc = net.grapheme_encoding
    label = _label(np.random.RandomState(frames), enc, 400)
    encoded = enc.encode(label)
    assert 380 < len(encoded) <= 400 and enc.asg_twice in encoded
    x = _recording(frames, seed=4)
    t_b = frames // 2
    a, stitched = _spied(net, lambda: net.asg_align_recording(_Example(x, label), window_input_frames=WINDOW))
    assert len(stitched) == 1 and stitched[0].shape == (-(-frames // 2), 30)
    state = net.eval_engine.get_asg_state()
    # the restatement on the stitched logq
    ref_score, ref_path = asg_align_long_reference(stitched[0], state["trans"], state["init"], encoded, len(encoded), t_b)
    assert np.isfinite(ref_score)
    assert F32(a.log_probability).tobytes() == F32(ref_score).tobytes()
    assert a.frame_grapheme_positions.dtype == np.int32 and np.array_equal(a.frame_grapheme_positions, ref_path)
    # sl_asg_align on one forward() of the recording as a batch of one
    engine = net.eval_engine
    engine.forward(x[None])
    paths, scores = engine.asg_align(np.asarray([encoded], dtype=np.int32), [len(encoded)], [t_b])
    assert paths[0].tobytes() == a.frame_grapheme_positions.tobytes() and F32(scores[0]).tobytes() == F32(a.log_probability).tobytes()
    # the grapheme ranges tile [0, T_b)
    assert a.feasible and a.label == label and a.encoded_label == encoded and len(a.grapheme_frames) == len(encoded)
    assert a.grapheme_frames[0][0] == 0 and a.grapheme_frames[-1][1] == t_b
    assert all(p[1] == q[0] and p[0] < p[1] for p, q in zip(a.grapheme_frames[:-1], a.grapheme_frames[1:]))
    assert (a.frame_grapheme_positions[t_b:] == -1).all()
    assert len(a.character_frames) == len(label) and [w for w, _ in a.word_frames] == label.split()


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_predict_recording_decodes_the_viterbi_path_of_the_stitched_emissions(kind):
    net = _net(kind)
    enc = net.grapheme_encoding
    state = net.eval_engine.get_asg_state()
    for frames in (1999, 2000):
        x = _recording(frames, seed=2)
        text, stitched = _spied(net, lambda: net.predict_recording(x, window_input_frames=WINDOW))
        assert len(stitched) == 1
        assert text == net.predict_batch_greedily([x])[0]
        t_b = frames // 2
        _, path = asg_viterbi(stitched[0][:t_b], state["trans"], state["init"], t_b)
        merged = [int(g) for i, g in enumerate(path) if i == 0 or g != path[i - 1]]
        assert text == enc.decode_graphemes(merged, merge_repeated=False)
    # a recording that fits one window is a single pass: the transcript of predict_batch_greedily
    x = _recording(401, seed=3)
    assert net.predict_recording(x) == net.predict_batch_greedily([x])[0]
    assert net.predict_recording(_Example(x, "")) == net.predict_batch_greedily([x])[0]


def test_word_timings_of_a_recording():
    from speechless_amd import cut_sections
    net = _net("f32")
    label = _label(np.random.RandomState(5), net.grapheme_encoding, 300)
    example = _Example(_recording(2000, seed=6), label)
    a = net.asg_align_recording(example, window_input_frames=WINDOW)
    pl = net.asg_positional_label_of_recording(example, seconds_per_input_step=0.008, window_input_frames=WINDOW)
    ratio = net.input_to_prediction_length_ratio
    assert pl is not None and pl.labels == label.split() and len(pl.labels) > 40
    want = a.positional_label(ratio * 0.008)
    assert pl.labeled_sections == want.labeled_sections
    ranges = [r for _, r in pl.labeled_sections]
    assert all(start < end for start, end in ranges)  # ordered and non-overlapping
    assert all(p[1] <= q[0] for p, q in zip(ranges[:-1], ranges[1:]))
    assert ranges[0][0] >= 0 and ranges[-1][1] <= 1000 * ratio * 0.008
    for (_, (start, end)), (_, (first, last)) in zip(pl.labeled_sections, a.word_frames):
        assert start == first * (ratio * 0.008) and end == last * (ratio * 0.008)
    with pytest.raises(ValueError, match="seconds_per_input_step"):  # (the example carries no sample rate to go by)
        net.asg_positional_label_of_recording(example, window_input_frames=WINDOW)
    sections = cut_sections(a, 200)  # the sections a corpus reader needs: whole words, in order, abutting
    assert " ".join(text for text, _ in sections) == " ".join(label.split()) and len(sections) > 3
    assert all(q[1][0] == p[1][1] for p, q in zip(sections, sections[1:]))


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_a_label_beyond_511_encoded_graphemes(kind):
    """About 600 graphemes over 1400 input frames: asg_alignment_batch refuses it, asg_align_recording returns the
    restatement's score and path on the logq forward_long stitched."""
    net = _net(kind)
    enc = net.grapheme_encoding
    label = _label(np.random.RandomState(9), enc, 600)
    encoded = enc.encode(label)
    assert 580 < len(encoded) <= 600
    example = _Example(_recording(1400, seed=1), label)
    with pytest.raises(Exception, match="511"):
        net.asg_alignment_batch([example])
    a, stitched = _spied(net, lambda: net.asg_align_recording(example, window_input_frames=WINDOW))
    state = net.eval_engine.get_asg_state()
    ref_score, ref_path = asg_align_long_reference(stitched[0], state["trans"], state["init"], encoded, len(encoded), 700)
    assert np.isfinite(ref_score) and stitched[0].shape == (700, 30)
    assert F32(a.log_probability).tobytes() == F32(ref_score).tobytes()
    assert np.array_equal(a.frame_grapheme_positions, ref_path)
    assert a.grapheme_frames[0][0] == 0 and a.grapheme_frames[-1][1] == 700 and len(a.grapheme_frames) == len(encoded)
    assert [w for w, _ in a.word_frames] == label.split()


def test_refusals():
    import torch
    from speechless_amd import Wav2Letter, english_frequent_characters
    x = _recording(300)
    ctc = Wav2Letter(128, english_frequent_characters, seed=1, layer_sizes=LAYER_SIZES)
    with pytest.raises(ValueError, match="criterion='asg'"):
        ctc.asg_align_recording(_Example(x, "abc"))
    with pytest.raises(ValueError, match="criterion='asg'"):
        ctc.asg_positional_label_of_recording(_Example(x, "abc"), seconds_per_input_step=0.008)
    logq = torch.zeros((1, 150, 29), dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError, match="criterion='asg'"):
        ctc.eval_engine.asg_align_long(logq, np.zeros((1, 3), dtype=np.int32), [3], [150])
    with pytest.raises(ValueError, match="criterion='asg'"):
        ctc.eval_engine.asg_viterbi_long(logq)
    wave = Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, seed=1, layer_sizes=LAYER_SIZES,
                      criterion="asg")
    for call in (lambda: wave.asg_align_recording(_Example(x[:, :1], "abc")),
                 lambda: wave.asg_positional_label_of_recording(_Example(x[:, :1], "abc"), seconds_per_input_step=0.008),
                 lambda: wave.predict_recording(x[:, :1])):
        with pytest.raises(ValueError, match="use_raw_wave_input=True is not supported .*out of scope"):
            call()
    net = _net("f32")
    long_label = "ab" * 4096  # 8192 encoded graphemes, no run at all
    assert len(net.grapheme_encoding.encode(long_label)) == 8192
    with pytest.raises(ValueError, match="at most 8191"):
        _, stitched = _spied(net, lambda: net.asg_align_recording(_Example(x, long_label)))
    engine = net.eval_engine
    seen = []
    original = _spy_on_forward_long(engine, seen)
    try:
        with pytest.raises(ValueError, match="at most 8191"):
            net.asg_positional_label_of_recording(_Example(x, long_label), seconds_per_input_step=0.008)
    finally:
        engine.forward_long = original
    assert seen == []  # refused before any GPU work
    # 8191 encoded graphemes written with runs of two and three pass the check of the label (and find too few frames)
    a = net.asg_align_recording(_Example(x, "aab" * 2730 + "a"))
    assert len(a.encoded_label) == 8191 and not a.feasible and a.word_frames == []
    logq = engine.forward_long(x)[1]
    with pytest.raises(ValueError, match="at most 8191"):
        engine.asg_align_long(logq, np.zeros((1, 8192), dtype=np.int32), [8192], [150])
    with pytest.raises(ValueError, match="outside"):
        engine.asg_align_long(logq, np.full((1, 4), 30, dtype=np.int32), [4], [150])


def test_the_ctc_entry_points_still_refuse_an_asg_net():
    net = _net("f32")
    x = _recording(300)
    with pytest.raises(ValueError, match="criterion='asg'"):
        net.align_recording(_Example(x, "abc"))
    with pytest.raises(ValueError, match="criterion='asg'"):
        net.positional_label_of_recording(_Example(x, "abc"), seconds_per_input_step=0.008)
    with pytest.raises(ValueError, match="criterion='asg'"):
        net.eval_engine.ctc_align_long(net.eval_engine.forward_long(x)[1], np.zeros((1, 3), dtype=np.int32), [3], [150])
