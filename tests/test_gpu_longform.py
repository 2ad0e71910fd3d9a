"""Long recordings on the GPU: Engine.forward_long against one forward() of the same recording, and Wav2Letter.align_recording /
positional_label_of_recording / predict_recording end to end, on the reference signature (f16x3 evaluation engine) and on
compute_dtype="f32"."""
import numpy as np
import pytest

from test_ctc_align import viterbi

pytestmark = pytest.mark.gpu

LAYER_SIZES = dict(out_filter_count=256)  # (the stack's geometry -- kernel sizes, strides, halo -- is the reference's)
WINDOW = 512
WEIGHT_SEED = 26

# Whether forward_long (windows of 512 input frames in batches of 8) returns the BYTES of one forward() over the whole recording
# as a batch of one, per evaluation arithmetic.  Measured: they are, on both paths, at 1999 and 2000 input
# frames -- an output frame is computed from the same operands in the same order whatever the batch and its place in it.  The
# bound a path that is not would have to keep is asserted beside it: d_ref, the single pass's own distance from the torch-CPU
# float32 port, measured 9.2e-7 .. 9.3e-7 here; on the CPU port the top-two logq margin of these recordings is <= 2e-5 on 2 of
# 1000 frames at most (smallest 8.5e-6), so a d_ref up to ten times the measured one excuses well under the 1 % cap.
BIT_IDENTICAL = {"f16x3": True, "f32": True}

_nets = {}


def _net(kind):
    """one net per arithmetic for the whole module, with fixed glorot weights (the constructor's draw is flat: near-ties)"""
    from oracle import w2l_oracle as o
    from speechless_amd import Wav2Letter, english_frequent_characters
    if kind not in _nets:
        net = Wav2Letter(128, english_frequent_characters, seed=3, layer_sizes=LAYER_SIZES,
                         **({} if kind == "f16x3" else {"compute_dtype": kind}))
        assert net.eval_dtype == kind
        net.predictive_net.set_weights(Wav2Letter._glorot_uniform(o.layer_specs(128, 29, **LAYER_SIZES), WEIGHT_SEED))
        _nets[kind] = net
    return _nets[kind]


def _recording(frames, seed=0):
    return np.random.RandomState(seed + frames).randn(frames, 128).astype(np.float32)


def _cpu_port_logq(net, x):
    """logq of the torch-CPU float32 port (oracle/w2l_torch_cpu.py), the project's yardstick, over the whole recording"""
    import torch
    from oracle import w2l_oracle as o
    from oracle import w2l_torch_cpu as tc
    specs = o.layer_specs(128, 29, **LAYER_SIZES)
    with torch.no_grad():
        w = tc.to_torch_weights(net.predictive_net.get_weights(), requires_grad=False)
        probs = tc.forward_probs(specs, w, torch.from_numpy(x[None])).numpy()
    return o.ctc_log_q(probs.astype(np.float64), 1e-8)[0]


def compare_long_with_single_pass(net, x, report=print):
    """(bit-identical, max |logq difference|, d_ref, frames excused, frames whose argmax differs although not excused)"""
    engine = net.eval_engine
    engine.forward(x[None])
    single_probs = engine.cur.probs.cpu().numpy()[0]
    single = engine.cur.logq.cpu().numpy()[0]
    probs, logq = engine.forward_long(x, WINDOW)
    assert probs.shape == logq.shape == (1, -(-x.shape[0] // 2), 29) and probs.is_cuda and logq.is_cuda
    probs, logq = probs.cpu().numpy()[0], logq.cpu().numpy()[0]
    assert single.shape == logq.shape
    identical = single.tobytes() == logq.tobytes() and single_probs.tobytes() == probs.tobytes()
    diff = float(np.max(np.abs(logq.astype(np.float64) - single)))
    d_ref = float(np.max(np.abs(single.astype(np.float64) - _cpu_port_logq(net, x))))
    top = np.sort(single.astype(np.float64), axis=1)
    margin = top[:, -1] - top[:, -2]
    excused = margin <= 2 * d_ref
    wrong = int(np.sum((np.argmax(logq, axis=1) != np.argmax(single, axis=1)) & ~excused))
    report("forward_long vs forward: {} frames {}: bit-identical {}, max |dlogq| {:.3e}, d_ref {:.3e}, excused {} of {}, "
           "argmax differs on {} others".format(net.eval_dtype, x.shape[0], identical, diff, d_ref, int(excused.sum()),
                                                len(margin), wrong))
    return identical, diff, d_ref, int(excused.sum()), wrong


@pytest.mark.parametrize("frames", [1999, 2000])
@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_forward_long_against_one_forward_pass(kind, frames):
    net = _net(kind)
    x = _recording(frames)
    identical, diff, d_ref, excused, wrong = compare_long_with_single_pass(net, x)
    if BIT_IDENTICAL[kind]:
        assert identical
    # (and in any case what the issue asks of a path that is not: within the single pass's own distance from the CPU port)
    assert diff <= d_ref
    assert excused <= 0.01 * -(-frames // 2)
    assert wrong == 0


class _Example:
    def __init__(self, spectrogram, label):
        self.id, self.label, self._x = "rec", label, spectrogram

    def z_normalized_transposed_spectrogram(self):
        return self._x


def _spy_on_forward_long(engine, seen):
    original = engine.forward_long

    def spy(*args, **kwargs):
        out = original(*args, **kwargs)
        seen.append(out)
        return out
    engine.forward_long = spy
    return original


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_align_recording_end_to_end(kind):
    """A label of about 600 letters over 3000 input frames: alignment_batch refuses it, align_recording returns the restatement's
    score and path on the very logq forward_long stitched."""
    net = _net(kind)
    rng = np.random.RandomState(7)
    words = ["she", "was", "abc", "a", "zoo", "quiet", "morning"]
    label = " ".join(rng.choice(words, size=150))[:600].strip()
    assert 560 < len(label) <= 600
    example = _Example(_recording(3000, seed=1), label)
    with pytest.raises(Exception, match="511"):
        net.alignment_batch([example])
    engine = net.eval_engine
    seen = []
    original = _spy_on_forward_long(engine, seen)
    try:
        a = net.align_recording(example, window_input_frames=WINDOW)
        pl = net.positional_label_of_recording(example, seconds_per_input_step=0.008, window_input_frames=WINDOW)
    finally:
        engine.forward_long = original
    assert len(seen) == 2
    logq = seen[0][1].cpu().numpy()[0]
    assert logq.shape == (1500, 29)
    encoded = [int(c) for c in net.grapheme_encoding.encode_label_batch([label])[0]]
    ref_score, ref_path = viterbi(logq, encoded, 1500, 28)
    assert np.isfinite(ref_score)
    assert np.float32(a.log_probability).tobytes() == np.float32(ref_score).tobytes()
    assert np.array_equal(a.frame_label_positions, np.where(ref_path % 2 == 1, (ref_path - 1) // 2, -1))
    assert a.label == label and len(a.character_frames) == len(label)
    for i, (first, end) in enumerate(a.character_frames):
        assert np.all(a.frame_label_positions[first:end] == i)
        assert np.sum(a.frame_label_positions == i) == end - first
    assert [w for w, _ in a.word_frames] == label.split()
    step = net.input_to_prediction_length_ratio * 0.008
    assert pl is not None and pl.labels == label.split()
    for (_, (s, e)), (_, (first, end)) in zip(pl.labeled_sections, a.word_frames):
        assert s == first * step and e == end * step
    # the sections sections() needs: whole words, in order, none longer than asked unless a single word is
    from speechless_amd import cut_sections
    sections = cut_sections(a, 200)
    assert " ".join(text for text, _ in sections) == " ".join(label.split()) and len(sections) > 3
    assert all(b[1][0] == a_[1][1] for a_, b in zip(sections, sections[1:]))


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_predict_recording(kind):
    from oracle import w2l_oracle as o
    net = _net(kind)
    engine = net.eval_engine
    for frames in (1999, 2000):
        x = _recording(frames, seed=2)
        seen = []
        original = _spy_on_forward_long(engine, seen)
        try:
            text = net.predict_recording(x, window_input_frames=WINDOW)
        finally:
            engine.forward_long = original
        probs = seen[0][0].cpu().numpy()
        want = o.greedy_decode_indices(probs, [frames // 2])[0]
        assert text == net.grapheme_encoding.decode_graphemes(want, merge_repeated=False)
    # a recording that fits one window is a single pass: the transcript of predict_batch_greedily
    x = _recording(401, seed=3)
    assert net.predict_recording(x) == net.predict_batch_greedily([x])[0]
    assert net.predict_recording(_Example(x, "")) == net.predict_batch_greedily([x])[0]


def test_refusals():
    from speechless_amd import Wav2Letter, english_frequent_characters
    x = _recording(300)
    asg = Wav2Letter(128, english_frequent_characters, seed=1, layer_sizes=LAYER_SIZES, criterion="asg")
    with pytest.raises(ValueError, match="criterion='asg'"):
        asg.align_recording(_Example(x, "abc"))
    with pytest.raises(ValueError, match="criterion='asg'"):
        asg.positional_label_of_recording(_Example(x, "abc"), seconds_per_input_step=0.008)
    wave = Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, seed=1, layer_sizes=LAYER_SIZES)
    for call in (lambda: wave.align_recording(_Example(x[:, :1], "abc")), lambda: wave.predict_recording(x[:, :1])):
        with pytest.raises(ValueError, match="use_raw_wave_input=True is not supported .*out of scope"):
            call()
    net = _net("f32")
    with pytest.raises(ValueError, match="at most 8191"):
        net.align_recording(_Example(x, "ab" * 4096))
    with pytest.raises(ValueError, match="at most 8191"):
        net.eval_engine.ctc_align_long(net.eval_engine.forward_long(x)[1], np.zeros((1, 8192), dtype=np.int32), [8192], [150])
