"""Long recordings without a GPU: the window plan (speechless_amd/longform.py) as a property test and against the float64 oracle
run over whole recordings, alignment.cut_sections, and the host-side refusals of sl_ctc_align_long."""
import numpy as np
import pytest

from speechless_amd.longform import Window, halo, valid_output_range, window_plan
from speechless_amd.plan import LayerPlan, wav2letter_layer_specs

WINDOWS = (256, 512, 513)


def _frame_counts(window):
    return sorted({1, 2, 47, 48, window - 1, window, window + 1, window + 2, 1999, 2000, 5001})


def _default_plans():
    specs = wav2letter_layer_specs(128, 29)
    return [LayerPlan(i, s, 128, 128, 0, 0) for i, s in enumerate(specs)]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("layers", ["specs", "plans"])
def test_window_plan_tiles_the_output_exactly_once(window, layers):
    stack = wav2letter_layer_specs(128, 29) if layers == "specs" else _default_plans()
    ratio = 2
    for total in _frame_counts(window):
        plan = window_plan(total, stack, window)
        frames_out = -(-total // ratio)
        assert all(isinstance(w, Window) for w in plan)
        # the destination ranges tile [0, ceil(T / ratio)) exactly once, in order
        assert plan[0].out_start == 0 and plan[-1].out_end == frames_out
        for a, b in zip(plan, plan[1:]):
            assert a.out_end == b.out_start
        for w in plan:
            assert w.out_end > w.out_start and w.out_end - w.out_start == w.keep_end - w.keep_start
            assert w.input_start % ratio == 0
            assert w.out_start == w.input_start // ratio + w.keep_start      # kept frames land where they came from
            assert 0 <= w.keep_start and w.keep_end <= -(-w.input_length // ratio)
            assert 0 <= w.input_start and w.input_start + w.input_length <= total
        assert len({w.input_length for w in plan}) == 1 and plan[0].input_length <= window
        assert plan[0].input_start == 0 and plan[-1].input_start + plan[-1].input_length == total
        if total <= window:
            assert plan == [Window(0, total, 0, frames_out, 0, frames_out)]
        else:
            assert len(plan) >= 2


def test_halo_is_derived_from_the_layers():
    """Default stack: striding_conv (48 taps, stride 2, pad 23 | 24 or 23) loses ceil(23 / 2) = 12 | 12 output frames, seven
    inner layers (7 taps) 3 each, big_conv_1 (32 taps, pad 15 | 16) 15 | 16; the 1 x 1 layers nothing."""
    assert halo(wav2letter_layer_specs(128, 29)) == (12 + 21 + 15, 12 + 21 + 16)
    assert halo(_default_plans()) == (48, 49)
    # a stack of 1 x 1 layers loses nothing; a shallower one less
    assert halo(wav2letter_layer_specs(128, 29, inner_count=0, big_kernel=1, striding_kernel=2)) == (0, 0)
    assert halo(wav2letter_layer_specs(128, 29, inner_count=2)) == (12 + 6 + 15, 12 + 6 + 16)
    assert valid_output_range(512, _default_plans(), True, True) == (0, 256, 256)
    assert valid_output_range(512, _default_plans(), False, False) == (48, 256 - 49, 256)
    with pytest.raises(ValueError, match="too short"):
        window_plan(1000, wav2letter_layer_specs(128, 29), 190)  # 95 output frames < 48 + 49 + 1
    with pytest.raises(ValueError, match="depends on the frame count"):
        window_plan(1000, wav2letter_layer_specs(128, 29, striding_kernel=47), 512)


@pytest.mark.parametrize("total", [700, 701, 1500])
def test_window_plan_reproduces_a_single_float64_pass(total):
    """forward_stack over the whole recording == the same function over the planned windows, stitched: <= 1e-12 in float64.
    (With the halo reduced by one output frame, on the left or on the right, the difference is 2e-8 .. 2e-7 at each of the three
    lengths -- one frame of padding reaches the kept frame through a single tap of every layer -- so the check fails: shown by
    hand, not kept as a test.)"""
    from oracle import w2l_oracle as o
    specs = o.layer_specs(16, 29, main_filter_count=8, out_filter_count=16)
    weights = o.glorot_uniform_weights(specs, seed=3, dtype=np.float64)
    # (biases away from zero: a frame computed from padding must differ from the real one in every layer)
    rng = np.random.RandomState(total)
    weights = [(w, rng.uniform(-0.2, 0.2, size=b.shape)) for w, b in weights]
    x = rng.randn(total, 16)
    whole = o.forward_stack(specs, weights, x[None])[0]
    plan = window_plan(total, specs, 256)
    assert len(plan) > 3
    stitched = np.full_like(whole, np.nan)
    for w in plan:
        part = o.forward_stack(specs, weights, x[None, w.input_start:w.input_start + w.input_length])[0]
        stitched[w.out_start:w.out_end] = part[w.keep_start:w.keep_end]
    assert whole.shape == (-(-total // 2), 29)
    assert np.max(np.abs(stitched - whole)) <= 1e-12


class _Aligned:
    def __init__(self, word_frames):
        self.word_frames = word_frames


def test_cut_sections():
    from speechless_amd import CtcAlignment, cut_sections
    words = [("a", (10, 20)), ("bb", (24, 40)), ("c", (45, 50)), ("dd", (60, 90)), ("e", (95, 100))]
    # exact fit: 10..50 and 60..100 are 40 frames each; "dd" would make the first 80.  The gap 50..60 is cut at 55
    assert cut_sections(_Aligned(words), 40) == [("a bb c", (10, 55)), ("dd e", (55, 100))]
    # one frame less: nothing fits exactly any more.  The gaps 40..45 and 90..95 (odd width) are cut at 42 and 92
    assert cut_sections(_Aligned(words), 39) == [("a bb", (10, 42)), ("c", (42, 55)), ("dd", (55, 92)), ("e", (92, 100))]
    # a single word longer than max_frames is a section by itself
    assert cut_sections(_Aligned(words), 5) == [("a", (10, 22)), ("bb", (22, 42)), ("c", (42, 55)), ("dd", (55, 92)),
                                                ("e", (92, 100))]
    assert cut_sections(_Aligned(words), 1000) == [("a bb c dd e", (10, 100))]
    assert cut_sections(_Aligned([("long", (3, 500))]), 10) == [("long", (3, 500))]
    # from a real alignment object; an infeasible one has no sections
    a = CtcAlignment.from_path("ab  c", -1.0, [0, 0, 1, 1, 3, 4, 5, 6, 7, 7, 8, 9, 9, 10, -1, -1])
    assert a.word_frames == [("ab", (2, 5)), ("c", (11, 13))]
    assert cut_sections(a, 4) == [("ab", (2, 8)), ("c", (8, 13))]
    assert cut_sections(a, 11) == [("ab c", (2, 13))]
    assert cut_sections(CtcAlignment.from_path("abc", -np.inf, [-1] * 4), 100) == []


def test_long_alignment_symbols_are_exported():
    from speechless_amd import _lib
    assert "sl_ctc_align_long" in _lib.SIGNATURES and "sl_ctc_align_long_workspace_bytes" in _lib.SIGNATURES
    assert _lib.SIGNATURES["sl_ctc_align_long"] == _lib.SIGNATURES["sl_ctc_align"]


def test_long_alignment_host_side_checks(hip_lib):
    """Without a GPU: the workspace size is monotonic and 0 out of range; bad arguments are refused before any launch."""
    size = hip_lib.raw("sl_ctc_align_long_workspace_bytes")
    assert size(1, 1000, 0) == 1000 * 256 and size(2, 1000, 511) == 2 * 1000 * 256
    assert size(1, 1000, 512) == 1000 * 512 and size(1, 30000, 8191) == 30000 * 4096
    for l_max in (0, 1, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 8191):
        assert size(1, 100, l_max) <= size(1, 101, l_max) <= size(1, 101, min(l_max + 1, 8191))
    lens = sorted({0, 1, 8191} | {m + d for m in (511, 1023, 2047, 4095) for d in (0, 1)})
    sizes = [size(3, 777, l) for l in lens]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(0, 10, 10) == 0 and size(1, 0, 10) == 0 and size(1, 10, -1) == 0 and size(1, 10, 8192) == 0
    align = hip_lib.raw("sl_ctc_align_long")
    buf = np.zeros((64,), dtype=np.float32).ctypes.data  # a valid host address: nothing may be launched on it
    ok = (buf, buf, buf, buf, buf, buf)
    assert align(*ok, 1, 10, 29, 8192, buf, 1 << 30, None) == -2 and "l_max = 8192" in hip_lib.last_error()
    assert align(*ok, 1, 10, 65, 100, buf, 1 << 30, None) == -2 and "k = 65" in hip_lib.last_error()
    assert align(*ok, 1, 10, 1, 100, buf, 1 << 30, None) == -2 and "k = 1" in hip_lib.last_error()
    for i, name in enumerate(("logq", "labels", "label_len", "input_len", "path", "score")):
        args = list(ok)
        args[i] = None
        assert align(*args, 1, 10, 29, 100, buf, 1 << 30, None) == -1
        assert name + " is a null pointer" in hip_lib.last_error()
    assert align(*ok, 1, 10, 29, 600, buf, 10 * 512 - 1, None) == -3 and "workspace too small" in hip_lib.last_error()
    assert align(*ok, 1, 10, 29, 600, None, 1 << 30, None) == -3
    assert align(*ok, 0, 10, 29, 600, buf, 1 << 30, None) == -1
