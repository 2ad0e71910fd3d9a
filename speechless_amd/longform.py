"""Windows over a long recording (Engine.forward_long, Wav2Letter.predict_recording / align_recording / asg_align_recording):
pure Python.

The engine zero-pads every layer at the edges of a batch row; the reference's "same" padding (net.py:304-305) does so at the
recording's true edges only.  A window cut out of a recording therefore computes WRONG frames next to its interior edges: an
output frame of a layer is right only if every input frame it reads is right, or lies beyond a true edge of the recording (where
the zero is the reference's own padding).  window_plan() follows that rule through the layers to find the range of output
frames of each window that equal a single pass over the whole recording, and lays the windows so that these ranges tile the
output."""
from collections import namedtuple

DEFAULT_WINDOW = 8000             # input frames per window: the longest batch row the engine is exercised at (8 x 8000)
ALIGN_MAX_LABEL = 8191            # sl_ctc_align_long: letters per label (16 383 lattice states)
ASG_ALIGN_MAX_LABEL = 8191        # sl_asg_align_long: ENCODED graphemes per label (a run of two or three equal letters is two)
CTC_LOSS_MAX_LABEL = 2047         # sl_ctc_loss_grad: letters per label (4095 lattice states; two lattices in doubles per utterance)
SEGMENT_MAX_LABEL = 511           # sl_ctc_segment_scores: letters per SEGMENT (1023 lattice states in one wave's registers)
ASG_SEGMENT_MAX_LABEL = 511       # sl_asg_segment_scores: ENCODED graphemes per SEGMENT (8 states per lane of one wave)
SPOT_MAX_PHRASE = 511             # sl_ctc_spot: letters per phrase (the filler and 1021 lattice states in one wave's registers)
SPOT_MAX_HITS = 64                # sl_ctc_spot: hits per query (one lane per hit slot)
GREEDY_DECODE_MAX_FRAMES = 38144  # sl_greedy_decode: output frames per recording ((t_out + 256) ints in 150 KB of LDS)


class RecordingTooLongError(ValueError):
    """a recording beyond what a kernel of the long-recording path holds"""


# input_start, input_length: the window's input frames; keep_start, keep_end: the output frames of the window (counted from the
# window's first output frame) that are kept; out_start, out_end: where they go in the recording's output
Window = namedtuple("Window", "input_start input_length keep_start keep_end out_start out_end")


def _geometry(layer):
    """(kernel_size, stride, pad_left) of a LayerPlan (its own pad_left) or a layer spec (TF 'SAME': plan.same_padding)"""
    spec = getattr(layer, "spec", layer)
    k, s = int(spec.kernel_size), int(spec.stride)
    pad_left = getattr(layer, "pad_left", None)
    if pad_left is None:
        # 'SAME' pads max(k - s, 0) in all when s divides T and max(k - T % s, 0) otherwise, the smaller half on the left
        lefts = {max(k - r, 0) // 2 for r in range(1, s + 1)}
        if len(lefts) != 1:
            raise ValueError("layer {}: the left padding of kernel size {} at stride {} depends on the frame count; "
                             "no window plan".format(getattr(spec, "name", "?"), k, s))
        pad_left = lefts.pop()
    return k, s, int(pad_left)


def input_to_output_ratio(layers):
    ratio = 1
    for layer in layers:
        ratio *= _geometry(layer)[1]
    return ratio


def valid_output_range(input_frames, layers, at_start, at_end):
    """(first, end, output frames) of a window of `input_frames`: the output frames [first, end) equal those of a pass over
    the whole recording.  at_start / at_end: the window's edge is the recording's own (nothing is lost there)."""
    first, end, n = 0, input_frames, input_frames
    for layer in layers:
        k, s, pad_left = _geometry(layer)
        n_out = -(-n // s)
        # output frame j reads input frames s j - pad_left .. s j - pad_left + k - 1
        first = 0 if at_start else -(-(first + pad_left) // s)
        end = n_out if at_end else min(n_out, (end - k + pad_left) // s + 1)
        n = n_out
    return first, max(end, first), n


def halo(layers):
    """(left, right): the output frames an interior edge of a (long, even-length) window loses on either side"""
    ratio = input_to_output_ratio(layers)
    span = ratio * 4 * (sum(_geometry(l)[0] for l in layers) + 1)
    first, end, n = valid_output_range(span, layers, False, False)
    return first, n - end


def window_plan(total_input_frames, layers, window_input_frames):
    """Windows over a recording of `total_input_frames` whose kept output frames, stitched, are those of one pass over the
    whole recording.  layers: LayerPlans or layer specs (kernel_size, stride) of the stack, first layer first.  Returns a
    list of Window: all of one input length (<= window_input_frames), starts at multiples of the stack's input-to-output
    ratio, the first at input frame 0, the last ending at the recording's last frame; the out ranges tile [0, ceil(T /
    ratio)) in order.  A recording that fits one window is one window."""
    total, limit = int(total_input_frames), int(window_input_frames)
    if total <= 0:
        raise ValueError("a recording needs at least one input frame")
    layers = list(layers)
    ratio = input_to_output_ratio(layers)
    frames_out = valid_output_range(total, layers, True, True)[2]
    if total <= limit:
        return [Window(0, total, 0, frames_out, 0, frames_out)]
    # the last window ends at the recording's end and starts at a multiple of the ratio
    length = limit - (limit - total) % ratio
    first_mid, end_mid, _ = valid_output_range(length, layers, False, False) if length > 0 else (0, 0, 0)
    if length <= 0 or end_mid <= first_mid:
        left, right = halo(layers)
        raise ValueError("window_input_frames = {} is too short: an interior window loses {} + {} output frames ({} input "
                         "frames) to its edges".format(limit, left, right, (left + right) * ratio))
    windows, start, done = [], 0, 0
    while True:
        at_start, at_end = start == 0, start + length == total
        first, end, _ = valid_output_range(length, layers, at_start, at_end)
        offset = start // ratio
        assert offset + first <= done < offset + end
        windows.append(Window(start, length, done - offset, end, done, offset + end))
        done = offset + end
        if at_end:
            break
        # the next window's first valid frame is the first one still missing -- or the last window, if that reaches it
        start = min((done - first_mid) * ratio, total - length)
    assert done == frames_out
    return windows
