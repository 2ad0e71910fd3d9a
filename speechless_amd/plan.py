"""Topology and per-layer plans of the Wav2Letter stack (reference net.py:291-341): layer specs, TF 'SAME' padding, padded
channel counts and the layer's place in the flat parameter buffers.  Shared by the engine and its buffer sets.
StackPlan is the planning half of the engine: the layout of a whole stack, which layers share a launch and the gradient
buckets of the data-parallel exchange -- a function of the layer specs and a few knobs that needs no device."""
import os

from ._lib import SL_TIME_TILE as TIME_TILE  # the conv kernels read whole time tiles of up to 256 rows

HALO = 16


def _round_up(x, m):
    return (x + m - 1) // m * m


class LayerSpec:
    def __init__(self, name, kernel_size, stride, cin, cout, activation):
        self.name = name
        self.kernel_size = kernel_size
        self.stride = stride
        self.cin = cin
        self.cout = cout
        self.activation = activation


def wav2letter_layer_specs(input_size_per_time_step, grapheme_set_size, activation="relu",
                           output_activation="softmax", main_filter_count=250, out_filter_count=2000, inner_count=7,
                           striding_kernel=48, inner_kernel=7, big_kernel=32, use_raw_wave_input=False, wave_kernel=250,
                           wave_stride=160):
    """Topology of reference net.py:307-330; use_raw_wave_input: `wave_conv` (250 taps at stride 160 over the samples,
    net.py:310-312) in front of striding_conv, which then reads its filters instead of spectrogram bins.  Sizes are
    parameters only so that tests can build shrunken stacks of the same structure."""
    specs = []
    if use_raw_wave_input:
        specs.append(LayerSpec("wave_conv", wave_kernel, wave_stride, input_size_per_time_step, main_filter_count, activation))
        input_size_per_time_step = main_filter_count
    specs.append(LayerSpec("striding_conv", striding_kernel, 2, input_size_per_time_step, main_filter_count, activation))
    for i in range(1, inner_count + 1):
        specs.append(LayerSpec("inner_conv_{}".format(i), inner_kernel, 1, main_filter_count, main_filter_count,
                               activation))
    specs.append(LayerSpec("big_conv_1", big_kernel, 1, main_filter_count, out_filter_count, activation))
    specs.append(LayerSpec("big_conv_2", 1, 1, out_filter_count, out_filter_count, activation))
    specs.append(LayerSpec("output_conv", 1, 1, out_filter_count, grapheme_set_size, output_activation))
    return specs


def same_padding(t_in, kernel_size, stride):
    """TF 'SAME': T_out = ceil(T/s); pad_total = max((T_out-1)*s + k - T, 0); extra padding goes right."""
    t_out = -(-t_in // stride)
    pad_total = max((t_out - 1) * stride + kernel_size - t_in, 0)
    return t_out, pad_total // 2, pad_total - pad_total // 2


class LayerPlan:
    def __init__(self, index, spec, cin_pad, cout_pad, w_off, b_off):
        self.index = index
        self.spec = spec
        self.cin_pad = cin_pad
        self.cout_pad = cout_pad
        k = spec.kernel_size
        if spec.stride == 2:
            if k % 2:
                raise NotImplementedError("stride-2 layers need an even kernel size (pair view)")
            self.taps_view = k // 2
            self.cin_view = 2 * cin_pad
            # pair view needs pad_left odd/even consistent with row offset; pad_left of SAME stride 2, even k is k/2-1
            self.pad_left = (k - 2) // 2 if k >= 2 else 0
            self.pad_right = None  # depends on T parity, not needed in the pair view
        else:
            self.taps_view = k
            self.cin_view = cin_pad
            self.pad_left = (k - 1) // 2
            self.pad_right = (k - 1) - self.pad_left
        self.w_off = w_off
        self.w_numel = k * cin_pad * cout_pad
        self.b_off = b_off


class StackPlan:
    """The planning half of Engine (its first base class): where each layer lies in the flat parameter, gradient and moment
    buffers, the runs of identical layers, which layers share a grouped or balanced weight-gradient launch, which take
    their bias gradient from the ones channel, and the gradient buckets in the order backward() completes them.  Touches
    no tensor and asks the library nothing, so a launcher or a test can build one without a device.  The knobs are plain
    attributes read at call time: a plan follows the last value set."""

    def __init__(self, specs, grapheme_set_size, dtype="bf16", frozen_layer_count=0):
        self.dtype = dtype
        if dtype not in ("bf16", "f32", "bf16x3", "f16x3"):
            raise ValueError("dtype must be 'bf16', 'f32', 'bf16x3' or 'f16x3'")
        self.planes = 3 if dtype in ("bf16x3", "f16x3") else 1  # (the plane schemes: engine_x3.py)
        # Raw-wave input (reference net.py:310-312: `wave_conv`, 250 taps at stride 160 over the samples, in front of
        # striding_conv): the FRONT layer.  It is a GEMM over gathered sample windows (sl_wave_frames: K = 250 * Cin
        # columns per output frame, 3 GFLOP per 32 x 8 s -- nothing next to the stack) whose output lands directly in the
        # pair-view input buffer of the stack below; the eleven layers behind it, their plans, indices and launches are
        # untouched.  Internally the front plan has index len(plans) (its parameters sit at the END of the flat buffers);
        # the public order of set_weights / get_weights / get_gradients puts it first, as the reference's layer list does.
        self.front_spec = None
        self.front_frozen = False
        if specs and specs[0].stride > 2:
            self.front_spec = specs[0]
            specs = list(specs[1:])
            self.front_frozen = frozen_layer_count >= 1
            frozen_layer_count = max(frozen_layer_count - 1, 0)
            if self.front_spec.activation not in ("relu", "elu"):
                raise NotImplementedError("the raw-wave layer takes a relu / elu activation")
        self.specs = specs
        self.all_specs = ([self.front_spec] if self.front_spec is not None else []) + list(specs)
        self.grapheme_set_size = grapheme_set_size
        self.frozen_layer_count = frozen_layer_count
        for i, s in enumerate(specs):
            if s.stride not in (1, 2) or (s.stride == 2 and i != 0):
                raise NotImplementedError("only the first layer may stride (spectrogram-input stack, net.py:317)")
            hidden_ok = s.activation in ("relu", "elu") if i < len(specs) - 1 else s.activation == "softmax"
            if not hidden_ok:
                raise NotImplementedError(
                    "HIP path supports relu/elu hidden layers and a softmax output layer (got {!r} on {})".format(
                        s.activation, s.name))
        if specs[-1].cout != grapheme_set_size:
            raise ValueError("output layer width must equal the grapheme set size")
        self.plans = []
        off = 0
        # pair view of the striding layer = 2*cin_pad channels; the wgrad tile needs that to be a multiple of 128
        # (a first layer that does not stride reads plain rows: its own padded width must be that multiple -- ADVICE r5)
        cin_pad = _round_up(specs[0].cin, 64 if specs[0].stride == 2 else 128)
        for i, s in enumerate(specs):
            cout_pad = _round_up(s.cout, 128)
            w_off = off
            off += s.kernel_size * cin_pad * cout_pad
            b_off = off
            off += cout_pad
            self.plans.append(LayerPlan(i, s, cin_pad, cout_pad, w_off, b_off))
            cin_pad = cout_pad
        self.front_plan = None
        if self.front_spec is not None:
            fs = self.front_spec
            p0 = self.plans[0]
            if fs.cout != specs[0].cin or p0.cin_pad % 128:
                raise NotImplementedError("the raw-wave layer's filters must be the next layer's inputs, padded to a multiple "
                                          "of 128 (250 -> 256)")
            k_real = fs.kernel_size * fs.cin
            gemm = LayerSpec(fs.name, 1, 1, k_real, fs.cout, fs.activation)  # the layer as the 1 x 1 GEMM it is launched as
            self.front_plan = LayerPlan(len(self.plans), gemm, _round_up(k_real, 128), p0.cin_pad, off, off + _round_up(k_real, 128) * p0.cin_pad)
            off = self.front_plan.b_off + p0.cin_pad
        self.all_plans = self.plans + ([self.front_plan] if self.front_plan is not None else [])
        self.param_numel = off
        # runs of >= 2 consecutive stride-1 layers with identical padded geometry (net.py:321-323: inner_conv_1..7)
        self.runs = []
        i = 1
        while i < len(self.plans):
            j = i
            key = lambda q: (q.spec.kernel_size, q.spec.stride, q.cin_pad, q.cout_pad)  # noqa: E731
            while j + 1 < len(self.plans) and key(self.plans[j + 1]) == key(self.plans[i]) and \
                    self.plans[i].cin_pad == self.plans[i].cout_pad:
                j += 1
            if j > i:
                self.runs.append((i, j))
            i = j + 1
        self.group_wgrad = self.planes == 1  # (the grouped launch reads and writes single-plane bf16 tensors)
        # "ones channel": the last padded output channel of every hidden layer carries the constant 1 (bias 1, zero weights),
        # so the next layer's weight-gradient GEMM -- which multiplies the padding through anyway -- leaves that layer's
        # BIAS gradient in row cin_pad - 1 of dW (sl_bias_grad_from_wgrad, include/speechless_hip.h): ten of the eleven
        # sl_bias_grad passes over g (two launches each, on the side stream, 0.07 ms of the config-3 step by taking
        # bandwidth and power from the GEMMs beside them) become one small launch.  SL_ONES_CHANNEL=0: the old passes.
        self.ones_channel = os.environ.get("SL_ONES_CHANNEL", "1") == "1"
        # the weight gradients of the layers with few 256 x 256 tiles (the run of inner layers, striding_conv) in ONE launch
        # whose (tile, 64-frame step) space is cut into one equal range per CU (sl_conv1d_wgrad_multi) instead of a grouped
        # launch + a 128 x 128-tile launch with utterance-granular batch splits.  SL_WGRAD_MULTI=0: those launches.
        self.use_wgrad_multi = os.environ.get("SL_WGRAD_MULTI", "1") != "0"
        # ... also for a layer whose input channels are not a multiple of the 256-wide tile (257 bins: the 640-wide pair view
        # of striding_conv): its last tile starts at cin - 256 and overlaps the one before (A/B knob)
        self.multi_overlap_tiles = True
        self.nt_cfg = {}  # optional per-launch tile configuration overrides {("fwd"|"dgrad", layer name): cfg word}
        # Data-parallel runs, A/B knob for the first N > 1 run (SL_SPLIT_LAST_BUCKET=1): the one exchange
        # nothing covers is the last bucket {striding_conv, inner_conv_1..7} (19 MB), closed by the last kernel of backward.
        # With the flag the run of identical layers is cut at `split_last_at`: its fused input-gradient launch and the balanced
        # weight-gradient launch become two each (+2 launches per step), and the upper part's gradients (inner_conv_4..7,
        # 7 MB) close as a bucket of their own under the lower part's launches.  Off by default: on one GPU it only costs.
        self.split_last_bucket = os.environ.get("SL_SPLIT_LAST_BUCKET", "0") == "1"
        self.split_last_at = 4

    def _public_plans(self):
        """the plans in the public layer order (the reference's layer list): the front layer first"""
        return ([self.front_plan] if self.front_plan is not None else []) + self.plans

    def _dropout_layers(self):
        """Indices of the layers with a Dropout in front of them (all but the last three, net.py:326-330)."""
        return range(0, max(len(self.plans) - 3, 0))

    def _trainable_layers(self):
        """internal indices of the layers the optimizer updates (the front layer, if any, has index len(plans))"""
        layers = list(range(self.frozen_layer_count, len(self.plans)))
        if self.front_plan is not None and not self.front_frozen:
            layers.append(self.front_plan.index)
        return layers

    def _trainable_ranges(self):
        """[lo, hi) ranges of the flat gradient buffer that hold the trainable layers (frozen layers contribute nothing).
        Whole padded blocks: every padding element of the gradient buffer is zero once backward has run (padded channels
        carry zeros through every GEMM; the ones-channel rows are zeroed by sl_bias_grad_from_wgrad) --
        tests/test_gpu_optimizer_clip.py holds the norm over these ranges to the norm of the logical elements."""
        out = []
        for i in self._trainable_layers():
            p = self.all_plans[i]
            lo, hi = p.w_off, p.b_off + p.cout_pad
            if out and out[-1][1] == lo:
                out[-1] = (out[-1][0], hi)
            else:
                out.append((lo, hi))
        return out

    # ------------------------------------------------------------------ ones channel

    def _has_ones_output(self, plan):
        """hidden layer whose output has channel padding: its last padded channel is the constant 1"""
        hidden = plan is self.front_plan or plan.index < len(self.plans) - 1
        return self.ones_channel and hidden and plan.cout_pad > plan.spec.cout

    def _has_ones_input(self):
        """the packed INPUT carries a ones channel (sl_pack_input_ones) where its bins leave a padding channel free: 257 bins in
        rows of 320 (configuration 5) -- not 128 mel bins, which fill their rows.  Single-plane paths only."""
        if self.front_plan is not None:  # the front layer's last padded filter is the constant 1 (its bias; _has_ones_output)
            return self._has_ones_output(self.front_plan)
        return self.ones_channel and self.planes == 1 and self.plans[0].cin_pad > self.specs[0].cin

    def _ones_input_layers(self, first):
        """trainable layers whose input carries a ones channel: their bias gradient is row cin_pad - 1 of dW"""
        lower = [0] if (first == 0 and self._has_ones_input()) else []
        return lower + [i for i in range(max(first, 1), len(self.plans)) if self._has_ones_output(self.plans[i - 1])]

    # ------------------------------------------------------------------ weight-gradient launches

    def _grouped_wgrad_runs(self, first):
        """layer index -> (lo, hi) of the run whose weight gradients are one grouped launch (bf16 path)"""
        grouped = {}
        if self.group_wgrad and self.dtype == "bf16":
            for (s0, e0) in self.runs:
                lo = max(s0, first)
                if e0 > lo:
                    for q in range(lo, e0 + 1):
                        grouped[q] = (lo, e0)
        return grouped

    def _wgrad_multi_layers(self, first, grouped=None):
        """layers whose weight gradients go into ONE sl_conv1d_wgrad_multi launch (at the lowest of them): the runs of
        identical layers and the striding layer below them.  The same with and without a data-parallel exchange (the step
        is then bit-identical either way); bucket_plan() closes the striding layer's bucket together with the run's."""
        if self.planes > 1:
            # bf16x3: no launch writes the weight gradients of the striding layer AND of a run (bucket_plan() merges nothing)
            return []
        if grouped is None:
            grouped = self._grouped_wgrad_runs(first)
        if not self.use_wgrad_multi or self.dtype != "bf16" or not grouped:
            return []

        def fits(i):  # (input channels: whole 256-wide tiles, or -- round 4 -- a last tile overlapping its neighbour)
            cin = self.plans[i].cin_view
            return cin >= 256 and cin % (64 if self.multi_overlap_tiles else 256) == 0 and \
                self.plans[i].cout_pad % 256 == 0 and ("wgrad", self.specs[i].name) not in self.nt_cfg
        layers = sorted(grouped)
        if not all(fits(i) for i in layers) or len(layers) > 15:
            return []
        if first == 0 and self.plans[0].spec.stride == 2 and layers[0] == 1 and fits(0):
            layers = [0] + layers
        return layers

    def _split_last_cut(self, first):
        """split_last_bucket: the layer at which the balanced weight-gradient launch (and the fused input-gradient launch of
        the run it covers) is cut in two, or None"""
        if not self.split_last_bucket or self.planes > 1:
            return None
        multi = self._wgrad_multi_layers(first)
        cut = self.split_last_at
        if not multi or multi[0] != 0 or not (multi[0] < cut <= multi[-1]) or cut <= first:
            return None
        return cut

    def _wgrad_multi_groups(self, first, grouped=None):
        """the balanced weight-gradient launches of backward, in the order they are enqueued: one for all of
        _wgrad_multi_layers, or -- split_last_bucket -- the layers from the cut up first, then the rest"""
        multi = self._wgrad_multi_layers(first, grouped)
        if not multi:
            return []
        cut = self._split_last_cut(first)
        if cut is None:
            return [multi]
        return [[i for i in multi if i >= cut], [i for i in multi if i < cut]]

    def _x3_multi_runs(self, first):
        """bf16x3: the runs of identical layers whose 2 partial weight gradients per layer are jobs of ONE
        sl_conv1d_wgrad_multi launch at the lowest layer of the run (16 jobs at most): x operands of whole 256-wide tiles
        against 256-wide output tiles.  Shapes only (the same for every buffer set)."""
        out = []
        if not self.use_wgrad_multi:
            return out
        for (s0, e0) in self.runs:
            lo = max(s0, first)
            layers = list(range(lo, e0 + 1))

            def fits_run(i):
                p = self.plans[i]  # A: the [hi | lo] prefix (2 cin_pad) against g_hi, B: x_hi (cin_pad) against g_lo
                return p.cin_pad % 256 == 0 and p.cout_pad % 256 == 0 and p.spec.stride == 1 and \
                    ("wgrad", self.specs[i].name) not in self.nt_cfg
            if len(layers) >= 2 and 2 * len(layers) <= 16 and all(fits_run(i) for i in layers):
                # (round 5: striding_conv's two partials as jobs of the same launch -- 144 more tiles over the 768-wide pair
                # rows -- were measured SLOWER: 6.328 against 6.215 ms per config-3 step in a same-box A/B,
                # profiles/r05_x3_multi_striding_ab.txt; they stay two 128 x 128-tile launches)
                out.append(layers)
        return out

    # ------------------------------------------------------------------ gradient buckets

    def bucket_plan(self):
        """Gradient buckets of the data-parallel exchange in the order backward() completes them: a list of
        (layer indices, (lo, hi)) with [lo, hi) the bucket's contiguous range of the flat gradient buffer.
        {output_conv, big_conv_2} (17 % of the bytes, complete after the second weight gradient of the step), {big_conv_1}
        (64 %, its exchange runs under big_conv_1's input gradient and the whole inner run), the run of identical inner layers
        (one grouped weight-gradient launch at the very end of backward), then what is left (striding_conv, whose weight
        gradient is the last kernel of backward: the only exchange nothing covers) -- one bucket with the run when
        sl_conv1d_wgrad_multi writes both (_wgrad_multi_layers).  Frozen layers are in no bucket."""
        n = len(self.plans)
        first = self.frozen_layer_count
        groups = []
        if n >= 3:
            groups.append(list(range(max(n - 2, first), n)))
            groups.append(list(range(max(n - 3, first), n - 2)))
        else:
            groups.append(list(range(first, n)))
        rest_hi = max(n - 3, first) if n >= 3 else first
        for (s0, e0) in reversed(self.runs):  # runs inside the remaining layers become buckets of their own
            lo = max(s0, first)
            if e0 < rest_hi and e0 >= lo:
                if e0 + 1 < rest_hi:
                    groups.append(list(range(e0 + 1, rest_hi)))
                groups.append(list(range(lo, e0 + 1)))
                rest_hi = lo
        if rest_hi > first:
            groups.append(list(range(first, rest_hi)))
        # one launch writes the weight gradients of the striding layer and of the run above it: one bucket
        multi = self._wgrad_multi_layers(first)
        if multi and multi[0] == 0:
            # every bucket that holds a layer of the launch becomes part of ONE bucket closed at the launch (its lowest
            # layer) -- whole buckets, so that with several runs a layer between them is neither left out of the merged
            # range nor reduced twice; the merged layers are then contiguous from layer 0 up
            span = set(range(multi[0], multi[-1] + 1))
            merged = sorted(set(l for g in groups if set(g) & span for l in g))
            groups = [g for g in groups if not set(g) & span]
            assert merged == list(range(merged[0], merged[-1] + 1)), merged
            parts = self._wgrad_multi_groups(first)
            if len(parts) == 2 and sorted(parts[0] + parts[1]) == merged:
                groups += parts  # split_last_bucket: the upper part of the run closes first, as a bucket of its own
            else:
                groups.append(merged)
        plan = []
        for layers in groups:
            if layers:
                hi_layer = self.plans[layers[-1]]
                plan.append((layers, (self.plans[layers[0]].w_off, hi_layer.b_off + hi_layer.cout_pad)))
        if self.front_plan is not None and not self.front_frozen and first == 0:
            fp = self.front_plan  # (raw-wave front layer: its gradients are the last launches of backward)
            plan.append(([fp.index], (fp.w_off, fp.b_off + fp.cout_pad)))
        return plan

    def bucket_ranges(self):
        """Flat-gradient ranges of bucket_plan(), in completion order (what GradBucketReducer takes)."""
        return [r for _, r in self.bucket_plan()]
