"""plan.StackPlan, the planning half of Engine, built without a device: the layout of the flat buffers, the runs of identical
layers, the layers of the balanced weight-gradient launches, the ones-channel layers and the gradient buckets in the order
backward() completes them.  The expected lists are the ones the GPU tests of the bucket plan assert on a live engine
(test_gpu_round3 / 4 / 6)."""
import pytest

from speechless_amd.plan import LayerSpec, StackPlan, wav2letter_layer_specs


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in ("SL_WGRAD_MULTI", "SL_SPLIT_LAST_BUCKET", "SL_ONES_CHANNEL"):
        monkeypatch.delenv(name, raising=False)


def r(lo, hi):
    """layers lo .. hi, both included"""
    return list(range(lo, hi + 1))


def bucket_layers(plan):
    return [layers for layers, _ in plan.bucket_plan()]


def test_default_stack_layout_and_buckets():
    plan = StackPlan(wav2letter_layer_specs(128, 29), 29, "bf16", 0)
    assert plan.runs == [(1, 7)] and plan.param_numel == 26024064
    assert bucket_layers(plan) == [[9, 10], [8], r(0, 7)]
    assert plan._trainable_ranges() == [(0, 26024064)]
    assert plan._ones_input_layers(0) == r(1, 10)


def test_default_stack_buckets_follow_the_knobs_at_call_time():
    plan = StackPlan(wav2letter_layer_specs(128, 29), 29, "bf16", 0)
    plan.use_wgrad_multi = False  # two launches: the run's bucket leaves while striding_conv's gradient is computed
    assert bucket_layers(plan) == [[9, 10], [8], r(1, 7), [0]]
    plan.use_wgrad_multi = True
    assert bucket_layers(plan) == [[9, 10], [8], r(0, 7)]
    plan.frozen_layer_count = 9  # transfer learning: only big_conv_2 and output_conv train
    assert bucket_layers(plan) == [[9, 10]]
    plan.frozen_layer_count = 3
    assert bucket_layers(plan) == [[9, 10], [8], r(3, 7)]
    plan.frozen_layer_count = 0
    plan.split_last_bucket = True  # the run is cut at inner_conv_4: its upper part closes first, as a bucket of its own
    assert bucket_layers(plan) == [[9, 10], [8], r(4, 7), r(0, 3)]
    assert plan._wgrad_multi_groups(0) == [r(4, 7), r(0, 3)]
    assert plan.bucket_ranges() == [rng for _, rng in plan.bucket_plan()]


def two_run_specs():
    """the stack of test_bucket_plan_of_a_stack_with_two_runs_of_identical_layers (test_gpu_round4.py)"""
    specs = [LayerSpec("striding_conv", 48, 2, 128, 250, "relu")]
    specs += [LayerSpec("a{}".format(i), 7, 1, 250, 250, "relu") for i in range(3)]
    specs += [LayerSpec("between", 5, 1, 250, 250, "relu")]
    specs += [LayerSpec("b{}".format(i), 7, 1, 250, 250, "relu") for i in range(3)]
    specs += [LayerSpec("big_conv_1", 8, 1, 250, 512, "relu"), LayerSpec("big_conv_2", 1, 1, 512, 512, "relu"),
              LayerSpec("output_conv", 1, 1, 512, 29, "softmax")]
    return specs


@pytest.mark.parametrize("dtype,want", [
    ("bf16", [[9, 10], [8], r(0, 7)]),  # the balanced launch writes both runs and layer 0: its bucket swallows `between`
    ("f32", [[9, 10], [8], [5, 6, 7], [4], [1, 2, 3], [0]]),
    ("bf16x3", [[9, 10], [8], [5, 6, 7], [4], [1, 2, 3], [0]]),
    ("f16x3", [[9, 10], [8], [5, 6, 7], [4], [1, 2, 3], [0]])])  # (no plan tells the two plane formats apart)
def test_two_runs_of_identical_layers(dtype, want):
    specs = two_run_specs()
    plan = StackPlan(specs, 29, dtype, 0)
    assert plan.runs == [(1, 3), (5, 7)]
    buckets = plan.bucket_plan()
    assert [layers for layers, _ in buckets] == want
    covered = sorted(l for layers, _ in buckets for l in layers)
    assert covered == list(range(len(specs))), buckets                        # every layer in exactly one bucket
    spans = sorted(rng for _, rng in buckets)
    assert spans[0][0] == 0 and spans[-1][1] == plan.param_numel
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans         # disjoint, contiguous cover
    for layers, (lo, hi) in buckets:
        assert layers == list(range(layers[0], layers[-1] + 1))               # contiguous layers
        assert (lo, hi) == (plan.plans[layers[0]].w_off, plan.plans[layers[-1]].b_off + plan.plans[layers[-1]].cout_pad)


def test_raw_wave_front_layer():
    specs = wav2letter_layer_specs(1, 29, use_raw_wave_input=True)
    plan = StackPlan(specs, 29, "bf16", 0)
    assert plan.front_plan.index == 11 and plan.param_numel == 27662720
    assert plan.bucket_plan()[-1] == ([11], (27596928, 27662720))
    assert plan._trainable_layers() == r(0, 11)
    assert [p.index for p in plan._public_plans()] == [11] + r(0, 10)
    frozen = StackPlan(specs, 29, "bf16", 1)  # the public first layer is the front layer
    assert frozen.front_frozen and frozen.frozen_layer_count == 0
    assert all(11 not in layers for layers, _ in frozen.bucket_plan())
    assert frozen._trainable_layers() == r(0, 10)


def test_257_bins_pad_to_a_ones_input_and_an_overlapping_tile():
    plan = StackPlan(wav2letter_layer_specs(257, 29), 29, "bf16", 0)
    assert plan.plans[0].cin_pad == 320
    assert plan._wgrad_multi_layers(0) == r(0, 7)
    assert plan._has_ones_input() is True


def test_refusals_need_no_device():
    specs = wav2letter_layer_specs(128, 29)
    with pytest.raises(ValueError) as e:
        StackPlan(specs, 29, "f16", 0)
    assert str(e.value) == "dtype must be 'bf16', 'f32', 'bf16x3' or 'f16x3'"
    strided = wav2letter_layer_specs(128, 29)
    strided[3].stride = 2
    with pytest.raises(NotImplementedError) as e:
        StackPlan(strided, 29, "bf16", 0)
    assert str(e.value) == "only the first layer may stride (spectrogram-input stack, net.py:317)"
    hidden = wav2letter_layer_specs(128, 29)
    hidden[9].activation = "softmax"
    with pytest.raises(NotImplementedError) as e:
        StackPlan(hidden, 29, "bf16", 0)
    assert str(e.value) == ("HIP path supports relu/elu hidden layers and a softmax output layer "
                            "(got 'softmax' on big_conv_2)")
    with pytest.raises(ValueError) as e:
        StackPlan(specs, 30, "bf16", 0)
    assert str(e.value) == "output layer width must equal the grapheme set size"
