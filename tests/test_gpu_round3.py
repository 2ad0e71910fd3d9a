"""GPU tests added in round 3 (run with -m gpu on an MI355X).  Helpers come from test_gpu_parity.py."""
import numpy as np
import pytest

from oracle import w2l_oracle as o
from speechless_amd.launch_list import entry_points
from test_gpu_parity import _report, make_case, make_engine, rel_l2, run_loss_and_grads

pytestmark = pytest.mark.gpu


def _labels(rng, batch, lengths, k=29):
    return o.pack_label_batch([list(rng.randint(0, k - 1, size=n)) for n in lengths])


# ------------------------------------------------------------------------------------------ ADVICE r2 regressions
def test_ctc_workspace_survives_long_then_short_labels():
    """One buffer set: a batch whose longest label exceeds the wave lattice's 255 graphemes (log-domain lattice, smaller
    workspace layout) followed by an ordinary batch (wave lattice).  The workspace must never shrink, and the library's
    own size function is monotonic in l_max."""
    import torch
    from speechless_amd._lib import lib
    need = [lib().raw("sl_ctc_workspace_bytes")(32, 1280, l) for l in (1, 100, 240, 255, 256, 270, 400, 511)]
    assert all(a <= b for a, b in zip(need, need[1:])), need
    case = make_case(b=2, t=1400, seed=3)
    eng = make_engine(case, "f32")
    results = {}
    for name, lengths in (("long", [300, 40]), ("short", [100, 30]), ("long_again", [300, 40])):
        labels = _labels(np.random.RandomState(5 if name != "short" else 6), 2, lengths)
        eng.load_input(case["x"])
        eng.set_labels(labels, lengths, [700, 690])
        eng.forward()
        losses = eng.ctc().cpu().numpy().copy()
        eng.backward()
        torch.cuda.synchronize()
        probs = eng.cur.probs.cpu().numpy().astype(np.float64)
        want, _ = o.ctc_batch_cost(probs, labels, [700, 690], lengths)
        np.testing.assert_allclose(losses, want, rtol=2e-5)
        results[name] = losses
    assert np.array_equal(results["long"], results["long_again"])


def test_length_first_seen_by_predict_then_trained_on():
    """A length first seen forward-only (no backward workspaces sized for it), then another one trained on, then the
    first one trained on in the same buffer set: its dgrad split-K workspace is sized when training reaches it
     and the gradients equal those of a fresh engine bit for bit."""
    import torch
    case_a = make_case(b=4, t=900, seed=11)   # t_out 450
    case_b = make_case(b=4, t=1000, seed=12)  # t_out 500, same 512-row buffer set
    eng = make_engine(case_a, "bf16")
    eng.forward(case_a["x"])                                   # predict at A: forward workspaces only
    for case in (case_b, case_a):
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
        eng.forward(training=True)
        eng.ctc()
        eng.backward()
    torch.cuda.synchronize()
    got = eng.get_gradients()
    fresh = make_engine(case_a, "bf16")
    fresh.load_input(case_a["x"])
    fresh.set_labels(case_a["labels"], case_a["label_lengths"], case_a["prediction_lengths"])
    fresh.forward(training=True)
    fresh.ctc()
    fresh.backward()
    torch.cuda.synchronize()
    for (a, ab), (b, bb) in zip(got, fresh.get_gradients()):
        assert np.array_equal(a, b) and np.array_equal(ab, bb)


def test_evicted_buffer_sets_are_released():
    """max_cached_shapes bounds HBM: a buffer set that was evicted is actually freed (its chain tables used to pin it;
    ADVICE r2, medium)."""
    import gc
    import weakref
    import torch
    case = make_case(b=2, t=300, seed=1)
    eng = make_engine(case, "bf16")
    eng.max_cached_shapes = 1
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
    eng.train_step_resident()
    first = weakref.ref(eng.cur)
    x2 = np.random.RandomState(2).randn(2, 900, 128).astype(np.float32)
    eng.load_input(x2)  # another (batch, padded frames) geometry: the first set is evicted
    eng.set_labels(case["labels"], case["label_lengths"], [400, 390])
    eng.train_step_resident()
    torch.cuda.synchronize()
    gc.collect()
    assert first() is None, "the evicted buffer set is still referenced"


def test_bf16x3_weight_pack_in_one_launch_equals_the_five_launch_sequence(hip_lib):
    """sl_split3_pack_weights (master -> both [w_hi | w_hi | w_lo] operand copies in one pass) against sl_split3_weights +
    2 x sl_pack_weights + 2 x sl_split3_assemble, the sequence it replaces in the bf16x3 optimisation step: bit for bit,
    with and without the dgrad copy, for a first-layer and a 2048-channel shape."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(3)
    st = torch.cuda.current_stream().cuda_stream
    for k, cin, cout, with_dgrad in ((7, 256, 256, True), (48, 128, 256, False), (1, 2048, 64, True), (32, 256, 2048, True)):
        w = torch.from_numpy((rng.randn(k, cin, cout) * 10 ** rng.uniform(-6, 1, size=(1, 1, cout))).astype(np.float32)).cuda()
        hi32, lo32 = torch.empty_like(w), torch.empty_like(w)
        b16 = dict(dtype=torch.bfloat16, device="cuda")
        fh, fl, dh, dl = (torch.empty((w.numel(),), **b16) for _ in range(4))
        f_old, d_old = torch.zeros((3 * w.numel(),), **b16), torch.zeros((3 * w.numel(),), **b16)
        f_new, d_new = torch.zeros_like(f_old), torch.zeros_like(d_old)
        hip_lib.call("sl_split3_weights", w.data_ptr(), hi32.data_ptr(), lo32.data_ptr(), w.numel(), st)
        for src, (f, d) in ((hi32, (fh, dh)), (lo32, (fl, dl))):
            hip_lib.call("sl_pack_weights", src.data_ptr(), f.data_ptr(), d.data_ptr() if with_dgrad else None, k, cin, cout,
                         _lib.SL_BF16, st)
        hip_lib.call("sl_split3_assemble", fh.data_ptr(), fl.data_ptr(), f_old.data_ptr(), cout * k, cin, st)
        if with_dgrad:
            hip_lib.call("sl_split3_assemble", dh.data_ptr(), dl.data_ptr(), d_old.data_ptr(), cin * k, cout, st)
        hip_lib.call("sl_split3_pack_weights", w.data_ptr(), f_new.data_ptr(), d_new.data_ptr() if with_dgrad else None, k,
                     cin, cout, st)
        torch.cuda.synchronize()
        assert torch.equal(f_new.view(torch.int16), f_old.view(torch.int16)), (k, cin, cout)
        assert torch.equal(d_new.view(torch.int16), d_old.view(torch.int16)), (k, cin, cout)


def test_bf16x3_fused_adam_equals_the_elementwise_update_and_a_repack():
    """sl_split3_adam_pack_layers (Adam on the masters and the [w_hi | w_hi | w_lo] operand rows in one pass) against
    sl_adam_step + sl_split3_pack_weights per layer: masters, moments and both operand copies bit for bit, over three steps."""
    import torch
    case = make_case(b=2, t=96, seed=44)
    engines = []
    for fused in (True, False):
        eng = make_engine(case, "bf16x3", lr=1e-3)
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        for _ in range(3):
            eng.forward(training=True)
            eng.ctc(grad_scale=0.5)
            eng.backward()
            eng.adam_step(fused=fused)
            if not fused:
                eng.repack_weights()
        torch.cuda.synchronize()
        engines.append(eng)
    a, b = engines
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    for i in range(len(a.plans)):
        assert torch.equal(a.w_fwd[i].view(torch.int16), b.w_fwd[i].view(torch.int16)), i
        if a.w_dgrad[i] is not None:
            assert torch.equal(a.w_dgrad[i].view(torch.int16), b.w_dgrad[i].view(torch.int16)), i


def test_bf16x3_inner_layer_weight_gradients_in_one_balanced_launch():
    """bf16x3 backward: the 2 x 7 partial weight gradients of inner_conv_1..7 as jobs of one sl_conv1d_wgrad_multi launch
    against the fourteen sl_conv1d_wgrad launches they replace: the same fp32 sums in another split order (1e-6), every
    other tensor bit-identical."""
    import torch
    case = make_case(b=3, t=300, seed=46)
    res = {}
    for multi in (True, False):
        eng = make_engine(case, "bf16x3")
        eng.use_wgrad_multi = multi
        losses, grads = run_loss_and_grads(eng, case)
        res[multi] = (losses, grads)
        torch.cuda.synchronize()
    assert np.array_equal(res[True][0], res[False][0])
    for i, ((wa, ba), (wb, bb)) in enumerate(zip(res[True][1], res[False][1])):
        if 1 <= i <= 7:
            assert rel_l2(wa, wb) < 2e-6 and rel_l2(ba, bb) < 2e-6, (i, rel_l2(wa, wb), rel_l2(ba, bb))
        else:
            assert np.array_equal(wa, wb) and np.array_equal(ba, bb), i


@pytest.mark.parametrize("b,t", [(3, 300), (2, 77), (4, 1000)])
def test_bf16x3_activation_and_plane_split_in_the_kernel_epilogue(b, t):
    """bf16x3: bias + ReLU (forward) resp. the ReLU mask (input gradients) and the split into [hi | lo | hi] planes inside the
    NT kernel's epilogue (sl_conv1d_nt with out_f32 = 2; also behind split K) against the fp32 staging buffer + sl_split3 it
    replaces: the same operations in the same order -- every activation, gradient, loss and weight gradient bit for bit."""
    import torch
    case = make_case(b=b, t=t, seed=47 + t)
    res = {}
    for fused in (True, False):
        eng = make_engine(case, "bf16x3")
        eng.x3_fused_epilogue = fused
        losses, grads = run_loss_and_grads(eng, case)
        res[fused] = (losses, [y.clone() for y in eng.cur.y[:-1]], [g.clone() for g in eng.cur.g], grads)
        torch.cuda.synchronize()
    assert np.array_equal(res[True][0], res[False][0])
    for k in (1, 2):
        for i, (a, c) in enumerate(zip(res[True][k], res[False][k])):
            assert torch.equal(a.view(torch.int16), c.view(torch.int16)), (k, i)
    for (wa, ba), (wb, bb) in zip(res[True][3], res[False][3]):
        assert np.array_equal(wa, wb) and np.array_equal(ba, bb)


# ------------------------------------------------------------------------------------------ fused inner layers: 48-frame tiles
@pytest.mark.parametrize("b,t", [(3, 300), (2, 77), (8, 1200), (1, 96)])
def test_fused_inner_layers_with_48_frame_tiles_are_bit_identical(hip_lib, b, t):
    """sl_conv1d_chain picks 48 instead of 64 output frames per work-group where that fills the chip's rounds of 256
    work-groups better (long utterances in small batches: config 5).  An output row is the same sequence of MFMA
    accumulations whatever tile it sits in, so activations, gradients and losses must be BIT-identical between the two
    tile sizes (and the automatic choice is one of them)."""
    import torch
    case = make_case(b=b, t=t, seed=80 + t)
    res = {}
    try:
        for rows in (64, 48, 0):
            hip_lib.call("sl_conv1d_chain_select", rows)
            eng = make_engine(case, "bf16")
            losses, grads = run_loss_and_grads(eng, case)
            tags = [name for ops in eng.cur.launch_lists.values() for name, _ in entry_points(ops)]
            assert tags.count("sl_conv1d_chain") == 2
            res[rows] = (losses, [y.clone() for y in eng.cur.y[:8]], [g.clone() for g in eng.cur.g[:8]], grads)
            torch.cuda.synchronize()
    finally:
        hip_lib.call("sl_conv1d_chain_select", 0)
    for rows in (48, 0):
        assert np.array_equal(res[rows][0], res[64][0])
        for ya, yb in zip(res[rows][1], res[64][1]):
            assert torch.equal(ya, yb)
        for ga, gb in zip(res[rows][2], res[64][2]):
            assert torch.equal(ga, gb)
        for (wa, ba), (wb, bb) in zip(res[rows][3], res[64][3]):
            assert np.array_equal(wa, wb) and np.array_equal(ba, bb)


# ------------------------------------------------------------------------------------------ output layer: weights in registers
@pytest.mark.parametrize("out_filters,t", [(2000, 1000), (1000, 130), (500, 77), (250, 200)])
def test_output_softmax_with_register_weights_matches_the_lds_kernel(hip_lib, out_filters, t):
    """sl_output_softmax's two kernels -- the weight matrix in LDS behind one ring for the work-group, or a quarter of the
    input channels per wave with its weights in registers and its own ring (cin = 2048 / 1024 / 512 / 256 after padding) --
    and the two-launch path: the same probabilities and log q to the rounding of a different summation order over the
    input channels (four partial sums added in wave order instead of one running sum)."""
    import torch
    case = make_case(b=3, t=t, seed=60 + t, sizes=dict(out_filter_count=out_filters))
    outs = {}
    try:
        for name, fuse, variant in (("two launches", False, 0), ("lds", True, 1), ("registers", True, 2)):
            hip_lib.call("sl_output_softmax_select", variant)
            eng = make_engine(case, "bf16")
            eng.fuse_output_softmax = fuse
            probs = eng.forward(case["x"]).cpu().numpy().copy()
            outs[name] = (probs, eng.cur.logq.cpu().numpy().copy())
            torch.cuda.synchronize()
    finally:
        hip_lib.call("sl_output_softmax_select", 0)
    for name in ("lds", "registers"):
        np.testing.assert_allclose(outs[name][0], outs["two launches"][0], rtol=5e-6, atol=1e-9)
        np.testing.assert_allclose(outs[name][1], outs["two launches"][1], rtol=5e-6, atol=5e-6)
        np.testing.assert_allclose(outs[name][0].sum(-1), 1.0, atol=1e-5)
    _report("output_softmax_register_weights_vs_lds_max_rel_prob_diff_cin_{}".format(out_filters),
            float(np.max(np.abs(outs["registers"][0] - outs["lds"][0]) / outs["lds"][0])))


# ------------------------------------------------------------------------------------------ CTC: the regime of a trained net
def _aligned_logits(rng, labels_list, t, k, strength, noise=1.0):
    """logits of a net that has LEARNT its labels: a random monotone alignment of every label (blank between repeats, the
    frames in between held with blank) gets `strength` on top of N(0, noise) logits -> p ~ 1 on the path, ~e^-strength off"""
    lg = (rng.randn(len(labels_list), t, k) * noise).astype(np.float32)
    for i, lab in enumerate(labels_list):
        seq = []
        for j, c in enumerate(lab):
            if j and c == lab[j - 1]:
                seq.append(k - 1)
            seq.append(int(c))
        cuts = np.sort(rng.choice(np.arange(1, t), size=len(seq) - 1, replace=False))
        bounds = np.concatenate([[0], cuts, [t]]).astype(int)
        for j, sym in enumerate(seq):
            lg[i, bounds[j], sym] += strength
            lg[i, bounds[j] + 1:bounds[j + 1], k - 1] += strength
    return lg


@pytest.mark.parametrize("strength,mismatch", [(12.0, 0.0), (20.0, 0.0), (35.0, 0.0), (20.0, 0.3), (35.0, 1.0)])
def test_ctc_wave_lattice_needs_no_repair_once_the_net_has_learnt_its_labels(hip_lib, strength, mismatch):
    """The regime every successful training run ENDS in: p ~ 1 along one alignment, every other symbol at the eps floor.
    The mass ahead of the alignment's front then pays eps at every frame the front does not and falls thousands of binades
    below it; round 2's lattice (rows rescaled to 2^500, no bound between neighbouring lanes' exponents) overflowed when
    the front crossed into those lanes -- NaN loss, every utterance through the repair pass, 0.9 ms per call instead of 0.1
    from the first epoch that fits anything (found with tools/e2e_train_throughput.py --steps 150: the resident step went
    from 2.1 to 2.9 ms once the loss had fallen).  With the exponent floor between neighbouring lanes (ctc.hip: FLOOR) the
    double lattice handles it alone: variant 2 (no repair pass at all) matches the float64 oracle, and the default gives
    bit-identical results (the repair pass, had it run, would have replaced them with the fp32 log-domain lattice's).
    mismatch > 0: the net is sure of a transcript that disagrees with the label in that fraction of its graphemes."""
    from test_gpu_parity import run_ctc_kernel
    rng = np.random.RandomState(int(strength) + int(100 * mismatch))
    k, t = 29, 500
    lab_len = [200, 150, 97, 20, 180, 1]
    labels_list = [list(rng.randint(0, 28, size=n)) for n in lab_len]
    labels_list[3] = [5] * 20  # repeats only: a blank between every two
    labels = o.pack_label_batch(labels_list)
    input_len = [t] * len(lab_len)
    logits = _aligned_logits(rng, labels_list, t, k, strength)
    if mismatch:  # ... and is WRONG about this fraction of the graphemes: sure of a transcript the label disagrees with
        for lab in labels_list:
            for j in range(len(lab)):
                if rng.rand() < mismatch:
                    lab[j] = int((lab[j] + 1 + rng.randint(0, 27)) % 28)
        labels = o.pack_label_batch(labels_list)
    ref_p = o.softmax(logits.astype(np.float64))
    ref_loss, ref_dp = o.ctc_batch_cost(ref_p, labels, input_len, lab_len)
    ref_dl = o.softmax_backward(ref_p, ref_dp)
    assert np.isfinite(ref_loss).all()
    results = {}
    try:
        for variant in (2, 0, 1, 11):
            hip_lib.call("sl_ctc_select", variant)
            _, loss, dl = run_ctc_kernel(hip_lib, logits, labels, lab_len, input_len)
            results[variant] = (loss.copy(), dl.copy())
    finally:
        hip_lib.call("sl_ctc_select", 0)
    for variant in (2, 0, 11):  # (11: the helped lattice of round 6, without the repair pass)
        loss, dl = results[variant]
        assert np.isfinite(loss).all(), (variant, loss)
        # the loss itself is ~1e-4 here -- the sum of 500 per-frame terms of O(1e-7) each, kept in fp32 as TensorFlow's own
        # op keeps them: absolute 2e-4 (+ relative 1e-5)
        assert np.all(np.abs(loss - ref_loss) < 2e-4 + 1e-5 * np.abs(ref_loss)), (variant, loss - ref_loss)
        assert np.abs(dl - ref_dl).max() < 2e-5, (variant, np.abs(dl - ref_dl).max())
    _report("ctc_learnt_regime_strength_{}_mismatch_{}_loss_abs_err_and_gradient_max_abs_err".format(int(strength), mismatch),
            [float(np.abs(results[0][0] - ref_loss).max()), float(np.abs(results[0][1] - ref_dl).max()),
             float(np.abs(results[1][1] - ref_dl).max())])  # (last: the fp32 log-domain lattice, for comparison)
    assert np.array_equal(results[0][0], results[2][0]) and np.array_equal(results[0][1], results[2][1])


# ------------------------------------------------------------------------------------------ data parallel plan
def test_bucket_plan_covers_every_trainable_parameter_in_completion_order():
    case = make_case(b=2, t=64)
    eng = make_engine(case, "bf16")
    names = [s.name for s in eng.specs]
    plan = eng.bucket_plan()
    # the balanced weight-gradient launch writes striding_conv and the seven inner layers: one bucket, closed by it
    assert [[names[i] for i in layers] for layers, _ in plan] == [
        ["big_conv_2", "output_conv"], ["big_conv_1"],
        ["striding_conv"] + ["inner_conv_{}".format(i) for i in range(1, 8)]]
    eng.use_wgrad_multi = False  # two launches: the run's bucket leaves while striding_conv's gradient is computed
    assert [[names[i] for i in layers] for layers, _ in eng.bucket_plan()] == [
        ["big_conv_2", "output_conv"], ["big_conv_1"], ["inner_conv_{}".format(i) for i in range(1, 8)],
        ["striding_conv"]]
    eng.use_wgrad_multi = True
    covered = sorted(plan, key=lambda e: e[1][0])
    assert covered[0][1][0] == 0 and covered[-1][1][1] == eng.param_numel
    for (_, (_, hi)), (_, (lo, _)) in zip(covered, covered[1:]):
        assert hi == lo
    eng.frozen_layer_count = 9  # transfer learning: only big_conv_2 and output_conv train
    assert [layers for layers, _ in eng.bucket_plan()] == [[9, 10]]
    eng.frozen_layer_count = 3
    assert [layers for layers, _ in eng.bucket_plan()] == [[9, 10], [8], [3, 4, 5, 6, 7]]


def test_sharded_pack_layers_equals_the_fused_adam_operands():
    """sl_pack_layers (operand rewrite alone, one launch for several layers) reproduces the operand copies the fused
    Adam + repack kernel writes for the same masters."""
    import torch
    case = make_case(b=2, t=96, seed=4)
    eng = make_engine(case, "bf16")
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
    eng.train_step_resident()
    torch.cuda.synchronize()
    want_f = [w.clone() for w in eng.w_fwd]
    want_d = [w.clone() if w is not None else None for w in eng.w_dgrad]
    for w in eng.w_fwd:
        w.zero_()
    for w in eng.w_dgrad:
        if w is not None:
            w.zero_()
    eng._pack_layers(range(len(eng.plans)), eng._stream())
    torch.cuda.synchronize()
    for a, b in zip(eng.w_fwd, want_f):
        assert torch.equal(a, b)
    for a, b in zip(eng.w_dgrad, want_d):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------------------------------ fused output-layer backward
def _output_layer_backward_reference(eng):
    """float64 dx / dw of the output layer from the EXACT bf16 operands the kernels read (buffers of the current step)."""
    from speechless_amd.engine import HALO
    buf = eng.cur
    n = len(eng.plans)
    t = buf.t_out
    x = buf.y[n - 2][:, HALO:HALO + t].float().cpu().numpy().astype(np.float64)      # (B, T', 2048)
    g = buf.g[n - 1][:, HALO:HALO + t].float().cpu().numpy().astype(np.float64)      # (B, T', 128)
    w = eng.w_dgrad[n - 1][:, 0, :].float().cpu().numpy().astype(np.float64)          # (2048, 128)
    pre = g @ w.T
    if eng.specs[n - 2].activation == "elu":
        dx = pre * np.where(x > 0, 1.0, x + 1.0)
    else:
        dx = pre * (x > 0)
    dw = np.einsum("btc,btk->ck", x, g)
    return dx, dw


@pytest.mark.parametrize("b,t,activation", [(32, 1000, "relu"), (3, 150, "relu"), (8, 8000, "relu"), (5, 333, "elu")])
def test_fused_output_backward_against_float64_and_the_two_launches(b, t, activation):
    """sl_conv1d_backward_1x1 (weight and input gradient of output_conv in one launch, the layer's input read once) on
    the production geometry (32 x 1000 frames), an odd one, configuration 5's (8 x 8000 frames) and behind an ELU:
    against float64 on the exact bf16 operands, against the dgrad + wgrad launches it replaces, and twice (bitwise)."""
    import torch
    from speechless_amd.engine import HALO, Engine, wav2letter_layer_specs
    case = make_case(b=b, t=t, seed=9)
    specs = wav2letter_layer_specs(128, 29, activation=activation)
    eng = Engine(specs, 29, dtype="bf16")
    eng.set_weights(case["weights"])
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
    eng.use_launch_lists = False
    eng.forward(training=True)
    eng.ctc()
    n = len(eng.plans)
    results = {}
    for mode in ("fused", "fused_again", "two_launches"):
        eng.fuse_output_backward = mode != "two_launches"
        eng.grads.zero_()
        eng.cur.g[n - 2].zero_()
        eng.timeline = []
        eng.backward()
        torch.cuda.synchronize()
        tags = [tag for tag, _, _ in eng.timeline]
        eng.timeline = None
        assert ("bwd:output_conv" in tags) == (mode != "two_launches"), tags
        dw, db = eng.layer_param_views(eng.grads, eng.plans[n - 1])
        results[mode] = (eng.cur.g[n - 2].clone(), dw.clone(), db.clone())
    assert torch.equal(results["fused"][0], results["fused_again"][0])           # deterministic
    assert torch.equal(results["fused"][1], results["fused_again"][1])
    dx_ref, dw_ref = _output_layer_backward_reference(eng)
    t_out = eng.cur.t_out
    for mode in ("fused", "two_launches"):
        gprev, dw, db = results[mode]
        got_dx = gprev[:, HALO:HALO + t_out].float().cpu().numpy()
        # bf16 output rounding: 2^-9 relative per element
        assert np.abs(got_dx - dx_ref).max() <= 2.0 ** -8 * np.abs(dx_ref).max() + 1e-30, mode
        assert rel_l2(got_dx, dx_ref) < 3e-3, mode
        got_dw = dw[0].cpu().numpy()                                                # (2048, 128) fp32
        assert rel_l2(got_dw[:2000, :29], dw_ref[:2000, :29]) < 2e-6, (mode, rel_l2(got_dw[:2000, :29], dw_ref[:2000, :29]))
        assert (got_dw[:, 29:] == 0).all() and (got_dw[2000:] == 0).all()  # (row 2047 was moved to the bias gradient)
        assert rel_l2(db.cpu().numpy()[:29], dw_ref[2047, :29]) < 2e-6, mode     # ones channel: sum of g over the frames
        # layout invariant of the gradient tensor: halo rows, rows beyond the valid time and the ones channel stay zero
        full = gprev.float().cpu().numpy()
        assert (full[:, :HALO] == 0).all() and (full[:, HALO + t_out:] == 0).all()
    # bias gradient of output_conv: from the ones channel in both modes (row cin_pad - 1), same value
    assert torch.allclose(results["fused"][2], results["two_launches"][2], rtol=1e-5, atol=1e-7)
    assert rel_l2(results["fused"][0].float().cpu().numpy(), results["two_launches"][0].float().cpu().numpy()) < 1e-3


# ------------------------------------------------------------------------------------------ production launches at B = 32
def _conv_ref64(x, w, bias, stride):
    """Conv1D(padding="same") in float64 on the GPU (torch matmul per tap: an implementation that shares nothing with the
    HIP kernels).  x (B, T, Cin), w (k, Cin, Cout) -> (B, T', Cout); differentiable."""
    import torch
    k = w.shape[0]
    t_in = x.shape[1]
    t_out, pad_l, pad_r = o.same_padding(t_in, k, stride)
    xp = torch.nn.functional.pad(x, (0, 0, pad_l, pad_r))
    y = None
    for tap in range(k):
        term = xp[:, tap: tap + (t_out - 1) * stride + 1: stride] @ w[tap]
        y = term if y is None else y + term
    return y + bias


def test_production_step_at_batch_32_layer_by_layer_against_float64():
    """The launches the benchmark times -- 32 x 1000 frames, bf16: slab kernel with split-K, the fused inner-layer launches
    in both directions, interleaved weight gradients with their batch splits and the balanced multi-layer launch for the
    inner and striding layers, output layer fused with the softmax and its one-launch backward -- each checked on the EXACT operands it read: every stored activation / gradient tensor is
    bf16, so the float64 result from the stored inputs of a launch is what that launch had to produce, up to fp32
    accumulation order (weight gradients: fp32 out) and one bf16 rounding (activations, input gradients)."""
    import torch
    import bench
    from speechless_amd.engine import HALO, Engine, wav2letter_layer_specs
    from speechless_amd.net import Wav2Letter
    specs = wav2letter_layer_specs(bench.MEL, bench.K_CLASSES)
    eng = Engine(specs, bench.K_CLASSES, dtype="bf16")
    eng.set_weights(Wav2Letter._glorot_uniform(specs, 2))
    x, labels, lab_len, pred_len = bench.synthetic_batch(0, bench.BATCH_PER_GPU)
    eng.load_input(torch.from_numpy(x).cuda())
    eng.set_labels(labels, lab_len, pred_len)
    eng.timeline = []
    eng.forward(training=True)
    eng.ctc()
    eng.backward()
    torch.cuda.synchronize()
    tags = {tag for tag, _, _ in eng.timeline}
    eng.timeline = None
    for tag in ("fwd:inner_conv_1..inner_conv_7", "dgrad:inner_conv_7..inner_conv_1", "wgrad:striding_conv..inner_conv_7",
                "bwd:output_conv", "fwd:output_conv", "wgrad:big_conv_1", "dgrad:big_conv_1"):
        assert tag in tags, (tag, sorted(tags))  # the production launches, not their fallbacks
    buf = eng.cur
    n, t_out = len(eng.plans), buf.t_out
    f64 = torch.float64
    # the input as the first layer read it (bf16, pair-view buffer: frame f at row pad_left + f)
    p0 = eng.plans[0]
    stored_in = buf.x0[:, p0.pad_left:p0.pad_left + x.shape[1], :specs[0].cin].to(f64)
    report = {}
    for i, (p, s) in enumerate(zip(eng.plans, specs)):
        w = eng.w_fwd[i].to(f64).permute(1, 2, 0)[:, :s.cin, :s.cout].contiguous()       # the bf16 operand copy
        bias = eng.layer_param_views(eng.params, p)[1][:s.cout].to(f64)
        xin = (stored_in if i == 0 else buf.y[i - 1][:, HALO:HALO + t_out, :s.cin].to(f64)).detach().requires_grad_(True)
        wl = w.detach().requires_grad_(True)
        pre = _conv_ref64(xin, wl, bias, s.stride)
        # ---- forward
        if i < n - 1:
            got = buf.y[i][:, HALO:HALO + t_out, :s.cout].to(f64)
            want = torch.relu(pre.detach())
            err = float((got - want).norm() / want.norm())
            # measured 1.66e-3 on every layer = the rel-L2 of one bf16 rounding (2^-9 / sqrt(3) ... 2^-9), nothing else
            assert err < 2e-3 and float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()), (s.name, err)
        else:
            want = torch.softmax(pre.detach(), dim=2)
            err = float((buf.probs.to(f64) - want).abs().max())
            assert err < 2e-6, (s.name, err)                                               # probabilities: fp32 out
        report["fwd:" + s.name] = err
        # ---- backward from the stored gradient w.r.t. this layer's pre-activation
        g = buf.g[i][:, HALO:HALO + t_out, :s.cout].to(f64)
        pre.backward(g)
        dw, db = eng.layer_param_views(eng.grads, p)
        e_w = float((dw[:, :s.cin, :s.cout].to(f64) - wl.grad).norm() / wl.grad.norm())
        e_b = float((db[:s.cout].to(f64) - g.sum(dim=(0, 1))).norm() / g.sum(dim=(0, 1)).norm())
        assert e_w < 2e-6 and e_b < 1e-6, (s.name, e_w, e_b)  # measured: 1.6e-7 .. 6.5e-7 (fp32 accumulation order)
        report["wgrad:" + s.name], report["bgrad:" + s.name] = e_w, e_b
        if i > 0:
            want = xin.grad * (xin.detach() > 0)
            got = buf.g[i - 1][:, HALO:HALO + t_out, :s.cin].to(f64)
            e_x = float((got - want).norm() / want.norm())
            assert e_x < 2e-3, (s.name, e_x)
            report["dgrad:" + s.name] = e_x
        del xin, wl, pre, g
    _report("production_launches_batch32_vs_float64", report)


# ------------------------------------------------------------------------------------------ bf16x3: the fast parity path
@pytest.mark.parametrize("t", [64, 77])
def test_bf16x3_loss_and_gradients_against_the_float64_oracle(t):
    """Engine(dtype='bf16x3'): every value as hi + lo bf16 planes, products as three bf16 MFMA terms (csrc/split3.hip), on
    the small cases the fp32 path is held to 1e-4 on: loss 1e-5, gradients measured 2e-6 (output_conv) .. 2.5e-4
    (striding_conv) at 64 frames -- the rounding of the stored activations to 16-17 bits, not the kernels.  With ~100 output
    frames in the whole batch ONE ReLU sign flip is 1 / sqrt(n) = 3e-3 of a layer's signal (77 frames: striding_conv
    2.6e-3), hence 5e-3 here; the bar of 1e-3 is checked where a batch has frames to average over (the full-length test)."""
    from test_gpu_parity import run_loss_and_grads, weights64
    case = make_case(b=3, t=t, seed=5)
    eng = make_engine(case, "bf16x3")
    losses, grads = run_loss_and_grads(eng, case)
    ref = o.loss_and_gradients(case["ospecs"], weights64(case), case["x"].astype(np.float64), case["labels"],
                               case["prediction_lengths"], case["label_lengths"])
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5)
    report = {}
    for spec, (dw, db), (rw, rb) in zip(case["specs"], grads, ref["grads"]):
        report[spec.name] = [rel_l2(dw, rw), rel_l2(db, rb)]
        assert report[spec.name][0] < 5e-3 and report[spec.name][1] < 5e-3, (spec.name, report[spec.name])
    _report("grads_bf16x3_rel_l2_t{}".format(t), report)
    decoded, _ = eng.greedy_decode(case["prediction_lengths"])
    assert decoded == o.greedy_decode_indices(ref["probs"], case["prediction_lengths"])
    # an optimisation step through the plane operands: weights move, padded lanes stay zero, the loss goes down
    import torch
    eng.adam_step()
    eng.forward(training=True)
    eng.ctc()
    eng.backward()
    for _ in range(5):
        eng.train_step_resident()
    torch.cuda.synchronize()
    assert float(eng.cur.loss.mean().item()) < float(np.mean(losses))
    full = eng.layer_param_views(eng.params, eng.plans[1])[0].cpu().numpy()
    assert not full[:, 250:255, :].any() and not full[:, :, 250:].any()


def test_bf16x3_config2_greedy_decode_bit_exact_at_batch_32():
    """BASELINE config 2 (32 x 128-mel x 1000 frames, forward + greedy decode) on the bf16x3 path: every frame's argmax
    and the decoded indices bit-exact against the torch-CPU fp32 path, probabilities within 2e-5 -- what the exact-fp32
    MFMA path delivers at 4.5 k utt/s, here on the bf16 matrix cores."""
    import torch
    from oracle import w2l_torch_cpu as tc
    case = make_case(b=32, t=1000, seed=2)
    pred_len = [500] * 32
    with torch.no_grad():
        ref_probs = tc.forward_probs(case["ospecs"], tc.to_torch_weights(case["weights"], requires_grad=False),
                                     torch.from_numpy(case["x"])).numpy()
    eng = make_engine(case, "bf16x3")
    probs = eng.forward(case["x"]).cpu().numpy()
    decoded, frame_argmax = eng.greedy_decode(pred_len)
    _report("config2_b32_bf16x3_max_abs_prob_error", float(np.abs(probs - ref_probs).max()))
    assert np.abs(probs - ref_probs).max() < 2e-5
    assert np.array_equal(frame_argmax, ref_probs.argmax(axis=2))
    assert decoded == o.greedy_decode_indices(ref_probs, pred_len)


def test_bf16x3_gradients_at_full_length_against_the_cpu_path():
    """4 x 1000 frames, labels up to 200 (the case of test_bf16_gradients_at_full_length_against_the_cpu_path): the bf16x3
    path per tensor against torch-CPU fp32.  The bounds are those of the exact-fp32 path (its floor of 2.5e-4 is the
    reference's own fp32 CTC lattice, the ReLU flips of two fp32 summation orders show in the lowest layers)."""
    import torch
    from oracle import w2l_torch_cpu as tc
    case = make_case(b=4, t=1000, seed=41)
    rng = np.random.RandomState(41)
    lab_len = [200, 137, 20, 75]
    labels = o.pack_label_batch([list(rng.randint(0, case["k"] - 1, size=n)) for n in lab_len])
    pred_len = [500, 500, 480, 500]
    ref = tc.loss_and_gradients(case["ospecs"], case["weights"], case["x"], labels, pred_len, lab_len)
    eng = make_engine(case, "bf16x3")
    eng.load_input(case["x"])
    eng.set_labels(labels, np.array(lab_len), np.array(pred_len))
    eng.forward()
    losses = eng.ctc().cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, ref["losses"], rtol=2e-5)
    errs = {s.name: [rel_l2(dw, rw), rel_l2(db, rb)] for s, (dw, db), (rw, rb) in
            zip(case["specs"], eng.get_gradients(), ref["grads"])}
    _report("full_length_gradient_rel_l2_vs_cpu_bf16x3", errs)
    bounds = {"striding_conv": 1e-2, "inner_conv_1": 2e-3, "inner_conv_2": 1.5e-3}
    for name, (ew, eb) in errs.items():
        assert ew < bounds.get(name, 1e-3) and eb < bounds.get(name, 1e-3), (name, ew, eb)


# ------------------------------------------------------------------------------------------ balanced multi-layer weight gradient
@pytest.mark.parametrize("b,t,f", [(32, 1000, 128), (3, 150, 128), (5, 333, 128), (8, 4000, 257), (1, 70, 128)])
def test_wgrad_multi_against_the_per_layer_launches(b, t, f):
    """sl_conv1d_wgrad_multi (the inner layers' and the striding layer's weight gradients in one launch whose (tile, step)
    space is cut into one equal range per CU) against the grouped + single launches it replaces: same gradients up to fp32
    summation order, bitwise reproducible, every padded lane still zero.  257 bins: the striding layer's pair view of 640
    channels is three 256-wide tiles, the last one starting at 384 and overlapping its neighbour (round 4)."""
    import torch
    case = make_case(b=b, t=t, f=f, seed=13)
    eng = make_engine(case, "bf16")
    eng.use_launch_lists = False
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
    eng.forward(training=True)
    eng.ctc()
    results = {}
    for mode in ("multi", "multi_again", "single"):
        eng.use_wgrad_multi = mode != "single"
        eng.grads.zero_()
        eng.timeline = []
        eng.backward()
        torch.cuda.synchronize()
        tags = [tag for tag, _, _ in eng.timeline]
        eng.timeline = None
        want_tag = "wgrad:striding_conv..inner_conv_7"  # (257 bins too since round 4: overlapping last 256-wide tile)
        assert (want_tag in tags) == (mode != "single") or mode == "single", (mode, tags)
        if mode == "single":
            assert "wgrad:inner_conv_1..inner_conv_7" in tags and "wgrad:striding_conv" in tags  # grouped + single launch
        results[mode] = eng.grads.clone()
    assert torch.equal(results["multi"], results["multi_again"])
    for p in eng.plans[:8]:
        a = eng.layer_param_views(results["multi"], p)
        s = eng.layer_param_views(results["single"], p)
        assert rel_l2(a[0].cpu().numpy(), s[0].cpu().numpy()) < 2e-6, p.spec.name
        assert rel_l2(a[1].cpu().numpy(), s[1].cpu().numpy()) < 2e-6, p.spec.name
        full = a[0].cpu().numpy()
        assert not full[:, :, p.spec.cout:].any() and not full[:, p.spec.cin:p.cin_pad, :].any(), p.spec.name


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_pack_input_for_any_bin_count(hip_lib, dtype):
    """sl_pack_input (a wave per input row, eight 64-bin loads in flight, a tail loop beyond 512 bins) for bin counts that are
    not multiples of anything and for more than 512, odd row counts: every element where it belongs, nothing else touched."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(8)
    st = torch.cuda.current_stream().cuda_stream
    code, tdt = (_lib.SL_BF16, torch.bfloat16) if dtype == "bf16" else (_lib.SL_F32, torch.float32)
    for b, t, f in ((1, 1, 3), (2, 7, 64), (3, 33, 257), (2, 5, 513), (1, 9, 700), (5, 130, 128)):
        row_stride = (f + 63) // 64 * 64
        rows = t + 6
        x = torch.from_numpy(rng.randn(b, t, f).astype(np.float32)).cuda()
        dst = torch.full((b, rows, row_stride), 7.0, dtype=tdt, device="cuda")
        hip_lib.call("sl_pack_input", x.data_ptr(), dst.data_ptr(), b, t, f, 2, row_stride, rows * row_stride, code, st)
        torch.cuda.synchronize()
        want = torch.full((b, rows, row_stride), 7.0, dtype=tdt, device="cuda")
        want[:, 2:2 + t, :f] = x.to(tdt)
        assert torch.equal(dst, want), (b, t, f)


# ------------------------------------------------------------------------------------------ random shapes
def test_random_shapes_through_both_paths():
    """tools/fuzz_shapes.py, twelve cases: random batch sizes, frame counts across the buffer buckets, ragged input lengths,
    labels from empty to long -- finite, deterministic, bf16 within 2e-3 of fp32 (400 cases: worst 2.4e-5)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    res = subprocess.run([sys.executable, str(root / "tools" / "fuzz_shapes.py"), "--cases", "12", "--seed", "3"],
                         capture_output=True, text=True, cwd=str(root), timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    assert "all 12 cases passed" in res.stdout


def test_ctc_random_regimes_against_the_float64_oracle():
    """tools/fuzz_ctc.py, fifteen cases: class counts 5..29, 20..700 frames, ragged input lengths, labels from empty to too
    long, emission regimes mixed per utterance and along the time axis (near-uniform, sharp random, blank collapse, a learnt
    alignment, a learnt alignment of a partly different transcript): loss and gradient against the oracle (300 cases: worst
    3.4e-6 / 2.6e-6), and the repair pass runs in none of them."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    res = subprocess.run([sys.executable, str(root / "tools" / "fuzz_ctc.py"), "--cases", "15", "--seed", "5"],
                         capture_output=True, text=True, cwd=str(root), timeout=900)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    assert "all 15 cases passed" in res.stdout and "the repair pass ran in 0 case(s)" in res.stdout


def test_ctc_mid_random_regimes():
    """tools/fuzz_ctc.py --mid, eight cases: K of 5, 29, 63 or 64, labels of 200 .. 511 letters that fill 50 .. 100 % of their
    frames, two regimes per utterance -- what the wave lattice does not take below 512 letters, on the double log-domain
    lattice: the same bounds and the same pass line.  (Seed 25: its eight cases hold every one of the four class counts and two
    utterances with at most two frames of slack.)"""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    res = subprocess.run([sys.executable, str(root / "tools" / "fuzz_ctc.py"), "--mid", "--cases", "8", "--seed", "25"],
                         capture_output=True, text=True, cwd=str(root), timeout=900)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    assert "all 8 cases passed" in res.stdout and "the repair pass ran in 0 case(s)" in res.stdout
