"""Raw-wave nets on f16x3 (run with -m gpu on an MI355X): sl_wave_frames_planes against the two launches it replaces and the
numpy restatement, Engine(dtype="f16x3") with a wave_conv front layer against the float64 oracle (ReLU, ELU, quiet audio,
dropout, launch lists, RCCL on one rank), Wav2Letter on that path, random shapes.  Helpers come from the earlier GPU modules."""
import functools

import numpy as np
import pytest

import wave_planes_ref as wref
from oracle import w2l_oracle as o
from test_gpu_parity import _report, rel_l2, weights64
from test_gpu_round4 import _wave_case

pytestmark = pytest.mark.gpu

LENGTHS = (24055, 20007)


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("batch,cin,channels,t_in", [(2, 1, 256, 1), (2, 1, 256, 159), (2, 1, 256, 160), (2, 1, 256, 161),
                                                     (2, 1, 256, 409), (2, 1, 256, 24055), (3, 2, 512, 20007)])
@pytest.mark.parametrize("fmt,scale", [("f16", 1024.0), ("bf16", 1.0)])
def test_wave_frames_planes_against_the_two_launches_and_numpy(fmt, scale, batch, cin, channels, t_in):
    """byte-equal to sl_wave_frames(SL_F32) on the pre-scaled samples + sl_splitf16 / sl_split3 mode 0 and to wave_planes_ref;
    an utterance holds more rows than t_out, and the rows >= t_out keep their sentinel"""
    import torch
    from speechless_amd import _lib
    lib = _lib.lib()
    k, stride, extra, sentinel = 250, 160, 3, 0x5A5A
    t_out, pad_l = wref.same_padding(t_in, k, stride)
    rows = t_out + extra
    rng = np.random.RandomState(t_in + cin)
    x = (rng.randn(batch, t_in, cin) * (2.0 ** -6 if fmt == "f16" else 1.0)).astype(np.float32)
    audio = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    code = _lib.SL_F16 if fmt == "f16" else _lib.SL_BF16

    def planes():
        return torch.full((batch, rows, 3 * channels), sentinel, dtype=torch.int16, device="cuda")
    fused, two = planes(), planes()
    lib.call("sl_wave_frames_planes", audio.data_ptr(), fused.data_ptr(), batch, t_in, cin, k, stride, pad_l, t_out, channels,
             fused.stride(0), scale, code, st)
    scaled = audio * scale
    frames32 = torch.zeros((batch, rows, channels), dtype=torch.float32, device="cuda")
    lib.call("sl_wave_frames", scaled.data_ptr(), frames32.data_ptr(), batch, t_in, cin, k, stride, pad_l, t_out, channels,
             frames32.stride(0), _lib.SL_F32, st)
    lib.call("sl_splitf16" if fmt == "f16" else "sl_split3", frames32.data_ptr(), two.data_ptr(), None, batch, t_out, channels,
             frames32.stride(0), 0, two.stride(0), 0, st)
    torch.cuda.synchronize()
    assert torch.equal(fused, two)
    got = fused.cpu().numpy().view(np.uint16)
    assert (got[:, t_out:] == sentinel).all()
    assert np.array_equal(got[:, :t_out], wref.wave_frames_planes(x, k, stride, pad_l, t_out, channels, scale, fmt))


# ------------------------------------------------------------------------------------------ the engine
@functools.lru_cache(maxsize=None)
def _case(cin=1, activation="relu"):
    return _wave_case(cin=cin, activation=activation)


@functools.lru_cache(maxsize=None)
def _oracle(cin, activation, t_audio, quiet=False):
    """float64 oracle of a case's batch cut to t_audio samples, computed once and shared"""
    case = _case(cin, activation)
    x = _samples(case, t_audio, quiet)
    pred_len = _pred_len(case, t_audio)
    return o.loss_and_gradients(case["ospecs"], weights64(case), x.astype(np.float64), case["labels"], pred_len,
                                case["label_lengths"])


def _samples(case, t_audio, quiet=False):
    x = case["x"][:, :t_audio]
    return (x * np.float32(2.0 ** -10)).astype(np.float32) if quiet else x


def _pred_len(case, t_audio):
    return [min(n, t_audio // 320) for n in case["prediction_lengths"]]


def _engine(case, dtype):
    from speechless_amd.engine import Engine
    eng = Engine(case["specs"], 29, dtype=dtype)
    eng.set_weights(case["weights"])
    return eng


def _step(eng, case, t_audio, quiet=False):
    import torch
    eng.load_input(_samples(case, t_audio, quiet))
    eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(_pred_len(case, t_audio)))
    eng.forward(training=True)
    losses = eng.ctc().cpu().numpy().copy()
    eng.backward()
    torch.cuda.synchronize()
    return losses, eng.get_gradients()


def _errors(grads, ref):
    return [max(rel_l2(dw, rw), rel_l2(db, rb)) for (dw, db), (rw, rb) in zip(grads, ref["grads"])]


@pytest.mark.parametrize("cin", [1, 2])
def test_raw_wave_f16x3_against_the_float64_oracle(cin):
    """Engine(dtype="f16x3") with a wave_conv front layer: the windows as fp16 planes of x_scale * x from ONE launch (no fp32
    window buffer), loss, every gradient and the greedy decode against the float64 oracle at the bounds bf16x3 is held to on
    the same cases (tests/test_gpu_round4.py), two lengths through one buffer set, the input buffer's layout, then
    optimisation steps."""
    import torch
    from speechless_amd.engine import Engine
    case = _case(cin)
    eng = _engine(case, "f16x3")
    assert eng.x_scale == 1024.0 and Engine(case["specs"], 29, dtype="bf16x3").x_scale == 1.0
    with pytest.raises(ValueError):
        eng.x_scale = 1000.0
    for t_audio in LENGTHS:
        losses, grads = _step(eng, case, t_audio)
        ref = _oracle(cin, "relu", t_audio)
        assert len(grads) == 12 and grads[0][0].shape == (250, cin, 250)
        errs = _errors(grads, ref)
        _report("raw_wave_f16x3_gradient_errors_cin{}_t{}".format(cin, t_audio), errs)
        _report("raw_wave_f16x3_loss_error_cin{}_t{}".format(cin, t_audio), float(np.max(np.abs(losses / ref["losses"] - 1))))
        print("f16x3 cin", cin, "t", t_audio, "errs", errs, "loss", losses, ref["losses"])
        np.testing.assert_allclose(losses, ref["losses"], rtol=2e-5)
        assert errs[-1] < 5e-4 and max(errs) < 2e-2, errs
        pred_len = _pred_len(case, t_audio)
        decoded, _ = eng.greedy_decode(pred_len)
        assert decoded == o.greedy_decode_indices(ref["probs"], pred_len)
        buf = eng.cur
        assert buf.frames32 is None and buf.frames.dtype == torch.float16
        p0 = eng.plans[0]
        t1 = -(-t_audio // 160)
        x0 = buf.x0.float()
        assert bool((x0[:, p0.pad_left:p0.pad_left + t1, 255] == 1).all())          # ones channel from wave_conv's bias
        assert not x0[:, :p0.pad_left].any() and not x0[:, p0.pad_left + t1:].any()  # layout invariant of the input buffer
        gx0 = buf.gx0.float()
        assert not gx0[:, p0.pad_left + t1:].any() and not gx0[:, :p0.pad_left].any()
    with pytest.raises(ValueError):
        eng.x_scale = 512.0                                                          # fixed once a batch is loaded
    first = float(np.mean(losses))
    for _ in range(8):
        eng.train_step_resident()
    torch.cuda.synchronize()
    assert float(eng.cur.loss.mean().item()) < first
    fw = eng.layer_param_views(eng.params, eng.front_plan)[0]
    assert not fw[:, 250 * cin:, :].any() and not fw[:, :, 250:].any()


def test_raw_wave_f16x3_elu_against_the_float64_oracle():
    """an ELU wave_conv on fp16 planes (fp32 staging + sl_splitf16, mode elu / elu mask): no decisions to flip, every one of
    the twelve gradients tight -- the bounds of tests/test_gpu_round5.py on bf16x3 -- on a long batch and a shorter one"""
    case = _case(1, "elu")
    eng = _engine(case, "f16x3")
    for t_audio in LENGTHS:
        losses, grads = _step(eng, case, t_audio)
        ref = _oracle(1, "elu", t_audio)
        errs = _errors(grads, ref)
        _report("raw_wave_f16x3_elu_gradient_errors_t{}".format(t_audio), errs)
        print("f16x3 elu t", t_audio, "errs", errs)
        np.testing.assert_allclose(losses, ref["losses"], rtol=2e-5)
        assert max(errs) < 2e-4, errs


@pytest.mark.parametrize("activation", ["relu", "elu"])
def test_quiet_audio_is_what_the_input_scale_is_for(activation):
    """the samples x 2^-10 (exact): fp16 planes of the unscaled windows would carry an absolute 2^-25 only; with x_scale they
    carry 22 bits.  f32, bf16x3 and f16x3 against the float64 oracle in one run; f16x3 at the bounds of the loud case -- where
    the exact-fp32 path itself is beyond one of them on this input (ReLU decisions near zero), at twice the fp32 path's error
    of this run."""
    case = _case(1, activation)
    engines = {dtype: _engine(case, dtype) for dtype in ("f32", "bf16x3", "f16x3")}
    for t_audio in LENGTHS:
        ref = _oracle(1, activation, t_audio, True)
        loss_err, errs = {}, {}
        for dtype, eng in engines.items():
            losses, grads = _step(eng, case, t_audio, quiet=True)
            loss_err[dtype] = float(np.max(np.abs(losses - ref["losses"]) / np.abs(ref["losses"])))
            errs[dtype] = _errors(grads, ref)
            _report("raw_wave_quiet_{}_{}_gradient_errors_t{}".format(activation, dtype, t_audio), errs[dtype])
            _report("raw_wave_quiet_{}_{}_loss_error_t{}".format(activation, dtype, t_audio), loss_err[dtype])
            print("quiet", activation, dtype, "t", t_audio, "loss err", loss_err[dtype], "errs", errs[dtype])

        def bound(base, f32_err):
            return base if f32_err <= base else 2.0 * f32_err
        got, f32 = errs["f16x3"], errs["f32"]
        assert loss_err["f16x3"] <= bound(2e-5, loss_err["f32"]), loss_err
        if activation == "elu":
            assert max(got) <= bound(2e-4, max(f32)), (got, f32)
        else:
            assert got[-1] <= bound(5e-4, f32[-1]) and max(got) <= bound(2e-2, max(f32)), (got, f32)


@pytest.mark.parametrize("activation", ["relu", "elu"])
def test_raw_wave_f16x3_dropout_draws_the_masks_of_the_f32_path(activation):
    """Dropout on the f16x3 raw-wave path: the samples dropped in fp32 before the gather (seed offset 63), every plane tensor by
    sl_splitf16_dropout with the (seed, element) keep decisions of the single-plane kernels -- the exact-fp32 path with the same
    seed sees the same masks and the two agree as they do without dropout (the bounds of tests/test_gpu_round5.py); a second
    step draws new masks, evaluation ignores the rate."""
    case = _case(1, activation)
    out = {}
    for dtype in ("f32", "f16x3"):
        eng = _engine(case, dtype)
        eng.dropout_rate, eng.dropout_seed = 0.2, 11
        out[dtype] = _step(eng, case, 24055)
        second = _step(eng, case, 24055)
        assert not np.array_equal(second[0], out[dtype][0])
        probs = eng.forward(case["x"][:, :20007]).cpu().numpy().copy()
        eng.dropout_rate = None
        assert np.array_equal(eng.forward(case["x"][:, :20007]).cpu().numpy(), probs)
    (l32, g32), (lx3, gx3) = out["f32"], out["f16x3"]
    errs = [max(rel_l2(a, c), rel_l2(ab, cb)) for (a, ab), (c, cb) in zip(gx3, g32)]
    _report("raw_wave_f16x3_dropout_{}_vs_f32".format(activation), errs)
    print("dropout", activation, "errs", errs)
    np.testing.assert_allclose(lx3, l32, rtol=2e-5)
    assert np.isfinite(errs).all() and errs[-1] < 5e-4 and max(errs) < (2e-4 if activation == "elu" else 3e-2), errs


def test_raw_wave_f16x3_launch_lists_and_rccl_single_rank():
    """Recorded launch lists over batches of two lengths in one buffer set, and the bucketed exchange through RCCL on one rank
    (the front layer's bucket announced last): both bit-identical to the plain eager step on the f16x3 raw-wave path."""
    import os
    import torch
    import torch.distributed as dist
    from speechless_amd.parallel import GradBucketReducer
    case = _case()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29539")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        finals = []
        for lists, use_reducer in ((True, False), (False, False), (True, True)):
            eng = _engine(case, "f16x3")
            eng.use_launch_lists = lists
            announced = []
            reducer = None
            if use_reducer:
                reducer = GradBucketReducer(eng.grads, eng.bucket_ranges(), force=True)
                inner = reducer.reduce_bucket
                reducer.reduce_bucket = lambda b, inner=inner: (announced.append(b), inner(b))[1]
            losses = []
            for step in range(4):
                t_audio = LENGTHS[step % 2]
                loss = eng.train_step(case["x"][:, :t_audio], case["labels"], np.array(case["label_lengths"]),
                                      np.array(_pred_len(case, t_audio)), reducer)
                losses.append(loss.cpu().numpy().copy())
            torch.cuda.synchronize()
            if use_reducer:
                nb = len(eng.bucket_plan())
                assert eng.bucket_plan()[-1][0] == [eng.front_plan.index] and announced == list(range(nb)) * 4, announced
            finals.append((np.stack(losses), eng.params.clone()))
    finally:
        if created:
            dist.destroy_process_group()
    for other in finals[1:]:
        assert np.array_equal(finals[0][0], other[0]) and torch.equal(finals[0][1], other[1])
    assert np.isfinite(finals[0][0]).all() and finals[0][0][2].mean() < finals[0][0][0].mean()


# ------------------------------------------------------------------------------------------ Wav2Letter
def test_wav2letter_api_with_raw_wave_input_on_f16x3(tmp_path):
    """opt-in only: compute_dtype="f16x3" trains (the loss goes down, an HDF5 checkpoint round-trips into the fp32 path),
    eval_dtype="f16x3" evaluates the same weights to the fp32 net's transcripts and losses; without either argument a raw-wave
    net still evaluates on bf16x3; a sample beyond the fp16 planes' range is refused by name; a weight beyond it sends
    evaluation to bf16x3."""
    from speechless_amd import Wav2Letter, english_frequent_characters
    from speechless_amd.net import Adam, LabeledSpectrogram
    rng = np.random.RandomState(4)
    words = ["she", "was", "abc", "a", "zoo"]
    batch = [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(words, size=rng.randint(1, 3))),
                                spectrogram=0.1 * rng.randn(int(rng.randint(9000, 12000)), 1)) for i in range(4)]
    sizes = dict(out_filter_count=256)

    def make(**kw):
        return Wav2Letter(1, english_frequent_characters, use_raw_wave_input=True, optimizer=Adam(1e-3), layer_sizes=sizes, **kw)
    net = make(seed=5, compute_dtype="f16x3")
    assert net.engine.dtype == "f16x3" and net.eval_engine is net.engine and net.engine.x_scale == 1024.0
    before = net.test_and_predict_batch(batch).average_loss
    for _ in range(10):
        net.train_on_batch(batch)
    after = net.test_and_predict_batch(batch)
    assert after.average_loss < before and isinstance(net.predict(batch[0]), str)
    net.predictive_net.save_weights(tmp_path / "w.h5")
    exact = make(seed=9, compute_dtype="f32")
    exact.predictive_net.load_weights(str(tmp_path / "w.h5"))
    same = exact.test_and_predict_batch(batch)
    assert [r.predicted for r in same.results] == [r.predicted for r in after.results]
    np.testing.assert_allclose([r.loss for r in after.results], [r.loss for r in same.results], rtol=1e-5)
    # evaluation alone on f16x3 (training stays on the bf16 engine)
    ev = make(seed=7, eval_dtype="f16x3")
    ev.predictive_net.load_weights(str(tmp_path / "w.h5"))
    assert ev.engine.dtype == "bf16" and ev.eval_engine.dtype == "f16x3" and ev.eval_engine.forward_only
    got = ev.test_and_predict_batch(batch)
    assert [r.predicted for r in got.results] == [r.predicted for r in same.results]
    np.testing.assert_allclose([r.loss for r in got.results], [r.loss for r in same.results], rtol=1e-5)
    # the default does not move
    assert make(seed=1).eval_dtype == "bf16x3"
    # a sample beyond the planes' range
    loud = [LabeledSpectrogram(id="loud", label="a", spectrogram=np.full((9000, 1), 100.0))] + batch[1:]
    with pytest.raises(ValueError, match="x_scale"):
        ev.test_and_predict_batch(loud)
    with pytest.raises(ValueError, match="x_scale"):
        net.train_on_batch(loud)
    # a weight beyond it: evaluation falls back to bf16 planes, as for spectrogram input
    w = ev.predictive_net.get_weights()
    w[-1][0][0, 3, 5] = 1500.0
    ev.predictive_net.set_weights(w)
    far = ev.test_and_predict_batch(batch)
    assert ev.eval_dtype == "bf16x3" and ev.eval_engine.dtype == "bf16x3" and np.isfinite([r.loss for r in far.results]).all()


def test_random_shapes_through_the_raw_wave_topology_on_f16x3():
    """tools/fuzz_shapes.py --wave --x3 --wave-f16x3, ten cases: the whole optimisation step of the 12-layer raw-wave net on the
    bf16, fp32, bf16x3 and f16x3 paths -- finite, deterministic, the plane paths' loss within 2e-6 of fp32"""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    res = subprocess.run([sys.executable, str(root / "tools" / "fuzz_shapes.py"), "--wave", "--x3", "--wave-f16x3", "--cases", "10",
                          "--seed", "31", "--max-frames", "400", "--max-batch", "4"], capture_output=True, text=True,
                         cwd=str(root), timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    assert "all 10 cases passed" in res.stdout
