"""GPU tests of gradient clipping (clipnorm, clipvalue) and learning-rate decay on the device: the squared-norm reduction, the
norm over the padded gradient buffer, the clipped Adam twins against the float64 restatement of Keras 2.0
(test_optimizer_clip.py), decay and resume, the unchanged default launch sequence, two data-parallel ranks, Wav2Letter.

Shapes: test_gpu_parity.make_case on the REAL layer widths (250 -> 256 and 2000 -> 2048 channel padding, the ones channel),
b = 2, t = 64 and b = 3, t = 77."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from test_gpu_parity import make_case, make_engine, run_loss_and_grads
from test_optimizer_clip import keras_adam_step_clipped
from test_parallel import _engine_case, _free_port

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "default_step_launches.json"
_CASES = {}


def case_with_norm(b, t, dtype):
    """(case, unclipped gradient norm n0 of its first step on `dtype`, median |g| of that step) -- computed once"""
    key = (b, t, dtype)
    if key not in _CASES:
        import torch
        case = make_case(b=b, t=t, seed=3)
        eng = make_engine(case, dtype)
        _, grads = run_loss_and_grads(eng, case)
        flat = np.concatenate([np.concatenate([w.ravel(), bb.ravel()]) for w, bb in grads]).astype(np.float64)
        _CASES[key] = (case, float(np.sqrt(np.sum(flat * flat))), float(np.median(np.abs(flat))))
        del eng
        torch.cuda.empty_cache()
    return _CASES[key]


def logical_norm(grads, first=0):
    return float(np.sqrt(sum(float(np.sum(w.astype(np.float64) ** 2) + np.sum(bb.astype(np.float64) ** 2))
                             for w, bb in grads[first:])))


def train(eng, case):
    return eng.train_step(case["x"], case["labels"], case["label_lengths"], case["prediction_lengths"])


# ------------------------------------------------------------------------------------------ 1. the reduction alone
def run_sqnorm(hip_lib, x, ranges):
    import torch
    from speechless_amd import _lib
    table = (_lib.NormRange * len(ranges))()
    for entry, (off, count) in zip(table, ranges):
        entry.offset, entry.count = off, count
    need = hip_lib.raw("sl_grad_sqnorm_workspace_bytes")(table, len(ranges))
    assert need >= 8
    ws = torch.empty((need // 8,), dtype=torch.float64, device="cuda:0")
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda:0")
    floats = torch.full((2,), -1.0, dtype=torch.float32, device="cuda:0")
    hip_lib.call("sl_grad_sqnorm", x.data_ptr(), table, len(ranges), 0.0, out.data_ptr(), floats.data_ptr(),
                 floats[1:].data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0], floats.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4097, (1 << 20) + 5])
def test_squared_norm_reduction_matches_float64_and_repeats_bit_for_bit(hip_lib, n):
    """double accumulation of at most 2^21 terms stays far inside 1e-12 relative; values span 1e-20 ... 1e3"""
    import torch
    rng = np.random.RandomState(n % 1000)
    x = (rng.randn(n) * 10.0 ** rng.uniform(-20, 3, size=n)).astype(np.float32)
    dev = torch.tensor(x, device="cuda:0")
    want = np.sum(x.astype(np.float64) ** 2)
    got, floats = run_sqnorm(hip_lib, dev, [(0, n)])
    print("n", n, "got", got, "want", want, "rel", abs(got - want) / want)
    assert abs(got - want) <= 1e-12 * want
    again, _ = run_sqnorm(hip_lib, dev, [(0, n)])
    assert got.tobytes() == again.tobytes()
    assert floats[0] == np.float32(np.sqrt(got)) and floats[1] == 1.0  # clipnorm 0: the factor is exactly 1


def test_squared_norm_over_two_unaligned_ranges(hip_lib):
    import torch
    n = (1 << 20) + 5
    rng = np.random.RandomState(5)
    x = (rng.randn(n) * 10.0 ** rng.uniform(-20, 3, size=n)).astype(np.float32)
    dev = torch.tensor(x, device="cuda:0")
    ranges = [(3, 16384 + 7), (40001, n - 40001 - 2)]  # offsets 3 and 1 mod 4; the first crosses a chunk edge; a gap between
    want = sum(np.sum(x[o:o + c].astype(np.float64) ** 2) for o, c in ranges)
    got, _ = run_sqnorm(hip_lib, dev, ranges)
    print("got", got, "want", want, "rel", abs(got - want) / want)
    assert abs(got - want) <= 1e-12 * want
    again, _ = run_sqnorm(hip_lib, dev, ranges)
    assert got.tobytes() == again.tobytes()
    # a partial range (the slice a rank holds under the sharded optimizer) and an empty one beside it
    part, _ = run_sqnorm(hip_lib, dev, [(40001, 1001), (7, 0)])
    assert abs(part - np.sum(x[40001:41002].astype(np.float64) ** 2)) <= 1e-12 * part


def test_clip_scale_kernel(hip_lib):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    sq = torch.tensor([9.0, 16.0, 144.0], dtype=torch.float64, device="cuda:0")  # n = 13
    for clipnorm, want in ((6.5, np.float32(0.5)), (13.0, np.float32(1.0)), (26.0, np.float32(1.0)), (0.0, np.float32(1.0))):
        out = torch.full((2,), -1.0, dtype=torch.float32, device="cuda:0")
        hip_lib.call("sl_clip_scale", sq.data_ptr(), 3, clipnorm, out[1:].data_ptr(), out.data_ptr(), st)
        got = out.cpu().numpy()
        assert got[0] == 13.0 and got[1] == want, (clipnorm, got)
    sq = torch.tensor([float("nan")], dtype=torch.float64, device="cuda:0")  # no guard: the comparison is false
    out = torch.zeros((2,), dtype=torch.float32, device="cuda:0")
    hip_lib.call("sl_clip_scale", sq.data_ptr(), 1, 1.0, out[1:].data_ptr(), out.data_ptr(), st)
    assert np.isnan(out.cpu().numpy()[0]) and out.cpu().numpy()[1] == 1.0


# ------------------------------------------------------------------------------------------ 2. norm over the padded buffer
@pytest.mark.parametrize("dtype,b,t,frozen,dropout", [
    ("bf16", 2, 64, 0, None), ("bf16", 3, 77, 3, None), ("bf16x3", 3, 77, 0, None), ("bf16x3", 2, 64, 3, None),
    ("f16x3", 2, 64, 0, None), ("f16x3", 3, 77, 3, None), ("bf16", 3, 77, 0, 0.2), ("bf16x3", 2, 64, 0, 0.2)])
def test_norm_over_the_padded_buffer_equals_the_norm_of_the_logical_gradients(dtype, b, t, frozen, dropout):
    """The reduction runs over whole padded layer blocks: every padding element of the gradient buffer must be zero behind
    backward (the ones-channel rows are zeroed by sl_bias_grad_from_wgrad), on all three arithmetics, with frozen layers and
    with dropout -- so the norm equals the float64 norm of the logical arrays of get_gradients() over the trainable layers."""
    import torch
    case = make_case(b=b, t=t, seed=3)
    eng = make_engine(case, dtype, frozen_layer_count=frozen, track_grad_norm=True)
    if dropout:
        eng.dropout_rate, eng.dropout_seed = dropout, 11
    for _ in range(2):  # the second pass replays the recorded lists (no dropout), the reduction among them
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], case["label_lengths"], case["prediction_lengths"])
        eng.forward(training=True)
        eng.ctc()
        eng.backward()
        torch.cuda.synchronize()
        got = float(eng.grad_norm.item())
        assert eng.grad_norm.dim() == 0 and eng.grad_norm.is_cuda
        want = logical_norm(eng.get_gradients(), frozen)
        print(dtype, b, t, frozen, dropout, "norm", got, "logical", want, "rel", abs(got - want) / want)
        assert want > 0 and abs(got - want) <= 1e-6 * want


def test_the_norm_is_not_tracked_unless_asked_for():
    case = make_case(b=2, t=64, seed=3)
    assert make_engine(case, "bf16").grad_norm is None
    assert make_engine(case, "bf16", clipvalue=1.0).grad_norm is None
    assert make_engine(case, "bf16", clipnorm=1.0).grad_norm is not None
    with pytest.raises(ValueError):
        make_engine(case, "bf16", clipnorm=-1.0)


# ------------------------------------------------------------------------------------------ 3. clipped steps
def restated_steps(eng, case, steps, **settings):
    """`steps` train_steps of eng, each restated in float64 from the engine's own (unclipped) gradients of that step"""
    import torch
    params = [a.astype(np.float64) for pair in case["weights"] for a in pair]
    ms = [np.zeros_like(p) for p in params]
    vs = [np.zeros_like(p) for p in params]
    norms = []
    for it in range(steps):
        train(eng, case)
        torch.cuda.synchronize()
        grads = [a for pair in eng.get_gradients() for a in pair]
        params, ms, vs, n = keras_adam_step_clipped(params, grads, ms, vs, it, **settings)
        norms.append((float(eng.grad_norm.item()) if eng.grad_norm is not None else None, n))
    return params, ms, vs, norms


def assert_matches_restatement(eng, case, params, ms, vs, lr=1e-4, steps=3):
    """Moments and masters against the float64 restatement with the tolerances of
    test_gpu_parity.test_adam_matches_keras_formula (p: rtol 1e-6, atol 1e-9; m: rtol 1e-5, atol 1e-7; v: rtol 2e-5, atol 1e-12).

    One element class takes the step-relative bound of test_parallel.test_two_engine_ranks_equal_one_rank_on_the_global_batch
    instead (largest difference <= 2e-2 of the tensor's largest step, fewer than 1e-3 of the elements above 1e-3 of it): masters
    with |p| < 3e-3.  Why: the kernels hold beta_2 in fp32, as Keras does; 1 - 0.999f differs from the float64 1 - 0.999 by 1.3e-5
    relative, so v differs by 1.3e-5 (that is what the rtol of 2e-5 on v is for) and every update after the first by up to
    6.5e-6 of its size: 1.3e-9 after three updates of lr = 1e-4 (2.8e-9 was measured with the rounding of the updates on top).
    test_adam_matches_keras_formula never sees that, its parameters are ~1 and rtol 1e-6 covers 1e-6; here most weights are
    0.001 ... 0.05, and below 3e-3 the rtol term (< 3e-9) no longer covers it while atol stays 1e-9."""
    assert lr <= 1e-4 and steps <= 3  # (the class boundary above was worked out for these settings)
    state = eng.get_optimizer_state()
    got_p = [a for pair in eng.get_weights() for a in pair]
    got_m = [a for pair in state["m"] for a in pair]
    got_v = [a for pair in state["v"] for a in pair]
    start = [a for pair in case["weights"] for a in pair]
    for i in range(len(params)):
        small = np.abs(params[i]) < 3e-3
        np.testing.assert_allclose(got_p[i][~small], params[i][~small], rtol=1e-6, atol=1e-9, err_msg="p {}".format(i))
        step_size = np.abs(params[i] - start[i]).max()
        diff = np.abs(got_p[i] - params[i])[small]
        print("tensor", i, "small-|p| elements", int(small.sum()), "max diff", diff.max() if diff.size else 0.0, "step", step_size)
        assert step_size > 0.5 * lr
        if diff.size:
            assert diff.max() <= 2e-2 * step_size and np.mean(diff > 1e-3 * step_size) < 1e-3, (i, diff.max(), step_size)
        np.testing.assert_allclose(got_m[i], ms[i], rtol=1e-5, atol=1e-7, err_msg="m {}".format(i))
        np.testing.assert_allclose(got_v[i], vs[i], rtol=2e-5, atol=1e-12, err_msg="v {}".format(i))


def assert_engines_bit_equal(a, b):
    import torch
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for wa, wb in zip(a.w_fwd + a.w_dgrad, b.w_fwd + b.w_dgrad):
        assert (wa is None and wb is None) or torch.equal(wa, wb)


@pytest.mark.parametrize("dtype,b,t", [("bf16", 2, 64), ("bf16x3", 3, 77), ("f16x3", 2, 64)])
def test_clipped_steps_match_the_keras_restatement_and_inactive_clipping_changes_nothing(dtype, b, t):
    """Active: clipnorm = n0 / 2 (the norm clip halves every gradient of the first step) and clipvalue = the median |g| after
    that scaling (half of the elements are clamped); three steps against the float64 restatement fed the engine's own
    unclipped gradients.  Inactive: clipnorm = 2 n0 and clipvalue 0 go through the clipped kernels with a factor of exactly 1
    and must leave masters, moments and operand copies bit-identical to an engine built without the arguments."""
    case, n0, median = case_with_norm(b, t, dtype)
    settings = dict(lr=1e-4, clipnorm=0.5 * n0, clipvalue=0.5 * median)
    eng = make_engine(case, dtype, **settings)
    params, ms, vs, norms = restated_steps(eng, case, 3, **settings)
    print(dtype, "n0", n0, "median", median, "norms (device, float64)", norms)
    assert abs(norms[0][1] - n0) <= 1e-6 * n0 and norms[0][0] >= settings["clipnorm"]
    for got, want in norms:
        assert abs(got - want) <= 1e-6 * want
    assert_matches_restatement(eng, case, params, ms, vs)
    # (the gradient buffer was not rewritten: restated_steps read the unclipped gradient, whose norm is `want` above)
    del eng
    # lr = 1e-6 for this pair: at random init three updates of 1e-4 raise the gradient norm fivefold (42.9 -> 225 on the first
    # case), past 2 n0 -- the clip would turn active; updates of 1e-6 leave the norm where it is, and every step is checked
    plain = make_engine(case, dtype, lr=1e-6)
    inactive = make_engine(case, dtype, lr=1e-6, clipnorm=2.0 * n0, clipvalue=0.0)
    for _ in range(3):
        train(plain, case)
        train(inactive, case)
        norm = float(inactive.grad_norm.item())
        print(dtype, "inactive: norm", norm, "clipnorm", 2.0 * n0)
        assert norm < 2.0 * n0
    assert_engines_bit_equal(plain, inactive)
    import torch
    assert not torch.equal(plain.params, make_engine(case, dtype).params)  # (the steps did move the masters)


def test_clipvalue_alone_and_the_unfused_step():
    """clipvalue without clipnorm (no reduction runs, the kernels get a NULL factor); adam_step(fused=False) takes the same path
    through the flat twin and ends with the same masters as the fused one"""
    import torch
    case, n0, median = case_with_norm(2, 64, "bf16")
    settings = dict(lr=1e-4, clipvalue=median)
    eng = make_engine(case, "bf16", **settings)
    params, ms, vs, norms = restated_steps(eng, case, 2, **settings)
    assert norms[0][0] is None
    assert_matches_restatement(eng, case, params, ms, vs, steps=2)
    flat = make_engine(case, "bf16", clipnorm=0.5 * n0, **settings)
    fused = make_engine(case, "bf16", clipnorm=0.5 * n0, **settings)
    for e, how in ((flat, False), (fused, True)):
        run_loss_and_grads(e, case)
        e.adam_step(fused=how)
    torch.cuda.synchronize()
    assert torch.equal(flat.params, fused.params) and torch.equal(flat.adam_v, fused.adam_v)


# ------------------------------------------------------------------------------------------ 4. decay
def test_decay_matches_the_restatement_and_a_resumed_run_continues_bit_identically():
    import torch
    case, _, _ = case_with_norm(2, 64, "bf16")
    settings = dict(lr=1e-4, decay=0.5)
    eng = make_engine(case, "bf16", **settings)
    params, ms, vs, _ = restated_steps(eng, case, 2, **settings)
    saved_weights, saved_state = eng.get_weights(), eng.get_optimizer_state()
    assert saved_state["iterations"] == 2
    params, ms, vs, _ = restated_steps_continue(eng, case, params, ms, vs, 2, **settings)
    assert_matches_restatement(eng, case, params, ms, vs)
    resumed = make_engine(case, "bf16", **settings)
    resumed.set_weights(saved_weights)
    resumed.set_optimizer_state(saved_state)
    train(resumed, case)
    torch.cuda.synchronize()
    assert resumed.adam_iterations == 3
    assert_engines_bit_equal(eng, resumed)
    # the decayed rate is what made the third step: an engine without decay ends elsewhere
    other = make_engine(case, "bf16", lr=1e-4)
    other.set_weights(saved_weights)
    other.set_optimizer_state(saved_state)
    train(other, case)
    assert not torch.equal(other.params, eng.params)


def restated_steps_continue(eng, case, params, ms, vs, it, **settings):
    import torch
    train(eng, case)
    torch.cuda.synchronize()
    grads = [a for pair in eng.get_gradients() for a in pair]
    return keras_adam_step_clipped(params, grads, ms, vs, it, **settings)


# ------------------------------------------------------------------------------------------ 5. twins with NULL / 0
def test_the_four_twins_with_no_clipping_are_their_originals_bit_for_bit(hip_lib):
    import torch
    from speechless_amd import _lib
    k, cin, cout = 3, 64, 128
    n = k * cin * cout + cout
    st = torch.cuda.current_stream().cuda_stream
    how = (2, 1e-3, 0.9, 0.999, 1e-8)

    def fresh(width, dt):
        rng = np.random.RandomState(1)  # param, grad, m, v (>= 0): the same values for the original and its twin
        t = [torch.tensor(rng.randn(n).astype(np.float32), device="cuda:0") for _ in range(3)]
        t.append(torch.tensor(np.abs(rng.randn(n)).astype(np.float32), device="cuda:0"))
        wf = torch.zeros((cout, k, cin * width), dtype=dt, device="cuda:0")
        wd = torch.zeros((cin, k, cout * width), dtype=dt, device="cuda:0")
        table = (_lib.AdamLayer * 1)()
        table[0].offset, table[0].w_fwd, table[0].w_dgrad = 0, wf.data_ptr(), wd.data_ptr()
        table[0].k, table[0].cin_pad, table[0].cout_pad = k, cin, cout
        return t, wf, wd, table

    def ptrs(t):
        return tuple(a.data_ptr() for a in t)

    runs = {
        "sl_adam_step": (1, torch.float32, lambda t, table, tail: ptrs(t) + (n,) + how + tail),
        "sl_adam_pack_layers": (1, torch.bfloat16, lambda t, table, tail: ptrs(t) + (table, 1, _lib.SL_BF16) + how + tail),
        "sl_split3_adam_pack_layers": (3, torch.bfloat16, lambda t, table, tail: ptrs(t) + (table, 1) + how + tail),
        "sl_splitf16_adam_pack_layers": (3, torch.float16, lambda t, table, tail: ptrs(t) + (table, 1) + how + (64.0,) + tail),
    }
    for name, (width, dt, args) in runs.items():
        results = []
        for entry, tail in ((name, ()), (name + "_clipped", (None, 0.0))):
            t, wf, wd, table = fresh(width, dt)
            hip_lib.call(entry, *args(t, table, tail), st)
            torch.cuda.synchronize()
            results.append(t + [wf, wd])
        for a, b in zip(*results):
            assert torch.equal(a, b), name
        assert not torch.equal(results[0][0], torch.tensor(np.random.RandomState(1).randn(n).astype(np.float32),
                                                            device="cuda:0")), name  # (the update did run)


def test_a_twin_clips_what_the_original_does_not(hip_lib):
    """sl_adam_step_clipped with a factor of 0.5 and clipvalue on random data against the restatement"""
    import torch
    n = 4096
    rng = np.random.RandomState(12)
    p, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    tp, tg = torch.tensor(p, device="cuda:0"), torch.tensor(g, device="cuda:0")
    tm, tv = torch.zeros_like(tp), torch.zeros_like(tp)
    scale = torch.tensor([0.5], dtype=torch.float32, device="cuda:0")
    hip_lib.call("sl_adam_step_clipped", tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), n, 1, 1e-4, 0.9, 0.999,
                 1e-8, scale.data_ptr(), 0.25, torch.cuda.current_stream().cuda_stream)
    from oracle import w2l_oracle as o
    gc = np.clip(g.astype(np.float64) * 0.5, -0.25, 0.25)
    rp, rm, rv = o.keras_adam_step(p.astype(np.float64), gc, np.zeros(n), np.zeros(n), 1)
    np.testing.assert_allclose(tp.cpu().numpy(), rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(tm.cpu().numpy(), rm, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(tv.cpu().numpy(), rv, rtol=2e-5, atol=1e-12)
    assert np.array_equal(tg.cpu().numpy(), g)  # the gradient itself is not rewritten


# ------------------------------------------------------------------------------------------ 6. the default launch sequence
def normalized(arg):
    """an argument of a recorded launch with what changes from process to process (addresses) taken out"""
    if arg is None or isinstance(arg, (bool, str)):
        return arg
    if isinstance(arg, int):
        return "address" if abs(arg) >= 1 << 32 else arg
    if isinstance(arg, float):
        return repr(arg)
    return type(arg).__name__  # ctypes tables and references


def default_step_launches(engine_module):
    """names, tags and normalized arguments of everything a default-settings training step launches on a sized-down
    configuration-3 batch (4 x 200 frames, bf16): the recorded forward and backward lists, then what a step launches outside
    them (input packing, CTC, the optimizer)"""
    import torch
    from speechless_amd.launch_list import LAUNCH
    case = make_case(b=4, t=200, seed=3)
    eng = engine_module.Engine(case["specs"], case["k"], dtype="bf16")
    eng.set_weights(case["weights"])
    train(eng, case)
    out = {}
    for key, ops in eng.cur.launch_lists.items():
        out[key[0]] = [[op.name, op.tag, [normalized(a) for a in op.args]] for op in ops if op.kind == LAUNCH]
    seen = []
    launch = eng._launch
    eng._launch = lambda tag, name, *args: (seen.append([name, tag, [normalized(a) for a in args]]), launch(tag, name, *args))
    train(eng, case)
    torch.cuda.synchronize()
    out["eager"] = seen
    return out


def test_default_settings_launch_what_was_launched_before_the_settings_existed():
    """tests/golden/default_step_launches.json was captured with default_step_launches on the commit before Engine took
    clipnorm / clipvalue / decay / track_grad_norm: with the defaults there is no new launch and no changed argument."""
    from speechless_amd import engine
    want = json.loads(GOLDEN.read_text())
    got = json.loads(json.dumps(default_step_launches(engine)))
    assert sorted(got) == sorted(want) == ["bwd", "eager", "fwd"]
    for part in want:
        assert [e[:2] for e in got[part]] == [e[:2] for e in want[part]], part
        assert got[part] == want[part], part
    assert got["eager"][-1][0] == "sl_adam_pack_layers" and len(got["bwd"]) > 5 and len(got["fwd"]) > 3


# ------------------------------------------------------------------------------------------ 7. two ranks
def _clip_worker(rank, world, port, out_dir, shard, dtype, clipnorm):
    import torch
    import torch.distributed as dist
    from speechless_amd.engine import Engine
    from speechless_amd.parallel import GradBucketReducer, shard_range
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # both ranks share cuda:0: gloo moves the bytes
    specs, weights, x, labels, lab_len, pred_len = _engine_case()
    eng = Engine(specs, 29, dtype=dtype, device="cuda:0", lr=1e-3, clipnorm=clipnorm)
    eng.set_weights(weights)
    reducer = GradBucketReducer(eng.grads, eng.bucket_ranges(), shard_optimizer=shard)
    lo, hi = shard_range(x.shape[0], rank, world)
    norms = []
    for _ in range(2):
        eng.train_step(x[lo:hi], labels[lo:hi], lab_len[lo:hi], pred_len[lo:hi], reducer)
        norms.append(eng.grad_norm.item())
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank{}.npz".format(rank)), *[w for w, _ in eng.get_weights()])
    np.save(os.path.join(out_dir, "norm{}.npy".format(rank)), np.array(norms, dtype=np.float32))
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
@pytest.mark.parametrize("shard", [False, True])
def test_two_clipping_ranks_equal_one_rank_on_the_global_batch(tmp_path, shard, dtype):
    """test_parallel.test_two_engine_ranks_equal_one_rank_on_the_global_batch with clipnorm = n0 / 2 of the global batch: the
    ranks agree bit for bit, match the single process within that test's bounds, and report the same norm (exactly among
    themselves -- the same reduced buffer, or the all-reduced sum of their slices' sums; to 1e-5 against the single process).
    (Observed on this borrowed case: after its first update of lr = 1e-3 the second step's gradient norm is 0.0 on every path,
    the single process included, so the clip acts on the first step; the second still moves the weights through the moments.)"""
    import torch
    import torch.multiprocessing as mp
    from speechless_amd.engine import Engine
    world = 2
    specs, weights, x, labels, lab_len, pred_len = _engine_case()
    probe = Engine(specs, 29, dtype=dtype, device="cuda:0", track_grad_norm=True)
    probe.set_weights(weights)
    run_loss_and_grads(probe, dict(x=x, labels=labels, label_lengths=lab_len, prediction_lengths=pred_len))
    n0 = float(probe.grad_norm.item())
    del probe
    mp.spawn(_clip_worker, args=(world, _free_port(), str(tmp_path), shard, dtype, 0.5 * n0), nprocs=world, join=True)
    eng = Engine(specs, 29, dtype=dtype, device="cuda:0", lr=1e-3, clipnorm=0.5 * n0)
    eng.set_weights(weights)
    norms = []
    for _ in range(2):
        eng.train_step(x, labels, lab_len, pred_len)
        norms.append(eng.grad_norm.item())
    torch.cuda.synchronize()
    assert abs(norms[0] - n0) <= 1e-6 * n0
    ref = [w for w, _ in eng.get_weights()]
    ranks = [np.load(str(tmp_path / "rank{}.npz".format(rank))) for rank in range(world)]
    rank_norms = [np.load(str(tmp_path / "norm{}.npy".format(rank))) for rank in range(world)]
    print(dtype, shard, "norms", norms, rank_norms)
    assert np.array_equal(rank_norms[0], rank_norms[1])
    np.testing.assert_allclose(rank_norms[0], norms, rtol=1e-5)
    moved = 0.0
    for i in range(len(ref)):
        assert np.array_equal(ranks[0]["arr_{}".format(i)], ranks[1]["arr_{}".format(i)])
    for rank in range(world):
        for i, r in enumerate(ref):
            g = ranks[rank]["arr_{}".format(i)]
            step_size = np.abs(r - weights[i][0]).max()
            diff = np.abs(g - r)
            assert diff.max() <= 2e-2 * step_size and np.mean(diff > 1e-3 * step_size) < 1e-3, (rank, i, diff.max())
            moved = max(moved, float(step_size))
    assert moved > 1e-4


# ------------------------------------------------------------------------------------------ 8. Wav2Letter
def test_wav2letter_passes_the_optimizer_settings_to_its_engine():
    import torch
    from speechless_amd import Wav2Letter, english_frequent_characters
    from speechless_amd.engine import Engine
    from speechless_amd.net import Adam, LabeledSpectrogram
    rng = np.random.RandomState(3)
    words = ["she", "was", "abc", "a", "zoo"]
    batch = [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(words, size=rng.randint(1, 3))),
                                spectrogram=rng.randn(int(rng.randint(60, 78)), 128)) for i in range(3)]
    probe = Wav2Letter(128, english_frequent_characters, optimizer=Adam(1e-3), compute_dtype="bf16", seed=5,
                       track_gradient_norm=True)
    probe.train_on_batch(batch)
    n0 = probe.last_gradient_norm()
    assert isinstance(n0, float) and n0 > 0
    del probe
    net = Wav2Letter(128, english_frequent_characters, optimizer=Adam(1e-3, clipnorm=0.5 * n0), compute_dtype="bf16", seed=5)
    assert net.engine.clipnorm == 0.5 * n0 and net.engine.clipvalue == 0.0 and net.engine.decay == 0.0
    inputs = net._input_dictionary_for_loss_net(batch)
    names = Wav2Letter.InputNames
    eng = Engine(net.engine.all_specs, net.grapheme_encoding.grapheme_set_size, dtype="bf16", lr=1e-3, clipnorm=0.5 * n0)
    eng.set_weights(net.predictive_net.get_weights())
    net.train_on_batch(batch)
    eng.train_step(inputs[names.input_batch], inputs[names.label_batch], inputs[names.label_lengths],
                   inputs[names.prediction_lengths])
    torch.cuda.synchronize()
    assert torch.equal(net.engine.params, eng.params)
    assert net.last_gradient_norm() == float(eng.grad_norm.item()) == pytest.approx(n0, rel=1e-6)
    unclipped = Wav2Letter(128, english_frequent_characters, optimizer=Adam(1e-3), compute_dtype="bf16", seed=5)
    unclipped.train_on_batch(batch)
    assert unclipped.last_gradient_norm() is None
    assert not torch.equal(unclipped.engine.params, net.engine.params)  # (the clip did change the step)
