"""sl_ctc_loss_grad for labels of 512 .. 2047 letters (csrc/ctc_long.hip) on the GPU: against the float64 oracle fed the kernel's own
fp32 probabilities, across the instantiation boundary at 511 / 512 letters, through the engine and through Wav2Letter.
(tests/test_gpu_ctc_mid.py: the same kernels at 256 .. 511 letters and at 64 classes, with this module's helpers and bounds.)

Bounds (the project's own, from test_ctc_kernel_edge_cases / test_ctc_kernel_long_labels):
  loss, feasible utterance : |got - ref| <= 1e-5 |ref| + T_b * 1.2e-6   (the absolute term: the kernel reads fp32 logq, each entry
                             within 2^-24 |log q| <= 2^-24 * 18.5 = 1.1e-6 of the float64 value at eps = 1e-8, and the loss moves
                             by at most the sum over the frames of the largest perturbation in the frame;
                             tests/test_ctc_long.py::test_loss_bound_covers_fp32_logq checks that margin on the CPU)
  gradient                 : every entry within 1e-4 * grad_scale; "uniform" regime also relative L2 < 1e-3
  infeasible utterance     : loss +inf from kernel and oracle, gradient within the same absolute bound; rows >= input_len exactly 0
"""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import w2l_oracle as o

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
from fuzz_ctc import regime_logits  # noqa: E402

pytestmark = pytest.mark.gpu

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED, SL_ERR_WORKSPACE_TOO_SMALL = -1, -2, -3
REGIMES = ("uniform", "sharp", "collapse", "learnt", "wrong")
FILL = 7.5  # what the outputs hold before a call: an entry the kernel does not write shows


def adjacent_repeats(label):
    return sum(1 for a, b in zip(label, label[1:]) if a == b)


def min_frames(label):
    """the frames the shortest alignment of a label takes: its letters and a blank between equal neighbours"""
    return len(label) + adjacent_repeats(label)


def run_kernel(hip_lib, logits, labels, label_len, input_len, eps=1e-8, grad_scale=1.0, l_max=None, ws=None):
    """sl_softmax_logq + sl_ctc_loss_grad into fp32 outputs that start from FILL.  Returns (probs, loss, dlogits) as numpy.
    l_max: pad the label batch to that many columns; ws: a uint8 tensor to use as the workspace, whatever it holds, instead of
    a fresh one of exactly sl_ctc_workspace_bytes."""
    import torch
    from speechless_amd import _lib
    b, t, k = logits.shape
    dev = "cuda:0"
    labels = np.asarray(labels, dtype=np.int32)
    if l_max is not None and l_max > labels.shape[1]:
        labels = np.concatenate([labels, -np.ones((b, l_max - labels.shape[1]), dtype=np.int32)], axis=1)
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.zeros((b, t, k), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor(np.asarray(label_len), dtype=torch.int32, device=dev)
    il = torch.tensor(np.asarray(input_len), dtype=torch.int32, device=dev)
    loss = torch.full((b,), FILL, dtype=torch.float32, device=dev)
    dl = torch.full((b, t, k), FILL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    need = hip_lib.raw("sl_ctc_workspace_bytes")(b, t, lab.shape[1])
    assert need > 0
    if ws is None:
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    hip_lib.call("sl_ctc_loss_grad", probs.data_ptr(), logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(),
                 loss.data_ptr(), dl.data_ptr(), b, t, k, lab.shape[1], 0, k, t * k, _lib.SL_F32, eps, grad_scale,
                 ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return probs.cpu().numpy(), loss.cpu().numpy(), dl.cpu().numpy()


def check_against_oracle(probs, loss, dl, labels, label_len, input_len, regimes, eps=1e-8, grad_scale=1.0, infeasible=()):
    """the bounds of the module docstring, utterance by utterance; prints every figure before it asserts"""
    p64 = probs.astype(np.float64)
    ref_loss, ref_dp = o.ctc_batch_cost(p64, labels, input_len, label_len, eps=eps)
    ref_dl = o.softmax_backward(p64, ref_dp) * grad_scale
    for i in range(len(label_len)):
        t_b = int(input_len[i])
        err_g = float(np.abs(dl[i] - ref_dl[i]).max())
        print("utterance %d: %4d letters, %4d frames, %-8s loss %.7g (oracle %.7g, bound %.2e), gradient error %.2e" % (
            i, label_len[i], t_b, regimes[i], loss[i], ref_loss[i], 1e-5 * abs(ref_loss[i]) + t_b * 1.2e-6, err_g))
        if i in infeasible:
            assert np.isposinf(ref_loss[i]) and np.isposinf(loss[i]), (i, loss[i], ref_loss[i])
        else:
            assert np.isfinite(ref_loss[i]), (i, "the case is meant to be feasible")
            assert abs(loss[i] - ref_loss[i]) <= 1e-5 * abs(ref_loss[i]) + t_b * 1.2e-6, (i, loss[i], ref_loss[i])
        assert err_g <= 1e-4 * grad_scale, (i, regimes[i], err_g)
        if regimes[i] == "uniform" and i not in infeasible:
            rel = float(np.linalg.norm(dl[i] - ref_dl[i]) / np.linalg.norm(ref_dl[i]))
            assert rel < 1e-3, (i, rel)
        assert not dl[i, t_b:].any(), (i, "rows at and beyond input_len must be exactly zero")


def build_batch(rng, k, specs):
    """specs: (label length, slack frames, regime) per utterance -> (logits, labels, label_len, input_len).  An utterance gets
    min_frames(label) + slack frames; t_out is the longest."""
    labels_list = [list(rng.randint(0, k - 1, size=n)) for n, _, _ in specs]
    input_len = [max(min_frames(lab) + slack, 1) for lab, (_, slack, _) in zip(labels_list, specs)]
    t_out = max(input_len)
    logits = np.zeros((len(specs), t_out, k), dtype=np.float32)
    for i, (lab, (_, _, regime)) in enumerate(zip(labels_list, specs)):
        logits[i, :input_len[i]] = regime_logits(rng, lab, input_len[i], k, regime)
    labels = o.pack_label_batch([lab if lab else [-1] for lab in labels_list])
    return logits, labels, [len(lab) for lab in labels_list], input_len


def check_bf16_destination(hip_lib, logits, labels, label_len, input_len, first, halo=3, rs=40):
    """The same case into a bf16 tensor with a halo row offset, a row stride wider than K and a padded batch stride: the fp32
    result `first` (run_kernel's) rounded to nearest even, every element outside [halo, halo + t) x [0, K) still FILL bit for
    bit, and the same loss bytes."""
    import torch
    from speechless_amd import _lib
    b, t, k = logits.shape
    assert rs > k
    dev = "cuda:0"
    bs = (t + 2 * halo) * rs + 24
    lg = torch.tensor(logits, device=dev)
    probs = torch.zeros((b, t, k), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    lab = torch.tensor(np.asarray(labels, dtype=np.int32), dtype=torch.int32, device=dev)
    ll = torch.tensor(label_len, dtype=torch.int32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    loss = torch.zeros((b,), dtype=torch.float32, device=dev)
    dst = torch.full((b * bs,), FILL, dtype=torch.bfloat16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, 1e-8, st)
    need = hip_lib.raw("sl_ctc_workspace_bytes")(b, t, lab.shape[1])
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_ctc_loss_grad", probs.data_ptr(), logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(),
                 loss.data_ptr(), dst.data_ptr(), b, t, k, lab.shape[1], halo, rs, bs, _lib.SL_BF16, 1e-8, 1.0, ws.data_ptr(),
                 need, st)
    torch.cuda.synchronize()
    got = dst.cpu()
    want = torch.full((b * bs,), FILL, dtype=torch.bfloat16)
    ref16 = torch.from_numpy(first[2]).to(torch.bfloat16)  # round to nearest even, as the library rounds
    for i in range(b):
        rows = want[i * bs:i * bs + (t + 2 * halo) * rs].view(t + 2 * halo, rs)
        rows[halo:halo + t, :k] = ref16[i]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert loss.cpu().numpy().tobytes() == first[1].tobytes()


# 1 ------------------------------------------------------------------------------------------ boundaries of every instantiation
@pytest.mark.parametrize("index,length", list(enumerate((512, 513, 1023, 1024, 2047))))
def test_boundaries_of_every_instantiation(hip_lib, index, length):
    """Label lengths at both ends of the two instantiations (2 states per thread: 512 .. 1023, 4: 1024 .. 2047), each with zero
    slack (as many frames as the label has letters and adjacent repeats), one frame of slack and L / 4 frames; the five regimes
    in turn over the fifteen utterances."""
    rng = np.random.RandomState(100 + length)
    specs = [(length, slack, REGIMES[(3 * index + j) % 5]) for j, slack in enumerate((0, 1, length // 4))]
    logits, labels, label_len, input_len = build_batch(rng, 29, specs)
    assert labels.shape[1] == length and logits.shape[1] <= 2700
    probs, loss, dl = run_kernel(hip_lib, logits, labels, label_len, input_len)
    check_against_oracle(probs, loss, dl, labels, label_len, input_len, [s[2] for s in specs])


# 2 ------------------------------------------------------------------------------------------ mixed batch at the limit
def test_mixed_batch_at_2047(hip_lib):
    """l_max = 2047: a tight 2047-letter label beside an empty one, a single letter, 300 letters and 700 letters in 650 frames
    (infeasible); ragged input lengths, one below t_out."""
    rng = np.random.RandomState(7)
    k = 29
    lengths = [2047, 0, 1, 300, 700]
    regimes = ["learnt", "collapse", "sharp", "uniform", "wrong"]
    labels_list = [list(rng.randint(0, k - 1, size=n)) for n in lengths]
    t_out = min_frames(labels_list[0])
    input_len = [t_out, t_out - 1, 333, t_out - 400, 650]
    assert min_frames(labels_list[4]) > 650 and all(n <= t_out for n in input_len)
    logits = np.zeros((5, t_out, k), dtype=np.float32)
    for i in range(5):
        logits[i, :input_len[i]] = regime_logits(rng, labels_list[i], input_len[i], k, regimes[i])
    labels = o.pack_label_batch([lab if lab else [-1] for lab in labels_list])
    assert labels.shape[1] == 2047
    probs, loss, dl = run_kernel(hip_lib, logits, labels, lengths, input_len)
    check_against_oracle(probs, loss, dl, labels, lengths, input_len, regimes, infeasible=(4,))


# 3 ------------------------------------------------------------------------------------------ few classes, many classes
@pytest.mark.parametrize("k,length", [(5, 600), (64, 520)])
def test_few_and_many_classes(hip_lib, k, length):
    """K = 5: a quarter of the neighbours are equal letters, so the skip rule fires and fails to fire on consecutive states;
    K = 64: every lane of the gradient kernel's wave holds a class."""
    rng = np.random.RandomState(k)
    specs = [(length, 0, "sharp"), (length, 9, "uniform"), (length // 2, 40, "learnt")]
    logits, labels, label_len, input_len = build_batch(rng, k, specs)
    if k == 5:
        assert adjacent_repeats(list(labels[0])) > length // 6
    probs, loss, dl = run_kernel(hip_lib, logits, labels, label_len, input_len)
    check_against_oracle(probs, loss, dl, labels, label_len, input_len, [s[2] for s in specs])


# 4 ------------------------------------------------------------------------------------------ continuity across the dispatch
def _learnt_at_strength(rng, label, t, k, strength):
    """the "learnt" regime of tools/fuzz_ctc.regime_logits with its strength given instead of drawn from 6 .. 40"""
    lg = rng.randn(t, k).astype(np.float32)
    seq = []
    for j, c in enumerate(label):
        if j and c == label[j - 1]:
            seq.append(k - 1)
        seq.append(int(c))
    cuts = np.sort(rng.choice(np.arange(1, t), size=len(seq) - 1, replace=False)) if len(seq) > 1 else np.array([], int)
    bounds = np.concatenate([[0], cuts, [t]]).astype(int) if seq else np.array([0, 0])
    for j, sym in enumerate(seq):
        lg[bounds[j], sym] += strength
        lg[bounds[j] + 1:bounds[j + 1], k - 1] += strength
    if not seq:
        lg[:, k - 1] += strength
    return lg


def _both_paths(hip_lib, specs, seed, strength=None):
    rng = np.random.RandomState(seed)
    logits, labels, label_len, input_len = build_batch(rng, 29, specs)
    if strength is not None:
        for i in range(len(specs)):
            logits[i, :input_len[i]] = _learnt_at_strength(rng, list(labels[i, :label_len[i]]), input_len[i], 29, strength)
    assert labels.shape[1] == 511
    probs, loss_s, dl_s = run_kernel(hip_lib, logits, labels, label_len, input_len)
    _, loss_l, dl_l = run_kernel(hip_lib, logits, labels, label_len, input_len, l_max=600)
    # measurement beside the assertions: where each path stands against the oracle
    p64 = probs.astype(np.float64)
    ref_loss, ref_dp = o.ctc_batch_cost(p64, labels, input_len, label_len)
    ref_dl = o.softmax_backward(p64, ref_dp)
    for i in range(len(specs)):
        print("utterance %d (%d letters, %d frames, %s): loss %.7g at l_max 511, %.7g at 600, oracle %.7g; gradient: paths differ by "
              "%.2e, l_max 511 is %.2e from the oracle, l_max 600 %.2e" % (
                  i, label_len[i], input_len[i], specs[i][2], loss_s[i], loss_l[i], ref_loss[i], np.abs(dl_s[i] - dl_l[i]).max(),
                  np.abs(dl_s[i] - ref_dl[i]).max(), np.abs(dl_l[i] - ref_dl[i]).max()))
    assert np.isfinite(loss_s).all()
    return loss_s, dl_s, loss_l, dl_l, ref_dl


def test_continuity_across_the_dispatch(hip_lib):
    """One batch with labels of up to 511 letters: at l_max = 511 and padded to l_max = 600; losses to 1e-5 relative, gradients
    to 1e-4 absolute, the two calls against each other.  (Both widths run ctc_long.hip now; when this test was written l_max =
    511 ran the fp32 log-domain lattice of ctc.hip, and the cases below were chosen for what that one could meet.)

    The cases: at l_max = 511 the path was ctc_lattice_kernel, whose lattice values are fp32 logarithms.  A value of
    magnitude V carries ulp(V) / 2 from every frame (ctc.hip: 2.4e-4 each at 2^12, over 500 frames; DESIGN.md section 6 measured
    7e-5 .. 2e-3 absolute on the gradient), so it is itself within 1e-4 of anything only where |log2 alpha| stays below about 2^6
    (ulp 3.8e-6, over 650 frames) -- utterances whose loss is some nats.  And a relative 1e-5 on the loss means something only
    where the loss is not near 0.  Both hold in the "learnt" regime at a moderate strength: 8 added to the aligned symbol's
    logit leaves about 0.025 nats per frame, 0.8 .. 16 nats per utterance here; label lengths 0, 1, 40, 200 and 511, tight and
    slack.  test_both_paths_on_every_regime holds the other regimes to what the short path can give."""
    specs = [(511, 0, "learnt"), (511, 120, "learnt"), (200, 300, "learnt"), (0, 50, "learnt"), (40, 3, "learnt"),
             (1, 39, "learnt")]
    loss_s, dl_s, loss_l, dl_l, _ = _both_paths(hip_lib, specs, 11, strength=8.0)
    np.testing.assert_allclose(loss_l, loss_s, rtol=1e-5)
    assert np.abs(dl_s - dl_l).max() <= 1e-4


def test_both_paths_on_every_regime(hip_lib):
    """The same comparison on regimes whose losses run into the thousands: the losses of the two paths agree to 1e-5 relative and
    the gradient at l_max = 600 is within 1e-4 of the oracle.  When l_max = 511 still ran the fp32 log-domain lattice of ctc.hip
    (sl_ctc_select(1) runs it to this day; tests/test_gpu_ctc_mid.py holds what runs now to the oracle) this test measured: on the tight "sharp" utterance of 511 letters the two paths' gradients differ
    by 2.7e-3, all of it the short path's distance from the oracle (2.7e-3; relative L2 over the batch 1.1e-3) -- the long path is
    1.4e-6 from it; "uniform" 1.7e-4 against 2.8e-7, "wrong" 2.1e-5 against 5.5e-7."""
    specs = [(511, 0, "sharp"), (511, 120, "uniform"), (200, 300, "learnt"), (0, 50, "collapse"), (40, 3, "wrong")]
    loss_s, dl_s, loss_l, dl_l, ref_dl = _both_paths(hip_lib, specs, 11)
    np.testing.assert_allclose(loss_l, loss_s, rtol=1e-5)
    assert np.abs(dl_l - ref_dl).max() <= 1e-4


# 5 ------------------------------------------------------------------------------------------ determinism and destination
def test_determinism_scale_eps_and_bf16_destination(hip_lib):
    rng = np.random.RandomState(13)
    k = 29
    specs = [(700, 0, "wrong"), (1030, 30, "uniform"), (5, 100, "learnt")]
    logits, labels, label_len, input_len = build_batch(rng, k, specs)
    regimes = [s[2] for s in specs]
    first = run_kernel(hip_lib, logits, labels, label_len, input_len)
    again = run_kernel(hip_lib, logits, labels, label_len, input_len)
    assert first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    check_against_oracle(*first, labels, label_len, input_len, regimes)
    scaled = run_kernel(hip_lib, logits, labels, label_len, input_len, eps=1e-6, grad_scale=1.0 / 7)
    check_against_oracle(*scaled, labels, label_len, input_len, regimes, eps=1e-6, grad_scale=1.0 / 7)

    check_bf16_destination(hip_lib, logits, labels, label_len, input_len, first, halo=3, rs=40)


# 6 ------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(hip_lib):
    import torch
    from speechless_amd import _lib
    dev = "cuda:0"
    b, t, k = 2, 40, 29
    probs = torch.full((b, t, k), 1.0 / k, dtype=torch.float32, device=dev)
    logq = torch.log(probs)
    ll = torch.tensor([3, 3], dtype=torch.int32, device=dev)
    il = torch.tensor([t, t], dtype=torch.int32, device=dev)
    loss = torch.full((b,), FILL, dtype=torch.float32, device=dev)
    dl = torch.full((b, t, k), FILL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    size = hip_lib.raw("sl_ctc_workspace_bytes")
    call = hip_lib.raw("sl_ctc_loss_grad")

    def launch(l_max, ws, ws_bytes):
        lab = torch.zeros((b, l_max), dtype=torch.int32, device=dev)
        rc = call(probs.data_ptr(), logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), loss.data_ptr(),
                  dl.data_ptr(), b, t, k, l_max, 0, k, t * k, _lib.SL_F32, 1e-8, 1.0, ws.data_ptr(), ws_bytes, st)
        torch.cuda.synchronize()
        return rc

    assert size(b, t, 2048) == 0 and size(b, t, 2047) > 0
    big = torch.full((size(b, t, 2047),), 3, dtype=torch.uint8, device=dev)
    assert launch(2048, big, big.numel()) == SL_ERR_UNSUPPORTED
    assert "l_max" in hip_lib.last_error() and "2047" in hip_lib.last_error()
    for l_max in (600, 2047):
        assert launch(l_max, big, size(b, t, l_max) - 1) == SL_ERR_WORKSPACE_TOO_SMALL
        assert "workspace too small" in hip_lib.last_error()
    assert (loss == FILL).all() and (dl == FILL).all() and (big == 3).all()
    assert launch(600, big, size(b, t, 600)) == 0 and np.isfinite(loss.cpu().numpy()).all() and not (dl == FILL).any()


# 7 ------------------------------------------------------------------------------------------ engine
def test_engine_long_short_long_in_one_buffer_set():
    """An f32 engine, one buffer set: label batches [600, 40], [100, 30] and [600, 40] again.  Losses against the oracle on the
    engine's own probabilities, first and third run identical, the workspace never shrinks, and every weight gradient of the
    long batch against the float64 stack oracle to test_gpu_parity's bound for the f32 path (rel-L2 1e-4).

    The stack is a shrunken one (32 / 64 filters, two inner layers).  A ReLU whose pre-activation fp32 and float64 put on different
    sides of zero moves the gradients below it by far more than rounding does, and how many there are grows with the number of
    activations: test_loss_and_gradients_f32, where the 1e-4 comes from, has 96 frames of 6000 (5.8e5 decisions); this stack has
    1400 frames of 224 (3.1e5).  With the full-width lower stack and 256 top filters (3.5e6 decisions) striding_conv's dW was measured 1.7e-3 from
    float64 on this batch -- the distance README.md reports for that tensor at the benchmark's batch, whatever the labels."""
    import torch
    from test_gpu_parity import make_case, make_engine, rel_l2, weights64
    case = make_case(b=2, t=1400, seed=3, sizes=dict(main_filter_count=32, out_filter_count=64, inner_count=2))
    eng = make_engine(case, "f32")
    pred = [700, 690]
    results, sizes, grads = {}, [], None
    batches = {}
    for name, lengths in (("long", [600, 40]), ("short", [100, 30]), ("long_again", [600, 40])):
        rng = np.random.RandomState(5 if name != "short" else 6)
        labels = o.pack_label_batch([list(rng.randint(0, 28, size=n)) for n in lengths])
        batches[name] = (labels, lengths)
        eng.load_input(case["x"])
        eng.set_labels(labels, lengths, pred)
        eng.forward()
        losses = eng.ctc().cpu().numpy().copy()
        eng.backward()
        torch.cuda.synchronize()
        sizes.append(eng.cur.ctc_ws.numel())
        probs = eng.cur.probs.cpu().numpy().astype(np.float64)
        want, _ = o.ctc_batch_cost(probs, labels, pred, lengths)
        print(name, losses, want)
        assert np.isfinite(want).all()
        np.testing.assert_allclose(losses, want, rtol=2e-5)
        results[name] = (losses, eng.grads.clone())
        if name == "long":
            grads = eng.get_gradients()
    assert sizes[0] >= eng_need(2, eng.cur.tt_pad, 600) and sizes[1] >= sizes[0] and sizes[2] >= sizes[1]
    assert np.array_equal(results["long"][0], results["long_again"][0]) and torch.equal(results["long"][1], results["long_again"][1])
    labels, lengths = batches["long"]
    ref = o.loss_and_gradients(case["ospecs"], weights64(case), case["x"].astype(np.float64), labels, pred, lengths)
    np.testing.assert_allclose(results["long"][0], ref["losses"], rtol=1e-5)
    errors = [(rel_l2(dw, rw), rel_l2(db, rb)) for (dw, db), (rw, rb) in zip(grads, ref["grads"])]
    print("dW, db relative L2 per layer:", errors)
    for i, (ew, eb) in enumerate(errors):
        assert ew < 1e-4 and eb < 1e-4, "layer {}: dW rel-L2 {}, db rel-L2 {}".format(i, ew, eb)


def eng_need(batch, t_pad, l_max):
    from speechless_amd._lib import lib
    return lib().raw("sl_ctc_workspace_bytes")(batch, t_pad, l_max)


def test_split_top_and_launch_lists_at_600_letters():
    """The split-top engine (each half's CTC on a side stream, half-batch workspaces) and the recorded launch lists with a label
    batch 600 columns wide: bit-identical to the eager split steps, and the whole-batch trajectory within bf16 noise."""
    import torch
    from test_gpu_parity import make_case, make_engine
    case = make_case(b=4, t=1400, seed=4, sizes=dict(out_filter_count=256))
    rng = np.random.RandomState(8)
    lengths = [600, 40, 300, 10]
    labels = o.pack_label_batch([list(rng.randint(0, 28, size=n)) for n in lengths])
    pred = np.array([700, 690, 700, 650])
    finals = {}
    for mode in ("lists", "eager", "whole"):
        eng = make_engine(case, "bf16")
        eng.use_launch_lists = mode != "eager"
        eng.split_top = mode != "whole"
        eng.split_min_tiles = 0
        losses = [eng.train_step(case["x"], labels, np.array(lengths), pred).cpu().numpy().copy() for _ in range(3)]
        torch.cuda.synchronize()
        if mode != "whole":
            assert eng.cur.ctc_ws.numel() >= 2 * eng_need(3, eng.cur.tt_pad, 600)
        finals[mode] = (np.stack(losses), eng.params.clone())
    assert np.isfinite(finals["lists"][0]).all()
    assert np.array_equal(finals["lists"][0], finals["eager"][0]) and torch.equal(finals["lists"][1], finals["eager"][1])
    np.testing.assert_allclose(finals["lists"][0], finals["whole"][0], rtol=5e-3)


# 8 ------------------------------------------------------------------------------------------ Wav2Letter
class _Example:
    def __init__(self, spectrogram, label):
        self.id, self.label, self._x = "long", label, spectrogram

    def z_normalized_transposed_spectrogram(self):
        return self._x


def test_wav2letter_trains_on_a_600_letter_label():
    """compute_dtype="f32": one engine trains and evaluates, so train_on_batch's loss (the state before its step) and
    test_and_predict_batch's come from the same kernels on the same weights -- equal to fp32 rounding of the batch mean (1e-6
    relative).  Three more steps at Adam's 1e-4 lower the loss.  A 2048-letter label is a ValueError that names 2047."""
    from speechless_amd import Wav2Letter, english_frequent_characters
    net = Wav2Letter(128, english_frequent_characters, seed=3, layer_sizes=dict(out_filter_count=256), compute_dtype="f32")
    net.predictive_net.set_weights(Wav2Letter._glorot_uniform(o.layer_specs(128, 29, out_filter_count=256), 26))
    rng = np.random.RandomState(7)
    words = ["she", "was", "abc", "a", "zoo", "quiet", "morning"]
    label = " ".join(rng.choice(words, size=160))[:600].strip()
    assert 560 < len(label) <= 600
    example = _Example(np.random.RandomState(1).randn(1500, 128).astype(np.float32), label)
    before = net.test_and_predict_batch([example]).results[0].loss
    first = net.train_on_batch([example])
    print("loss before the step: evaluation", before, "training", first)
    assert np.isfinite(first) and abs(first - before) <= 1e-6 * abs(before)
    later = [net.train_on_batch([example]) for _ in range(3)]
    print("three more steps:", later)
    assert later[-1] < first
    too_long = _Example(example._x, "ab" * 1024)
    with pytest.raises(ValueError, match="2047"):
        net.train_on_batch([too_long])
    with pytest.raises(ValueError, match="2047"):
        net.test_and_predict_batch([too_long])
