"""sl_ctc_loss_grad alone on what the wave lattice does not take below 512 letters -- labels of 256 .. 511 letters, and 64 classes
at any label length -- and at the dispatch boundary 255 / 256, against the float64 oracle fed the kernel's own fp32 probabilities.

Helpers and bounds are those of tests/test_gpu_ctc_long.py (its module docstring), unchanged: loss within 1e-5 |ref| + T_b *
1.2e-6, every gradient entry within 1e-4 * grad_scale, "uniform" also relative L2 < 1e-3, an infeasible utterance +inf from kernel
and oracle, rows at and beyond input_len exactly zero.  No case has more than about 900 frames.

Until these tests existed this regime ran ctc_lattice_kernel, the log-domain lattice in fp32.  Measured with that library
(MI355X): 13 cases fail, all on the gradient's 1e-4 -- test_boundaries at 256, 257, 383 and 511 letters (1.3e-3, 3.9e-4, 7.4e-4,
9.4e-3), K = 64 from 127 letters on (5.0e-4 .. 8.8e-3; 40 letters: 8.5e-5), K = 5 (2.7e-3), the mixed batch (6.1e-3), l_max = 256
in the continuity test (1.0e-4) and the 64-class destination case (3.4e-4); DESIGN.md section 6 has the table.  With the double
log-domain lattice the worst gradient error of the module is 1.7e-6.  sl_ctc_select(1) still runs the fp32 lattice, and
test_variant_1_still_runs_the_fp32_log_lattice reports where it stands.
"""
import functools

import numpy as np
import pytest

from oracle import w2l_oracle as o
from test_gpu_ctc_long import (FILL, REGIMES, _learnt_at_strength, adjacent_repeats, build_batch, check_against_oracle,
                               check_bf16_destination, min_frames, run_kernel)
from fuzz_ctc import regime_logits  # (tools/ is on the path once test_gpu_ctc_long is imported)

pytestmark = pytest.mark.gpu

# both sides of: the gradient kernel instantiations of the fp32 log lattice (row stride <= 256 / <= 512 / beyond: l_max 127 | 128,
# 255 | 256), the dispatch from the wave lattice (255 | 256), a change of the thread count of ctc_long_lattice_kernel<2> in the
# middle (383: 384 threads, 384: 448), and the last length below the long labels
BOUNDARY_LENGTHS = (127, 128, 255, 256, 257, 383, 384, 511)
MAX_FRAMES = 900


@functools.lru_cache(maxsize=None)
def boundary_case(index):
    """three utterances of BOUNDARY_LENGTHS[index] letters with zero slack, one frame and L / 4 frames of slack, the five
    regimes in turn over the cases; built once, shared by the default path's test and variant 1's, never written to"""
    length = BOUNDARY_LENGTHS[index]
    rng = np.random.RandomState(300 + length)
    specs = [(length, slack, REGIMES[(3 * index + j) % 5]) for j, slack in enumerate((0, 1, length // 4))]
    logits, labels, label_len, input_len = build_batch(rng, 29, specs)
    assert labels.shape[1] == length and logits.shape[1] <= MAX_FRAMES
    for a in (logits, labels):
        a.setflags(write=False)
    return logits, labels, tuple(label_len), tuple(input_len), tuple(s[2] for s in specs)


# 1 ------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("index", range(len(BOUNDARY_LENGTHS)), ids=[str(n) for n in BOUNDARY_LENGTHS])
def test_boundaries(hip_lib, index):
    logits, labels, label_len, input_len, regimes = boundary_case(index)
    assert labels.shape[1] == BOUNDARY_LENGTHS[index]
    probs, loss, dl = run_kernel(hip_lib, logits, labels, label_len, input_len)
    check_against_oracle(probs, loss, dl, labels, label_len, input_len, regimes)


# 2 ------------------------------------------------------------------------------------------ many classes, few classes
@pytest.mark.parametrize("k,length", [(64, 1), (64, 40), (64, 127), (64, 128), (64, 255), (63, 255), (64, 300), (64, 511), (5, 300)])
def test_many_and_few_classes(hip_lib, k, length):
    """K = 64 (every lane of the gradient kernel's wave holds a class; the wave lattice stops at 63) from a one-letter label
    batch -- a work-group of one wave with 62 dead lanes, an empty label beside it -- to 511 letters; K = 63 at 255, the last
    shape the wave lattice takes, beside it; K = 5: a quarter of the neighbours are equal letters."""
    rng = np.random.RandomState(1000 * k + length)
    specs = [(length, 0, "sharp"), (length, 9, "uniform"), (length // 2, 40, "learnt")]
    logits, labels, label_len, input_len = build_batch(rng, k, specs)
    assert labels.shape[1] == length and logits.shape[1] <= MAX_FRAMES
    if k == 5:
        assert adjacent_repeats(list(labels[0])) > length // 6
    probs, loss, dl = run_kernel(hip_lib, logits, labels, label_len, input_len)
    check_against_oracle(probs, loss, dl, labels, label_len, input_len, [s[2] for s in specs])


# 3 ------------------------------------------------------------------------------------------ mixed batch at 511
def test_mixed_batch_at_511(hip_lib):
    """l_max = 511: a tight 511-letter label beside an empty one, a single letter, 300 letters and 400 letters in 380 frames
    (infeasible); ragged input lengths, one below t_out."""
    rng = np.random.RandomState(7)
    k = 29
    lengths = [511, 0, 1, 300, 400]
    regimes = ["sharp", "collapse", "learnt", "uniform", "wrong"]
    labels_list = [list(rng.randint(0, k - 1, size=n)) for n in lengths]
    t_out = min_frames(labels_list[0])
    input_len = [t_out, t_out - 1, 333, t_out - 100, 380]
    assert min_frames(labels_list[4]) > 380 and min_frames(labels_list[3]) <= t_out - 100 and t_out <= MAX_FRAMES
    logits = np.zeros((5, t_out, k), dtype=np.float32)
    for i in range(5):
        logits[i, :input_len[i]] = regime_logits(rng, labels_list[i], input_len[i], k, regimes[i])
    labels = o.pack_label_batch([lab if lab else [-1] for lab in labels_list])
    assert labels.shape[1] == 511
    probs, loss, dl = run_kernel(hip_lib, logits, labels, lengths, input_len)
    check_against_oracle(probs, loss, dl, labels, lengths, input_len, regimes, infeasible=(4,))


# 4 ------------------------------------------------------------------------------------------ continuity at 255 / 256
@pytest.mark.parametrize("strength", [8.0, None], ids=["learnt8", "regimes"])
def test_continuity_at_255_256(hip_lib, strength):
    """One batch with labels of 0, 1, 40, 200 and 255 letters at l_max = 255 (the wave lattice) and padded to l_max = 256
    (ctc_long.hip): both against the oracle, and gradients within 1e-4 of each other.  "learnt8": every utterance a learnt
    alignment of strength 8 (about 0.025 nats per frame, so every loss is some tenths of a nat to some nats: a relative bound on
    the loss means something only away from 0) -- losses of the two paths to 1e-5 relative; "regimes": the five regimes, one per utterance."""
    lengths, slacks = (0, 1, 40, 200, 255), (50, 39, 3, 300, 0)
    regimes = ["learnt"] * 5 if strength is not None else list(REGIMES)
    rng = np.random.RandomState(21)
    specs = [(n, s, r) for n, s, r in zip(lengths, slacks, regimes)]
    logits, labels, label_len, input_len = build_batch(rng, 29, specs)
    if strength is not None:
        for i in range(len(specs)):
            logits[i, :input_len[i]] = _learnt_at_strength(rng, list(labels[i, :label_len[i]]), input_len[i], 29, strength)
    assert labels.shape[1] == 255 and logits.shape[1] <= MAX_FRAMES
    probs, loss_w, dl_w = run_kernel(hip_lib, logits, labels, label_len, input_len)
    _, loss_l, dl_l = run_kernel(hip_lib, logits, labels, label_len, input_len, l_max=256)
    padded = np.concatenate([labels, -np.ones((5, 1), dtype=np.int32)], axis=1)
    for i in range(5):
        print("utterance %d (%d letters, %d frames, %s): loss %.7g at l_max 255, %.7g at 256; gradients differ by %.2e" % (
            i, label_len[i], input_len[i], regimes[i], loss_w[i], loss_l[i], np.abs(dl_w[i] - dl_l[i]).max()))
    check_against_oracle(probs, loss_w, dl_w, labels, label_len, input_len, regimes)
    check_against_oracle(probs, loss_l, dl_l, padded, label_len, input_len, regimes)
    assert np.abs(dl_w - dl_l).max() <= 1e-4
    if strength is not None:
        np.testing.assert_allclose(loss_l, loss_w, rtol=1e-5)


# 5 ------------------------------------------------------------------------------------------ destination and determinism
DESTINATION_CASES = {
    "300_letters": (29, 40, [(300, 0, "wrong"), (280, 30, "uniform"), (5, 100, "learnt")]),
    "64_classes": (64, 72, [(100, 0, "sharp"), (90, 20, "uniform"), (3, 50, "learnt")]),
    "wave_lattice_60": (29, 40, [(60, 0, "sharp"), (50, 10, "learnt"), (0, 30, "collapse")]),
}


@pytest.mark.parametrize("name", list(DESTINATION_CASES))
def test_determinism_scale_eps_and_bf16_destination(hip_lib, name):
    """The same call twice gives the same bytes; eps = 1e-6 with grad_scale = 1 / 7 stays within the oracle bounds; a bf16
    destination with halo 3, a row stride wider than K and a padded batch stride holds the fp32 result rounded to nearest even
    and FILL everywhere else, bit for bit.  At 300 letters, at 64 classes, and on the wave lattice (60 letters), whose
    destination never had such a test either."""
    k, rs, specs = DESTINATION_CASES[name]
    rng = np.random.RandomState(13 + k + specs[0][0])
    logits, labels, label_len, input_len = build_batch(rng, k, specs)
    assert labels.shape[1] == specs[0][0]
    regimes = [s[2] for s in specs]
    first = run_kernel(hip_lib, logits, labels, label_len, input_len)
    again = run_kernel(hip_lib, logits, labels, label_len, input_len)
    assert first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    check_against_oracle(*first, labels, label_len, input_len, regimes)
    scaled = run_kernel(hip_lib, logits, labels, label_len, input_len, eps=1e-6, grad_scale=1.0 / 7)
    check_against_oracle(*scaled, labels, label_len, input_len, regimes, eps=1e-6, grad_scale=1.0 / 7)
    assert not (first[2] == FILL).any()
    check_bf16_destination(hip_lib, logits, labels, label_len, input_len, first, halo=3, rs=rs)


# 6 ------------------------------------------------------------------------------------------ workspace
def test_workspace_size_never_shrinks_with_l_max(hip_lib):
    """host arithmetic: every l_max from 1 to 2047"""
    size = hip_lib.raw("sl_ctc_workspace_bytes")
    for batch, t_out in ((1, 40), (4, 700), (8, 4000)):
        sizes = [size(batch, t_out, l_max) for l_max in range(1, 2048)]
        assert sizes[0] > 0
        drops = [l_max for l_max in range(2, 2048) if sizes[l_max - 1] < sizes[l_max - 2]]
        assert not drops, (batch, t_out, drops[:5])


def test_a_workspace_sized_for_2047_serves_shorter_labels(hip_lib):
    """ONE workspace of sl_ctc_workspace_bytes(b, t, 2047), used for l_max = 300, 200 (the wave lattice) and 511 in turn with
    whatever the call before left in it: the same bytes as with a fresh workspace of exactly the call's own size."""
    import torch
    rng = np.random.RandomState(5)
    cases = [build_batch(rng, 29, [(n, 0, "sharp"), (n // 2, 25, "learnt")]) for n in (300, 200, 511)]
    t_max = max(c[0].shape[1] for c in cases)
    big = torch.full((hip_lib.raw("sl_ctc_workspace_bytes")(2, t_max, 2047),), 0x5A, dtype=torch.uint8, device="cuda:0")
    for logits, labels, label_len, input_len in cases:
        assert hip_lib.raw("sl_ctc_workspace_bytes")(2, logits.shape[1], labels.shape[1]) <= big.numel()
        exact = run_kernel(hip_lib, logits, labels, label_len, input_len)
        shared = run_kernel(hip_lib, logits, labels, label_len, input_len, ws=big)
        assert np.isfinite(exact[1]).all()
        assert exact[1].tobytes() == shared[1].tobytes() and exact[2].tobytes() == shared[2].tobytes(), labels.shape


# 7 ------------------------------------------------------------------------------------------ variant 1, for the record
@pytest.mark.parametrize("index", range(len(BOUNDARY_LENGTHS)), ids=[str(n) for n in BOUNDARY_LENGTHS])
def test_variant_1_still_runs_the_fp32_log_lattice(hip_lib, index):
    """sl_ctc_select(1) on the boundary cases: the fp32 log-domain lattice of ctc.hip (ctc_lattice_kernel with
    ctc_grad_kernel<4>, <8> and <16> -- row strides 256, 512 and beyond) for every label up to 511 letters.  Its gradient's
    distance from the oracle is REPORTED (test_gpu_parity._report's parity.json), not bounded: 7e-5 .. 3e-3 on labels with little slack is
    what that lattice gives.  Asserted is what test_ctc_lattice_variants_against_the_oracle asserts of
    variant 1 and this lattice can meet on such cases: the loss to 1e-5 relative (with this module's T_b * 1.2e-6 for the fp32
    logq, which alone decides where the loss is near 0), zeros past input_len -- and that the selector
    is what made the difference (another gradient than the default's at 256 letters and beyond)."""
    from test_gpu_parity import _report
    logits, labels, label_len, input_len, regimes = boundary_case(index)
    default = run_kernel(hip_lib, logits, labels, label_len, input_len)
    try:
        hip_lib.call("sl_ctc_select", 1)
        probs, loss, dl = run_kernel(hip_lib, logits, labels, label_len, input_len)
    finally:
        hip_lib.call("sl_ctc_select", 0)
    p64 = probs.astype(np.float64)
    ref_loss, ref_dp = o.ctc_batch_cost(p64, labels, input_len, label_len)
    ref_dl = o.softmax_backward(p64, ref_dp)
    errors = [float(np.abs(dl[i] - ref_dl[i]).max()) for i in range(3)]
    for i in range(3):
        print("variant 1, %d letters, %d frames, %-8s loss %.7g (oracle %.7g), gradient error %.2e (default path %.2e)" % (
            label_len[i], input_len[i], regimes[i], loss[i], ref_loss[i], errors[i], np.abs(default[2][i] - ref_dl[i]).max()))
    _report("ctc_mid_variant1_gradient_abs_error_l{}".format(BOUNDARY_LENGTHS[index]), dict(zip(regimes, errors)))
    assert np.isfinite(ref_loss).all()
    for i in range(3):
        assert abs(loss[i] - ref_loss[i]) <= 1e-5 * abs(ref_loss[i]) + input_len[i] * 1.2e-6, (i, loss[i], ref_loss[i])
        assert not dl[i, input_len[i]:].any()
    if BOUNDARY_LENGTHS[index] >= 256:
        assert dl.tobytes() != default[2].tobytes()


# 8 ------------------------------------------------------------------------------------------ engine
def test_engine_mid_short_long_mid_in_one_buffer_set(hip_lib):
    """A bf16 engine, one buffer set: label batches [300, 40], [100, 30], [600, 40] and [300, 40] again -- ctc_long.hip with two
    thread counts, the wave lattice between them, one workspace that only grows.  Every step's losses equal, bit for bit, those
    of sl_ctc_loss_grad alone on the engine's own probabilities with a fresh workspace of exactly its size; first and last step
    give the same losses, the same gradient of the logits and the same weight gradients."""
    import torch
    from speechless_amd import _lib
    from test_gpu_parity import make_case, make_engine
    case = make_case(b=2, t=1400, seed=3, sizes=dict(out_filter_count=256))
    eng = make_engine(case, "bf16")
    pred = [700, 690]
    results, sizes = [], []
    st = torch.cuda.current_stream().cuda_stream
    for lengths, seed in (([300, 40], 5), ([100, 30], 6), ([600, 40], 7), ([300, 40], 5)):
        rng = np.random.RandomState(seed)
        labels = o.pack_label_batch([list(rng.randint(0, 28, size=n)) for n in lengths])
        eng.load_input(case["x"])
        eng.set_labels(labels, lengths, pred)
        eng.forward()
        losses = eng.ctc().cpu().numpy().copy()
        buf = eng.cur
        dlogits = buf.g[len(eng.plans) - 1].clone()
        eng.backward()
        torch.cuda.synchronize()
        sizes.append(buf.ctc_ws.numel())
        b, t_out, k, l_max = buf.batch, buf.t_out, eng.grapheme_set_size, buf.labels.shape[1]
        assert l_max == lengths[0] and (b, k) == (2, 29)
        need = hip_lib.raw("sl_ctc_workspace_bytes")(b, t_out, l_max)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda:0")
        alone = torch.full((b,), FILL, dtype=torch.float32, device="cuda:0")
        dl = torch.zeros((b, t_out, k), dtype=torch.float32, device="cuda:0")
        hip_lib.call("sl_ctc_loss_grad", buf.probs.data_ptr(), buf.logq.data_ptr(), buf.labels.data_ptr(), buf.label_len.data_ptr(),
                     buf.input_len.data_ptr(), alone.data_ptr(), dl.data_ptr(), b, t_out, k, l_max, 0, k, t_out * k, _lib.SL_F32,
                     eng.ctc_epsilon, 1.0 / b, ws.data_ptr(), need, st)
        torch.cuda.synchronize()
        print(lengths, losses, alone.cpu().numpy())
        assert np.isfinite(losses).all() and losses.tobytes() == alone.cpu().numpy().tobytes()
        results.append((losses, dlogits, eng.grads.clone()))
    assert sizes == sorted(sizes)
    assert np.array_equal(results[0][0], results[3][0])
    assert torch.equal(results[0][1], results[3][1]) and torch.equal(results[0][2], results[3][2])
