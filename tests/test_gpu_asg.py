"""ASG criterion on the GPU: sl_asg_loss_grad against the float64 restatement of tests/test_asg.py, sl_asg_viterbi bit for bit
against its float32 restatement, the engine's ASG training step against torch-CPU autograd of the same net, and the
Wav2Letter(criterion="asg") API."""
import sys
from pathlib import Path

import numpy as np
import pytest

from test_asg import EPS, asg_loss_torch_from_probs, asg_reference, asg_reference_batch, asg_viterbi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
REGIMES = ("uniform", "sharp", "collapse")  # tools/fuzz_ctc.py regime_logits: uniform, peaked, collapsed


def regime_logits(rng, label, t, k, kind):
    sys.path.insert(0, str(ROOT / "tools"))
    from fuzz_ctc import regime_logits as fuzz_regime_logits
    return fuzz_regime_logits(rng, label, t, k, kind)


def softmax_logq(hip_lib, logits, eps=EPS):
    import torch
    b, t, k = logits.shape
    lg = torch.tensor(logits, dtype=torch.float32, device="cuda:0")
    probs = torch.zeros((b, t, k), dtype=torch.float32, device="cuda:0")
    logq = torch.zeros_like(probs)
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps,
                 torch.cuda.current_stream().cuda_stream)
    return probs, logq


def run_asg_kernel(hip_lib, logits, g, g0, labels_list, input_len, eps=EPS, grad_scale=1.0, l_max=None, softmax=True):
    """probs from sl_softmax_logq (softmax=False: `logits` are taken as the probabilities), then sl_asg_loss_grad with an
    fp32 destination.  Everything as numpy; the outputs start from a fill value, so that what the kernel does not write shows."""
    import torch
    from speechless_amd import _lib
    b, t, k = logits.shape
    dev = "cuda:0"
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, l_max), dtype=np.int32)
    for i, l in enumerate(labels_list):
        labels[i, :len(l)] = l
    if softmax:
        probs, logq = softmax_logq(hip_lib, logits, eps)
    else:
        probs = torch.tensor(logits, dtype=torch.float32, device=dev)
        logq = torch.log(probs + eps)
    tg = torch.tensor(g, dtype=torch.float32, device=dev)
    tg0 = torch.tensor(g0, dtype=torch.float32, device=dev)
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor([len(l) for l in labels_list], dtype=torch.int32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    loss = torch.full((b,), 7.0, dtype=torch.float32, device=dev)
    dl = torch.full((b, t, k), 7.0, dtype=torch.float32, device=dev)
    dg = torch.full((k, k), 7.0, dtype=torch.float32, device=dev)
    dg0 = torch.full((k,), 7.0, dtype=torch.float32, device=dev)
    need = hip_lib.raw("sl_asg_workspace_bytes")(b, t, k, l_max)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    rc = hip_lib.raw("sl_asg_loss_grad")(probs.data_ptr(), logq.data_ptr(), tg.data_ptr(), tg0.data_ptr(), lab.data_ptr(),
                                         ll.data_ptr(), il.data_ptr(), loss.data_ptr(), dl.data_ptr(), dg.data_ptr(),
                                         dg0.data_ptr(), b, t, k, l_max, 0, k, t * k, _lib.SL_F32, eps, grad_scale,
                                         ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, probs.cpu().numpy(), loss.cpu().numpy(), dl.cpu().numpy(), dg.cpu().numpy(), dg0.cpu().numpy()


def make_batch(rng, k, t, lengths, kinds=REGIMES):
    """lengths: [(T_b, L)] -> (logits (B, t, k) with zero rows past T_b, labels, input lengths); the regimes in turn.  Labels
    are drawn with adjacent equal letters allowed (the kernel must accept them)."""
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for _, n in lengths]
    logits = np.zeros((len(lengths), t, k), dtype=np.float32)
    for i, (t_b, _) in enumerate(lengths):
        if t_b > 0:
            logits[i, :t_b] = regime_logits(rng, labels_list[i], t_b, k, kinds[i % len(kinds)])
    return logits, labels_list, [t_b for t_b, _ in lengths]


def check_against_float64(hip_lib, rng, k, t, lengths, grad_scale=1.0):
    """The bounds tests/test_gpu_parity.py holds sl_ctc_loss_grad to against its float64 oracle (test_ctc_kernel_edge_cases):
    loss to 1e-5 relative, every entry of dlogits (O(1) at grad_scale 1) to 1e-4 absolute.  dtrans / dinit are sums of such
    entries over frames and utterances: the same 1e-4 absolute plus the loss's 1e-5 relative."""
    g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
    g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
    logits, labels_list, input_len = make_batch(rng, k, t, lengths)
    rc, probs, loss, dl, dg, dg0 = run_asg_kernel(hip_lib, logits, g, g0, labels_list, input_len, grad_scale=grad_scale)
    assert rc == 0
    ref_loss, ref_dl, ref_dg, ref_dg0 = asg_reference_batch(probs, g, g0, labels_list, input_len, grad_scale=grad_scale)
    feasible = np.array([0 < len(l) <= t_b for l, t_b in zip(labels_list, input_len)])
    assert np.isfinite(ref_loss[feasible]).all() and (ref_loss[feasible] >= 0).all()
    assert np.isinf(ref_loss[~feasible]).all() and np.isinf(loss[~feasible]).all() and (loss[~feasible] > 0).all()
    np.testing.assert_allclose(loss[feasible], ref_loss[feasible], rtol=1e-5)
    for i, t_b in enumerate(input_len):
        assert np.abs(dl[i] - ref_dl[i]).max() < 1e-4 * grad_scale, (i, lengths[i], np.abs(dl[i] - ref_dl[i]).max())
        assert not dl[i, max(t_b, 0):].any()  # rows past the utterance: exactly zero
        if not feasible[i]:
            assert not dl[i].any()
    np.testing.assert_allclose(dg, ref_dg, rtol=1e-5, atol=1e-4 * grad_scale)
    np.testing.assert_allclose(dg0, ref_dg0, rtol=1e-5, atol=1e-4 * grad_scale)
    return loss, dl, dg, dg0


def grid_lengths(rng, t):
    """utterances of a T'-frame batch: every label length of the grid that fits, the first at full length, zero slack
    (L = T_b) included, the others with input_len < T' where T' allows"""
    out = []
    for n in (1, 2, t, 63, 64, 65):
        if n <= t and (t, n) not in out:
            out.append((t, n))
    for n in (1, 2, 63, 64, 65):
        if n < t:
            t_b = int(rng.randint(n, t))
            out.append((t_b, n))
            out.append((n, n))  # zero slack
    return out


@pytest.mark.parametrize("k", [5, 30, 34, 64])
def test_loss_and_gradients_match_float64_on_the_shape_grid(hip_lib, k):
    rng = np.random.RandomState(100 + k)
    for t in (1, 2, 3, 64, 65, 130):
        check_against_float64(hip_lib, rng, k, t, grid_lengths(rng, t))


def test_long_labels_single_utterance_and_a_full_batch(hip_lib):
    rng = np.random.RandomState(7)
    check_against_float64(hip_lib, rng, 30, 256, [(256, 200), (201, 200), (230, 137)])  # 4 label states per lane
    check_against_float64(hip_lib, rng, 30, 65, [(65, 20)])                              # B = 1
    check_against_float64(hip_lib, rng, 34, 130, [(130, 128)])                           # 2 label states per lane
    check_against_float64(hip_lib, rng, 5, 310, [(310, 300), (305, 257)])                # 8 label states per lane
    lengths = []
    for _ in range(32):  # B = 32, mixed lengths, the mean's scale
        t_b = int(rng.randint(2, 66))
        lengths.append((t_b, int(rng.randint(1, t_b + 1))))
    check_against_float64(hip_lib, rng, 30, 65, lengths, grad_scale=1.0 / 32)


def test_infeasible_utterances_next_to_feasible_ones(hip_lib):
    """L = 0, L = T_b + 1 and T_b = 0 between feasible utterances: +inf, zero rows, and dtrans / dinit bit for bit those of
    the feasible utterances run alone"""
    rng = np.random.RandomState(21)
    k, t = 30, 40
    lengths = [(40, 7), (40, 0), (33, 12), (9, 10), (0, 3), (40, 40)]
    g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
    g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
    logits, labels_list, input_len = make_batch(rng, k, t, lengths)
    rc, probs, loss, dl, dg, dg0 = run_asg_kernel(hip_lib, logits, g, g0, labels_list, input_len)
    assert rc == 0
    keep = [0, 2, 5]
    for i in (1, 3, 4):
        assert loss[i] == np.inf and not dl[i].any()
    ref_loss, ref_dl, ref_dg, ref_dg0 = asg_reference_batch(probs, g, g0, labels_list, input_len)
    np.testing.assert_allclose(loss[keep], ref_loss[keep], rtol=1e-5)
    assert np.abs(dl - ref_dl).max() < 1e-4
    np.testing.assert_allclose(dg, ref_dg, rtol=1e-5, atol=1e-4)
    rc, _, loss2, dl2, dg2, dg02 = run_asg_kernel(hip_lib, logits[keep], g, g0, [labels_list[i] for i in keep],
                                                  [input_len[i] for i in keep])
    assert rc == 0
    assert dg2.tobytes() == dg.tobytes() and dg02.tobytes() == dg0.tobytes()
    assert loss2.tobytes() == loss[keep].tobytes() and dl2.tobytes() == dl[keep].tobytes()


def test_the_same_call_twice_gives_the_same_bits(hip_lib):
    rng = np.random.RandomState(5)
    k, t = 30, 65
    lengths = [(int(t_b), int(rng.randint(1, t_b + 1))) for t_b in rng.randint(2, t + 1, size=32)]
    g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
    g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
    logits, labels_list, input_len = make_batch(rng, k, t, lengths)
    first = run_asg_kernel(hip_lib, logits, g, g0, labels_list, input_len, grad_scale=1.0 / 32)
    second = run_asg_kernel(hip_lib, logits, g, g0, labels_list, input_len, grad_scale=1.0 / 32)
    assert first[0] == 0 and second[0] == 0
    for a, b in zip(first[2:], second[2:]):
        assert a.tobytes() == b.tobytes()


def test_limits_are_refused_and_nothing_is_written(hip_lib):
    rng = np.random.RandomState(1)
    for k, l_max in ((65, 4), (30, 512)):
        probs = np.full((1, 6, k), 1.0 / k, dtype=np.float32)
        assert hip_lib.raw("sl_asg_workspace_bytes")(1, 6, k, l_max) == 0
        rc, _, loss, dl, dg, dg0 = run_asg_kernel(hip_lib, probs, np.zeros((k, k)), np.zeros(k), [[1, 2]], [6], l_max=l_max,
                                                  softmax=False)
        assert rc == -2, (k, l_max, hip_lib.last_error())  # SL_ERR_UNSUPPORTED
        assert (loss == 7).all() and (dl == 7).all() and (dg == 7).all() and (dg0 == 7).all()
    assert hip_lib.raw("sl_asg_viterbi_workspace_bytes")(1, 6, 65) == 0
    assert hip_lib.raw("sl_asg_workspace_bytes")(2, 6, 64, 511) > 0


# ------------------------------------------------------------------------------------------------------------- Viterbi
def run_viterbi_kernel(hip_lib, emis, g, g0, input_len):
    import torch
    b, t, k = emis.shape
    dev = "cuda:0"
    e = torch.tensor(emis, dtype=torch.float32, device=dev)
    tg = torch.tensor(g, dtype=torch.float32, device=dev)
    tg0 = torch.tensor(g0, dtype=torch.float32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    path = torch.full((b, t), 7, dtype=torch.int32, device=dev)
    score = torch.zeros((b,), dtype=torch.float32, device=dev)
    need = hip_lib.raw("sl_asg_viterbi_workspace_bytes")(b, t, k)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_asg_viterbi", e.data_ptr(), tg.data_ptr(), tg0.data_ptr(), il.data_ptr(), path.data_ptr(),
                 score.data_ptr(), b, t, k, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return path.cpu().numpy(), score.cpu().numpy(), need


def check_viterbi_bits(emis, g, g0, input_len, paths, scores):
    for i, t_b in enumerate(input_len):
        ref_score, ref_path = asg_viterbi(emis[i], g, g0, min(max(t_b, 0), emis.shape[1]))
        assert np.array_equal(paths[i], ref_path), (i, t_b, np.flatnonzero(paths[i] != ref_path)[:5])
        assert np.float32(scores[i]).tobytes() == np.float32(ref_score).tobytes(), (i, scores[i], ref_score)


@pytest.mark.parametrize("k", [5, 30, 34, 64])
def test_viterbi_is_bit_identical_to_the_float32_restatement(hip_lib, k):
    rng = np.random.RandomState(300 + k)
    for t in (1, 2, 3, 64, 65, 130):
        input_len = [t, int(rng.randint(0, t + 1)), 0, t + 5][:4 if t > 1 else 2]
        lengths = [(min(t_b, t), 1) for t_b in input_len]
        logits, _, _ = make_batch(rng, k, t, lengths)
        _, logq = softmax_logq(hip_lib, logits)
        emis = logq.cpu().numpy()
        g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
        g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
        paths, scores, need = run_viterbi_kernel(hip_lib, emis, g, g0, input_len)
        assert need == 0
        check_viterbi_bits(emis, g, g0, input_len, paths, scores)
        if t > 1:
            assert scores[2] == -np.inf and (paths[2] == -1).all()


def test_viterbi_ties_forced_transitions_and_backpointers_in_hbm(hip_lib):
    k, t = 30, 12
    zeros = np.zeros((2, t, k), dtype=np.float32)
    paths, scores, _ = run_viterbi_kernel(hip_lib, zeros, np.zeros((k, k)), np.zeros(k), [12, 7])
    assert (paths[0] == 0).all() and (paths[1][:7] == 0).all() and (paths[1][7:] == -1).all() and (scores == 0).all()
    # a strongly negative g(i, i): the best path may not stay, so it differs from the per-frame argmax
    rng = np.random.RandomState(2)
    emis = np.log(np.full((1, t, k), 0.01, dtype=np.float32))
    emis[0, :, 4] = np.log(np.float32(0.71))
    g = np.zeros((k, k), dtype=np.float32)
    g[np.arange(k), np.arange(k)] = -50.0
    paths, scores, _ = run_viterbi_kernel(hip_lib, emis, g, np.zeros(k), [t])
    assert (emis[0].argmax(1) == 4).all() and (paths[0][::2] == 4).all() and (paths[0][1::2] != 4).all()
    check_viterbi_bits(emis, g, np.zeros(k, dtype=np.float32), [t], paths, scores)
    # 2200 frames x 64 letters: the backpointers do not fit LDS and go through the workspace
    k, t = 64, 2200
    emis = np.log(rng.dirichlet(np.ones(k) * 0.3, size=(2, t)).astype(np.float32) + np.float32(EPS))
    g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
    g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
    paths, scores, need = run_viterbi_kernel(hip_lib, emis, g, g0, [t, 1500])
    assert need == 2 * t * k
    check_viterbi_bits(emis, g, g0, [t, 1500], paths, scores)


# ------------------------------------------------------------------------------------------------------------- engine
SMALL = dict(main_filter_count=20, out_filter_count=40, inner_count=1)  # the toy stack of the other GPU tests
K_ASG = 30


def toy_case(t, seed=3):
    from test_gpu_parity import make_case
    case = make_case(b=3, t=t, k=K_ASG, seed=seed, sizes=SMALL)
    rng = np.random.RandomState(50 + t)
    case["g"] = rng.uniform(-1, 1, size=(K_ASG, K_ASG)).astype(np.float32)
    case["g0"] = rng.uniform(-1, 1, size=K_ASG).astype(np.float32)
    return case


def toy_engine(case, dtype, **kw):
    from test_gpu_parity import make_engine
    eng = make_engine(case, dtype, criterion="asg", **kw)
    eng.set_asg_scores(case["g"], case["g0"])
    return eng


_AUTOGRAD = {}


def autograd_reference(case, t):
    """float64 torch-CPU autograd of the same net under the mean ASG loss (computed once per T, shared, never changed)"""
    if t in _AUTOGRAD:
        return _AUTOGRAD[t]
    import torch
    from oracle import w2l_torch_cpu as tc
    tw = [(torch.tensor(np.ascontiguousarray(np.transpose(w, (2, 1, 0))), dtype=torch.float64, requires_grad=True),
           torch.tensor(b, dtype=torch.float64, requires_grad=True)) for w, b in case["weights"]]
    g = torch.tensor(case["g"], dtype=torch.float64, requires_grad=True)
    g0 = torch.tensor(case["g0"], dtype=torch.float64, requires_grad=True)
    probs = tc.forward_probs(case["ospecs"], tw, torch.tensor(case["x"], dtype=torch.float64))
    losses = torch.stack([asg_loss_torch_from_probs(probs[i, :case["prediction_lengths"][i]], g, g0,
                                                    case["labels"][i][:case["label_lengths"][i]])
                          for i in range(probs.shape[0])])
    losses.mean().backward()
    _AUTOGRAD[t] = dict(losses=losses.detach().numpy(), dg=g.grad.numpy(), dg0=g0.grad.numpy(),
                        grads=[(np.ascontiguousarray(np.transpose(w.grad.numpy(), (2, 1, 0))), b.grad.numpy()) for w, b in tw])
    return _AUTOGRAD[t]


def asg_loss_and_grads(eng, case):
    import torch
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
    eng.forward()
    losses = eng.asg().cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    return losses


# the bounds these engines meet for the CTC loss: f32 tests/test_gpu_parity.py::test_loss_and_gradients_f32 (1e-4), bf16x3
# tests/test_gpu_round3.py (5e-3), f16x3 tests/test_gpu_round6.py::test_f16x3_loss_and_gradients_against_the_float64_oracle
# (1e-3; 2e-3 on striding_conv's dW); loss 1e-5 relative on all three
GRAD_BOUND = {"f32": 1e-4, "bf16x3": 5e-3, "f16x3": 1e-3}


@pytest.mark.parametrize("t", [64, 77])
@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16x3"])
def test_engine_asg_step_gradients_against_torch_autograd(dtype, t):
    from test_gpu_parity import rel_l2
    case = toy_case(t)
    ref = autograd_reference(case, t)
    eng = toy_engine(case, dtype)
    losses = asg_loss_and_grads(eng, case)
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5)
    bound = GRAD_BOUND[dtype]
    for spec, (dw, db), (rw, rb) in zip(case["specs"], eng.get_gradients(), ref["grads"]):
        ew, eb = rel_l2(dw, rw), rel_l2(db, rb)
        print(dtype, t, spec.name, ew, eb)
        assert ew < (2e-3 if (dtype == "f16x3" and spec.name == "striding_conv") else bound) and eb < bound, (spec.name, ew, eb)
    et, ei = rel_l2(eng.asg_dtrans.cpu().numpy(), ref["dg"]), rel_l2(eng.asg_dinit.cpu().numpy(), ref["dg0"])
    print(dtype, t, "asg tables", et, ei)
    assert et < bound and ei < bound, (et, ei)
    # the evaluation side: a forward_only engine over the same scores computes the same loss and needs no gradient buffers
    decoded, paths = eng.asg_viterbi(case["prediction_lengths"])
    logq = eng.cur.logq.cpu().numpy()
    for i, t_b in enumerate(case["prediction_lengths"]):
        score, path = asg_viterbi(logq[i], case["g"], case["g0"], t_b)
        assert np.array_equal(paths[i], path)
        assert decoded[i] == [int(c) for j, c in enumerate(path[:t_b]) if j == 0 or c != path[j - 1]]


def test_engine_asg_on_bf16_loss_and_thirty_steps():
    import torch
    case = toy_case(64)
    ref = autograd_reference(case, 64)
    eng = toy_engine(case, "bf16", lr=1e-3)
    losses = asg_loss_and_grads(eng, case)
    np.testing.assert_allclose(losses, ref["losses"], rtol=2e-3)  # tests/test_gpu_parity.py: the bf16 engine's CTC loss bound
    before = eng.asg_trans.cpu().numpy().copy()
    for _ in range(30):
        eng.train_step_resident()
    torch.cuda.synchronize()
    after = eng.cur.loss.cpu().numpy()
    assert np.isfinite(after).all() and after.mean() < losses.mean()
    assert eng.adam_iterations == 30 and np.abs(eng.asg_trans.cpu().numpy() - before).max() > 1e-3
    assert np.abs(eng.asg_init.cpu().numpy() - case["g0"]).max() > 1e-3


def test_asg_step_replays_its_recorded_lists_and_refuses_the_split_schedule():
    case = toy_case(64)
    eng = toy_engine(case, "bf16")
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
    for _ in range(2):
        eng.train_step_resident()
    assert not eng.split_top
    with pytest.raises(ValueError, match="split-top"):
        eng.forward(split_ctc=(1.0, 1))


# ---------------------------------------------------------------------------------------------------------------- API
def asg_net(**kw):
    from speechless_amd.grapheme_encoding import english_frequent_characters
    from speechless_amd.net import Wav2Letter
    return Wav2Letter(128, english_frequent_characters, criterion="asg", layer_sizes=SMALL, seed=4, **kw)


def examples(labels, frames=(80, 64, 72)):
    from speechless_amd.net import LabeledSpectrogram
    rng = np.random.RandomState(8)
    return [LabeledSpectrogram(str(i), l, rng.randn(frames[i % len(frames)], 128).astype(np.float32))
            for i, l in enumerate(labels)]


def test_api_losses_equal_the_restatement_on_the_engines_own_probabilities():
    net = asg_net()
    assert net.grapheme_encoding.grapheme_set_size == 30 and net.engine.asg_trans.shape == (30, 30)
    rng = np.random.RandomState(3)
    net.engine.set_asg_scores(rng.uniform(-1, 1, size=(30, 30)), rng.uniform(-1, 1, size=30))
    batch = examples(["hello there", "aaa bb", "x"])
    result = net.test_and_predict_batch(batch)
    engine = net.eval_engine
    probs = engine.cur.probs.cpu().numpy()
    state = engine.get_asg_state()
    labels = [net.grapheme_encoding.encode(x.label) for x in batch]
    assert labels[0][3] == net.grapheme_encoding.asg_twice and labels[1] == [0, 29, 26, 1, 28]
    ref = asg_reference_batch(probs, state["trans"], state["init"], labels, [40, 32, 36])[0]
    got = np.array([r.loss for r in result.results])
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-5)
    assert all(isinstance(r.predicted, str) for r in result.results)


def test_api_predict_decodes_the_viterbi_path_with_repeat_marks():
    net = asg_net()
    enc = net.grapheme_encoding
    e = enc.encode_character("e")
    kernel, bias = net.predictive_net.layers[-1].get_weights()
    bias = np.full_like(bias, -10.0)
    bias[e], bias[enc.asg_twice] = 10.0, 10.5  # every frame: asg_twice a little ahead of "e", nothing else in sight
    net.predictive_net.layers[-1].set_weights([np.zeros_like(kernel), bias])
    g = np.zeros((30, 30), dtype=np.float32)
    g[enc.asg_twice, :] = -50.0              # ... but the scores let a path start on "e" only and never leave asg_twice
    g[enc.asg_twice, enc.asg_twice] = 0.0
    g0 = np.full(30, -50.0, dtype=np.float32)
    g0[e] = 0.0
    net.engine.set_asg_scores(g, g0)
    example = examples(["ee"])[0]
    assert net.predict(example) == "ee"
    assert net.predict_batch_greedily([example.z_normalized_transposed_spectrogram()]) == ["ee"]


def test_api_asg_state_round_trips_through_the_epoch_files(tmp_path):
    net = asg_net(asg_transition_probabilities=np.full((31, 31), 0.25), asg_initial_probabilities=np.full(30, 0.5))
    assert np.allclose(net.engine.asg_trans.cpu().numpy(), np.log(0.25)) and np.allclose(net.engine.asg_init.cpu().numpy(), np.log(0.5))
    batch = examples(["hello there", "aaa bb", "x"])
    for _ in range(3):
        loss = net.train_on_batch(batch)
    assert np.isfinite(loss)
    net.predictive_net.save_weights(tmp_path / net.model_file_name(1))
    net.save_asg_state(tmp_path, 1)
    net.save_optimizer_state(tmp_path, 1)
    assert (tmp_path / "asg-epoch1.npz").exists()
    saved = net.engine.get_asg_state()
    assert sorted(saved) == ["init", "init_m", "init_v", "trans", "trans_m", "trans_v"] and saved["trans_v"].any()
    again = asg_net(load_model_from_directory=tmp_path, load_epoch=1, load_optimizer_state=True)
    for name, value in again.engine.get_asg_state().items():
        assert value.tobytes() == saved[name].tobytes(), name
    scores_only = asg_net(load_model_from_directory=tmp_path, load_epoch=1)
    state = scores_only.engine.get_asg_state()
    assert state["trans"].tobytes() == saved["trans"].tobytes() and not state["trans_m"].any()


def test_api_refuses_what_asg_does_not_cover():
    from speechless_amd.grapheme_encoding import english_frequent_characters
    from speechless_amd.net import Adam, Wav2Letter
    with pytest.raises(ValueError, match="kenlm_directory"):
        asg_net(kenlm_directory="no/such/directory")
    with pytest.raises(ValueError, match="clip"):
        asg_net(optimizer=Adam(1e-4, clipnorm=1.0))
    with pytest.raises(ValueError, match="clip"):
        asg_net(optimizer=Adam(1e-4, clipvalue=0.5))
    with pytest.raises(ValueError, match="track_gradient_norm"):
        asg_net(track_gradient_norm=True)
    with pytest.raises(ValueError, match="criterion"):
        Wav2Letter(128, english_frequent_characters, criterion="nope")
    with pytest.raises(NotImplementedError):
        Wav2Letter(128, english_frequent_characters, use_asg=True)
    net = asg_net()
    batch = examples(["ab", "c"])
    with pytest.raises(ValueError, match="forced alignment"):
        net.alignment_batch(batch)
    with pytest.raises(ValueError, match="forced alignment"):
        net.positional_label_batch(batch, seconds_per_input_step=0.01)

    class TwoRanks:
        world_size, force, shard_optimizer, comm_cus = 2, False, False, 0

    with pytest.raises(ValueError, match="data-parallel"):
        net.train_on_batch(batch, reducer=TwoRanks())
    ctc_net = Wav2Letter(128, english_frequent_characters, layer_sizes=SMALL, seed=4,
                         asg_transition_probabilities=np.ones((3, 3)))  # ignored under "ctc", as ever
    assert ctc_net.engine.asg_params is None
    with pytest.raises(ValueError, match="criterion='asg'"):
        ctc_net.engine.asg()
