"""sl_asg_segment_scores on the GPU: against the float64 restatement (tests/asg_segment_ref.py) at both ends of every
instantiation's range, under a shift of every logq row, with closed paths, against minus the ASG loss, its refusals, and end to
end through Engine and Wav2Letter.

Tolerance against the restatement: 1e-6 * (frames + |reference|) nats per segment (the header's).  A log-sum-exp step of the
numerator passes on at most the largest error of its inputs (its derivatives are weights that sum to 1) and adds the error of
the fp32 exp2 / log2 of a sum in [1, 2], which is below 1e-6; the lattice values themselves are doubles.  The denominator is
double arithmetic in the probability domain: about frames * k * 2^-53.  The second term covers the float32 result (2^-24 = 6e-8
relative).  -inf must match exactly.  Every comparison prints its worst |error| / bound before it asserts."""
import numpy as np
import pytest

from asg_cases import EPS, asg_regime_logits, asg_scores, build_asg_batch, run_asg
from asg_segment_ref import forward_score, segment_frames, segment_scores

pytestmark = pytest.mark.gpu

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED = -1, -2
SENTINEL = 123.0
KINDS = ("learnt", "sharp", "uniform", "collapse")
# label states per lane of asg_segment_kernel<NS> -> the seg_l_max it serves (csrc/asg_segment.hip: states_per_lane)
INSTANTIATIONS = {1: (1, 64), 2: (65, 128), 4: (129, 256), 8: (257, 511)}
TABLES = (("random", None), ("bigram", 30), ("hostile", 30), ("bigram", 12))


def softmax_logq(hip_lib, logits, eps=EPS):
    """sl_softmax_logq of (B, T, k) logits -> logq numpy"""
    import torch
    b, t, k = logits.shape
    lg = torch.tensor(logits, dtype=torch.float32, device="cuda:0")
    probs = torch.zeros_like(lg)
    logq = torch.zeros_like(lg)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    torch.cuda.synchronize()
    return logq.cpu().numpy()


def run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, seg_l_max, spare=3):
    """sl_asg_segment_scores on a float32 logq (B, T, k) into an output of n + spare floats that start from SENTINEL.  Returns
    the n results numpy; the spare entries are checked here."""
    import torch
    b, t, k = logq.shape
    dev = "cuda:0"
    labels = np.asarray(labels, dtype=np.int32)
    assert labels.ndim == 2 and labels.shape[0] == b and logq.dtype == np.float32
    segments = np.ascontiguousarray(segments, dtype=np.int32).reshape(-1, 5)
    n = segments.shape[0]
    lq = torch.tensor(logq, dtype=torch.float32, device=dev)
    tg = torch.tensor(np.asarray(trans), dtype=torch.float32, device=dev)
    tg0 = torch.tensor(np.asarray(init), dtype=torch.float32, device=dev)
    assert tuple(tg.shape) == (k, k) and tuple(tg0.shape) == (k,)
    lab = torch.tensor(labels if labels.size else np.zeros((b, 1), dtype=np.int32), dtype=torch.int32, device=dev)
    il = torch.tensor(np.asarray(input_len), dtype=torch.int32, device=dev)
    sg = torch.tensor(segments, dtype=torch.int32, device=dev)
    out = torch.full((n + spare,), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    need = hip_lib.raw("sl_asg_segment_scores_workspace_bytes")(n, seg_l_max, k)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_asg_segment_scores", lq.data_ptr(), tg.data_ptr(), tg0.data_ptr(), lab.data_ptr(), il.data_ptr(),
                 sg.data_ptr(), out.data_ptr(), b, t, k, labels.shape[1], n, seg_l_max, ws.data_ptr(), need, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    return got[:n]


def check_against(ref, frames, got, what=""):
    """the module's tolerance, segment by segment, against a restatement's results; returns the worst |error| / bound"""
    finite = np.isfinite(ref)
    assert np.array_equal(got[~finite], ref[~finite].astype(np.float32)), (what, got[~finite], ref[~finite])
    assert np.all(np.isfinite(got[finite])), (what, got[finite])
    bound = 1e-6 * (frames[finite] + np.abs(ref[finite]))
    zero = bound == 0  # (T = 0 and L = 0: exactly 0)
    assert np.all(got[finite][zero] == 0.0)
    ratio = np.abs(got[finite][~zero].astype(np.float64) - ref[finite][~zero]) / bound[~zero]
    worst = float(ratio.max()) if ratio.size else 0.0
    print("ASG segment scores {}: {} segments ({} -inf), worst |error| / bound {:.3e}, most negative score {:.1f}".format(
        what, len(ref), int((~finite).sum()), worst, float(ref[finite].min()) if finite.any() else 0.0))
    assert worst <= 1.0, (what, worst)
    return worst


def check_against_restatement(logq, trans, init, labels, input_len, segments, seg_l_max, got, what=""):
    labels = np.asarray(labels)
    ref = segment_scores(logq, trans, init, labels, input_len, segments, seg_l_max)
    frames = segment_frames(segments, input_len, logq.shape[1], labels.shape[1], seg_l_max, logq.shape[0])
    return check_against(ref, frames, got, what), ref, frames


def _label(rng, n, k, ns):
    """n random graphemes, with adjacent equal ones across and inside lane boundaries (a lane holds ns graphemes)"""
    label = [int(c) for c in rng.randint(0, k, size=n)]
    for p in range(ns, n, 3 * ns):  # the first grapheme of a lane equals the last of the lane below
        label[p] = label[p - 1]
    for p in range(2 * ns + 1, n, 5 * ns):  # and a pair just behind a boundary (inside the lane where ns > 1)
        label[p] = label[p - 1]
    return label


_cases = {}


def _instantiation_case(seg_l_max, k, ns):
    """B = 3 utterances whose labels have seg_l_max graphemes, T_b = L + slack for slack 0 / 1 / 17, t_out 3 frames more, with
    their tables and the issue's list of segments, all for one launch.  Built once per (seg_l_max, k) and left unchanged."""
    if (seg_l_max, k) in _cases:
        return _cases[seg_l_max, k]
    rng = np.random.RandomState(1000 * ns + 10 * k + seg_l_max)
    n = seg_l_max
    labels_list = [_label(rng, n, k, ns) for _ in range(3)]
    input_len = [n + slack for slack in (0, 1, 17)]
    t_out = max(input_len) + 3
    logits = np.zeros((3, t_out, k), dtype=np.float32)
    for b in range(3):
        logits[b] = asg_regime_logits(rng, labels_list[b], t_out, k, KINDS[(seg_l_max + b + k) % len(KINDS)])
    score_kind, s = TABLES[(seg_l_max + k) % len(TABLES)]
    trans, init = asg_scores(rng, labels_list, k, score_kind, s)
    labels = np.array(labels_list, dtype=np.int32).reshape(3, n)
    segments = [(-1, 0, 5, 0, 1), (3, 0, 5, 0, 1)]  # b out of range
    for b in range(3):
        tb = input_len[b]
        segments += [
            (b, 0, tb, 0, n),                      # the whole utterance: frame 0 and the last frame, start scores g0
            (b, 0, t_out + 5, 0, n + 100),         # both ranges beyond their ends: clamped to the same
            (b, tb, t_out, 0, min(n, 3)),          # frames past input_len: clamped away
            (b, min(3, tb), min(20, tb), 1, 1),    # L = 0 with T > 0: -inf without a blank
            (b, 2, 2, 0, 0),                       # L = 0 and T = 0
            (b, 0, n - 1, 0, n),                   # one frame short: infeasible
        ]
        # parts of the label over parts of the frames, neither begin nor length a multiple of 16: begin > 0 starts from the
        # scores out of the grapheme before the segment
        for begin, count, first, spare in ((n // 3, n // 2, 5, 7), (1, min(n - 1, 9), 3, 2), (n - min(n, 5), min(n, 5), 1, 21)):
            if count < 1 or begin < 0:
                continue
            end = min(first + count + spare, tb)
            segments.append((b, first, end, begin, begin + count))  # (infeasible where the frames run out: -inf on both sides)
            segments.append((b, tb - (end - first), tb, begin, begin + count))  # the same up against the last frame
    case = (logits, trans, init, labels, input_len, np.array(segments, dtype=np.int64), (score_kind, s))
    _cases[seg_l_max, k] = case
    return case


def test_case_table_covers_the_dispatcher():
    bounds = sorted(v for lo_hi in INSTANTIATIONS.values() for v in lo_hi)
    assert bounds == [1, 64, 65, 128, 129, 256, 257, 511]
    assert all(hi <= 64 * ns and (lo == 1 or lo > 32 * ns) for ns, (lo, hi) in INSTANTIATIONS.items())
    assert any(s == 30 for _, s in TABLES)


INSTANTIATION_CASES = [(ns, bound, 31) for ns in sorted(INSTANTIATIONS) for bound in (0, 1)] + \
    [(ns, bound, k) for ns in (1, 8) for bound in (0, 1) for k in (2, 64)]


@pytest.mark.parametrize("ns,bound,k", INSTANTIATION_CASES)
def test_segment_scores_at_every_instantiation(hip_lib, ns, bound, k):
    seg_l_max = INSTANTIATIONS[ns][bound]
    logits, trans, init, labels, input_len, segments, tables = _instantiation_case(seg_l_max, k, ns)
    logq = softmax_logq(hip_lib, logits)
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, seg_l_max)
    what = "NS={} seg_l_max={} k={} tables={}".format(ns, seg_l_max, k, tables)
    _, ref, _ = check_against_restatement(logq, trans, init, labels, input_len, segments, seg_l_max, got, what)
    assert np.isfinite(ref[2]) and ref[0] == ref[1] == -np.inf  # (the whole first utterance is feasible; b out of range)
    assert got[2] == got[3]  # the clamped ranges are the whole utterance
    assert seg_l_max < 8 or np.isfinite(ref).sum() >= 12  # (the partial spans are scored, not all refused)


@pytest.mark.parametrize("ns,bound,k", [(1, 1, 31), (2, 0, 31), (8, 1, 31), (8, 1, 64), (1, 0, 2)])
def test_a_shift_of_every_logq_row_cancels(hip_lib, ns, bound, k):
    """Every logq row shifted by -2000 stays within the bound of the UNSHIFTED reference: an exp of the emissions as they are
    would underflow to 0 in every lane.  The rows are first rounded to multiples of 2^-12, so that the shifted float32 rows are
    the unshifted ones minus 2000 exactly (an fp32 ulp at 2000 is 1.2e-4: without that the shift itself would perturb the
    emissions by far more than the bound)."""
    seg_l_max = INSTANTIATIONS[ns][bound]
    logits, trans, init, labels, input_len, segments, tables = _instantiation_case(seg_l_max, k, ns)
    logq = (np.round(softmax_logq(hip_lib, logits).astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
    shifted = (logq.astype(np.float64) - 2000.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64) + 2000.0, logq.astype(np.float64))
    what = "NS={} seg_l_max={} k={}".format(ns, seg_l_max, k)
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, seg_l_max)
    _, ref, frames = check_against_restatement(logq, trans, init, labels, input_len, segments, seg_l_max, got, what + " rounded")
    got = run_segment_kernel(hip_lib, shifted, trans, init, labels, input_len, segments, seg_l_max)
    check_against(ref, frames, got, what + " shifted by -2000")
    assert np.isfinite(got[2])


def test_three_hundred_one_word_segments_in_one_launch(hip_lib):
    """words of 1 .. 9 graphemes anywhere in three utterances, the smallest instantiation, several launches' worth of waves"""
    rng = np.random.RandomState(300)
    k, t_out, l_max = 31, 237, 150
    labels = rng.randint(0, k, size=(3, l_max)).astype(np.int32)
    input_len = [237, 200, 101]
    logits = np.stack([asg_regime_logits(rng, list(labels[b]), t_out, k, kind)
                       for b, kind in enumerate(("learnt", "sharp", "uniform"))]).astype(np.float32)
    trans, init = asg_scores(rng, [list(r) for r in labels], k, "random")
    segments = []
    for _ in range(300):
        b = int(rng.randint(0, 3))
        n = int(rng.randint(1, 10))
        l0 = int(rng.randint(0, l_max - n + 1))
        f0 = int(rng.randint(0, input_len[b] - 2))
        segments.append((b, f0, min(f0 + n + int(rng.randint(0, 40)), t_out), l0, l0 + n))
    segments = np.array(segments, dtype=np.int64)
    logq = softmax_logq(hip_lib, logits)
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, 9)
    assert np.isfinite(got).sum() > 200
    check_against_restatement(logq, trans, init, labels, input_len, segments, 9, got, "300 words")
    # a seg_l_max below a segment's span cuts the span: the same launch at seg_l_max = 4
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, 4)
    check_against_restatement(logq, trans, init, labels, input_len, segments, 4, got, "300 words cut to 4 graphemes")


def test_closed_paths_give_minus_infinity_and_no_nan(hip_lib):
    rng = np.random.RandomState(77)
    k, n, t_out = 31, 70, 90
    label = [int(c) for c in rng.permutation(k)] * 3
    label = label[:n]  # no adjacent equal graphemes, every bigram of the label known
    labels = np.array([label], dtype=np.int32)
    logq = softmax_logq(hip_lib, asg_regime_logits(rng, label, t_out, k, "learnt")[None])
    trans, init = asg_scores(rng, [label], k, "random")
    segments = np.array([(0, 0, t_out, 0, n), (0, 10, 40, 20, 30), (0, 50, 90, 60, 70), (0, 5, 30, 0, 9)], dtype=np.int64)
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, [t_out], segments, n)
    check_against_restatement(logq, trans, init, labels, [t_out], segments, n, got, "open")
    assert np.all(np.isfinite(got))
    # one -inf move on the label's path (graphemes 24 -> 25): the segments that hold it are closed, exactly
    closed = trans.copy()
    closed[label[24], label[25]] = -np.inf
    got = run_segment_kernel(hip_lib, logq, closed, init, labels, [t_out], segments, n)
    _, ref, _ = check_against_restatement(logq, closed, init, labels, [t_out], segments, n, got, "one move closed")
    holds = np.array([label[i] == label[24] and label[i + 1] == label[25] for i in range(n - 1)])
    assert [bool(holds[b:e - 1].any()) for _, _, _, b, e in segments] == [True, True, False, False]
    assert np.array_equal(np.isfinite(got), [False, False, True, True]) and np.all(got[:2] == -np.inf)
    # -inf elsewhere: a finite result (Z shrinks)
    other = trans.copy()
    other[label[3], label[1]] = -np.inf
    got = run_segment_kernel(hip_lib, logq, other, init, labels, [t_out], segments, n)
    check_against_restatement(logq, other, init, labels, [t_out], segments, n, got, "a move off the path closed")
    assert np.all(np.isfinite(got))
    # every move into the label's graphemes closed: N = -inf, Z finite where the start scores are open
    block = trans.copy()
    block[:, sorted(set(label[:10]))] = -np.inf
    got = run_segment_kernel(hip_lib, logq, block, init, labels, [t_out], segments, n)
    check_against_restatement(logq, block, init, labels, [t_out], segments, n, got, "a column block closed")
    assert np.all(got[[0, 3]] == -np.inf)
    # everything closed: Z = -inf and N = -inf give -inf, never NaN
    got = run_segment_kernel(hip_lib, logq, np.full((k, k), -np.inf, dtype=np.float32), np.full(k, -np.inf, dtype=np.float32),
                             labels, [t_out], segments, n)
    assert np.all(got == -np.inf)
    got = run_segment_kernel(hip_lib, logq, trans, np.full(k, -np.inf, dtype=np.float32), labels, [t_out], segments, n)
    assert np.all(got[[0, 3]] == -np.inf) and np.all(np.isfinite(got[[1, 2]]))  # (only these two start from g0)
    # a frame whose emissions are all -inf: Z = -inf for the segments over it, the others as before
    dead = logq.copy()
    dead[0, 20] = -np.inf
    got = run_segment_kernel(hip_lib, dead, trans, init, labels, [t_out], segments, n)
    assert np.array_equal(np.isfinite(got), [False, False, True, False]) and not np.isnan(got).any()


@pytest.mark.parametrize("k,score_kind,s", [(31, "random", None), (64, "bigram", 30), (2, "hostile", 12)])
def test_whole_label_equals_minus_the_asg_loss(hip_lib, k, score_kind, s):
    """one segment per utterance that covers all of it against sl_asg_loss_grad on the same batch, within the sum of both
    kernels' bounds: 1e-6 (T + |score|) here, 1e-6 |loss| + 1e-6 there (tests/asg_cases.py)"""
    rng = np.random.RandomState(k)
    specs = [(1, 0, "learnt"), (40, 3, "learnt"), (100, 17, "sharp"), (255, 40, "uniform"), (300, 1, "collapse"), (12, -2, "learnt")]
    logits, labels_list, input_len = build_asg_batch(rng, k, specs)
    trans, init = asg_scores(rng, labels_list, k, score_kind, s)
    run = run_asg(hip_lib, logits, trans, init, labels_list, input_len, dlogits=False, tables=False)
    assert run.rc == 0
    l_max = max(len(l) for l in labels_list)
    labels = np.zeros((len(specs), l_max), dtype=np.int32)
    for row, l in zip(labels, labels_list):
        row[:len(l)] = l
    segments = np.array([(b, 0, input_len[b], 0, len(l)) for b, l in enumerate(labels_list)], dtype=np.int64)
    logq = softmax_logq(hip_lib, logits)
    got = run_segment_kernel(hip_lib, logq, trans, init, labels, input_len, segments, l_max)
    check_against_restatement(logq, trans, init, labels, input_len, segments, l_max, got, "whole utterances, k = {}".format(k))
    print("minus loss", -run.loss, "segment posterior", got)
    assert np.isposinf(run.loss[-1]) and got[-1] == -np.inf  # the infeasible utterance
    loss = run.loss[:-1].astype(np.float64)
    bound = 1e-6 * (np.array(input_len[:-1]) + np.abs(got[:-1])) + 1e-6 * np.abs(loss) + 1e-6
    print("worst |score + loss| / bound", float((np.abs(got[:-1] + loss) / bound).max()))
    assert np.all(np.isfinite(loss)) and np.all(np.abs(got[:-1] + loss) <= bound)


def test_refusals_leave_the_output_untouched(hip_lib):
    import torch
    dev = "cuda:0"
    k, t, l_max, n = 31, 20, 8, 4
    logq = torch.zeros((2, t, k), dtype=torch.float32, device=dev)
    trans = torch.zeros((k, k), dtype=torch.float32, device=dev)
    init = torch.zeros((k,), dtype=torch.float32, device=dev)
    lab = torch.zeros((2, l_max), dtype=torch.int32, device=dev)
    il = torch.full((2,), t, dtype=torch.int32, device=dev)
    sg = torch.tensor([[0, 0, 10, 0, 3]] * n, dtype=torch.int32, device=dev)
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.empty((16,), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    score = hip_lib.raw("sl_asg_segment_scores")
    ptrs = [x.data_ptr() for x in (logq, trans, init, lab, il, sg, out)]
    assert score(*ptrs, 2, t, k, l_max, n, 512, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED
    assert "seg_l_max = 512" in hip_lib.last_error() and "511" in hip_lib.last_error()
    assert score(*ptrs, 2, t, 65, l_max, n, 8, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED and "k = 65" in hip_lib.last_error()
    assert score(*ptrs, 2, t, 1, l_max, n, 8, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED and "k = 1" in hip_lib.last_error()
    assert score(*ptrs, 2, t, k, l_max, 0, 8, ws.data_ptr(), 16, st) == SL_ERR_UNSUPPORTED
    for i, name in enumerate(("logq", "trans", "init", "labels", "input_len", "segments", "log_posterior")):
        args = list(ptrs)
        args[i] = None
        assert score(*args, 2, t, k, l_max, n, 8, ws.data_ptr(), 16, st) == SL_ERR_INVALID_ARGUMENT
        assert name + " is a null pointer" in hip_lib.last_error()
    # the workspace: the entry point asks for none at any shape (a segment's lattices live in registers and LDS), so there is
    # no size below the one asked for; a null workspace of 0 bytes is taken
    need = hip_lib.raw("sl_asg_segment_scores_workspace_bytes")(n, 8, k)
    assert need == 0
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL).item()
    assert score(*ptrs, 2, t, k, l_max, n, 8, None, 0, st) == 0
    torch.cuda.synchronize()
    ref = segment_scores(np.zeros((2, t, k)), np.zeros((k, k)), np.zeros(k), np.zeros((2, l_max), dtype=np.int32), [t, t],
                         [(0, 0, 10, 0, 3)] * n, 8)
    assert np.all(np.abs(out.cpu().numpy() - ref) <= 1e-6 * (10 + np.abs(ref)))


# ---------------------------------------------------------------------------------------------- Engine
@pytest.mark.parametrize("dtype,forward_only", [("f32", False), ("f16x3", True)])
def test_engine_scores_on_its_own_emissions_and_on_a_tensor_handed_in(dtype, forward_only):
    import torch
    from test_gpu_asg import K_ASG, toy_case, toy_engine
    case = toy_case(64)
    eng = toy_engine(case, dtype, forward_only=forward_only)
    pred_len = np.array(case["prediction_lengths"]).reshape(-1)
    rng = np.random.RandomState(4)
    labels = rng.randint(0, K_ASG, size=(3, 12)).astype(np.int32)
    labels[0, :7] = [K_ASG - 1, 3, K_ASG - 2, 3, 3, 0, K_ASG - 1]  # the repeat marks are ordinary labels here
    eng.load_input(case["x"])
    eng.forward()
    eng.set_input_lengths(pred_len)
    t_out = eng.cur.t_out
    segments = np.array([(b, 0, int(pred_len[b]), 0, 12) for b in range(3)] +
                        [(0, 2, 11, 1, 6), (1, 0, 9, 3, 4), (2, 5, int(pred_len[2]), 7, 12), (2, 3, 3, 2, 2), (1, 0, 5, 0, 7)])
    got = eng.asg_segment_scores(labels, segments)
    assert got.dtype == np.float32 and got.shape == (len(segments),)
    logq = eng.cur.logq.cpu().numpy()
    trans, init = eng.asg_trans.cpu().numpy(), eng.asg_init.cpu().numpy()
    assert np.array_equal(trans, case["g"]) and np.array_equal(init, case["g0"])
    _, ref, frames = check_against_restatement(logq, trans, init, labels, list(pred_len), segments, 12, got, "engine " + dtype)
    assert np.isfinite(ref[:6]).all() and ref[6] == 0.0 and ref[7] == -np.inf
    assert np.array_equal(eng.asg_segment_scores(labels, segments), got)  # the tensors are reused
    # a tensor handed in, with lengths of its own
    own = torch.log_softmax(torch.tensor(rng.randn(2, 40, K_ASG).astype(np.float32), device=eng.device), dim=2)
    long_segments = np.array([(0, 0, 40, 0, 12), (1, 3, 33, 2, 9), (1, 0, 35, 0, 12), (1, 30, 40, 0, 2)])
    got = eng.asg_segment_scores_long(own, labels[:2], [40, 35], long_segments)
    check_against_restatement(own.cpu().numpy(), trans, init, labels[:2], [40, 35], long_segments, 12, got, "engine long")
    assert np.array_equal(eng.asg_segment_scores(labels, segments), eng.asg_segment_scores(labels, segments))
    # the engine's checks: the first bad row is named, labels a segment covers must be graphemes in [0, K)
    with pytest.raises(ValueError, match=r"segment 1 = \[3, .*sl_asg_segment_scores"):
        eng.asg_segment_scores(labels, np.array([segments[0], (3, 0, 5, 0, 1)]))
    with pytest.raises(ValueError, match=r"segment 0 = \[0, 0, 5, 0, 512\]"):
        eng.asg_segment_scores_long(own, labels[:2], [40, 35], np.array([(0, 0, 5, 0, 512)]))
    with pytest.raises(ValueError, match=r"outside \[0, {}\)$".format(K_ASG)):
        eng.asg_segment_scores(np.full((3, 12), K_ASG), segments)
    with pytest.raises(ValueError, match="outside"):
        eng.asg_segment_scores(np.full((3, 12), -1), segments)
    assert np.isfinite(eng.asg_segment_scores(np.where(np.arange(12) < 6, labels, K_ASG), np.array([(0, 0, 20, 0, 6)]))).all()
    with pytest.raises(ValueError, match="logq must be"):
        eng.asg_segment_scores_long(own[0], labels[:1], [40], long_segments[:1])
    assert t_out >= int(pred_len.max())


def test_ctc_engine_refuses_asg_segment_scores():
    import torch
    from test_gpu_asg import toy_case
    from test_gpu_parity import make_engine
    case = toy_case(64)
    eng = make_engine(case, "f32")
    segments = np.array([(0, 0, 5, 0, 1)])
    with pytest.raises(ValueError, match="criterion='asg'"):
        eng.asg_segment_scores(np.zeros((3, 3), dtype=np.int32), segments)
    with pytest.raises(ValueError, match="criterion='asg'"):
        eng.asg_segment_scores_long(torch.zeros((1, 8, eng.grapheme_set_size), device=eng.device), np.zeros((1, 3), dtype=np.int32),
                                    [8], segments)


def test_a_refused_alignment_leaves_no_wide_label_tensor_behind():
    """asg_confidence_of_recording follows other users of a net: labels of more than 511 graphemes, which sl_asg_align refuses,
    must not widen the aligner's tensors for good (their width is the l_max of every later call on the buffer set)"""
    from speechless_amd.launch_list import HipLibraryError
    from test_gpu_asg import K_ASG, toy_case, toy_engine
    case = toy_case(64)
    eng = toy_engine(case, "f32", forward_only=True)
    pred_len = np.array(case["prediction_lengths"]).reshape(-1)
    eng.load_input(case["x"])
    eng.forward()
    labels = np.random.RandomState(1).randint(0, K_ASG, size=(3, 9)).astype(np.int32)
    paths, scores = eng.asg_align(labels, [9, 9, 9], pred_len)
    with pytest.raises(HipLibraryError, match="511"):
        eng.asg_align(np.zeros((3, 598), dtype=np.int32), [9, 9, 9], pred_len)
    again, again_scores = eng.asg_align(labels, [9, 9, 9], pred_len)
    assert np.array_equal(again, paths) and again_scores.tobytes() == scores.tobytes() and np.isfinite(scores).all()


# ---------------------------------------------------------------------------------------------- Wav2Letter
def _net():
    from test_gpu_asg_longform import _net as asg_longform_net
    return asg_longform_net("f16x3")


def _batch(rng, n, frames):
    from speechless_amd.net import LabeledSpectrogram
    words = ("she", "was", "abc", "a", "zoo", "quiet", "all", "feet")  # (runs of two: repeat marks in the encoded label)
    return [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(words, size=rng.randint(1, 6))),
                               spectrogram=rng.randn(frames - 20 * i, 128).astype(np.float32)) for i in range(n)]


def _check_scored(net, scored, logq, frames, tolerance_factor=1.0):
    """a ScoredAlignment against the restatement applied to logq (T', K), the net's tables and the alignment it holds"""
    from speechless_amd import AsgAlignment, grapheme_spans, word_spans
    state = net.eval_engine.get_asg_state()
    trans, init = np.asarray(state["trans"], dtype=np.float64), np.asarray(state["init"], dtype=np.float64)
    label = scored.label
    encoded = net.grapheme_encoding.encode(label)
    assert isinstance(scored.alignment, AsgAlignment) and scored.alignment.encoded_label == encoded
    assert [w.word for w in scored.words] == label.split() == [w for w, _ in scored.alignment.word_frames]
    spans = grapheme_spans(label, word_spans(label))
    for w, (_, (first, end)), (begin, stop) in zip(scored.words, scored.alignment.word_frames, spans):
        assert (w.first, w.end) == (first, end)
        ref = forward_score(logq[first:end], trans, init if begin == 0 else trans[encoded[begin - 1]], encoded[begin:stop])
        assert abs(w.log_posterior - ref) <= tolerance_factor * 1e-6 * (end - first + abs(ref)), (w, ref)
        assert w.log_posterior <= 1e-6 * (end - first) and 0.0 <= w.confidence <= 1.0 + 1e-4
    ref = forward_score(logq[:frames], trans, init, encoded)
    if np.isfinite(scored.log_posterior) or np.isfinite(ref):
        assert abs(scored.log_posterior - ref) <= tolerance_factor * 1e-6 * (frames + abs(ref))
    return ref


def test_asg_word_confidence_batch_end_to_end():
    net = _net()
    rng = np.random.RandomState(12)
    batch = _batch(rng, 3, 301)
    scored = net.asg_word_confidence_batch(batch)
    logq = net.eval_engine.cur.logq.cpu().numpy()
    alignments = net.asg_alignment_batch(batch)
    losses = [r.loss for r in net.test_and_predict_batch(batch).results]
    assert len(scored) == 3
    for b, (s, a, x, loss) in enumerate(zip(scored, alignments, batch, losses)):
        frames = x.z_normalized_transposed_spectrogram().shape[0] // net.input_to_prediction_length_ratio
        assert s.label == x.label and s.alignment.word_frames == a.word_frames and len(s.words) == len(x.label.split()) > 0
        assert s.alignment.log_probability == a.log_probability
        assert np.array_equal(s.alignment.frame_grapheme_positions, a.frame_grapheme_positions)
        _check_scored(net, s, logq[b], frames)
        bound = 1e-6 * (frames + abs(s.log_posterior)) + 1e-6 * abs(loss) + 1e-6  # both kernels' bounds
        print("utterance {}: log posterior {:.6f}, minus loss {:.6f}, |sum| / bound {:.3e}".format(
            b, s.log_posterior, -loss, abs(s.log_posterior + loss) / bound))
        assert np.isfinite(loss) and abs(s.log_posterior + loss) <= bound


def test_asg_predict_with_confidence_returns_the_transcripts_of_predict():
    net = _net()
    enc = net.grapheme_encoding
    rng = np.random.RandomState(13)
    batch = _batch(rng, 3, 260)
    spectrograms = [x.z_normalized_transposed_spectrogram() for x in batch]
    scored = net.asg_predict_with_confidence_batch(spectrograms)
    logq = net.eval_engine.cur.logq.cpu().numpy()
    transcripts = net.predict_batch_greedily(spectrograms)
    assert len(scored) == 3 and any(s is not None for s in scored)
    for b, (s, x, transcript) in enumerate(zip(scored, spectrograms, transcripts)):
        if s is None:  # a transcript the encoding cannot write is not scored
            with pytest.raises(ValueError, match="fold repetition"):
                enc.encode(transcript)
            continue
        assert s.label == transcript
        _check_scored(net, s, logq[b], x.shape[0] // net.input_to_prediction_length_ratio)
        assert np.isfinite(s.log_posterior) == (len(transcript) > 0)
    one = net.asg_predict_with_confidence(batch[0])
    assert (one.label if one is not None else transcripts[0]) == net.predict(batch[0]) == transcripts[0]
    assert one is None or [w.word for w in one.words] == one.label.split()


def test_asg_confidence_of_recording_matches_the_batch_and_tiles_like_cut_sections():
    from speechless_amd import cut_sections
    from speechless_amd.net import LabeledSpectrogram
    from test_gpu_asg_longform import _label
    from test_gpu_longform import WINDOW, _Example, _recording
    net = _net()
    enc = net.grapheme_encoding
    label = _label(np.random.RandomState(14), enc, 200)
    x = _recording(1100, seed=5)  # three windows of 512, 550 output frames, and short enough for one forward pass
    example = _Example(x, label)
    single = net.asg_word_confidence_batch([LabeledSpectrogram(id="r", label=label, spectrogram=x)])[0]
    scored, sections = net.asg_confidence_of_recording(example, max_section_frames=120, window_input_frames=WINDOW)
    n_words = len(label.split())
    assert scored.alignment.word_frames == single.alignment.word_frames and len(scored.words) == n_words > 30
    # the stitched frames are bit-identical to a single pass: the same path and score, and scores within both launches' bounds
    assert np.array_equal(scored.alignment.frame_grapheme_positions[:550], single.alignment.frame_grapheme_positions[:550])
    assert scored.alignment.log_probability == single.alignment.log_probability
    for w, v in zip(scored.words, single.words):
        assert (w.word, w.first, w.end) == (v.word, v.first, v.end)
        assert abs(w.log_posterior - v.log_posterior) <= 2e-6 * (w.end - w.first + abs(v.log_posterior))
    assert abs(scored.log_posterior - single.log_posterior) <= 2e-6 * (550 + abs(single.log_posterior))
    assert [(text, frames) for text, frames, _ in sections] == cut_sections(scored.alignment, 120) and len(sections) > 3
    assert all(b[1][0] == a[1][1] for a, b in zip(sections, sections[1:]))
    assert all(np.isfinite(score) and score < 0 for _, _, score in sections)
    # without max_section_frames: the words alone
    scored2, none = net.asg_confidence_of_recording(example, window_input_frames=WINDOW)
    assert none == [] and [w.log_posterior for w in scored2.words] == [w.log_posterior for w in scored.words]
    # a section of more than 511 encoded graphemes names the argument to lower; without sections the whole label is nan
    long_label = " ".join(["ab"] * 180)  # 539 graphemes over 550 frames
    assert len(enc.encode(long_label)) == 539
    with pytest.raises(ValueError, match="max_section_frames.*encoded graphemes.*sl_asg_segment_scores"):
        net.asg_confidence_of_recording(_Example(x, long_label), max_section_frames=100000, window_input_frames=WINDOW)
    scored3, _ = net.asg_confidence_of_recording(_Example(x, long_label), window_input_frames=WINDOW)
    assert len(scored3.words) == 180 and np.isnan(scored3.log_posterior)


def test_a_ctc_net_refuses_the_asg_confidence_methods():
    from speechless_amd import Wav2Letter, english_frequent_characters
    from test_gpu_longform import LAYER_SIZES, _Example, _recording
    x = _recording(300)
    ctc = Wav2Letter(128, english_frequent_characters, seed=1, layer_sizes=LAYER_SIZES)
    for call in (lambda: ctc.asg_confidence_of_recording(_Example(x, "abc")), lambda: ctc.asg_predict_with_confidence_batch([x]),
                 lambda: ctc.asg_predict_with_confidence(_Example(x, "abc")),
                 lambda: ctc.asg_word_confidence_batch([_Example(x, "abc")])):
        with pytest.raises(ValueError, match="criterion='asg'"):
            call()
