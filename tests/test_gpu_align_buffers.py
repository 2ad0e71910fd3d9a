"""The forced aligners' and asg_viterbi_long's tensors (buffers._AlignBuffers) across calls of different sizes: an engine that
has served a wider, a narrower, a smaller and a larger call returns the bytes a freshly built engine returns for each of them
-- same kernel, same inputs, no tolerance -- the short and the long aligner still agree where both apply, and the loss's own
tensors are left alone.  Also: the launches ctc() and asg() record, by tag."""
import numpy as np
import pytest

from test_gpu_asg import toy_case, toy_engine
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

T = 64
WIDTHS = (12, 3, 20)           # the short aligner's label widths in call order: its tensors shrink-fit nothing, then grow
LONG_SHAPES = ((3, 12), (1, 5), (3, 20))  # (rows of logq, label width) of the long aligner's calls, in order


def build(kind, case):
    """an engine of `kind` with the case's weights (and scores) behind forward()"""
    eng = make_engine(case, "f32") if kind == "ctc" else toy_engine(case, "f16x3", forward_only=True)
    eng.load_input(case["x"])
    eng.forward()
    return eng


def label_batch(rows, width):
    """`rows` labels without equal neighbours (feasible in T / 2 frames at every width used here) of width, width - 1, ...
    letters, padded with -1"""
    labels = np.full((rows, width), -1, dtype=np.int32)
    lengths = [max(width - i, 1) for i in range(rows)]
    for i, n in enumerate(lengths):
        labels[i, :n] = (7 * i + 3 * np.arange(n)) % 28
    return labels, lengths


def calls(kind, case, step):
    """the calls of round `step` as (name, function of an engine and its cloned logq -> tuple of arrays)"""
    lens = case["prediction_lengths"]
    short, long = ("ctc_align", "ctc_align_long") if kind == "ctc" else ("asg_align", "asg_align_long")
    width = WIDTHS[step]
    rows, long_width = LONG_SHAPES[step]
    out = [("short", lambda eng, logq: getattr(eng, short)(*label_batch(3, width), lens)),
           ("long", lambda eng, logq: getattr(eng, long)(logq[:rows], *label_batch(rows, long_width), lens[:rows]))]
    if kind == "asg":
        out.append(("viterbi_long", lambda eng, logq: eng.asg_viterbi_long(logq[:rows])[1:]))
    return out


def run_round(kind, case, eng, step):
    logq = eng.cur.logq.clone()
    return {name: tuple(np.array(a) for a in call(eng, logq)) for name, call in calls(kind, case, step)}


def same_bytes(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                                         for a, b in zip(got, want))


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_reused_tensors_give_the_bytes_of_a_fresh_engine(kind):
    import torch
    case = toy_case(T)
    eng = build(kind, case)
    if kind == "ctc":
        eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        loss_before = eng.ctc().cpu().numpy().tobytes()
        grad_before = eng.cur.g[-1].cpu().numpy().tobytes()
        loss_labels = eng.cur.labels.cpu().numpy().tobytes()
    reused = [run_round(kind, case, eng, step) for step in range(3)]
    for step in range(3):
        fresh = run_round(kind, case, build(kind, case), step)  # (one new engine per round: each call meets no tensors)
        assert fresh.keys() == reused[step].keys()
        for name, want in fresh.items():
            paths, scores = want[0], want[-1]
            assert paths.dtype == np.int32 and paths.shape == (LONG_SHAPES[step][0] if name != "short" else 3, T // 2)
            assert (paths[:, 0] >= 0).all(), (kind, step, name)  # (every label is feasible: real paths are compared)
            if name != "viterbi_long":
                assert scores.dtype == np.float32 and scores.shape == paths.shape[:1] and np.isfinite(scores).all()
            assert same_bytes(reused[step][name], want), (kind, step, name)
    # the short and the long aligner on the shapes both take, after the reuse (rounds 0 and 2: the same labels, all rows)
    for step in (0, 2):
        assert WIDTHS[step] == LONG_SHAPES[step][1] and same_bytes(reused[step]["short"], reused[step]["long"]), (kind, step)
    if kind == "asg":
        # the decode of the same three rows before and after the one-row call
        assert same_bytes(reused[0]["viterbi_long"], reused[2]["viterbi_long"])
        assert all(g is None for g in eng.cur.g)  # forward_only: aligning has allocated no gradient buffers
    else:
        assert eng.cur.labels.cpu().numpy().tobytes() == loss_labels
        assert eng.ctc().cpu().numpy().tobytes() == loss_before and eng.cur.g[-1].cpu().numpy().tobytes() == grad_before
    torch.cuda.synchronize()


@pytest.mark.parametrize("criterion, dtype, want", [("ctc", "bf16", ["ctc"]), ("ctc", "f16x3", ["ctc", "split:ctc"]),
                                                    ("asg", "f16x3", ["asg", "scale:asg", "split:asg"])])
def test_the_criterion_records_its_launches_by_tag(criterion, dtype, want):
    from speechless_amd import launch_list
    case = toy_case(T)
    eng = make_engine(case, dtype) if criterion == "ctc" else toy_engine(case, dtype)
    eng.load_input(case["x"])
    eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
    eng.forward()
    eng._rec = launch_list.Recorder(eng.lib.last_error)
    try:
        eng.ctc() if criterion == "ctc" else eng.asg()
        recorded = launch_list.entry_points(eng._rec)
    finally:
        eng._rec = None
    if eng.g_scale == 1:  # (the table gradients are rescaled only where the planes carry a scale)
        want = [tag for tag in want if tag != "scale:asg"]
    assert [tag for _, tag in recorded] == want
    assert [name for name, _ in recorded][0] == ("sl_ctc_loss_grad" if criterion == "ctc" else "sl_asg_loss_grad")
