"""sl_ctc_align_long on the GPU: score and path bytes equal to the float32 restatement (tests/test_ctc_align.py: viterbi) at
every instantiation its dispatcher can choose, on hand-built labels, and equal to sl_ctc_align's where both accept the shape."""
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_ctc_align import FUZZ_KINDS, FUZZ_SHAPES, check_against_restatement, fuzz_case, run_align_kernel

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

# The dispatcher's table (csrc/ctc_align_long.hip: waves_for): waves of the work-group -> label lengths l_max it serves.
# 16 states per lane, 1024 per wave; S = 2 l_max + 1 states.
INSTANTIATIONS = {1: (0, 511), 2: (512, 1023), 4: (1024, 2047), 8: (2048, 4095), 16: (4096, 8191)}


def run_long_kernel(hip_lib, logits, labels_list, input_len, eps=1e-8, l_max=None, one_wave=False):
    """logq from sl_softmax_logq, then sl_ctc_align_long (and, one_wave=True, sl_ctc_align on the same logq).  Returns
    (logq, paths, scores) as numpy, or (logq, paths, scores, one-wave paths, one-wave scores)."""
    import torch
    b, t, k = logits.shape
    dev = "cuda:0"
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, l_max), dtype=np.int32)
    for i, l in enumerate(labels_list):
        labels[i, :len(l)] = l
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.zeros((b, t, k), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor([len(l) for l in labels_list], dtype=torch.int32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    results = []
    for name in ("sl_ctc_align_long",) + (("sl_ctc_align",) if one_wave else ()):
        path = torch.full((b, t), 7, dtype=torch.int32, device=dev)
        score = torch.full((b,), 123.0, dtype=torch.float32, device=dev)
        need = hip_lib.raw(name + "_workspace_bytes")(b, t, l_max)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        hip_lib.call(name, logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(),
                     b, t, k, l_max, ws.data_ptr(), need, st)
        torch.cuda.synchronize()
        results += [path.cpu().numpy(), score.cpu().numpy()]
    return (logq.cpu().numpy(),) + tuple(results)


def _repeats(label):
    return sum(1 for i in range(1, len(label)) if label[i] == label[i - 1])


def _regime_launch(rng, k, cases, extra_frames=3):
    """One launch of several recordings: cases = [(L, slack, kind)], T_b = L + repeats + slack (slack 0: the only path is the
    diagonal, every lane and wave boundary is crossed on consecutive frames), logits of tools/fuzz_ctc.regime_logits.  The
    launch has a few frames more than its longest recording, so every row ends in a -1 fill."""
    sys.path.insert(0, str(ROOT / "tools"))
    from fuzz_ctc import regime_logits
    labels_list = [[int(c) for c in rng.randint(0, k - 1, size=n)] for n, _, _ in cases]
    input_len = [len(l) + _repeats(l) + slack for l, (_, slack, _) in zip(labels_list, cases)]
    t = max(input_len) + extra_frames
    logits = np.zeros((len(cases), t, k), dtype=np.float32)
    for i, (_, _, kind) in enumerate(cases):
        if input_len[i]:
            logits[i, :input_len[i]] = regime_logits(rng, labels_list[i], input_len[i], k, kind)
    return logits, labels_list, input_len


# waves -> the launches that reach the instantiation: (l_max of the launch, [(L, slack, kind)]).  Each instantiation is launched
# at the lower and at the upper bound of its l_max range; the lengths 0, 1, 511, 512, 513, 2047, 2048, 8191 are all there, and
# every slack of {0, 1, 64, L // 4} and every kind of {learnt, sharp, uniform} at every instantiation.
LAUNCHES = {
    1: [(0, [(0, 64, "learnt"), (0, 1, "sharp")]),
        (511, [(511, 0, "learnt"), (1, 0, "sharp"), (1, 64, "uniform"), (0, 17, "uniform"), (511, 511 // 4, "sharp"),
               (300, 1, "learnt")])],
    2: [(512, [(512, 0, "sharp"), (512, 64, "learnt")]),
        (1023, [(1023, 0, "learnt"), (513, 1, "uniform"), (513, 513 // 4, "sharp"), (700, 64, "learnt")])],
    4: [(1024, [(1024, 0, "learnt"), (1024, 1024 // 4, "uniform")]),
        (2047, [(2047, 0, "sharp"), (2047, 1, "learnt"), (1500, 64, "uniform")])],
    8: [(2048, [(2048, 0, "uniform"), (2048, 64, "sharp")]),
        (4095, [(4095, 0, "learnt"), (3000, 1, "sharp"), (2500, 2500 // 4, "learnt")])],
    16: [(4096, [(4096, 1, "uniform"), (4096, 4096 // 4, "sharp")]),
         (8191, [(8191, 0, "learnt"), (1200, 64, "sharp")])],
}


def test_launch_table_covers_the_dispatcher(hip_lib):
    assert sorted(LAUNCHES) == sorted(INSTANTIATIONS)
    size = hip_lib.raw("sl_ctc_align_long_workspace_bytes")
    for waves, (lo, hi) in INSTANTIATIONS.items():
        assert [l_max for l_max, _ in LAUNCHES[waves]] == [lo, hi]
        assert size(1, 1, lo) == 256 * waves == size(1, 1, hi)  # a backpointer row is 256 bytes per wave
        assert all(max(n for n, _, _ in cases) == l_max for l_max, cases in LAUNCHES[waves])
    assert size(1, 1, INSTANTIATIONS[16][1] + 1) == 0


@pytest.mark.parametrize("bound", [0, 1], ids=["lower", "upper"])
@pytest.mark.parametrize("waves", sorted(INSTANTIATIONS))
def test_long_align_bit_exact_at_every_instantiation(hip_lib, waves, bound):
    rng = np.random.RandomState(100 + 2 * waves + bound)
    k = 29
    l_max, cases = LAUNCHES[waves][bound]
    logits, labels_list, input_len = _regime_launch(rng, k, cases)
    logq, paths, scores = run_long_kernel(hip_lib, logits, labels_list, input_len, l_max=max(l_max, 1))
    assert all(np.isfinite(scores[i]) for i in range(len(cases)))  # (T_b = L + repeats + slack is always feasible)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k, full=l_max <= 1023)


def test_long_align_bit_exact_with_64_classes(hip_lib):
    """k = 64: every lane of a staging wave carries a class.  One large case and short ones beside it."""
    rng = np.random.RandomState(64)
    k = 64
    cases = [(6000, 6000 // 4, "learnt"), (100, 0, "sharp"), (2049, 1, "uniform"), (0, 5, "learnt")]
    logits, labels_list, input_len = _regime_launch(rng, k, cases)
    logq, paths, scores = run_long_kernel(hip_lib, logits, labels_list, input_len)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k, full=False)


def test_long_align_hand_built_labels(hip_lib):
    k, n = 29, 3000
    rng = np.random.RandomState(3)
    # all letters equal: no skip anywhere, a blank between any two, 2 L - 1 frames at least -- feasible with none to spare, and
    # one frame short (score -inf, the whole row -1)
    equal = [7] * n
    t = 2 * n - 1
    logits = rng.randn(2, t, k).astype(np.float32)
    logq, paths, scores = run_long_kernel(hip_lib, logits, [equal, equal], [t, t - 1])
    assert np.isfinite(scores[0]) and np.array_equal(paths[0], np.arange(1, 2 * n))
    assert scores[1] == -np.inf and np.all(paths[1] == -1)
    check_against_restatement(logq, [equal, equal], [t, t - 1], paths, scores, k, full=False)
    # all letters distinct from both neighbours: a skip everywhere
    distinct = [i % (k - 1) for i in range(n)]
    t = n + n // 3
    logits = (3.0 * rng.randn(1, t, k)).astype(np.float32)
    logq, paths, scores = run_long_kernel(hip_lib, logits, [distinct], [t])
    assert np.isfinite(scores[0])
    check_against_restatement(logq, [distinct], [t], paths, scores, k, full=False)


@pytest.mark.parametrize("n", [600, 5000])
def test_long_align_tie_rule_on_constant_rows(hip_lib, n):
    """Every path of a row scores the same up to rounding: the strict-> order stay / s-1 / s-2 decides, bit for bit."""
    k = 29
    rng = np.random.RandomState(n)
    labels_list = [[int(c) for c in rng.randint(0, k - 1, size=m)] for m in (n, n // 2, 3)]
    input_len = [len(l) + _repeats(l) + slack for l, slack in zip(labels_list, (n // 4, 0, 700))]
    logits = np.zeros((3, max(input_len), k), dtype=np.float32)
    logq, paths, scores = run_long_kernel(hip_lib, logits, labels_list, input_len)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k, full=n <= 600)


@pytest.mark.parametrize("k", [29, 64])
def test_long_align_agrees_with_the_one_wave_kernel(hip_lib, k):
    """The fuzz shapes of test_gpu_ctc_align.test_align_kernel_bit_exact_on_fuzz_regimes (l_max <= 511, 300 .. 4000 frames,
    backpointers of the one-wave kernel in LDS and in HBM): both kernels return the same bytes."""
    rng = np.random.RandomState(11 + k)
    for t, b, l_hi, tight in FUZZ_SHAPES:
        logits, labels_list, input_len = fuzz_case(rng, k, t, b, l_hi, FUZZ_KINDS, tight)
        _, paths, scores, paths1, scores1 = run_long_kernel(hip_lib, logits, labels_list, input_len, one_wave=True)
        assert paths.tobytes() == paths1.tobytes() and scores.tobytes() == scores1.tobytes()
    # the infeasible / empty / clamped rows of that test
    t = 40
    labels_list = [[1] * 30, list(range(20)) * 2, [], [], [3, 4], [5, 5, 5]]
    input_len = [40, 39, 17, 0, 0, 60]
    logits = rng.randn(len(labels_list), t, k).astype(np.float32)
    logq, paths, scores, paths1, scores1 = run_long_kernel(hip_lib, logits, labels_list, input_len, one_wave=True)
    assert paths.tobytes() == paths1.tobytes() and scores.tobytes() == scores1.tobytes()
    check_against_restatement(logq, labels_list, input_len, paths, scores, k)
    # and the helper of that module drives the one-wave kernel to the same result
    _, paths2, scores2 = run_align_kernel(hip_lib, logits, labels_list, input_len)
    assert paths2.tobytes() == paths.tobytes() and scores2.tobytes() == scores.tobytes()


def test_long_align_mixed_launch(hip_lib):
    """One launch: a recording of 8000 letters, an empty label, no frames for a label, and an input length beyond t_out."""
    k = 29
    rng = np.random.RandomState(8000)
    cases = [(8000, 64, "learnt"), (0, 100, "sharp"), (5, 40, "learnt"), (50, 300, "uniform")]
    logits, labels_list, input_len = _regime_launch(rng, k, cases, extra_frames=0)
    t = logits.shape[1]
    input_len[2] = 0         # T_b = 0 with L > 0: infeasible
    input_len[3] = t + 1000  # clamped to t_out
    logits[3] = rng.randn(t, k).astype(np.float32)
    logq, paths, scores = run_long_kernel(hip_lib, logits, labels_list, input_len)
    assert np.isfinite(scores[0]) and np.all(paths[0][input_len[0]:] == -1)
    assert np.all(paths[1][:100] == 0) and np.all(paths[1][100:] == -1)
    assert scores[2] == -np.inf and np.all(paths[2] == -1)
    assert np.isfinite(scores[3]) and np.all(paths[3] >= 0)
    check_against_restatement(logq, labels_list, input_len, paths, scores, k, full=False)
