"""sl_asg_align_long on the GPU: score bits and path bytes of EVERY row of every launch equal to the float32 restatement
(tests/asg_align_long_ref.py) at every instantiation its dispatcher can choose, at the wave seams, on hand-built rows, and equal
to sl_asg_align's where both accept the shape; the host-side refusals write nothing."""
import numpy as np
import pytest

from asg_align_long_ref import asg_align_long_reference
from test_asg_align import F32, NEG_INF, random_inputs

pytestmark = pytest.mark.gpu

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED, SL_ERR_WORKSPACE_TOO_SMALL = -1, -2, -3
SENTINEL = 7
STATES_PER_WAVE = 512  # 8 states per lane

# The dispatcher's table (include/speechless_hip.h, sl_asg_align_long; csrc/asg_align_long.hip: waves_for): waves of the
# work-group -> label lengths l_max it serves.  A backpointer row is 64 bytes per wave.
INSTANTIATIONS = {1: (1, 512), 2: (513, 1024), 4: (1025, 2048), 8: (2049, 4096), 16: (4097, 8191)}

# waves -> the launches that reach the instantiation: (l_max of the launch, [(L, slack)]), T_b = L + slack.  Each instantiation
# is launched at the lower and at the upper bound of its l_max range, with every slack of {0, 1, 64, L // 4} (slack 0 is the
# diagonal: every lane and wave boundary is crossed on consecutive frames); the lengths 1, 511, 512, 513, 2048 and 8191 are there.
LAUNCHES = {
    1: [(1, [(1, 0), (1, 1), (1, 64), (1, 1 // 4)]),
        (512, [(512, 0), (511, 1), (512, 64), (512, 512 // 4), (511, 0), (300, 300 // 4), (1, 64)])],
    2: [(513, [(513, 0), (513, 1), (513, 64), (513, 513 // 4)]),
        (1024, [(1024, 0), (1024, 1), (700, 64), (1024, 1024 // 4)])],
    4: [(1025, [(1025, 0), (1025, 1), (1025, 64), (1025, 1025 // 4)]),
        (2048, [(2048, 0), (2048, 1), (1500, 64), (2048, 2048 // 4)])],
    8: [(2049, [(2049, 0), (2049, 1), (2049, 64), (2049, 2049 // 4)]),
        (4096, [(4096, 0), (3000, 1), (4096, 64), (4096, 4096 // 4)])],
    16: [(4097, [(4097, 0), (4097, 1), (4097, 64), (4097, 4097 // 4)]),
         (8191, [(8191, 0), (8191, 1), (5000, 64), (8191, 8191 // 4)])],
}


def run_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=None, name="sl_asg_align_long",
               null=None, short_workspace=False):
    """One launch of `name` on sentinel-filled outputs.  null: the name of one pointer argument passed as NULL;
    short_workspace: one byte less than asked for is declared.  Returns (status, paths, scores, workspace bytes) as numpy."""
    import torch
    b, t, k = logq.shape
    dev = "cuda:0"
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, max(l_max, 1)), dtype=np.int32)
    for i, l in enumerate(labels_list):
        labels[i, :len(l)] = l
    dense = [torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev) for x in (logq, trans, init)]
    path = torch.full((b, t), SENTINEL, dtype=torch.int32, device=dev)
    score = torch.full((b,), float(SENTINEL), dtype=torch.float32, device=dev)
    need = hip_lib.raw(name + "_workspace_bytes")(b, t, l_max)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    args = {"logq": dense[0], "trans": dense[1], "init": dense[2],
            "labels": torch.tensor(labels, dtype=torch.int32, device=dev),
            "label_len": torch.tensor(label_len, dtype=torch.int32, device=dev),
            "input_len": torch.tensor(input_len, dtype=torch.int32, device=dev), "path": path, "score": score, "workspace": ws}
    ptr = {key: (None if key == null else value.data_ptr()) for key, value in args.items()}
    rc = hip_lib.raw(name)(ptr["logq"], ptr["trans"], ptr["init"], ptr["labels"], ptr["label_len"], ptr["input_len"],
                           ptr["path"], ptr["score"], b, t, k, l_max, ptr["workspace"], need - 1 if short_workspace else need,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, path.cpu().numpy(), score.cpu().numpy(), need


def check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores, l_max=None):
    """path and score of every row bit-identical to the restatement (labels padded to l_max, as the kernel sees them)"""
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    refs = []
    for i, label in enumerate(labels_list):
        padded = list(label) + [0] * (l_max - len(label))
        ref_score, ref_path = asg_align_long_reference(logq[i], trans, init, padded, label_len[i], input_len[i])
        assert np.array_equal(paths[i], ref_path), (i, label_len[i], input_len[i], np.flatnonzero(paths[i] != ref_path)[:5])
        assert F32(scores[i]).tobytes() == F32(ref_score).tobytes(), (i, scores[i], ref_score)
        refs.append((ref_score, ref_path))
    assert not np.isnan(scores).any()
    return refs


def launch_cases(hip_lib, rng, k, cases, l_max=None, extra_frames=3):
    """cases = [(L, slack)]: random labels and inputs, T_b = L + slack, t_out a few frames beyond the longest row (every row
    ends in a -1 fill).  Every row is feasible; a row without slack is the diagonal."""
    lengths = [n for n, _ in cases]
    input_len = [n + slack for n, slack in cases]
    t = max(input_len) + extra_frames
    logq, trans, init = random_inputs(rng, t, k, batch=len(cases))
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for n in lengths]
    rc, paths, scores, _ = run_kernel(hip_lib, logq, trans, init, labels_list, lengths, input_len, l_max=l_max)
    assert rc == 0, hip_lib.last_error()
    refs = check_bits(logq, trans, init, labels_list, lengths, input_len, paths, scores, l_max=l_max)
    for (n, slack), t_b, (ref_score, _), row in zip(cases, input_len, refs, paths):
        assert np.isfinite(ref_score) and row[0] == 0 and row[t_b - 1] == n - 1 and (row[t_b:] == -1).all()
        if slack == 0:
            assert np.array_equal(row[:t_b], np.arange(n))
    return paths, scores


def test_launch_table_covers_the_dispatcher(hip_lib):
    assert sorted(LAUNCHES) == sorted(INSTANTIATIONS)
    size = hip_lib.raw("sl_asg_align_long_workspace_bytes")
    previous = 0
    for waves, (lo, hi) in sorted(INSTANTIATIONS.items()):
        assert lo == previous + 1 and hi == min(waves * STATES_PER_WAVE, 8191)  # the ranges tile [1, 8191]
        previous = hi
        assert [l_max for l_max, _ in LAUNCHES[waves]] == [lo, hi]
        assert size(1, 1, lo) == 64 * waves == size(1, 1, hi)  # a backpointer row: one bit per state, 64 bytes per wave
        assert all(max(n for n, _ in cases) == l_max for l_max, cases in LAUNCHES[waves])
        slacks = {(slack, n) for _, cases in LAUNCHES[waves] for n, slack in cases}
        assert {0, 1, 64} <= {slack for slack, _ in slacks} and any(slack == n // 4 and n >= 4 for slack, n in slacks)
    lengths = {n for launches in LAUNCHES.values() for _, cases in launches for n, _ in cases}
    assert {1, 511, 512, 513, 2048, 8191} <= lengths
    assert size(1, 1, INSTANTIATIONS[16][1] + 1) == 0 and size(1, 1, 0) == 0 and size(0, 1, 5) == 0 and size(1, 0, 5) == 0
    assert size(3, 1000, 8191) == 3 * 1000 * 1024
    assert all(size(2, t, l) <= size(2, t + 1, l) and size(2, t, l) <= size(2, t, l + 1)  # monotonic in t_out and l_max
               for t in (1, 77) for l in (1, 511, 512, 1024, 2048, 4096, 8190))


@pytest.mark.parametrize("bound", [0, 1], ids=["lower", "upper"])
@pytest.mark.parametrize("waves", sorted(INSTANTIATIONS))
def test_long_align_bit_exact_at_every_instantiation(hip_lib, waves, bound):
    rng = np.random.RandomState(200 + 2 * waves + bound)
    l_max, cases = LAUNCHES[waves][bound]
    launch_cases(hip_lib, rng, 30, cases, l_max=l_max)


@pytest.mark.parametrize("k", [2, 64])
def test_long_align_bit_exact_with_the_fewest_and_the_most_letters(hip_lib, k):
    """k = 64: every lane of a staging wave carries a letter; k = 2: two.  One large row and shorter ones beside it."""
    launch_cases(hip_lib, np.random.RandomState(k), k, [(6000, 6000 // 4), (100, 0), (2049, 1), (1, 5)])


@pytest.mark.parametrize("n", [STATES_PER_WAVE * w + e for w in (1, 2) for e in (-1, 1)])
def test_wave_seams(hip_lib, n):
    """Labels of w S - 1 and w S + 1 states for the S = 512 states of a wave, without slack and with one frame of it: in the
    instantiation that l_max = L picks, and all of them side by side in one that holds the longest."""
    assert n in (511, 513, 1023, 1025)
    launch_cases(hip_lib, np.random.RandomState(n), 30, [(n, 0), (n, 1)], l_max=n)
    if n == 1025:
        launch_cases(hip_lib, np.random.RandomState(n + 1), 30, [(m, slack) for m in (511, 513, 1023, 1025) for slack in (0, 1)])


def test_hand_built_rows(hip_lib):
    k = 30
    rng = np.random.RandomState(4)
    # all labels equal: every stay and every move takes the same score g(7, 7)
    n, t = 3000, 3700
    logq, trans, init = random_inputs(rng, t + 2, k, batch=2)
    equal = [[7] * n, [7] * 600]
    rc, paths, scores, _ = run_kernel(hip_lib, logq, trans, init, equal, [n, 600], [t, 600])
    assert rc == 0 and np.isfinite(scores).all()
    check_bits(logq, trans, init, equal, [n, 600], [t, 600], paths, scores)
    # all inputs equal: the tie rule decides every frame -- a tie stays, so the states are entered as early as possible
    n, t = 3000, 4000
    logq = np.full((2, t + 1, k), np.log(F32(1.0 / k)), dtype=F32)
    zeros, zero = np.zeros((k, k), dtype=F32), np.zeros(k, dtype=F32)
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)], [int(c) for c in rng.randint(0, 3, size=1000)]]
    rc, paths, scores, _ = run_kernel(hip_lib, logq, zeros, zero, labels_list, [n, 1000], [t, 1000 + 513])
    assert rc == 0
    check_bits(logq, zeros, zero, labels_list, [n, 1000], [t, 1000 + 513], paths, scores)
    assert np.array_equal(paths[0][:t], np.minimum(np.arange(t), n - 1)) and paths[0][t] == -1
    assert np.array_equal(paths[1][:1513], np.minimum(np.arange(1513), 999)) and (paths[1][1513:] == -1).all()


def test_minus_infinity_scores_close_all_paths_but_one_and_all_of_them(hip_lib):
    """No letter may stay (g(c, c) = -inf) but one, which the label holds once at position p: the only open path waits there
    for all the spare frames.  Without that letter's stay no path is open: the row is infeasible, and no NaN appears."""
    k, n, p, slack = 30, 2500, 1300, 300
    rng = np.random.RandomState(31)
    t = n + slack
    logq, trans, init = random_inputs(rng, t + 3, k, batch=3)
    trans[np.arange(k - 1), np.arange(k - 1)] = NEG_INF  # letter k - 1 alone may stay
    label = [i % (k - 1) for i in range(n)]  # neighbours differ: every move is open
    label[p] = k - 1
    labels_list = [label, label, label[:700]]
    label_len, input_len = [n, n, 700], [t, n, 700]  # (rows 1 and 2: the diagonal never stays, so it is open)
    rc, paths, scores, _ = run_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len)
    assert rc == 0 and np.isfinite(scores).all()
    check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores)
    only = np.concatenate([np.arange(p), np.full(slack + 1, p), np.arange(p + 1, n)])
    assert np.array_equal(paths[0][:t], only) and np.array_equal(paths[1][:n], np.arange(n))
    closed = trans.copy()
    closed[k - 1, k - 1] = NEG_INF  # now nobody stays: a row with spare frames has no path
    shut = init.copy()
    shut[label[0]] = NEG_INF  # and a start score closes the diagonal, too
    for g, g0, feasible in ((closed, init, [False, True, True]), (trans, shut, [False, False, False])):
        rc, paths, scores, _ = run_kernel(hip_lib, logq, g, g0, labels_list, label_len, input_len)
        assert rc == 0 and not np.isnan(scores).any()
        check_bits(logq, g, g0, labels_list, label_len, input_len, paths, scores)
        for ok, row, value in zip(feasible, paths, scores):
            assert np.isfinite(value) if ok else (value == -np.inf and (row == -1).all())


def test_mixed_launch(hip_lib):
    """One launch: 8000 graphemes, an empty label, no frames for a label, more graphemes than frames, an input length beyond
    t_out, and label values outside [0, k)."""
    k = 30
    rng = np.random.RandomState(8000)
    t = 8000 + 64
    logq, trans, init = random_inputs(rng, t, k, batch=6)
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for n in (8000, 40, 5, 50, 60, 70)]
    labels_list[5][0], labels_list[5][33], labels_list[5][69] = -4, k, k + 100  # clamped to 0, k - 1, k - 1
    label_len = [8000, 0, 5, 50, 60, 70]
    input_len = [t, 100, 0, 49, t + 1000, 300]  # (row 4: clamped to t_out)
    rc, paths, scores, _ = run_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len)
    assert rc == 0, hip_lib.last_error()
    check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores)
    assert np.isfinite(scores[[0, 4, 5]]).all() and (scores[[1, 2, 3]] == -np.inf).all() and (paths[[1, 2, 3]] == -1).all()
    assert paths[0][t - 1] == 7999 and paths[4][t - 1] == 59 and (paths[4] >= 0).all() and (paths[5][300:] == -1).all()
    clamped = [list(l) for l in labels_list]
    clamped[5][0], clamped[5][33], clamped[5][69] = 0, k - 1, k - 1
    rc, paths2, scores2, _ = run_kernel(hip_lib, logq, trans, init, clamped, label_len, [t, 100, 0, 49, t, 300])
    assert rc == 0 and paths2.tobytes() == paths.tobytes() and scores2.tobytes() == scores.tobytes()


def both_kernels(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=None):
    rc, paths, scores, _ = run_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=l_max)
    rc1, paths1, scores1, need1 = run_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=l_max,
                                             name="sl_asg_align")
    assert rc == 0 and rc1 == 0, hip_lib.last_error()
    assert paths.tobytes() == paths1.tobytes() and scores.tobytes() == scores1.tobytes()
    check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores, l_max=l_max)
    return need1


def test_agrees_with_the_one_wave_kernel(hip_lib):
    """The shapes of tests/test_gpu_asg_align.py (l_max <= 511): both kernels return the same bytes."""
    # its lane and register seams, 64 letters, ragged lengths inside the batch
    for n in (63, 64, 65, 128, 129, 256, 257, 511):
        t = 520 if n == 511 else n + 5
        rng = np.random.RandomState(n)
        logq, trans, init = random_inputs(rng, t, 64, batch=3)
        label_len = [n, max(1, n - 7), n // 2]
        labels_list = [[int(c) for c in rng.randint(0, 64, size=n)] for _ in label_len]
        assert both_kernels(hip_lib, logq, trans, init, labels_list, label_len, [t, t - 2, t - 4]) == 0
    # its smallest shapes, clamped lengths and label values
    rng = np.random.RandomState(3)
    logq, trans, init = random_inputs(rng, 1, 2, batch=1)
    both_kernels(hip_lib, logq, trans, init, [[1]], [1], [1])
    k, t, l_max = 6, 20, 8
    logq, trans, init = random_inputs(rng, t, k, batch=3)
    labels_list = [[int(c) for c in rng.randint(0, k, size=l_max)] for _ in range(3)]
    labels_list[2][1], labels_list[2][4] = -3, k + 9
    both_kernels(hip_lib, logq, trans, init, labels_list, [5, l_max + 4, 6], [t + 9, t, t - 1], l_max=l_max)
    # its -inf scores: feasible and infeasible rows in one batch
    k, t, b, n = 8, 12, 16, 6
    rng = np.random.RandomState(12)
    logq, trans, init = random_inputs(rng, t, k, batch=b)
    trans[rng.rand(k, k) < 0.12] = NEG_INF
    init[rng.rand(k) < 0.25] = NEG_INF
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for _ in range(b)]
    both_kernels(hip_lib, logq, trans, init, labels_list, [int(rng.randint(1, n + 1)) for _ in range(b)],
                 [int(rng.randint(n, t + 1)) for _ in range(b)])
    # its ties: constant rows, labels with equal neighbours
    rng = np.random.RandomState(6)
    k, t = 30, 200
    logq = np.full((3, t, k), np.log(F32(1.0 / k)), dtype=F32)
    labels_list = [[int(c) for c in rng.randint(0, 3, size=150)] for _ in range(3)]
    both_kernels(hip_lib, logq, np.full((k, k), F32(-0.25)), np.full(k, F32(0.5)), labels_list, [150, 70, 1], [t, 150, 33])


def test_agrees_with_the_one_wave_kernel_on_both_sides_of_its_lds_limit(hip_lib):
    """The smallest t_out whose backpointers leave sl_asg_align's LDS and the frame count below it (16 states), and rows of
    eight words from HBM: the long kernel, whose rows always go to HBM, returns the same bytes."""
    query = hip_lib.raw("sl_asg_align_workspace_bytes")
    lo, hi = 1, 20000
    assert query(2, lo, 16) == 0 and query(2, hi, 16) > 0
    while hi - lo > 1:  # (monotonic in t_out)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if query(2, mid, 16) == 0 else (lo, mid)
    for t, l_max, label_len, input_len, in_hbm in ((lo, 16, [16, 11], [lo, lo // 2 + 1], False),
                                                   (hi, 16, [16, 11], [hi, hi // 2 + 1], True),
                                                   (2470, 257, [257, 40], [2470, 300], True)):
        rng = np.random.RandomState(t)
        logq, trans, init = random_inputs(rng, t, 30, batch=2)
        labels_list = [[int(c) for c in rng.randint(0, 30, size=l_max)] for _ in range(2)]
        need1 = both_kernels(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=l_max)
        assert (need1 > 0) == in_hbm


def test_refusals_are_made_on_the_host_and_write_nothing(hip_lib):
    def refused(k, l_max, want, **kw):
        logq = np.zeros((1, 6, k), dtype=F32)
        rc, paths, scores, _ = run_kernel(hip_lib, logq, np.zeros((k, k)), np.zeros(k), [[0]], [1], [6], l_max=l_max, **kw)
        assert rc == want, (k, l_max, kw, rc, hip_lib.last_error())
        assert (paths == SENTINEL).all() and (scores == SENTINEL).all()
    for k, l_max in ((30, 0), (30, 8192), (1, 4), (65, 4)):
        refused(k, l_max, SL_ERR_UNSUPPORTED)
    for name in ("logq", "trans", "init", "labels", "label_len", "input_len", "path", "score", "workspace"):
        refused(30, 4, SL_ERR_INVALID_ARGUMENT, null=name)
    refused(30, 4, SL_ERR_WORKSPACE_TOO_SMALL, short_workspace=True)
    refused(30, 8191, SL_ERR_WORKSPACE_TOO_SMALL, short_workspace=True)
    logq = np.zeros((1, 6, 30), dtype=F32)  # and the same arguments, none of them wrong, are served
    rc, paths, scores, need = run_kernel(hip_lib, logq, np.zeros((30, 30)), np.zeros(30), [[0]], [1], [6], l_max=4)
    assert rc == 0 and need == 6 * 64 and (paths == 0).all() and scores[0] == 0
