"""ASG forced alignment on the GPU: sl_asg_align bit-identical (path and score) to the float32 restatement of
tests/test_asg_align.py at the lane / register / LDS seams, with -inf scores and ties, against the full-graph Viterbi, and
through Engine.asg_align and Wav2Letter.asg_alignment_batch / asg_positional_label_batch."""
import numpy as np
import pytest

from test_asg import asg_viterbi
from test_asg_align import F32, NEG_INF, asg_align_reference, random_inputs
from test_gpu_asg import K_ASG, asg_net, examples, toy_case, toy_engine
from test_gpu_ctc_align import lds_limit

pytestmark = pytest.mark.gpu

SL_ERR_UNSUPPORTED = -2
SENTINEL = 7


def run_align_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=None):
    """One sl_asg_align launch on sentinel-filled outputs.  Returns (status, paths, scores, workspace bytes) as numpy."""
    import torch
    b, t, k = logq.shape
    dev = "cuda:0"
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, max(l_max, 1)), dtype=np.int32)
    for i, l in enumerate(labels_list):
        labels[i, :len(l)] = l
    tensors = [torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev) for x in (logq, trans, init)]
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor(label_len, dtype=torch.int32, device=dev)
    il = torch.tensor(input_len, dtype=torch.int32, device=dev)
    path = torch.full((b, t), SENTINEL, dtype=torch.int32, device=dev)
    score = torch.full((b,), float(SENTINEL), dtype=torch.float32, device=dev)
    need = hip_lib.raw("sl_asg_align_workspace_bytes")(b, t, l_max)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    rc = hip_lib.raw("sl_asg_align")(tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), lab.data_ptr(),
                                     ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(), b, t, k, l_max,
                                     ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, path.cpu().numpy(), score.cpu().numpy(), need


def check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores, l_max=None):
    """path and score of every row bit-identical to the restatement (labels padded to l_max, as the kernel sees them)"""
    l_max = max([len(l) for l in labels_list] + [1]) if l_max is None else l_max
    refs = []
    for i, label in enumerate(labels_list):
        padded = list(label) + [0] * (l_max - len(label))
        ref_score, ref_path = asg_align_reference(logq[i], trans, init, padded, label_len[i], input_len[i])
        assert np.array_equal(paths[i], ref_path), (i, label_len[i], input_len[i], np.flatnonzero(paths[i] != ref_path)[:5])
        assert F32(scores[i]).tobytes() == F32(ref_score).tobytes(), (i, scores[i], ref_score)
        refs.append((ref_score, ref_path))
    assert not np.isnan(scores).any()
    return refs


def align_and_check(hip_lib, rng, k, t, label_len, input_len, l_max=None, expect_workspace=None):
    logq, trans, init = random_inputs(rng, t, k, batch=len(label_len))
    width = max(label_len) if l_max is None else l_max
    labels_list = [[int(c) for c in rng.randint(0, k, size=width)] for _ in label_len]
    rc, paths, scores, need = run_align_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len, l_max=l_max)
    assert rc == 0, hip_lib.last_error()
    if expect_workspace is not None:
        assert (need > 0) == expect_workspace
    return check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores, l_max=l_max), paths, scores


def test_smallest_shapes_a_single_path_and_a_single_state(hip_lib):
    rng = np.random.RandomState(1)
    refs, paths, _ = align_and_check(hip_lib, rng, 2, 1, [1], [1])
    assert list(paths[0]) == [0] and np.isfinite(refs[0][0])
    refs, paths, _ = align_and_check(hip_lib, rng, 5, 9, [9], [9])  # L = T: zero slack, the diagonal
    assert list(paths[0]) == list(range(9))
    refs, paths, _ = align_and_check(hip_lib, rng, 5, 300, [1], [300])
    assert (paths[0] == 0).all()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 256, 257, 511])
def test_lane_and_register_seams(hip_lib, n):
    """1 / 2 / 4 / 8 states per lane on either side of where the count changes, and the longest label; 64 letters; ragged
    lengths inside the batch"""
    t = 520 if n == 511 else n + 5
    refs, paths, _ = align_and_check(hip_lib, np.random.RandomState(n), 64, t, [n, max(1, n - 7), n // 2], [t, t - 2, t - 4],
                                     expect_workspace=False)
    for (score, path), rows, frames in zip(refs, [n, max(1, n - 7), n // 2], [t, t - 2, t - 4]):
        assert np.isfinite(score) and path[0] == 0 and path[frames - 1] == rows - 1 and (path[frames:] == -1).all()


def test_lengths_beyond_the_tensors_are_clamped(hip_lib):
    rng = np.random.RandomState(3)
    k, t, l_max = 6, 20, 8
    logq, trans, init = random_inputs(rng, t, k, batch=3)
    labels_list = [[int(c) for c in rng.randint(0, k, size=l_max)] for _ in range(3)]
    labels_list[2][1], labels_list[2][4] = -3, k + 9  # label values clamp to [0, k)
    _, paths, scores, _ = run_align_kernel(hip_lib, logq, trans, init, labels_list, [5, l_max + 4, 6], [t + 9, t, t - 1], l_max)
    check_bits(logq, trans, init, labels_list, [5, l_max + 4, 6], [t + 9, t, t - 1], paths, scores, l_max)
    clamped = [list(l) for l in labels_list]
    clamped[2][1], clamped[2][4] = 0, k - 1
    _, paths2, scores2, _ = run_align_kernel(hip_lib, logq, trans, init, clamped, [5, l_max, 6], [t, t, t - 1], l_max)
    assert np.array_equal(paths, paths2) and scores.tobytes() == scores2.tobytes()
    assert np.isfinite(scores).all() and paths[1][t - 1] == l_max - 1


def test_backpointers_on_either_side_of_the_lds_limit(hip_lib):
    """The smallest t_out whose backpointers (one bit per state and frame, 16 states: 8 bytes per frame) leave LDS, and the
    frame count below it, so t_out itself reaches the HBM side."""
    query = hip_lib.raw("sl_asg_align_workspace_bytes")
    lo, hi = lds_limit(query, 2, 16)  # (the limit lies below 20 000 frames)
    assert query(2, hi, 16) == 2 * hi * 8
    for t, in_hbm in ((lo, False), (hi, True)):
        refs, _, _ = align_and_check(hip_lib, np.random.RandomState(t), 30, t, [16, 11], [t, t // 2 + 1], l_max=16,
                                     expect_workspace=in_hbm)
        assert all(np.isfinite(score) for score, _ in refs)
    # rows of eight words (8 states per lane) from HBM: 39 backtrace windows, and 5 with a partial last one
    t = 2470
    assert query(2, 2400, 257) == 0 and query(2, t, 257) == 2 * t * 64
    align_and_check(hip_lib, np.random.RandomState(9), 30, t, [257, 40], [t, 300], l_max=257, expect_workspace=True)


@pytest.mark.parametrize("l_max,ns", [(128, 2), (256, 4)])
def test_two_and_four_states_per_lane_with_backpointers_in_hbm(hip_lib, l_max, ns):
    """asg_align_kernel<2, false> and <4, false>, which the test above leaves out: the l_max ARGUMENT picks the states per lane
    and the first t_out past the LDS limit (9953 / 4961 frames, taken from the query) sends the rows of ns words to HBM.  The
    longest label over all frames beside a short row with few windows."""
    query = hip_lib.raw("sl_asg_align_workspace_bytes")
    _, t = lds_limit(query, 2, l_max)
    assert query(2, t, l_max) == 2 * t * 8 * ns
    refs, _, _ = align_and_check(hip_lib, np.random.RandomState(l_max), 30, t, [l_max, l_max // 3], [t, t // 16 + 1],
                                 l_max=l_max, expect_workspace=True)
    assert all(np.isfinite(score) for score, _ in refs)


def test_minus_infinity_scores_close_paths_without_a_nan(hip_lib):
    rng = np.random.RandomState(12)
    k, t, b, n = 8, 12, 16, 6
    logq, trans, init = random_inputs(rng, t, k, batch=b)
    trans[rng.rand(k, k) < 0.12] = NEG_INF
    init[rng.rand(k) < 0.25] = NEG_INF
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for _ in range(b)]
    label_len = [int(rng.randint(1, n + 1)) for _ in range(b)]
    input_len = [int(rng.randint(n, t + 1)) for _ in range(b)]
    rc, paths, scores, _ = run_align_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len)
    assert rc == 0
    refs = check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores)
    feasible = np.array([np.isfinite(score) for score, _ in refs])
    assert feasible.any() and not feasible.all()  # (a condition on the seed: both kinds in one batch)
    assert (scores[~feasible] == -np.inf).all() and (paths[~feasible] == -1).all()
    assert np.isfinite(scores[feasible]).all() and not np.isnan(scores).any()


def test_all_equal_inputs_take_the_tie_path(hip_lib):
    zeros = np.zeros((2, 5, 3), dtype=F32)
    rc, paths, scores, _ = run_align_kernel(hip_lib, zeros, np.zeros((3, 3)), np.zeros(3), [[0, 1, 2], [1, 1, 0]], [3, 2], [5, 4])
    assert rc == 0 and list(paths[0]) == [0, 1, 2, 2, 2] and list(paths[1]) == [0, 1, 1, 1, -1] and (scores == 0).all()
    # constant rows that are not zero, more than one state per lane, labels with equal neighbours
    rng = np.random.RandomState(6)
    k, t = 30, 200
    logq = np.full((3, t, k), np.log(F32(1.0 / k)), dtype=F32)
    trans, init = np.full((k, k), F32(-0.25)), np.full(k, F32(0.5))
    labels_list = [[int(c) for c in rng.randint(0, 3, size=150)] for _ in range(3)]
    rc, paths, scores, _ = run_align_kernel(hip_lib, logq, trans, init, labels_list, [150, 70, 1], [t, 150, 33])
    assert rc == 0
    check_bits(logq, trans, init, labels_list, [150, 70, 1], [t, 150, 33], paths, scores)


def test_unsupported_shapes_are_refused_and_nothing_is_written(hip_lib):
    for k, l_max in ((1, 4), (65, 4), (30, 0), (30, 512)):
        logq = np.zeros((1, 6, k), dtype=F32)
        rc, paths, scores, need = run_align_kernel(hip_lib, logq, np.zeros((k, k)), np.zeros(k), [[0]], [1], [6], l_max=l_max)
        assert rc == SL_ERR_UNSUPPORTED, (k, l_max, hip_lib.last_error())
        assert (paths == SENTINEL).all() and (scores == SENTINEL).all()
    query = hip_lib.raw("sl_asg_align_workspace_bytes")
    assert query(1, 6, 0) == 0 and query(1, 6, 512) == 0 and query(4, 100000, 511) == 4 * 100000 * 64


def tied_decisions(e, g, g0, path):
    """along `path` through the full graph (float32, sl_asg_viterbi's operations): how many of its decisions -- the end state
    and every predecessor -- had a second candidate of exactly the same value"""
    e, g, g0 = (np.asarray(x, dtype=F32) for x in (e, g, g0))
    vs = [g0 + e[0]]
    for t in range(1, len(path)):
        vs.append((vs[-1][:, None] + g).max(0) + e[t])
    ties = int(np.sum(vs[-1] == vs[-1][path[-1]]) - 1)
    for t in range(len(path) - 1, 0, -1):
        cand = vs[t - 1] + g[:, path[t]]
        assert cand[path[t - 1]] == cand.max()
        ties += int(np.sum(cand == cand.max()) - 1)
    return ties


def test_aligning_the_full_graph_decode_gives_its_path_and_score(hip_lib):
    """The label of the best path through the full graph, aligned: the constrained lattice holds that very path with the same
    operations along it, so the scores are the same bits, and where no decision of the decode was a tie, the same letters."""
    from test_gpu_asg import run_viterbi_kernel
    rng = np.random.RandomState(21)
    k, t, b = 30, 60, 4
    logq, trans, init = random_inputs(rng, t, k, batch=b)
    trans[np.arange(k), np.arange(k)] += F32(2)  # (staying pays: the decoded labels are shorter than the frames)
    input_len = [t, t - 7, 33, 1]
    vit_paths, vit_scores, _ = run_viterbi_kernel(hip_lib, logq, trans, init, input_len)
    labels_list = []
    for i, t_b in enumerate(input_len):
        ref_score, ref_path = asg_viterbi(logq[i], trans, init, t_b)
        assert np.array_equal(vit_paths[i], ref_path) and F32(vit_scores[i]).tobytes() == F32(ref_score).tobytes()
        assert tied_decisions(logq[i], trans, init, ref_path[:t_b]) == 0  # (a condition on the seed, checked for every row)
        row = vit_paths[i][:t_b]
        labels_list.append([int(c) for j, c in enumerate(row) if j == 0 or c != row[j - 1]])
    label_len = [len(l) for l in labels_list]
    assert max(label_len) > 8
    rc, paths, scores, _ = run_align_kernel(hip_lib, logq, trans, init, labels_list, label_len, input_len)
    assert rc == 0
    check_bits(logq, trans, init, labels_list, label_len, input_len, paths, scores)
    assert scores.tobytes() == vit_scores.tobytes()
    for i, t_b in enumerate(input_len):
        assert np.array_equal(np.asarray(labels_list[i])[paths[i][:t_b]], vit_paths[i][:t_b])
        assert (paths[i][t_b:] == -1).all()


# ------------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("dtype,forward_only", [("f32", False), ("f16x3", True)])
def test_engine_asg_align_on_its_own_emissions_leaves_the_loss_labels_alone(dtype, forward_only):
    """A training engine in fp32 and the default evaluation engine (f16x3, forward only): the restatement on the engine's own
    logq and tables, no gradient buffers from the alignment, and asg() before and after gives the same bits."""
    import torch
    case = toy_case(64)
    eng = toy_engine(case, dtype, forward_only=forward_only)
    lab_len, pred_len = np.array(case["label_lengths"]), np.array(case["prediction_lengths"])
    rng = np.random.RandomState(2)
    other_len = np.array([7, 1, 12])
    other = rng.randint(0, K_ASG, size=(3, 12)).astype(np.int32)
    other[0, :7] = [K_ASG - 1, 3, K_ASG - 2, 3, 3, 0, K_ASG - 1]  # the repeat marks are ordinary labels here
    eng.load_input(case["x"])
    eng.forward()
    first_paths, first_scores = eng.asg_align(other, other_len, pred_len)
    assert all(g is None for g in eng.cur.g)  # (the alignment needs no gradient buffers; set_labels allocates them)
    eng.set_labels(case["labels"], lab_len, pred_len)
    before = eng.asg().cpu().numpy().copy()
    paths, scores = eng.asg_align(other, other_len.reshape(3, 1), pred_len)
    assert np.array_equal(paths, first_paths) and scores.tobytes() == first_scores.tobytes()
    assert paths.dtype == np.int32 and paths.shape == (3, eng.cur.t_out) and scores.dtype == np.float32
    logq = eng.cur.logq.cpu().numpy()
    trans, init = eng.asg_trans.cpu().numpy(), eng.asg_init.cpu().numpy()
    assert np.array_equal(trans, case["g"]) and np.array_equal(init, case["g0"])
    check_bits(logq, trans, init, [list(r) for r in other], list(other_len), list(pred_len), paths, scores, l_max=12)
    assert np.isfinite(scores).all()
    after = eng.asg().cpu().numpy()
    torch.cuda.synchronize()
    assert before.tobytes() == after.tobytes() and np.isfinite(before).all()
    with pytest.raises(ValueError, match="outside"):
        eng.asg_align(np.full((3, 2), K_ASG), [2, 2, 2], pred_len)
    with pytest.raises(ValueError, match="label batch"):
        eng.asg_align(other[:2], other_len[:2], pred_len)


def test_ctc_engine_refuses_asg_align():
    from test_gpu_parity import make_engine
    case = toy_case(64)
    eng = make_engine(case, "f32")
    with pytest.raises(ValueError, match="criterion='asg'"):
        eng.asg_align(case["labels"], case["label_lengths"], case["prediction_lengths"])


# ---------------------------------------------------------------------------------------------------------------- API
def test_api_alignments_tile_the_frames_and_time_the_words():
    from speechless_amd import AsgAlignment
    net = asg_net()
    rng = np.random.RandomState(3)
    net.engine.set_asg_scores(rng.uniform(-1, 1, size=(30, 30)), rng.uniform(-1, 1, size=30))
    batch = examples(["hello there", "a zoo"], frames=(80, 64))
    alignments = net.asg_alignment_batch(batch)
    engine = net.eval_engine
    logq = engine.cur.logq.cpu().numpy()
    state = engine.get_asg_state()
    enc = net.grapheme_encoding
    ratio = net.input_to_prediction_length_ratio
    for x, a, lq in zip(batch, alignments, logq):
        encoded = enc.encode(x.label)
        t_b = x.z_normalized_transposed_spectrogram().shape[0] // ratio
        ref_score, ref_path = asg_align_reference(lq, state["trans"], state["init"], encoded, len(encoded), t_b)
        assert isinstance(a, AsgAlignment) and a.feasible and a.label == x.label and a.encoded_label == encoded
        assert F32(a.log_probability).tobytes() == F32(ref_score).tobytes()
        assert np.array_equal(a.frame_grapheme_positions, ref_path)
        assert a.grapheme_frames[0][0] == 0 and a.grapheme_frames[-1][1] == t_b and len(a.grapheme_frames) == len(encoded)
        assert all(p[1] == q[0] and p[0] < p[1] for p, q in zip(a.grapheme_frames[:-1], a.grapheme_frames[1:]))
        assert len(a.character_frames) == len(x.label) and [w for w, _ in a.word_frames] == x.label.split()
    hello = alignments[0]
    assert hello.encoded_label[3] == enc.asg_twice and len(hello.encoded_label) == len("hello there")
    assert hello.character_frames[2] == hello.grapheme_frames[2] and hello.character_frames[3] == hello.grapheme_frames[3]
    assert hello.character_frames[4] == hello.grapheme_frames[4]
    for seconds in (0.008, 0.02):  # seconds_per_input_step is honoured
        labels = net.asg_positional_label_batch(batch, seconds_per_input_step=seconds)
        for a, pl in zip(alignments, labels):
            assert pl.labels == [w for w, _ in a.word_frames]
            for (_, (start, end)), (_, (first, last)) in zip(pl.labeled_sections, a.word_frames):
                assert start == first * (ratio * seconds) and end == last * (ratio * seconds)
    with pytest.raises(ValueError, match="seconds_per_input_step"):  # (spectrograms carry no sample rate to go by)
        net.asg_positional_label_batch(batch)
    with pytest.raises(ValueError, match="forced alignment"):  # the CTC entry points keep refusing an ASG net
        net.alignment_batch(batch)


def test_api_refuses_asg_alignment_on_a_ctc_net():
    from speechless_amd.grapheme_encoding import english_frequent_characters
    from speechless_amd.net import Wav2Letter
    from test_gpu_asg import SMALL
    net = Wav2Letter(128, english_frequent_characters, layer_sizes=SMALL, seed=4)
    batch = examples(["ab", "c"])
    with pytest.raises(ValueError, match="criterion='asg'"):
        net.asg_alignment_batch(batch)
    with pytest.raises(ValueError, match="criterion='asg'"):
        net.asg_positional_label_batch(batch, seconds_per_input_step=0.01)
