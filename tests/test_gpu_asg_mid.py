"""sl_asg_loss_grad alone (csrc/asg.hip) at the shapes training uses: labels up to the limit of 511 letters, up to 900 frames,
2 .. 64 letters, the five emission regimes, score tables of the size a trained net has (and tables that contradict the label),
every documented call mode, a workspace that is larger than needed and holds what other calls left, and the engine.

Helpers, cases and bounds: tests/asg_cases.py (its module docstring has the bounds and where they come from; the floor of double
arithmetic under them is tests/test_asg_cases.py).  In short -- against the float64 restatement of tests/test_asg.py fed the
kernel's own fp32 probabilities: dlogits within 1e-6 * grad_scale per entry, loss within 1e-6 |ref| + 1e-6, dtrans / dinit within
1e-6 |ref| + 1e-6 * grad_scale, rows at and past T_b exactly zero, an infeasible utterance +inf with no gradient.  No call has
more than 900 frames or 8 utterances.  The worst distance per output and test group goes to test_gpu_parity._report as
asg_mid_* (DESIGN.md section 3.5 has the table).
"""
import numpy as np
import pytest

import asg_cases as ac
from asg_cases import FILL, MAX_FRAMES, build_asg_batch, asg_scores, check_tight, run_asg, same_bytes
from test_gpu_ctc_long import adjacent_repeats

pytestmark = pytest.mark.gpu

SL_ERR_UNSUPPORTED = -2


def report(key, worst):
    from test_gpu_parity import _report
    print(key, worst)
    _report("asg_mid_" + key, worst)


def merge_worst(into, worst):
    for name, value in worst.items():
        into[name] = max(into.get(name, 0.0), value)
    return into


# 1 ------------------------------------------------------------------------------------------ boundaries of every instantiation
@pytest.mark.parametrize("index", range(len(ac.BOUNDARY_LENGTHS)), ids=[str(n) for n in ac.BOUNDARY_LENGTHS])
def test_boundaries_of_every_lattice_instantiation(hip_lib, index):
    """l_max on both sides of 64 / 128 / 256 (1, 2, 4, 8 label states per lane) and at 511, the last state lane 63 can hold;
    three utterances each, with zero slack (T_b = L), one frame and L / 4 frames of slack; the five regimes in turn; K = 29,
    scores from uniform(-2, 2)"""
    n = ac.BOUNDARY_LENGTHS[index]
    rng = np.random.RandomState(700 + n)
    specs = ac.boundary_specs(index)
    logits, labels_list, input_len = build_asg_batch(rng, 29, specs)
    g, g0 = asg_scores(rng, labels_list, 29, "random")
    assert input_len[0] == n and logits.shape[1] <= MAX_FRAMES
    run = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
    report("boundary_l{}".format(n), check_tight(run, g, g0, labels_list, input_len, regimes=[s[2] for s in specs]))


# 2 ------------------------------------------------------------------------------------------ trained and hostile tables
@pytest.mark.parametrize("kind,s", ac.TABLE_SCORES, ids=["{}{}".format(*ks) for ks in ac.TABLE_SCORES])
@pytest.mark.parametrize("k,n", ac.TABLE_SHAPES, ids=["k{}_l{}".format(*kn) for kn in ac.TABLE_SHAPES])
def test_trained_and_hostile_tables(hip_lib, k, n, kind, s):
    """Scores of +-12 and +-30 (exp(g) from 1e-13 to 1e13 in the probability-domain denominator lattices), for the label
    ("bigram") and against it ("hostile"); a learnt alignment without slack, a partly different transcript with 9 frames of
    slack, a sharp and a collapsed distribution on shorter labels; K from 64 (every lane holds a letter) to 3 and 2, the limit
    (there a third and a half of the neighbouring letters are equal)."""
    rng = np.random.RandomState(1000 * k + n + s)
    specs = ac.table_specs(n)
    logits, labels_list, input_len = build_asg_batch(rng, k, specs)
    if k <= 3:
        assert adjacent_repeats(labels_list[0]) > n // 6
    g, g0 = asg_scores(rng, labels_list, k, kind, s)
    run = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
    report("tables_k{}_l{}_{}{}".format(k, n, kind, s), check_tight(run, g, g0, labels_list, input_len, regimes=[x[2] for x in specs]))


# 3 ------------------------------------------------------------------------------------------ frame chunking
def test_every_frame_count_of_the_three_chunkings(hip_lib):
    """CH = 8 frames per emission chunk of the lattices, FR = 8 per LDS chunk of asg_trans_kernel (which starts at frame 1), 4
    frames per work-group of asg_grad_kernel: T_b = L .. L + 17 for L = 5 and L = 300 in batches of six with a common t_out
    above every T_b -- T_b mod 8 and t_out mod 4 take every value -- and L = 1 at T_b = 7, 8, 9."""
    worst = {}
    for j, (specs, t_out) in enumerate(ac.chunk_batches()):
        rng = np.random.RandomState(40 + j)
        k = (29, 64, 5)[j % 3]
        logits, labels_list, input_len = build_asg_batch(rng, k, specs, t_out=t_out)
        kind, s = (("random", None), ("bigram", 12), ("hostile", 30))[j % 3]
        g, g0 = asg_scores(rng, labels_list, k, kind, s)
        print("batch", j, "t_out", t_out, "T_b", input_len, kind)
        run = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
        merge_worst(worst, check_tight(run, g, g0, labels_list, input_len, regimes=[x[2] for x in specs]))
    report("frame_chunking", worst)


# 4 ------------------------------------------------------------------------------------------ mixed batch at 511
def test_mixed_batch_at_511(hip_lib):
    """l_max = 511, bigram scores of 12: a 511-letter label in 511 frames beside L = 0, L = 1, 300 letters with input_len below
    t_out, 400 letters in 380 frames (infeasible) and T_b = 0.  The feasible utterances alone give the same bytes: dtrans,
    dinit, their losses, their dlogits rows."""
    rng = np.random.RandomState(21)
    k = 29
    logits, labels_list, input_len = build_asg_batch(rng, k, ac.MIXED_511_SPECS)
    assert [len(lab) for lab in labels_list] == [511, 0, 1, 300, 400, 3] and input_len == [511, 500, 333, 411, 380, 0]
    assert logits.shape[1] == 512
    g, g0 = asg_scores(rng, labels_list, k, "bigram", 12)
    run = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
    report("mixed_511", check_tight(run, g, g0, labels_list, input_len, regimes=[x[2] for x in ac.MIXED_511_SPECS]))
    keep = list(ac.MIXED_511_FEASIBLE)
    for i in range(6):
        assert np.isfinite(run.loss[i]) == (i in keep)
    alone = run_asg(hip_lib, logits[keep], g, g0, [labels_list[i] for i in keep], [input_len[i] for i in keep])
    assert alone.rc == 0
    assert same_bytes(alone.dg, run.dg) and same_bytes(alone.dg0, run.dg0)
    assert same_bytes(alone.loss, run.loss[keep]) and same_bytes(alone.dl, np.ascontiguousarray(run.dl[keep]))


# 5 ------------------------------------------------------------------------------------------ fuzz stream
@pytest.mark.parametrize("call", range(4))
def test_fuzz_stream_of_32_utterances(hip_lib, call):
    """32 utterances in four calls of eight: 1 .. 511 letters, 0 .. 300 frames of slack, K = 2, 29, 64, every regime, every
    kind of score table, grad_scale = 1 / 32"""
    k, kind, s, specs = ac.fuzz_stream()[call]
    rng = np.random.RandomState(900 + call)
    logits, labels_list, input_len = build_asg_batch(rng, k, specs)
    g, g0 = asg_scores(rng, labels_list, k, kind, s)
    run = run_asg(hip_lib, logits, g, g0, labels_list, input_len, grad_scale=1.0 / 32)
    worst = check_tight(run, g, g0, labels_list, input_len, grad_scale=1.0 / 32, regimes=[x[2] for x in specs])
    report("fuzz_call{}_k{}_{}".format(call, k, kind), worst)


# 6 ------------------------------------------------------------------------------------------ output modes
@pytest.mark.parametrize("name", list(ac.MODE_CASES))
def test_output_modes(hip_lib, name):
    """dlogits = NULL; dtrans = dinit = NULL; all three NULL (a forward_only engine); a bf16 and an fp32 destination with halo 3,
    a row stride wider than K and a padded batch stride (the bf16 engine).  What is computed is the full call's, byte for
    byte; what is not asked for is not written."""
    k, rs, specs = ac.MODE_CASES[name]
    rng = np.random.RandomState(60 + k)
    logits, labels_list, input_len = build_asg_batch(rng, k, specs)
    g, g0 = asg_scores(rng, labels_list, k, "bigram", 12)
    args = (hip_lib, logits, g, g0, labels_list, input_len)
    full = run_asg(*args)
    report("modes_" + name, check_tight(full, g, g0, labels_list, input_len, regimes=[x[2] for x in specs]))
    assert not (full.dl == FILL).any() and not (full.dg == FILL).any() and not (full.dg0 == FILL).any()

    no_dl = run_asg(*args, dlogits=False)
    assert no_dl.rc == 0 and same_bytes(no_dl.loss, full.loss) and same_bytes(no_dl.dg, full.dg) and same_bytes(no_dl.dg0, full.dg0)
    assert (no_dl.dest == FILL).all()
    no_tables = run_asg(*args, tables=False)
    assert no_tables.rc == 0 and same_bytes(no_tables.loss, full.loss) and same_bytes(no_tables.dl, full.dl)
    assert (no_tables.dg == FILL).all() and (no_tables.dg0 == FILL).all()
    loss_only = run_asg(*args, dlogits=False, tables=False)
    assert loss_only.rc == 0 and same_bytes(loss_only.loss, full.loss)
    assert (loss_only.dest == FILL).all() and (loss_only.dg == FILL).all() and (loss_only.dg0 == FILL).all()

    for dest in ("bf16", "f32"):
        placed = run_asg(*args, dest=dest, halo=3, rs=rs, pad=24)
        assert placed.rc == 0 and rs > k
        assert same_bytes(placed.dest, ac.expected_destination(full.dl, placed.geometry, dest == "bf16")), dest
        assert same_bytes(placed.loss, full.loss) and same_bytes(placed.dg, full.dg) and same_bytes(placed.dg0, full.dg0)


# 7 ------------------------------------------------------------------------------------------ determinism, eps, scale
def test_determinism_eps_and_grad_scale(hip_lib):
    rng = np.random.RandomState(77)
    k = 29
    specs = [(300, 0, "wrong"), (280, 30, "uniform"), (5, 100, "learnt"), (60, 4, "collapse")]
    logits, labels_list, input_len = build_asg_batch(rng, k, specs)
    g, g0 = asg_scores(rng, labels_list, k, "bigram", 12)
    first = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
    again = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
    assert first.rc == 0 and all(same_bytes(a, b) for a, b in zip(first.outputs(), again.outputs()))
    worst = check_tight(first, g, g0, labels_list, input_len, regimes=[x[2] for x in specs])
    scaled = run_asg(hip_lib, logits, g, g0, labels_list, input_len, eps=1e-6, grad_scale=1.0 / 7)
    merge_worst(worst, check_tight(scaled, g, g0, labels_list, input_len, eps=1e-6, grad_scale=1.0 / 7, regimes=[x[2] for x in specs]))
    # eps = 0 where no probability underflows: a near-uniform batch, and learnt alignments of strength 8
    for regime, strength in (("uniform", None), ("learnt", 8.0)):
        specs0 = [(300, 0, regime), (129, 17, regime), (1, 40, regime)]
        logits, labels_list, input_len = build_asg_batch(rng, k, specs0, strength=strength)
        g, g0 = asg_scores(rng, labels_list, k, "random")
        run = run_asg(hip_lib, logits, g, g0, labels_list, input_len, eps=0.0)
        assert run.probs.min() > 1e-30
        merge_worst(worst, check_tight(run, g, g0, labels_list, input_len, eps=0.0, regimes=[regime] * 3))
    report("eps_and_scale", worst)


# 8 ------------------------------------------------------------------------------------------ workspace
def test_workspace_size_never_shrinks_with_l_max_and_limits_are_refused(hip_lib):
    size = hip_lib.raw("sl_asg_workspace_bytes")
    for batch, t_out, k in ((1, 40, 2), (4, 700, 29), (8, 900, 64)):
        sizes = [size(batch, t_out, k, l_max) for l_max in range(1, 512)]
        assert sizes[0] > 0 and size(batch, t_out, k, 0) > 0
        drops = [l_max for l_max in range(2, 512) if sizes[l_max - 1] < sizes[l_max - 2]]
        assert not drops, (batch, t_out, k, drops[:5])
        assert size(batch, t_out, k, 512) == 0 and size(batch, t_out, 1, 40) == 0
    logits = np.zeros((1, 6, 2), dtype=np.float32)
    for k, l_max in ((2, 512), (1, 4)):
        run = run_asg(hip_lib, logits, np.zeros((k, k)), np.zeros(k), [[0, 0]], [6], l_max=l_max, k=k)
        assert run.rc == SL_ERR_UNSUPPORTED, (k, l_max, hip_lib.last_error())
        assert (run.loss == FILL).all() and (run.dest == FILL).all() and (run.dg == FILL).all() and (run.dg0 == FILL).all()


@pytest.mark.parametrize("fill", [0x5A, 0xFF], ids=["0x5A", "NaN"])
def test_a_workspace_sized_for_the_limits_serves_every_call(hip_lib, fill):
    """ONE workspace of sl_asg_workspace_bytes(b, t_max, 64, 511), as the engine's asg_ws that only grows: filled once (0xFF:
    every double in it is a NaN), then used for l_max = 300, 60 and 511 in turn with whatever the call before left behind.  Every
    output has the bytes a fresh workspace of exactly the call's own size gives.  The third utterance is infeasible: its part
    of the workspace is never written."""
    import torch
    rng = np.random.RandomState(5)
    k = 29
    cases = []
    for n in ac.WORKSPACE_LENGTHS:
        logits, labels_list, input_len = build_asg_batch(rng, k, ac.workspace_specs(n))
        cases.append((logits, *asg_scores(rng, labels_list, k, "bigram", 12), labels_list, input_len))
    t_max = max(c[0].shape[1] for c in cases)
    big = torch.full((hip_lib.raw("sl_asg_workspace_bytes")(3, t_max, 64, 511),), fill, dtype=torch.uint8, device="cuda:0")
    if fill == 0xFF:
        assert bool(torch.isnan(big.view(torch.float64)).all())
    for logits, g, g0, labels_list, input_len in cases:
        assert hip_lib.raw("sl_asg_workspace_bytes")(3, logits.shape[1], k, len(labels_list[0])) < big.numel()
        exact = run_asg(hip_lib, logits, g, g0, labels_list, input_len)
        shared = run_asg(hip_lib, logits, g, g0, labels_list, input_len, ws=big)
        assert exact.rc == 0 and shared.rc == 0 and np.isfinite(exact.loss[:2]).all() and np.isposinf(exact.loss[2])
        assert np.isfinite(exact.dg).all() and np.isfinite(exact.dl).all()
        assert all(same_bytes(a, b) for a, b in zip(exact.outputs(), shared.outputs())), len(labels_list[0])


# 9 ------------------------------------------------------------------------------------------ engine
def test_engine_mid_short_limit_mid_in_one_buffer_set(hip_lib):
    """A bf16 engine with criterion="asg", one buffer set, 700 output frames: label batches [300, 40], [60, 30], [511, 40] and
    [300, 40] again -- asg_lattice_kernel<8>, <1>, <8> at the limit -- with one asg_ws that only grows.  Every step's losses
    equal, bit for bit, those of sl_asg_loss_grad alone on the engine's own probabilities with a fresh workspace of exactly its
    size; first and last step give the same losses, logits gradient, table gradients and weight gradients; a 512-column label
    batch raises and names the limit."""
    import torch
    from oracle import w2l_oracle as o
    from speechless_amd import _lib
    from speechless_amd.launch_list import HipLibraryError
    from test_gpu_parity import make_case, make_engine
    case = make_case(b=2, t=1400, seed=3, sizes=dict(out_filter_count=256))
    k = case["k"]
    eng = make_engine(case, "bf16", criterion="asg")
    rng = np.random.RandomState(12)
    eng.set_asg_scores(rng.uniform(-2, 2, size=(k, k)).astype(np.float32), rng.uniform(-2, 2, size=k).astype(np.float32))
    pred = [700, 690]
    results, sizes = [], []
    st = torch.cuda.current_stream().cuda_stream
    for lengths, seed in (([300, 40], 5), ([60, 30], 6), ([511, 40], 7), ([300, 40], 5)):
        lrng = np.random.RandomState(seed)
        labels = o.pack_label_batch([list(lrng.randint(0, k, size=n)) for n in lengths])
        eng.load_input(case["x"])
        eng.set_labels(labels, lengths, pred)
        eng.forward()
        losses = eng.asg().cpu().numpy().copy()
        buf = eng.cur
        dlogits = buf.g[len(eng.plans) - 1].clone()
        tables = eng.asg_grads.clone()
        eng.backward()
        torch.cuda.synchronize()
        sizes.append(buf.asg_ws.numel())
        b, t_out, l_max = buf.batch, buf.t_out, buf.labels.shape[1]
        assert l_max == lengths[0] and (b, t_out, k) == (2, 700, 29)
        need = hip_lib.raw("sl_asg_workspace_bytes")(b, t_out, k, l_max)
        assert 0 < need <= sizes[-1]
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda:0")
        alone = torch.full((b,), FILL, dtype=torch.float32, device="cuda:0")
        trans, init = eng.asg_trans, eng.asg_init
        hip_lib.call("sl_asg_loss_grad", buf.probs.data_ptr(), buf.logq.data_ptr(), trans.data_ptr(), init.data_ptr(),
                     buf.labels.data_ptr(), buf.label_len.data_ptr(), buf.input_len.data_ptr(), alone.data_ptr(), None, None, None,
                     b, t_out, k, l_max, 0, k, t_out * k, _lib.SL_F32, eng.ctc_epsilon, 1.0 / b, ws.data_ptr(), need, st)
        torch.cuda.synchronize()
        print(lengths, losses, alone.cpu().numpy(), sizes[-1])
        assert np.isfinite(losses).all() and losses.tobytes() == alone.cpu().numpy().tobytes()
        results.append((losses, dlogits, tables, eng.grads.clone()))
    assert sizes == sorted(sizes) and sizes[2] > sizes[1] == sizes[0]
    assert np.array_equal(results[0][0], results[3][0])
    for a, c in zip(results[0][1:], results[3][1:]):
        assert torch.equal(a, c)
    assert results[0][2].any() and not torch.equal(results[0][2], results[2][2])
    too_long = np.zeros((2, 512), dtype=np.int32)
    with pytest.raises(HipLibraryError, match="511"):
        eng.set_labels(too_long, [300, 40], pred)
        eng.asg()
