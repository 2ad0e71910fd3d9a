"""tests/asg_cases.py without a GPU: what its generators produce, the floor of double arithmetic under the bounds of
tests/test_gpu_asg_mid.py (the float64 restatement against float64 autograd at 511 letters, 900 frames and scores of +-30), and
the shapes of the GPU module's cases."""
import numpy as np
import pytest

import asg_cases as ac
from test_asg import asg_loss_torch_from_probs, asg_reference


def softmax32(logits):
    """the fp32 distribution a kernel would be given, as float64"""
    z = logits.astype(np.float32) - logits.max(1, keepdims=True)
    e = np.exp(z, dtype=np.float32)
    return (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float64)


def one_utterance(seed, k, n, t, regime, kind, s, strength=None):
    rng = np.random.RandomState(seed)
    logits, labels_list, input_len = ac.build_asg_batch(rng, k, [(n, t - n, regime)], t_out=t, strength=strength)
    g, g0 = ac.asg_scores(rng, labels_list, k, kind, s)
    assert input_len == [t]
    return softmax32(logits[0]), g, g0, labels_list[0]


# 1 ---------------------------------------------------------------------------------------------------------- generators
def test_learnt_and_wrong_are_runs_of_the_label_without_a_blank():
    rng = np.random.RandomState(0)
    for k in (2, 3, 29, 64):
        label = [int(c) for c in rng.randint(0, k, size=40)]
        lg = ac.asg_regime_logits(rng, label, 100, k, "learnt", strength=25.0)
        path = lg.argmax(1)
        runs = [int(c) for i, c in enumerate(path) if i == 0 or c != path[i - 1]]
        assert runs == [c for i, c in enumerate(label) if i == 0 or c != label[i - 1]]  # equal neighbours merge into one run
        assert (np.sort(lg, axis=1)[:, -1] > 15).all()  # every frame belongs to a run: no blank, no frame left over
        wrong = ac.asg_regime_logits(rng, label, 40, k, "wrong", strength=25.0).argmax(1)  # zero slack: one frame per letter
        changed = int((wrong != np.array(label)).sum())
        assert 6 <= changed <= 26, (k, changed)  # 40 % of 40 letters, each replaced by ANOTHER letter
    lg = ac.asg_regime_logits(rng, [1, 2, 3], 2, 5, "learnt")  # a label that does not fit: noise, no error
    assert lg.shape == (2, 5) and np.abs(lg).max() < 6
    for kind in ("uniform", "sharp", "collapse"):  # tools/fuzz_ctc.regime_logits, draw for draw
        a = ac.asg_regime_logits(np.random.RandomState(4), [1, 2], 9, 5, kind)
        b = ac.fuzz_regime_logits(np.random.RandomState(4), [1, 2], 9, 5, kind)
        assert a.tobytes() == b.tobytes()


def test_score_tables():
    rng = np.random.RandomState(1)
    labels = [[0, 3, 3, 4], [2, 0]]
    g, g0 = ac.asg_scores(rng, labels, 5, "bigram", 12)
    assert g.dtype == np.float32 and g0.dtype == np.float32
    want = np.full((5, 5), -12.0)
    want[0, 3] = want[3, 4] = want[2, 0] = 12.0
    want[np.arange(5), np.arange(5)] = 6.0
    assert np.array_equal(g, want) and list(g0) == [12, -12, 12, -12, -12]
    h, h0 = ac.asg_scores(rng, labels, 5, "hostile", 12)
    assert np.array_equal(h, -g) and np.array_equal(h0, -g0)
    r, r0 = ac.asg_scores(rng, labels, 5, "random")
    assert np.abs(r).max() <= 2 and np.abs(r0).max() <= 2 and r.std() > 0.5
    with pytest.raises(ValueError):
        ac.asg_scores(rng, labels, 5, "bigram", 7)


@pytest.mark.parametrize("s", [12, 30])
def test_learnt_under_bigram_scores_is_nearly_solved_and_hostile_scores_punish_the_label(s):
    """Strength 25, 40 distinct letters of 64 in 200 frames (no equal neighbours, so Z >= N, and no pair adjacent in both
    orders: at s = 30 a detour a -> b -> a through two +s transitions is worth 5 nats more than two stays at +s / 2 and the
    25 nats of the wrong frame, and the loss of a label with such pairs is hundreds of nats -- the random labels of the other
    tests have them, which is what a half-trained table looks like)."""
    k, n, t = 64, 40, 200
    rng = np.random.RandomState(3)
    label = [int(c) for c in rng.permutation(k)[:n]]
    p = softmax32(ac.asg_regime_logits(rng, label, t, k, "learnt", strength=25.0))
    g, g0 = ac.asg_scores(rng, [label], k, "bigram", s)
    loss = asg_reference(p, g, g0, label)[0]
    print("bigram", s, loss)
    assert 0 <= loss < t / 100.0  # below 1 nat per 100 frames
    g, g0 = ac.asg_scores(rng, [label], k, "hostile", s)
    loss = asg_reference(p, g, g0, label)[0]
    print("hostile", s, loss)
    assert loss > s * (n - 1)  # above s nats per label transition
    # the labels build_asg_batch draws (equal neighbours allowed) under the same tables: finite, and hostile still punishes
    p, g, g0, label = one_utterance(3, 29, 120, 300, "learnt", "hostile", s, strength=25.0)
    assert asg_reference(p, g, g0, label)[0] > s * 119


@pytest.mark.parametrize("kind,s", [("bigram", 12), ("bigram", 30), ("hostile", 12), ("hostile", 30)])
def test_restatement_is_finite_at_511_letters_and_900_frames(kind, s):
    for j, regime in enumerate(ac.REGIMES):
        p, g, g0, label = one_utterance(10 * s + j, 29, 511, 900, regime, kind, s)
        loss, dl, dg, dg0 = asg_reference(p, g, g0, label)
        assert np.isfinite(loss), (regime, loss)
        assert np.isfinite(dl).all() and np.isfinite(dg).all() and np.isfinite(dg0).all(), regime
        assert np.abs(dl).max() <= 2.0 and np.abs(dg0).max() <= 1.0 + 1e-9


# 2 ---------------------------------------------------------------------------------------------------------- the floor
@pytest.mark.parametrize("k,n,t,regime,s", [(29, 511, 900, "learnt", 30), (64, 511, 511, "learnt", 30),
                                            (29, 511, 900, "wrong", 30), (2, 300, 900, "learnt", 12)])
def test_floor_of_double_arithmetic_under_the_tight_bounds(k, n, t, regime, s):
    """asg_reference against float64 autograd of the definition written with logsumexp: loss, dtrans and dinit within 1e-7
    (measured: at most 9.4e-10 on dtrans, 4.3e-11 on dinit and 7.3e-12 on a loss of 4114; three losses equal to the last bit) -- a tenth
    of the 1e-6 the GPU module allows, so that bound is not taken up by the reference's own error"""
    import torch
    p, g, g0, label = one_utterance(7, k, n, t, regime, "bigram", s)
    loss, _, dg, dg0 = asg_reference(p, g, g0, label)
    tg, tg0 = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (g, g0))
    tl = asg_loss_torch_from_probs(torch.tensor(p, dtype=torch.float64), tg, tg0, label)
    tl.backward()
    e_loss, e_dg, e_dg0 = abs(loss - tl.item()), np.abs(dg - tg.grad.numpy()).max(), np.abs(dg0 - tg0.grad.numpy()).max()
    print("loss %.12g: distance %.1e; dtrans (largest %.4g) %.1e; dinit %.1e" % (loss, e_loss, np.abs(dg).max(), e_dg, e_dg0))
    assert e_loss < 1e-7 and e_dg < 1e-7 and e_dg0 < 1e-7


# 3 ---------------------------------------------------------------------------------------------------------- the batches
def test_build_asg_batch_frames_and_t_out():
    rng = np.random.RandomState(2)
    specs = [(40, 0, "learnt"), (7, 1, "wrong"), (0, 9, "uniform"), (12, -2, "sharp"), (3, -3, "collapse")]
    logits, labels_list, input_len = ac.build_asg_batch(rng, 5, specs)
    assert input_len == [40, 8, 9, 10, 0] and [len(lab) for lab in labels_list] == [40, 7, 0, 12, 3]
    assert logits.shape == (5, 40, 5) and logits.dtype == np.float32  # 41 is no multiple of 4
    for i, t_b in enumerate(input_len):
        assert not logits[i, t_b:].any() and (t_b == 0 or logits[i, :t_b].any())
    assert max(max(lab) for lab in labels_list if lab) == 4  # every letter is a label: there is no blank
    assert ac.build_asg_batch(rng, 5, [(39, 0, "learnt")])[0].shape[1] == 40  # 39 + 1 is one: a full last group of 4 frames
    assert ac.build_asg_batch(rng, 5, [(38, 0, "learnt")])[0].shape[1] == 38
    assert ac.build_asg_batch(rng, 5, [(0, -4, "learnt")])[0].shape[1] == 1


def test_cases_of_the_gpu_module_stay_within_900_frames_and_cover_the_chunkings():
    cases = ac.all_gpu_specs()
    assert max(t_out for _, t_out in cases) <= ac.MAX_FRAMES
    for specs, t_out in cases:
        assert len(specs) <= 8 and max(ac.frames_of(specs)) <= t_out and max(n for n, _, _ in specs) <= 511
    assert max(n for specs, _ in cases for n, _, _ in specs) == 511
    for i, n in enumerate(ac.BOUNDARY_LENGTHS):  # zero slack: as many frames as letters
        specs = ac.boundary_specs(i)
        assert ac.frames_of(specs) == [n, n + 1, n + n // 4]
    assert {r for i in range(len(ac.BOUNDARY_LENGTHS)) for _, _, r in ac.boundary_specs(i)} == set(ac.REGIMES)
    chunks = ac.chunk_batches()
    assert {t_out % 4 for _, t_out in chunks[:6]} == {0, 1, 2, 3}
    for n, part in ((5, chunks[:3]), (300, chunks[3:6])):
        frames = sorted(t for specs, _ in part for t in ac.frames_of(specs))
        assert frames == list(range(n, n + 18)) and {t % 8 for t in frames} == set(range(8))
        assert all(len(specs) == 6 and max(ac.frames_of(specs)) < t_out for specs, t_out in part)
    assert ac.frames_of(chunks[6][0]) == [7, 8, 9]
    stream = ac.fuzz_stream()
    assert len(stream) == 4 and all(len(specs) == 8 for _, _, _, specs in stream)
    assert {k for k, _, _, _ in stream} == {2, 29, 64} and {kind for _, kind, _, _ in stream} == set(ac.SCORE_KINDS)
    lengths = [n for _, _, _, specs in stream for n, _, _ in specs]
    assert min(lengths) == 1 and max(lengths) == 511
    assert {r for _, _, _, specs in stream for _, _, r in specs} == set(ac.REGIMES)
    assert all(0 <= slack <= 300 for _, _, _, specs in stream for _, slack, _ in specs)
