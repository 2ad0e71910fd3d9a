"""ASG criterion without a GPU: the label codec, the float64 restatement of the definition ("ASG criterion";
include/speechless_hip.h, sl_asg_loss_grad) that the GPU tests judge the kernels by, its closed-form gradients against
autograd, both against brute-force enumeration, and the float32 restatement of the Viterbi decode (sl_asg_viterbi)."""
import itertools

import numpy as np
import pytest

from speechless_amd.grapheme_encoding import AsgGraphemeEncoding, english_frequent_characters

EPS = 1e-8


# ---------------------------------------------------------------------------------------------------------------- codec
def test_asg_encoding_reproduces_the_reference_known_answers():
    """speechless/test/test_grapheme_encoding.py:36-38 and :43-50, as data"""
    g = AsgGraphemeEncoding(english_frequent_characters)
    assert (g.grapheme_set_size, g.asg_twice, g.asg_thrice) == (30, 28, 29)
    e = g.encode_character("e")
    assert g.encode("ee") == [e, g.asg_twice]
    assert g.encode("eee") == [e, g.asg_thrice]
    letters = [g.encode_character(c) for c in "sssshhhheeeee      wasn't thre"] + [g.asg_twice] * 3 + \
        [g.encode_character(c) for c in "    aaaaaaa"] + [g.asg_thrice]
    assert g.decode_graphemes(letters) == "she wasn't three aaa"


def test_asg_encoding_round_trips_and_refuses_four_in_a_row():
    g = AsgGraphemeEncoding(english_frequent_characters)
    for bad in ("eeee", "xaaaaay"):
        with pytest.raises(ValueError):
            g.encode(bad)
        with pytest.raises(ValueError):
            g.encode_label_batch(["ab", bad])
    with pytest.raises(ValueError):
        g.encode("é")
    rng = np.random.RandomState(0)
    labels = ["", "a", "aa", "aaa", "aab", "baa", "aabbbcc a''' z", "she wasn't three"]
    for _ in range(50):
        runs = [c * rng.randint(1, 4) for c in rng.choice(list("ab '"), size=rng.randint(1, 12))]
        labels.append("".join(r for i, r in enumerate(runs) if i == 0 or r[0] != runs[i - 1][0]))
    for s in labels:
        code = g.encode(s)
        assert all(a != b for a, b in zip(code, code[1:])), s  # no adjacent equal graphemes
        assert g.decode_graphemes(code) == s == g.decode_graphemes(code, merge_repeated=False)
    batch = g.encode_label_batch(labels)
    assert batch.dtype == np.int32 and batch.shape[0] == len(labels)
    for row, s in zip(batch, labels):
        n = int((row >= 0).sum())
        assert list(row[:n]) == g.encode(s) and (row[n:] == -1).all()
    assert g.decode_grapheme_batch(batch, (batch >= 0).sum(1)) == labels
    # a repeat mark with nothing to repeat stands for nothing
    assert g.decode_graphemes([g.asg_twice, 0, g.asg_thrice, g.asg_twice]) == "aaa"
    with pytest.raises(ValueError):
        g.decode_grapheme(30)


# ------------------------------------------------------------------------------------------- float64 restatement (numpy)
def _lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def asg_reference(p, g, g0, label, eps=EPS):
    """One utterance, float64.  p: (T, K) probabilities; g: (K, K) [from][to]; g0: (K,); label: ints in [0, K).
    Returns (loss, dlogits (T, K), dg (K, K), dg0 (K,)) of the definition, the gradients in closed form; an infeasible
    utterance (L = 0, T = 0 or L > T) gives (+inf, zeros, zeros, zeros)."""
    p = np.asarray(p, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    g0 = np.asarray(g0, dtype=np.float64)
    t_n, k = p.shape
    lab = np.asarray(label, dtype=np.int64)
    n = len(lab)
    if n == 0 or t_n == 0 or n > t_n:
        return np.inf, np.zeros((t_n, k)), np.zeros((k, k)), np.zeros(k)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.log(p + eps)
        el = e[:, lab]
        gs, ga = g[lab, lab], g[lab[:-1], lab[1:]]
        ninf = np.array([-np.inf])
        a = np.full((t_n, n), -np.inf)
        a[0, 0] = g0[lab[0]] + el[0, 0]
        for t in range(1, t_n):
            a[t] = el[t] + np.logaddexp(a[t - 1] + gs, np.concatenate([ninf, a[t - 1, :-1] + ga]))
        num = a[-1, -1]
        bt = np.full((t_n, n), -np.inf)
        bt[-1, -1] = 0.0
        for t in range(t_n - 2, -1, -1):
            u = bt[t + 1] + el[t + 1]
            bt[t] = np.logaddexp(u + gs, np.concatenate([u[1:] + ga, ninf]))
        d = np.zeros((t_n, k))
        d[0] = g0 + e[0]
        for t in range(1, t_n):
            d[t] = e[t] + _lse(d[t - 1][:, None] + g, 0)
        z = _lse(d[-1], 0)
        db = np.zeros((t_n, k))
        for t in range(t_n - 2, -1, -1):
            db[t] = _lse(g + (e[t + 1] + db[t + 1])[None, :], 1)
        gnum = np.zeros((t_n, k))
        np.add.at(gnum, (np.arange(t_n)[:, None], lab[None, :]), np.exp(a + bt - num))
        big_g = np.exp(d + db - z) - gnum
        x = big_g * (p / (p + eps))
        dlogits = x - p * x.sum(1, keepdims=True)
        dg = np.zeros((k, k))
        for t in range(1, t_n):
            dg += np.exp(d[t - 1][:, None] + g + (e[t] + db[t])[None, :] - z)
        stay = np.exp(a[:-1] + gs + el[1:] + bt[1:] - num).sum(0)
        adv = np.exp(a[:-1, :-1] + ga + el[1:, 1:] + bt[1:, 1:] - num).sum(0)
        np.subtract.at(dg, (lab, lab), stay)
        np.subtract.at(dg, (lab[:-1], lab[1:]), adv)
    return float(z - num), dlogits, dg, big_g[0].copy()


def asg_reference_batch(probs, g, g0, labels_list, input_len, eps=EPS, grad_scale=1.0):
    """The batch form the kernel computes: per-utterance losses, dlogits (B, T', K) with zero rows past T_b, and the
    gradients of g / g0 summed over the batch, all times grad_scale."""
    b, t_out, k = probs.shape
    loss = np.zeros(b)
    dlogits = np.zeros((b, t_out, k))
    dg, dg0 = np.zeros((k, k)), np.zeros(k)
    for i, label in enumerate(labels_list):
        t_b = min(max(int(input_len[i]), 0), t_out)
        loss[i], dl, a, c = asg_reference(probs[i, :t_b], g, g0, label, eps)
        dlogits[i, :t_b] = grad_scale * dl
        dg += grad_scale * a
        dg0 += grad_scale * c
    return loss, dlogits, dg, dg0


def asg_loss_torch(logits, g, g0, label, eps=EPS):
    """The definition in torch (CPU, any float dtype) built from logsumexp, so that autograd differentiates it.  States that
    cannot be occupied yet carry -1e30 in place of -inf: the same values to the last bit (exp underflows to an exact 0 against
    any reachable state), but logsumexp over nothing but -inf has a NaN derivative."""
    import torch
    return asg_loss_torch_from_probs(torch.softmax(logits, dim=-1), g, g0, label, eps)


def asg_loss_torch_from_probs(p, g, g0, label, eps=EPS):
    """asg_loss_torch behind the softmax: p (T, K) is the output layer's distribution (any graph may have produced it)"""
    import torch
    e = torch.log(p + eps)
    lab = torch.as_tensor(list(label), dtype=torch.long)
    t_n, n = e.shape[0], len(lab)
    ninf = torch.full((1,), -1e30, dtype=e.dtype)
    gs, ga = g[lab, lab], g[lab[:-1], lab[1:]]
    a = torch.cat([(g0[lab[0]] + e[0, lab[0]]).reshape(1), ninf.expand(n - 1)])
    d = g0 + e[0]
    for t in range(1, t_n):
        a = e[t, lab] + torch.logsumexp(torch.stack([a + gs, torch.cat([ninf, a[:-1] + ga])]), dim=0)
        d = e[t] + torch.logsumexp(d[:, None] + g, dim=0)
    return torch.logsumexp(d, dim=0) - a[-1]


def random_case(rng, t_n, k, label, scale=1.0):
    logits = rng.randn(t_n, k) * scale
    g = rng.uniform(-2, 2, size=(k, k))
    g0 = rng.uniform(-2, 2, size=k)
    z = logits - logits.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    return logits, p, g, g0, list(label)


@pytest.mark.parametrize("t_n,k,label,scale", [(12, 6, [0, 3, 3, 5, 1], 1.0), (7, 4, [2, 2, 2, 2, 2, 2, 2], 3.0),
                                                (1, 5, [4], 1.0), (9, 3, [1], 8.0), (20, 30, [7, 28, 3, 3, 29, 0], 2.0)])
def test_closed_form_gradients_match_autograd(t_n, k, label, scale):
    import torch
    logits, p, g, g0, label = random_case(np.random.RandomState(t_n * 100 + k), t_n, k, label, scale)
    loss, dlogits, dg, dg0 = asg_reference(p, g, g0, label)
    tz, tg, tg0 = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (logits, g, g0))
    tl = asg_loss_torch(tz, tg, tg0, label)
    tl.backward()
    assert abs(loss - tl.item()) < 1e-9 * max(1.0, abs(loss)) and loss >= 0
    for mine, leaf in ((dlogits, tz), (dg, tg), (dg0, tg0)):
        auto = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)  # (T = 1: no transition enters the loss)
        assert np.abs(mine - auto.numpy()).max() < 1e-9


def brute_force_loss(e, g, g0, label):
    t_n, k = e.shape

    def score(letters):
        s = g0[letters[0]] + e[0, letters[0]]
        for t in range(1, t_n):
            s += g[letters[t - 1], letters[t]] + e[t, letters[t]]
        return s

    den = [score(seq) for seq in itertools.product(range(k), repeat=t_n)]
    num = []
    for steps in itertools.product((0, 1), repeat=t_n - 1):  # monotone alignments: state 0 first, L - 1 last
        states = np.concatenate([[0], np.cumsum(steps)]).astype(int)
        if states[-1] == len(label) - 1:
            num.append(score([label[s] for s in states]))
    lse = lambda v: np.max(v) + np.log(np.sum(np.exp(np.array(v) - np.max(v))))  # noqa: E731
    return lse(den) - lse(num)


@pytest.mark.parametrize("t_n,label", [(1, [2]), (2, [0, 1]), (3, [1, 1]), (4, [2, 0, 0]), (5, [1, 1, 1, 2]), (5, [0]),
                                       (5, [0, 1, 2, 1, 0]), (4, [2, 2, 2, 2])])
def test_restatement_matches_brute_force(t_n, label):
    _, p, g, g0, label = random_case(np.random.RandomState(17 * t_n + len(label)), t_n, 3, label, 2.0)
    loss = asg_reference(p, g, g0, label)[0]
    assert abs(loss - brute_force_loss(np.log(p + EPS), g, g0, label)) < 1e-10


def test_infeasible_utterances_have_infinite_loss_and_no_gradient():
    _, p, g, g0, _ = random_case(np.random.RandomState(3), 4, 3, [0])
    for t_b, label in ((4, []), (4, [0, 1, 2, 0, 1]), (0, [1])):
        loss, dl, dg, dg0 = asg_reference(p[:t_b], g, g0, label)
        assert loss == np.inf and not dl.any() and not dg.any() and not dg0.any()


# ---------------------------------------------------------------------------------------------------- Viterbi restatement
def asg_viterbi(e, g, g0, t_b, dtype=np.float32):
    """sl_asg_viterbi for one utterance: e (T', K) emissions as they are.  Returns (score, path int32 (T',), -1 past t_b).
    float32: every operation a max or one add in the kernel's order -- the bit-exact restatement."""
    e, g, g0 = (np.asarray(x, dtype=dtype) for x in (e, g, g0))
    t_out, k = e.shape
    path = np.full(t_out, -1, dtype=np.int32)
    if t_b <= 0:
        return dtype(-np.inf), path
    v = g0 + e[0]
    bp = np.zeros((t_b, k), dtype=np.int32)
    for t in range(1, t_b):
        best = v[0] + g[0]
        arg = np.zeros(k, dtype=np.int32)
        for i in range(1, k):
            cand = v[i] + g[i]
            better = cand > best
            best = np.where(better, cand, best)
            arg[better] = i
        v = best + e[t]
        bp[t] = arg
    s = int(np.argmax(v))  # the first maximal letter
    score = v[s]
    for t in range(t_b - 1, -1, -1):
        path[t] = s
        s = bp[t, s]
    return score, path


def path_score64(e, g, g0, path):
    e, g, g0 = (np.asarray(x, dtype=np.float64) for x in (e, g, g0))
    s = g0[path[0]] + e[0, path[0]]
    for t in range(1, len(path)):
        s += g[path[t - 1], path[t]] + e[t, path[t]]
    return s


@pytest.mark.parametrize("t_n,k,scale", [(1, 5, 1.0), (40, 30, 1.0), (130, 64, 6.0), (65, 34, 0.01)])
def test_float32_viterbi_finds_the_float64_best_path_score(t_n, k, scale):
    rng = np.random.RandomState(t_n + k)
    e = np.log(random_case(rng, t_n, k, [0], scale)[1] + EPS).astype(np.float32)
    g = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
    g0 = rng.uniform(-2, 2, size=k).astype(np.float32)
    score32, path32 = asg_viterbi(e, g, g0, t_n)
    score64, path64 = asg_viterbi(e, g, g0, t_n, dtype=np.float64)
    assert abs(path_score64(e, g, g0, path64) - score64) <= 1e-9 * abs(score64)
    assert abs(float(score32) - score64) <= 1e-5 * abs(score64)
    assert abs(path_score64(e, g, g0, path32) - score64) <= 1e-5 * abs(score64)
    if t_n <= 5 and k <= 5:
        assert score64 == max(path_score64(e, g, g0, q) for q in itertools.product(range(k), repeat=t_n))


def test_viterbi_tie_rule_and_forced_transitions():
    k, t_n = 4, 6
    score, path = asg_viterbi(np.zeros((t_n, k)), np.zeros((k, k)), np.zeros(k), 5)
    assert list(path) == [0, 0, 0, 0, 0, -1] and score == 0
    e = np.zeros((t_n, k), dtype=np.float32)
    e[:, 2] = 1.0  # letter 2 is every frame's argmax, but staying on a letter is heavily punished
    g = np.zeros((k, k), dtype=np.float32)
    g[np.arange(k), np.arange(k)] = -50.0
    e[:, 0] = 0.5
    score, path = asg_viterbi(e, g, np.zeros(k), t_n)
    assert list(path) == [2, 0, 2, 0, 2, 0] and score == np.float32(4.5)
    assert score == max(path_score64(e, g, np.zeros(k), q) for q in itertools.product(range(k), repeat=t_n))
    assert asg_viterbi(e, g, np.zeros(k), 0)[0] == -np.inf


# -------------------------------------------------------------------------------------------------------------- the ctor
def test_constructor_keywords_are_checked_before_any_device_is_touched():
    from speechless_amd.net import Wav2Letter
    with pytest.raises(ValueError, match="criterion"):
        Wav2Letter(128, english_frequent_characters, criterion="nope")
    with pytest.raises(NotImplementedError):  # as the reference: use_asg keeps raising, ASG is criterion="asg"
        Wav2Letter(128, english_frequent_characters, use_asg=True)
    with pytest.raises(NotImplementedError):
        Wav2Letter(128, english_frequent_characters, use_asg=True, criterion="asg")
