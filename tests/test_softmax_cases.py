"""tests/softmax_cases.py without a GPU: the float32 restatement of the softmax kernels stays within HALF of every bound on every
case (of the probs bound: half of all that is an allowance in it, the whole of the one known rounding: 0.59 of the bound at worst,
0.35 where d <= 32; logq 0.24), the bound helpers give what is known by hand, the cases hold what tests/test_gpu_softmax.py relies on, and the loss bound
of the chain test covers a logq that is off by the logq bound."""
import numpy as np
import pytest

import softmax_cases as sc
from exact_ints import is_bf16_exact
from oracle import w2l_oracle as o


# ------------------------------------------------------------------------------------------------------------ the restatement
def restatement_ratios(logits, eps, order):
    """the restatement's worst error in units of: the probs bound; the probs bound where d <= 32; the part of the probs bound
    that is an allowance (the error less p* r_i, over p* 40 u + 2^-148: softmax_cases' docstring); the logq bound"""
    probs, logq = sc.restate_f32(logits, eps, order=order)
    p, lq = sc.reference(logits, eps)
    err = np.abs(probs.astype(np.float64) - p)
    whole = err / sc.probs_bound(logits)
    near = whole[sc.distances(logits) <= 32.0]
    allowance = (err - p * sc.input_rounding(logits)) / sc.probs_slack(logits)
    rq = np.abs(logq.astype(np.float64) - lq) / sc.logq_bound(logits, eps)
    return float(whole.max()), float(near.max()), float(allowance.max()), float(rq.max())


def check_restatement(named_logits, order):
    worst = np.zeros(4)
    for name, logits, eps in named_logits:
        r = restatement_ratios(logits, eps, order)
        print("%-40s probs %.3f of its bound (%.3f where d <= 32, %.3f of the allowance), logq %.3f" % ((name,) + r))
        worst = np.maximum(worst, r)
        assert r[0] <= 1.0 and r[1] <= 0.5 and r[2] <= 0.5 and r[3] <= 0.5, (name, r)
    print("worst ratios (%s order): probs %.3f, %.3f where d <= 32, %.3f of the allowance; logq %.3f" % ((order,) + tuple(worst)))
    return worst


def test_restatement_stays_within_half_of_every_bound():
    """logq: within half of its bound on every case.  probs: within half of everything in its bound that is an allowance, within
    half of the whole bound where d <= 32, within the whole bound everywhere -- the d u term is a known rounding that every fp32
    evaluation attains (softmax_cases' docstring)."""
    worst = check_restatement([(c.name, c.logits, c.eps) for c in sc.all_cases()], "wave")
    assert worst[0] >= 0.1 and worst[3] >= 0.1, "the bounds are vacuous"


def test_restatement_in_the_fused_tails_order_stays_within_half_of_every_bound():
    cases = [(c.name, c.logits, c.eps) for c in sc.all_cases() if c.k <= 32]
    for cin, k, t_out, batch in sc.fused_shapes()[::5]:
        cases.append(("fused_cin{}_k{}_t{}_b{}".format(cin, k, t_out, batch), sc.fused_case(cin, k, t_out, batch).logits,
                      sc.FUSED_EPS))
    check_restatement(cases, "fused")


def test_the_two_orders_of_the_restatement_agree_to_their_bounds():
    case = next(c for c in sc.all_cases() if c.k == 29 and c.eps == 1e-8 and c.name.startswith("margins"))
    pw, qw = sc.restate_f32(case.logits, case.eps)
    pf, qf = sc.restate_f32(case.logits, case.eps, order="fused")
    assert (np.abs(pw.astype(np.float64) - pf) <= sc.probs_bound(case.logits)).all()
    assert (np.abs(qw.astype(np.float64) - qf) <= sc.logq_bound(case.logits, case.eps)).all()


# ------------------------------------------------------------------------------------------------------------ known by hand
@pytest.mark.parametrize("k", sc.CLASS_COUNTS)
def test_uniform_row_by_hand(k):
    for value in (0.0, -17.25, 1e4):
        row = np.full((1, k), value, dtype=np.float32)
        for eps in sc.EPS_VALUES:
            p, lq = sc.reference(row, eps)
            assert np.allclose(p, 1.0 / k, rtol=1e-15, atol=0) and np.allclose(lq, -np.log(k), rtol=1e-14, atol=0)
            assert np.allclose(sc.probs_bound(row), (1.0 / k) * 40 * 2.0 ** -24 + 2.0 ** -148, rtol=1e-12, atol=0)
            rp, rq = sc.restate_f32(row, eps)
            assert np.abs(rp - 1.0 / k).max() <= 2.0 ** -24 / k * 2 and np.abs(rq + np.log(k)).max() <= 1e-6


@pytest.mark.parametrize("k", sc.CLASS_COUNTS)
def test_margin_of_ten_thousand_by_hand(k):
    row = np.full((1, k), -1e4, dtype=np.float32)
    row[0, k // 2] = 0.0
    for eps in (1e-8, 1e-7):
        e32 = float(np.float32(eps))
        p, lq = sc.reference(row, eps)
        want_p = np.zeros(k)
        want_p[k // 2] = 1.0
        assert np.array_equal(p[0], want_p)
        lose = np.log(e32 / (1.0 + k * e32))
        win = np.log((1.0 + e32) / (1.0 + k * e32))
        want_q = np.full(k, lose)
        want_q[k // 2] = win
        assert np.allclose(lq[0], want_q, rtol=1e-13, atol=1e-14)
        bound = sc.probs_bound(row)[0]
        assert bound[k // 2] == 40 * 2.0 ** -24 + 2.0 ** -148 and (np.delete(bound, k // 2) == 2.0 ** -148).all()
        assert (sc.logq_bound(row, eps) == 1e-5).all()
        rp, rq = sc.restate_f32(row, eps)
        assert np.array_equal(rp[0], want_p.astype(np.float32)) and np.abs(rq[0] - want_q).max() <= 2.5e-6
    with pytest.raises(ValueError):
        sc.logq_bound(row, 0.0)
    with pytest.raises(ValueError):
        sc.logq_bound(row, 1e-9)


def test_eps0_bound_by_hand():
    """d = 0 at k = 2: 3 log 2 u + 40 u + 3.7e-6; at the edge d = 60 with k = 64 it stays below 2.1e-5"""
    tie = np.zeros((1, 2), dtype=np.float32)
    assert np.allclose(sc.logq_bound(tie, 0.0), (3 * np.log(2) + 40) * 2.0 ** -24 + 3.7e-6, rtol=1e-12, atol=0)
    edge = np.full((1, 64), -60.0, dtype=np.float32)
    edge[0, 0] = 0.0
    b = sc.logq_bound(edge, 0.0)
    assert b[0, 0] < 6.1e-6 and 1.3e-5 < b[0, 1] <= 2.1e-5
    _, lq = sc.reference(edge, 0.0)
    assert abs(lq[0, 1] + 60.0) < 1e-12  # log q* = -d - log(1 + 63 e^-60)


# ------------------------------------------------------------------------------------------------------------ the cases
def test_cases_cover_what_the_issue_lists():
    cases = sc.all_cases()
    assert {c.k for c in cases} == set(sc.CLASS_COUNTS)
    assert {(c.k, c.eps) for c in cases if c.name.startswith("margins")} == {(k, e) for k in sc.CLASS_COUNTS for e in sc.EPS_VALUES}
    frames = {c.batch * c.t_out for c in cases}
    assert {1, 5, 7} <= frames and any(f % 4 == 3 and f > 7 for f in frames) and max(frames) <= sc.MAX_FRAMES
    assert {c.k for c in cases if c.batch * c.t_out == 1} == set(sc.CLASS_COUNTS)
    assert any(c.padded for c in cases) and any(not c.padded for c in cases)
    for k in sc.CLASS_COUNTS:
        assert any(c.padded for c in cases if c.k == k and c.name.startswith("margins"))
    for c in cases:
        assert c.logits.dtype == np.float32 and np.isfinite(c.logits).all()
        if c.padded:
            assert c.logit_stride == c.k + 3 and c.batch_stride > c.t_out * c.logit_stride
        buf = c.buffer()
        assert int((buf != sc.PAD).sum()) == c.logits.size  # (no logit is 3e38)
        if c.eps == 0.0:
            assert sc.distances(c.logits).max() <= sc.EPS0_MAX_D


@pytest.mark.parametrize("k", sc.CLASS_COUNTS)
def test_margin_cases_hold_every_margin(k):
    case = next(c for c in sc.all_cases() if c.k == k and c.eps == 1e-8 and c.name.startswith("margins"))
    z = case.logits.reshape(-1, k).astype(np.float64)
    d = np.sort(z.max(axis=1, keepdims=True) - z, axis=1)
    top_margin = d[:, 1]
    near = [m for m in sc.MARGINS if not np.any(np.abs(top_margin - m) <= 2e-3 + 1e-6 * m)]
    assert not near, near
    assert np.any((d[:, 1] == 0) & ((d[:, 2] > 0) if k > 2 else True)), "an exact tie of two classes"
    assert np.any(d[:, -1] == 0), "an exact tie of all classes"
    assert np.any(np.abs(z).min(axis=1) > 9e3), "a row moved by 1e4 as a whole"
    for m in (87.0, 88.0, 104.0):  # the fp32 exp around its denormals: a second tier beyond the margin as well
        assert np.any(d[:, 1:] > m)
    # the generator is deterministic
    again = sc.margin_case(k, 1e-8, case.padded, seed=1000 + 10 * k + 0)
    assert np.array_equal(again.logits, case.logits)


def test_monotone_violations_counts_what_it_says():
    z = np.array([[0.0, 1.0, 1.0, 3.0]])
    assert sc.monotone_violations(z, np.array([[0.1, 0.2, 0.2, 0.5]])) == 0
    assert sc.monotone_violations(z, np.array([[0.1, 0.2, 0.3, 0.5]])) == 1  # equal logits, unequal values
    assert sc.monotone_violations(z, np.array([[0.3, 0.2, 0.2, 0.5]])) == 1
    assert sc.monotone_violations(z, np.array([[0.2, 0.2, 0.2, 0.2]])) == 0


# ------------------------------------------------------------------------------------------------------------ the fused cases
def test_fused_shapes_cover_what_the_issue_lists():
    shapes = sc.fused_shapes()
    assert len(shapes) == len(set(shapes)) == 48
    for cin in sc.FUSED_CIN:
        assert {(t, b) for c, _, t, b in shapes if c == cin} == set(sc.FUSED_FRAMES)
        assert {k for c, k, _, _ in shapes if c == cin} == set(sc.FUSED_K)
    for k in sc.FUSED_K:
        assert {(t, b) for _, kk, t, b in shapes if kk == k} == set(sc.FUSED_FRAMES)


@pytest.mark.parametrize("cin,k,t_out,batch", [(64, 2, 63, 1), (64, 32, 130, 3), (256, 17, 77, 1), (512, 29, 130, 1),
                                               (2048, 32, 130, 3), (2048, 5, 63, 3), (2048, 16, 1, 1)])
def test_fused_case_is_exact_and_covers_the_margins(cin, k, t_out, batch):
    case = sc.fused_case(cin, k, t_out, batch)
    assert is_bf16_exact(np.array(case.x)) and is_bf16_exact(np.array(case.w))
    unit = sc.FUSED_UNIT
    assert np.array_equal(np.rint(case.bias / unit) * unit, case.bias) and np.abs(case.bias).max() < 0.25
    # a fraction times a fraction never meets: fractional activations only in the fraction channel, whose weights are integers;
    # fractional weights only in the bias channel, whose activations are integers -> every product is a multiple of 2^-10
    xf = case.x != np.rint(case.x)
    wf = case.w != np.rint(case.w)
    assert not np.delete(xf, case.frac_ch, axis=2).any() and not np.delete(wf, case.bias_ch, axis=1).any()
    assert np.array_equal(np.rint(case.x / unit) * unit, case.x) and np.array_equal(np.rint(case.w / unit) * unit, case.w)
    assert sc.fused_accumulator_bound(case) < 2 ** 13  # with the unit 2^-10: 23 bits
    assert np.array_equal(case.logits.astype(np.float64), case.x @ case.w.T + case.bias)
    if t_out >= 63:
        z = case.logits.reshape(-1, k).astype(np.float64)
        d = np.sort(z.max(axis=1, keepdims=True) - z, axis=1)[:, 1]
        n_pat = len(sc.FUSED_INT_MARGINS)
        control = case.kinds.reshape(-1) < n_pat + 2
        assert set(sc.FUSED_MARGINS) <= set(d[control].tolist()), sorted(set(sc.FUSED_MARGINS) - set(d[control].tolist()))
        assert set(case.kinds.reshape(-1).tolist()) == set(range(sc.FUSED_TYPES))
        # every ordinary channel carries a non-zero activation in some frame, and a dense frame moves the bias in
        dense = case.x[case.kinds >= n_pat + 2]
        assert (np.abs(dense).sum(axis=0) > 0).sum() >= cin - n_pat - 2
        assert (dense[:, case.bias_ch] != 1).any()


# ------------------------------------------------------------------------------------------------------------ the loss bound
def test_chain_batches_are_what_the_issue_lists():
    for regime in sc.CHAIN_REGIMES:
        logits, labels_list, input_len = sc.chain_batch_29(regime)
        assert logits.shape[2] == 29 and logits.shape[1] <= 120
        assert sorted({len(lab) for lab in labels_list}) == [0, 1, 12, 40]
        need = [max(len(lab) + sum(1 for a, c in zip(lab, lab[1:]) if a == c), 1) for lab in labels_list]
        slack = [t - n for t, n in zip(input_len, need)]
        for n in (0, 1, 12, 40):
            mine = [s for s, lab in zip(slack, labels_list) if len(lab) == n]
            assert 0 in mine and max(mine) > 0
    logits, labels_list, input_len = sc.chain_batch_64()
    assert logits.shape[2] == 64 and logits.shape[1] <= 80
    big = sc.chain_regime_logits(np.random.RandomState(0), [1, 2, 2, 3], 30, 29, "confident")
    top2 = np.sort(big, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > 50).all() and (top2[:, 1] - top2[:, 0] < 110).all()


@pytest.mark.parametrize("regime", sc.CHAIN_REGIMES)
def test_loss_bound_covers_a_logq_off_by_its_bound(regime):
    """tests/test_ctc_long.py::test_loss_bound_covers_fp32_logq with the new term: the oracle on float64 logq against the oracle
    on a logq that is off by the step-1 bound in every entry -- all the same way (the worst case: every path's score moves by
    T times the bound) or with random signs -- and then rounded to fp32.  The relative term of the bound is left out."""
    logits, labels_list, input_len = sc.chain_batch_29(regime)
    rng = np.random.RandomState(5)
    for i, (label, t_b) in enumerate(zip(labels_list, input_len)):
        p = o.softmax(logits[i, :t_b].astype(np.float64))
        log_q = o.ctc_log_q(p[None], float(np.float32(1e-8)))[0]
        exact, _ = o.ctc_single(log_q, label, 28)
        assert np.isfinite(exact)
        bound = float(sc.loss_bound(0.0, t_b))
        assert bound == t_b * (1.2e-6 + 1e-5)
        for shift in (-sc.LOGQ_BOUND, sc.LOGQ_BOUND, sc.LOGQ_BOUND * rng.choice([-1.0, 1.0], size=log_q.shape)):
            moved, _ = o.ctc_single((log_q + shift).astype(np.float32).astype(np.float64), label, 28)
            assert abs(moved - exact) <= bound, (regime, i, t_b, exact, moved)
        worst, _ = o.ctc_single(log_q - sc.LOGQ_BOUND, label, 28)
        assert abs(worst - exact) >= 0.999 * t_b * sc.LOGQ_BOUND  # the new term is needed in full
