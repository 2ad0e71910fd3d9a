"""The output softmax against float64 computed FROM THE LOGITS (tests/softmax_cases.py has the cases, the bounds and their
derivation).  Every other CTC, ASG and alignment test feeds its oracle the kernel's own fp32 probabilities, which holds the
lattices tightly and the softmax not at all: an error in p = softmax(z) or log q = log_softmax(log(p + eps)) moves kernel and
oracle together.  Here: sl_softmax_logq alone, the chain sl_softmax_logq -> sl_ctc_loss_grad against the oracle run on the float64
logits, and the two fused kernels of sl_output_softmax on operands that make every logit an exactly known fp32 value.

Measured on an MI355X (the worst ratio of an error to its bound over the cases of this module):
  sl_softmax_logq (softmax_logq_kernel)      probs 0.582 (a second-tier class at d = 66.7: the rounding of z - m, as the
                                             restatement's 0.590); logq 0.338 at eps = 1e-8, 0.410 at 1e-7, 0.543 at 0;
                                             rows of probs sum to 1 within 2.4e-7; at worst 0.28 of the allowed k 2^-23
  sl_output_softmax, select 1 (LDS kernel)   logits bit for bit; probs 0.492, logq 0.285 (cin 64: 0.486 / 0.274, 256: 0.401 /
                                             0.285, 512: 0.492 / 0.283, 2048: 0.474 / 0.264)
  sl_output_softmax, select 0 (registers)    the same figures: with exact logits the shared tail gives both kernels' bytes
  the chain from the logits                  loss at most 0.025 of its bound, gradient within 2.2e-6 (0.022 of 1e-4)
Mutations tried on scratch builds of the library: `lane <= k` for `lane < k` in softmax_logq_kernel fails all 34 cases of
test_softmax_logq_against_float64_from_the_logits and test_one_frame_writes_k_values_and_nothing_behind_them with k < 64 (at
k = 64 it changes nothing); logf(e[i]) for logf(e[i] + eps) in output_softmax_finish fails 47 of the 48 cases of
test_output_softmax_on_exactly_known_logits (all but the one-frame case 64-2-1-1, whose only margin leaves p far above eps).
"""
import numpy as np
import pytest

import softmax_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _automatic_kernel_choice_afterwards(hip_lib):
    """sl_output_softmax_select is process-wide: whatever fails in here, the module leaves it at 0"""
    yield
    hip_lib.call("sl_output_softmax_select", 0)


def _ratios(run, logits, eps):
    return sc.worst_ratios(run.probs, run.logq, logits, eps)


# ------------------------------------------------------------------------------------------------------------ sl_softmax_logq
@pytest.mark.parametrize("name", sc.case_names())
def test_softmax_logq_against_float64_from_the_logits(hip_lib, name):
    case = sc.case_by_name(name)
    run = sc.run_softmax(hip_lib, case)
    k, n = case.k, case.batch * case.t_out * case.k
    p_ref, lq_ref = case.reference()
    rp, rq = _ratios(run, case.logits, case.eps)
    print("%s: probs %.3f of its bound, logq %.3f of its bound" % (name, rp, rq))
    assert np.isfinite(run.probs).all() and np.isfinite(run.logq).all()
    assert (np.abs(run.probs.astype(np.float64) - p_ref) <= sc.probs_bound(case.logits)).all(), rp
    assert (np.abs(run.logq.astype(np.float64) - lq_ref) <= sc.logq_bound(case.logits, case.eps)).all(), rq
    # the logits, their padding and the guard behind them: not a byte has changed; nothing is written behind the outputs
    assert run.logits_after.tobytes() == case.buffer().tobytes()
    assert (run.whole_probs[n:] == sc.FILL).all() and (run.whole_logq[n:] == sc.FILL).all()
    z = case.logits.reshape(-1, k)
    p, q = run.probs.reshape(-1, k), run.logq.reshape(-1, k)
    sums = p.astype(np.float64).sum(axis=1)
    print("row sums of probs: within %.3g of 1 (allowed %.3g)" % (np.abs(sums - 1).max(), k * 2.0 ** -23))
    assert (np.abs(sums - 1.0) <= k * 2.0 ** -23).all()
    assert np.array_equal(p.argmax(axis=1), z.argmax(axis=1))  # (numpy: the first of several maxima)
    assert sc.monotone_violations(z, p) == 0 and sc.monotone_violations(z, q) == 0
    again = sc.run_softmax(hip_lib, case)
    assert again.whole_probs.tobytes() == run.whole_probs.tobytes() and again.whole_logq.tobytes() == run.whole_logq.tobytes()


@pytest.mark.parametrize("k", sc.CLASS_COUNTS)
def test_one_frame_writes_k_values_and_nothing_behind_them(hip_lib, k):
    case = next(c for c in sc.all_cases() if c.k == k and c.batch * c.t_out == 1)
    run = sc.run_softmax(hip_lib, case)
    for whole in (run.whole_probs, run.whole_logq):
        assert whole.shape == (k + sc.GUARD,)
        assert (whole[:k] != sc.FILL).all() and (whole[k:] == sc.FILL).all()
    assert abs(float(run.probs.astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------ the chain
def _check_chain(hip_lib, logits, labels_list, input_len, what):
    ref_loss, ref_dl = sc.chain_reference(logits, labels_list, input_len)
    assert np.isfinite(ref_loss).all(), "the cases are meant to be feasible"
    loss, dl = sc.run_chain(hip_lib, logits, labels_list, input_len)
    bound = sc.loss_bound(ref_loss, input_len)
    for i, (lab, t_b) in enumerate(zip(labels_list, input_len)):
        e_loss, e_grad = abs(float(loss[i]) - ref_loss[i]), float(np.abs(dl[i] - ref_dl[i]).max())
        print("%s, utterance %d: %2d letters in %3d frames: loss %.9g (float64 %.9g): error %.2e = %.3f of its bound; gradient "
              "error %.2e = %.3f of its bound" % (what, i, len(lab), t_b, loss[i], ref_loss[i], e_loss, e_loss / bound[i],
                                                   e_grad, e_grad / sc.GRAD_BOUND))
    for i, t_b in enumerate(input_len):
        assert abs(float(loss[i]) - ref_loss[i]) <= bound[i], (i, loss[i], ref_loss[i], bound[i])
        assert np.abs(dl[i] - ref_dl[i]).max() <= sc.GRAD_BOUND, (i, np.abs(dl[i] - ref_dl[i]).max())
        assert not dl[i, t_b:].any(), (i, "rows at and beyond input_len must be exactly zero")


@pytest.mark.parametrize("regime", sc.CHAIN_REGIMES)
def test_ctc_from_the_logits_29_classes(hip_lib, regime):
    """the wave lattice: no letter, one, 12 and 40, each with no frame to spare and with some"""
    logits, labels_list, input_len = sc.chain_batch_29(regime)
    _check_chain(hip_lib, logits, labels_list, input_len, regime)


def test_ctc_from_the_logits_64_classes(hip_lib):
    """k = 64: the path through ctc_long.hip; every regime in one batch"""
    logits, labels_list, input_len = sc.chain_batch_64()
    _check_chain(hip_lib, logits, labels_list, input_len, "64 classes")


# ------------------------------------------------------------------------------------------------------------ the fused kernels
@pytest.mark.parametrize("cin,k,t_out,batch", sc.fused_shapes())
def test_output_softmax_on_exactly_known_logits(hip_lib, cin, k, t_out, batch):
    """select 1: the LDS kernel (cin 512 and 2048: its DMA weight path); select 0: the register kernel from cin = 256 on.  The
    optional logits output bit for bit, probs and logq to the bounds against float64 of those logits, with and without the
    logits output the same bytes, nothing written outside [0, t_out) x [0, k)."""
    case = sc.fused_case(cin, k, t_out, batch)
    n = batch * t_out * k
    p_ref, lq_ref = sc.reference(case.logits, sc.FUSED_EPS)
    bp, bq = sc.probs_bound(case.logits), sc.logq_bound(case.logits, sc.FUSED_EPS)
    runs = {}
    try:
        for select in (1, 0):
            hip_lib.call("sl_output_softmax_select", select)
            for want_logits in (True, False):
                runs[select, want_logits] = sc.run_output_softmax(hip_lib, case, want_logits)
    finally:
        hip_lib.call("sl_output_softmax_select", 0)
    for (select, want_logits), run in runs.items():
        what = (cin, k, t_out, batch, "select %d" % select, "logits" if want_logits else "no logits")
        assert run.whole_logits.tobytes() == sc.expected_logits_buffer(case, want_logits).tobytes(), what
        rp, rq = _ratios(run, case.logits, sc.FUSED_EPS)
        print("%s: probs %.3f of its bound, logq %.3f of its bound" % (what, rp, rq))
        assert (np.abs(run.probs.astype(np.float64) - p_ref) <= bp).all(), (what, rp)
        assert (np.abs(run.logq.astype(np.float64) - lq_ref) <= bq).all(), (what, rq)
        assert (run.whole_probs[n:] == sc.FILL).all() and (run.whole_logq[n:] == sc.FILL).all(), what
        assert (run.whole_probs[:n] != sc.FILL).all() and (run.whole_logq[:n] != sc.FILL).all(), what
    for select in (1, 0):
        a, b = runs[select, True], runs[select, False]
        assert a.whole_probs.tobytes() == b.whole_probs.tobytes() and a.whole_logq.tobytes() == b.whole_logq.tobytes(), select
    lds, reg = runs[1, True], runs[0, True]
    assert (np.abs(lds.probs.astype(np.float64) - reg.probs) <= 2 * bp).all()
    assert (np.abs(lds.logq.astype(np.float64) - reg.logq) <= 2 * bq).all()
