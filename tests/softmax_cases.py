"""Shared helpers of tests/test_softmax_cases.py (CPU) and tests/test_gpu_softmax.py (GPU): the cases that hold the output softmax
-- sl_softmax_logq and the fused tail of sl_output_softmax -- to float64 computed FROM THE LOGITS, the bounds, and a float32
restatement of the kernels' arithmetic that shows the bounds are neither vacuous nor too tight.  Not a test module.

Reference.  oracle.w2l_oracle.softmax and ctc_log_q in float64 on the fp32 logits cast to float64; eps reaches the kernels as a
float, so the reference is given float(np.float32(eps)).

Bounds, per entry, with d_i = max_j z_j - z_i (fp32 rounding model of the kernels' arithmetic, u = 2^-24 = half an ulp):

  probs   |p - p*| <= p* (d_i + 40) u + 2^-148
          z - m is rounded once (d u relative in exp); expf is good to 1 ulp (2 u); the sum's error is the p-weighted mean of its
          terms' errors, at most 63 max_d(d e^-d) u = 23 u; six butterfly additions (6 u; the fused tail's seven serial and two
          butterfly additions act on at most 32 terms and stay below that too); one division (1 u): d + 32 <= d + 40.  The
          absolute term is the fp32 denormals: expf's result below 2^-126 has an absolute error of an ulp of 2^-149, the division
          by a sum >= 1 adds half of one, and below 2^-150 the result is 0.
          The d u term is unlike the others: it is no allowance for a worst case that rarely happens but the size of one known
          rounding.  r_i = |fl32(z_i - m) - (z_i - m)| (input_rounding; exact in float64) is half an ulp of d at worst, which
          is between d u / 2 and d u -- just above a power of two, d = 64.1 say, it is 0.998 d u -- and exp turns it into the
          relative error r_i of e_i in full.  Any fp32 evaluation of expf(z - m), this module's restatement included, therefore
          comes as close as (0.96 d + 3) / (d + 40) = 0.63 to the bound at d = 67 (measured: 0.59), and "within half of the
          bound" cannot hold for 34 < d < 128 however exact the rest is.  The half that shows the bound is not too tight is
          asked of everything else: the restatement stays within p* r_i + HALF of (40 p* u + 2^-148) on every entry (measured:
          a quarter), within half of the whole bound wherever d <= 32, and within the whole bound everywhere.
  logq at eps >= 1e-8   |logq - logq*| <= 1e-5
          u = logf(p + eps) has |u| <= 18.5: 1 ulp = 1.9e-6; the error of p reaches u damped by p / (p + eps), worst near
          d = 15 at 3.3e-6; the normaliser lz (the p-weighted mean of the errors of u, the butterfly, logf of a sum in [1, 64],
          one addition) 2.5e-6; the final subtraction half an ulp of 18.5 = 1.1e-6.  Sum 8.8e-6.
  logq at eps = 0       |logq - logq*| <= 3 |logq*| u + (d_i + 40) u + 3.7e-6, cases with d <= 60 only
          (logq_bound_eps0) the same four terms with nothing damping them.  u = logf(p) has |u| <= |logq*| + |lz| where lz, the
          log of a sum of probabilities, is within 1e-5 of 0: logf's ulp is |logq*| 2^-23 = 2 |logq*| u and the final subtraction's
          half ulp |logq*| u; the relative error of p, (d + 40) u, is the absolute error of its logarithm; lz carries the p-weighted
          mean of that, at most (40 + max_d d e^-d ...) u = 2.5e-6, plus the rounding of u - um (below 1e-7 once weighted),
          six butterfly additions (3.6e-7), logf of a sum in [1, 64] (an ulp of 4.16: 4.8e-7) and the addition (2.4e-7): 3.7e-6.
          With |logq*| <= 60 + log k <= 64.16 this is at most 1.15e-5 + 5.96e-6 + 3.7e-6 = 2.1e-5, and 3.9e-6 at d = 0, k = 2.

Restatement (restate_f32): numpy, the kernels' operations in the kernels' order, every intermediate stored as np.float32 -- max by
butterfly (xor 32, 16, .. 1), expf(z - m), sum by butterfly, division, logf(p + eps), max and sum by butterfly again, um +
logf(usum), u - lz.  expf and logf are the float64 functions rounded once to float32.  order="fused" is output_softmax_finish's
order for k <= 32: a lane's eight classes (16 j + 4 g + r) summed serially, then the butterfly over the four lanes of a row.

Cases (all_cases): class counts at both sides of the lane edges; top-1 margins 0 (a tie of exactly two classes, and of all k),
1e-3, 15, 17, 18.4 (p = eps), 30, 87, 88, 104 (fp32 exp reaches its denormals and 0), 200, 1e4, the other classes spread between
a margin and the next one ("tier") or placed on the larger margins in turn ("ladder"); uniform rows; rows moved by +-1e4 as a
whole; B T of 1, 5, 7 and 4 n + 3 frames (the launch takes four frames per work-group); dense logits, or rows of k + 3 columns
in utterances 5 elements further apart than their rows need, every element that is no logit holding 3e38.
"""
import functools
import sys
from pathlib import Path

import numpy as np

from oracle import w2l_oracle as o

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
from fuzz_ctc import regime_logits as fuzz_regime_logits  # noqa: E402

FILL = 7.5                 # what every output holds before a call: an entry the kernel does not write shows
PAD = np.float32(3e38)     # what every element of a logits buffer that is no logit holds
GUARD = 64                 # elements behind every buffer, FILL / PAD as well
MAX_FRAMES = 2000
CLASS_COUNTS = (2, 5, 29, 32, 33, 63, 64)
MARGINS = (0.0, 1e-3, 15.0, 17.0, 18.4, 30.0, 87.0, 88.0, 104.0, 200.0, 1e4)
EPS_VALUES = (1e-8, 1e-7, 0.0)
EPS0_MAX_D = 60.0          # eps = 0: log q* = -d - log sum: cases are kept to d <= 60
U = 2.0 ** -24
PROBS_CONST = 40.0
PROBS_ABS = 2.0 ** -148
LOGQ_BOUND = 1e-5          # eps >= 1e-8
LOGQ_EPS0_LZ = 3.7e-6
LOSS_PER_FRAME = 1.2e-6    # the absolute term per frame the CTC tests allow for logq rounded to fp32 (tests/test_ctc_long.py)
GRAD_BOUND = 1e-4          # per entry, times grad_scale: the project's gradient bound


# ------------------------------------------------------------------------------------------------------------ reference, bounds
def reference(logits, eps):
    """(p*, logq*) in float64 from fp32 logits (..., k)"""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    p = o.softmax(z)
    return p, o.ctc_log_q(p, float(np.float32(eps)))


def distances(logits):
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    return z.max(axis=-1, keepdims=True) - z


def probs_bound(logits):
    p, _ = reference(logits, 1e-8)
    return p * (distances(logits) + PROBS_CONST) * U + PROBS_ABS


def input_rounding(logits):
    """r_i = |fl32(z_i - m) - (z_i - m)|: the one rounding of the kernels whose size is known (module docstring), float64"""
    z = np.asarray(logits, dtype=np.float32)
    m = z.max(axis=-1, keepdims=True)
    return np.abs((z - m).astype(np.float64) - (z.astype(np.float64) - m.astype(np.float64)))


def probs_slack(logits):
    """the probs bound without its d u term: p* 40 u + 2^-148"""
    p, _ = reference(logits, 1e-8)
    return p * PROBS_CONST * U + PROBS_ABS


def logq_bound_eps0(logits):
    d = distances(logits)
    if d.max() > EPS0_MAX_D:
        raise ValueError("eps = 0: a case must keep d <= {} (it has {})".format(EPS0_MAX_D, d.max()))
    _, lq = reference(logits, 0.0)
    return 3.0 * np.abs(lq) * U + (d + PROBS_CONST) * U + LOGQ_EPS0_LZ


def logq_bound(logits, eps):
    """per entry; eps >= 1e-8: the constant 1e-5; eps = 0: logq_bound_eps0; nothing in between has a derivation"""
    if eps == 0.0:
        return logq_bound_eps0(logits)
    if eps < 1e-8:
        raise ValueError("no bound is derived for 0 < eps < 1e-8")
    return np.full(np.asarray(logits).shape, LOGQ_BOUND)


def worst_ratios(probs, logq, logits, eps):
    """(largest |p - p*| / bound, largest |logq - logq*| / bound) over the entries"""
    p, lq = reference(logits, eps)
    rp = np.abs(probs.astype(np.float64) - p) / probs_bound(logits)
    rq = np.abs(logq.astype(np.float64) - lq) / logq_bound(logits, eps)
    return float(rp.max()), float(rq.max())


def loss_bound(ref_loss, frames):
    """the chain from the logits: 1e-5 |ref| + T_b (1.2e-6 + the logq bound)"""
    return 1e-5 * np.abs(ref_loss) + np.asarray(frames, dtype=np.float64) * (LOSS_PER_FRAME + LOGQ_BOUND)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _exp32(x):
    return np.exp(x.astype(np.float64)).astype(np.float32)


def _log32(x):
    with np.errstate(divide="ignore"):
        return np.log(x.astype(np.float64)).astype(np.float32)


def _butterfly(v, op, offsets):
    lanes = np.arange(v.shape[-1])
    for off in offsets:
        v = op(v, v[..., lanes ^ off])
        assert v.dtype == np.float32
    return v


def restate_f32(logits, eps, order="wave"):
    """(probs, logq) as float32 by the kernels' operations in the kernels' order (module docstring); logits (..., k)"""
    z = np.asarray(logits, dtype=np.float32)
    lead, k = z.shape[:-1], z.shape[-1]
    z = z.reshape(-1, k)
    eps = np.float32(eps)
    ninf = np.float32(-np.inf)
    if order == "wave":
        width, offsets = 64, (32, 16, 8, 4, 2, 1)
        cls = np.arange(64)
    elif order == "fused":
        assert k <= 32
        width, offsets = 4, (1, 2)  # lane ^ 16, lane ^ 32: the group index g ^ 1, g ^ 2
        g, i = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
        cls = ((i // 4) * 16 + 4 * g + (i % 4))  # [g][i]: class 16 j + 4 g + r, i = 4 j + r
    else:
        raise ValueError(order)
    on = cls < k
    zz = np.full((z.shape[0],) + cls.shape, ninf, dtype=np.float32)
    zz[:, on] = z[:, cls[on]]

    def reduce(v, op):
        if order == "fused":  # a lane's eight values serially, first to last, from the identity the kernel starts with
            acc = np.full(v.shape[:2], ninf if op is np.maximum else 0.0, dtype=np.float32)
            for j in range(8):
                acc = op(acc, v[:, :, j])
            v = acc
        out = _butterfly(v, op, offsets)
        return out[:, :1] if order == "wave" else out[:, :1, None]

    with np.errstate(invalid="ignore"):
        m = reduce(zz, np.maximum)
        e = np.where(on, _exp32(zz - m), np.float32(0.0)).astype(np.float32)
        s = reduce(e, np.add)
        p = (e / s).astype(np.float32)
        u = np.where(on, _log32(p + eps), ninf).astype(np.float32)
        um = reduce(u, np.maximum)
        usum = reduce(np.where(on, _exp32(u - um), np.float32(0.0)).astype(np.float32), np.add)
        lz = (um + _log32(usum)).astype(np.float32)
        lq = (u - lz).astype(np.float32)
    probs = np.zeros((z.shape[0], k), dtype=np.float32)
    logq = np.zeros((z.shape[0], k), dtype=np.float32)
    probs[:, cls[on]] = p[:, on]
    logq[:, cls[on]] = lq[:, on]
    return probs.reshape(lead + (k,)), logq.reshape(lead + (k,))


# ------------------------------------------------------------------------------------------------------------ generators
def margin_rows(rng, k, max_d=None):
    """(rows (n, k) float32, [(margin, layout)] per row).  For every margin M of MARGINS (up to max_d), layouts "tier" and
    "ladder" twice each: the top class holds base ~ uniform(-3, 3), one other class base - M, the rest base - d with d uniform
    between M and the next margin (tier) or on the margins >= M in turn (ladder); the top class is class 0, class k - 1 or any.
    max_d caps every d (a hundredth below it, so that a later common offset's rounding stays inside)."""
    cap = None if max_d is None else max_d - 0.01
    margins = [m for m in MARGINS if cap is None or m <= cap]
    rows, tags = [], []
    n = 0
    for mi, m in enumerate(margins):
        nxt = margins[mi + 1] if mi + 1 < len(margins) else (1.2 * m + 1.0 if cap is None else cap)
        for layout in ("tier", "ladder"):
            for _ in range(2):
                top = (0, k - 1, int(rng.randint(0, k)))[n % 3]
                n += 1
                others = [c for c in range(k) if c != top]
                second = others[int(rng.randint(0, len(others)))]
                base = np.float32(rng.uniform(-3, 3))
                if layout == "tier":
                    d = rng.uniform(m, nxt, size=k)
                    if m == 0.0:  # an exact tie of two classes only: nobody else within half a margin step
                        d = rng.uniform(0.5 * nxt, nxt, size=k)
                else:
                    ladder = [x for x in margins if x >= m and x > 0.0]
                    d = np.array([ladder[(j + n) % len(ladder)] for j in range(k)], dtype=np.float64)
                d[second] = m
                d[top] = 0.0
                rows.append((base - d.astype(np.float32)).astype(np.float32))
                tags.append((m, layout))
    return np.stack(rows), tags


def uniform_rows(rng, k):
    """a row of zeros and a row of one random value: an exact tie of all k classes"""
    return np.stack([np.zeros(k, dtype=np.float32), np.full(k, np.float32(rng.uniform(-30, 30)), dtype=np.float32)])


def offset_rows(rows, tags):
    """one row per margin moved by +1e4 and one by -1e4 as a whole (fp32 additions: at 1e4 an ulp is 2^-10)"""
    seen, out = set(), []
    for row, (m, layout) in zip(rows, tags):
        if layout == "tier" and m not in seen:
            seen.add(m)
            out.append((row + np.float32(1e4)).astype(np.float32))
            out.append((row - np.float32(1e4)).astype(np.float32))
    return np.stack(out)


def random_rows(rng, n, k, scale):
    return (rng.randn(n, k) * scale).astype(np.float32)


class SoftmaxCase:
    """logits (B, T, k) float32; padded: rows of k + 3 columns, utterances T (k + 3) + 5 elements apart"""

    def __init__(self, name, logits, eps, padded):
        self.name, self.logits, self.eps, self.padded = name, np.ascontiguousarray(logits, dtype=np.float32), float(eps), padded
        self.batch, self.t_out, self.k = self.logits.shape
        assert self.batch * self.t_out <= MAX_FRAMES and np.isfinite(self.logits).all()
        self.logit_stride = self.k + 3 if padded else self.k
        self.batch_stride = self.t_out * self.logit_stride + (5 if padded else 0)
        self._ref = None

    def reference(self):
        if self._ref is None:
            p, lq = reference(self.logits, self.eps)
            p.setflags(write=False)
            lq.setflags(write=False)
            self._ref = (p, lq)
        return self._ref

    def buffer(self):
        """the logits as the kernel gets them: float32 (B * batch_stride + GUARD,), PAD wherever there is no logit"""
        buf = np.full(self.batch * self.batch_stride + GUARD, PAD, dtype=np.float32)
        for b in range(self.batch):
            rows = buf[b * self.batch_stride: b * self.batch_stride + self.t_out * self.logit_stride]
            rows.reshape(self.t_out, self.logit_stride)[:, :self.k] = self.logits[b]
        return buf

    def __repr__(self):
        return self.name


def _shaped(rng, rows, k, batch, scale=3.0):
    """rows in a random order as (batch, T, k) with batch * T = 4 n + 3 >= len(rows), the rest N(0, scale) rows"""
    t = -(-len(rows) // batch)
    while (batch * t) % 4 != 3:
        t += 1
    extra = batch * t - len(rows)
    if extra:
        rows = np.concatenate([rows, random_rows(rng, extra, k, scale)])
    return rows[rng.permutation(len(rows))].reshape(batch, t, k)


def margin_case(k, eps, padded, seed):
    rng = np.random.RandomState(seed)
    rows, tags = margin_rows(rng, k, EPS0_MAX_D if eps == 0.0 else None)
    rows = np.concatenate([rows, uniform_rows(rng, k), offset_rows(rows, tags)])
    return SoftmaxCase("margins_k{}_eps{:g}_{}".format(k, eps, "padded" if padded else "dense"), _shaped(rng, rows, k, 3), eps,
                       padded)


def small_case(k, batch, t_out, eps, padded, seed):
    """B T of 1, 5 or 7 frames drawn from the margin rows (one of them the row of margin 18.4, p = eps)"""
    rng = np.random.RandomState(seed)
    rows, tags = margin_rows(rng, k, EPS0_MAX_D if eps == 0.0 else None)
    first = tags.index((18.4, "tier"))
    pick = [first] + list(rng.choice(len(rows), size=batch * t_out - 1, replace=False))
    return SoftmaxCase("frames_{}x{}_k{}_eps{:g}_{}".format(batch, t_out, k, eps, "padded" if padded else "dense"),
                       rows[pick].reshape(batch, t_out, k), eps, padded)


def many_blocks_case(k, eps, padded, seed):
    """3 x 333 = 999 = 4 * 249 + 3 frames of N(0, 8) logits: 250 work-groups, the last with three frames"""
    rng = np.random.RandomState(seed)
    return SoftmaxCase("blocks_999_k{}_eps{:g}_{}".format(k, eps, "padded" if padded else "dense"),
                       random_rows(rng, 999, k, 8.0).reshape(3, 333, k), eps, padded)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every case of the CPU and the GPU module, built once"""
    cases = []
    for ki, k in enumerate(CLASS_COUNTS):
        for ei, eps in enumerate(EPS_VALUES):
            cases.append(margin_case(k, eps, padded=(ei + ki) % 2 == 0, seed=1000 + 10 * k + ei))
    for ki, k in enumerate(CLASS_COUNTS):  # one frame: the whole launch is one wave of a work-group of four
        cases.append(small_case(k, 1, 1, EPS_VALUES[ki % 3], padded=ki % 2 == 1, seed=2000 + k))
    cases.append(small_case(33, 1, 5, 1e-8, True, 2101))
    cases.append(small_case(64, 5, 1, 1e-7, True, 2102))
    cases.append(small_case(29, 1, 7, 0.0, False, 2103))
    cases.append(small_case(2, 7, 1, 1e-8, True, 2104))
    cases.append(many_blocks_case(29, 1e-8, False, 2201))
    cases.append(many_blocks_case(64, 1e-7, True, 2202))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case_names():
    return [c.name for c in all_cases()]


def case_by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------------------ sl_softmax_logq
class SoftmaxRun:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_softmax(hip_lib, case):
    """sl_softmax_logq on case.buffer(); outputs of B T k + GUARD elements that start as FILL.  Everything comes back as numpy:
    probs / logq (B, T, k), the whole output buffers, and the logits buffer after the call."""
    import torch
    dev = "cuda:0"
    n = case.batch * case.t_out * case.k
    lg = torch.tensor(case.buffer(), dtype=torch.float32, device=dev)
    probs = torch.full((n + GUARD,), FILL, dtype=torch.float32, device=dev)
    logq = torch.full((n + GUARD,), FILL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), case.batch, case.t_out, case.k,
                 case.logit_stride, case.batch_stride, case.eps, st)
    torch.cuda.synchronize()
    whole_p, whole_q = probs.cpu().numpy(), logq.cpu().numpy()
    shape = (case.batch, case.t_out, case.k)
    return SoftmaxRun(probs=whole_p[:n].reshape(shape), logq=whole_q[:n].reshape(shape), whole_probs=whole_p, whole_logq=whole_q,
                      logits_after=lg.cpu().numpy())


def monotone_violations(z, v):
    """rows (n, k): the number of class pairs adjacent in the order of z with z_i >= z_j but v_i < v_j (equal z: either way)"""
    order = np.argsort(z, axis=-1, kind="stable")
    zs = np.take_along_axis(z, order, axis=-1)
    vs = np.take_along_axis(v, order, axis=-1)
    dz, dv = np.diff(zs, axis=-1), np.diff(vs, axis=-1)
    return int(((dv < 0) | ((dz == 0) & (dv != 0))).sum())


# ------------------------------------------------------------------------------------------------------------ the chain
CHAIN_REGIMES = ("sharp", "collapse", "learnt", "wrong", "confident")
# (letters, slack): no letter, one, 12 and 40, with no frame to spare and with some
CHAIN_SPECS_29 = ((0, 0), (0, 30), (1, 0), (1, 50), (12, 0), (12, 40), (40, 0), (40, 60))
CHAIN_SPECS_64 = ((0, 5, "collapse"), (1, 0, "sharp"), (12, 0, "learnt"), (12, 30, "confident"), (40, 0, "wrong"),
                  (40, 35, "confident"), (25, 20, "learnt"), (30, 11, "sharp"))


def chain_regime_logits(rng, label, t, k, kind):
    """tools/fuzz_ctc.regime_logits for its regimes; "confident": its "learnt" layout (one frame per symbol of the label with a
    blank between repeats, the frames in between held with blank) at a strength drawn from uniform(60, 100)"""
    if kind != "confident":
        return fuzz_regime_logits(rng, label, t, k, kind)
    lg = rng.randn(t, k).astype(np.float32)
    seq = []
    for j, c in enumerate(label):
        if j and c == label[j - 1]:
            seq.append(k - 1)
        seq.append(int(c))
    strength = np.float32(rng.uniform(60, 100))
    if len(seq) and len(seq) <= t:
        cuts = np.sort(rng.choice(np.arange(1, t), size=len(seq) - 1, replace=False)) if len(seq) > 1 else np.array([], int)
        bounds = np.concatenate([[0], cuts, [t]]).astype(int)
        for j, sym in enumerate(seq):
            lg[bounds[j], sym] += strength
            lg[bounds[j] + 1:bounds[j + 1], k - 1] += strength
    else:
        lg[:, k - 1] += strength
    return lg


def chain_batch(rng, k, specs):
    """specs [(letters, slack, regime)] -> (logits (B, T, k) with zero rows past T_b, labels_list, input_len): T_b is the fewest
    frames the label fits (its letters plus one per adjacent repeat, at least one) plus slack"""
    labels_list = [[int(c) for c in rng.randint(0, k - 1, size=n)] for n, _, _ in specs]
    input_len = [max(len(lab) + sum(1 for a, c in zip(lab, lab[1:]) if a == c), 1) + slack
                 for lab, (_, slack, _) in zip(labels_list, specs)]
    logits = np.zeros((len(specs), max(input_len), k), dtype=np.float32)
    for i, (lab, t_b, (_, _, regime)) in enumerate(zip(labels_list, input_len, specs)):
        logits[i, :t_b] = chain_regime_logits(rng, lab, t_b, k, regime)
    return logits, labels_list, input_len


def chain_batch_29(regime):
    rng = np.random.RandomState(2900 + CHAIN_REGIMES.index(regime))
    out = chain_batch(rng, 29, [(n, slack, regime) for n, slack in CHAIN_SPECS_29])
    assert out[0].shape[1] <= 120
    return out


def chain_batch_64():
    out = chain_batch(np.random.RandomState(6400), 64, CHAIN_SPECS_64)
    assert out[0].shape[1] <= 80
    return out


def chain_reference(logits, labels_list, input_len):
    """float64 from the logits: softmax, ctc_batch_cost, softmax_backward -> (loss (B,), dlogits (B, T, k))"""
    labels = o.pack_label_batch([lab if lab else [-1] for lab in labels_list])
    p = o.softmax(logits.astype(np.float64))
    loss, dp = o.ctc_batch_cost(p, labels, input_len, [len(lab) for lab in labels_list])
    return loss, o.softmax_backward(p, dp)


def run_chain(hip_lib, logits, labels_list, input_len, eps=1e-8):
    """sl_softmax_logq, then sl_ctc_loss_grad (grad_scale 1, fp32 destination without halo); loss and gradient start as FILL"""
    import torch
    from speechless_amd import _lib
    b, t, k = logits.shape
    dev = "cuda:0"
    labels = o.pack_label_batch([lab if lab else [-1] for lab in labels_list])
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.full((b, t, k), FILL, dtype=torch.float32, device=dev)
    logq = torch.full((b, t, k), FILL, dtype=torch.float32, device=dev)
    lab = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor([len(x) for x in labels_list], dtype=torch.int32, device=dev)
    il = torch.tensor(list(input_len), dtype=torch.int32, device=dev)
    loss = torch.full((b,), FILL, dtype=torch.float32, device=dev)
    dl = torch.full((b, t, k), FILL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, k, k, t * k, eps, st)
    need = hip_lib.raw("sl_ctc_workspace_bytes")(b, t, labels.shape[1])
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_ctc_loss_grad", probs.data_ptr(), logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(),
                 loss.data_ptr(), dl.data_ptr(), b, t, k, labels.shape[1], 0, k, t * k, _lib.SL_F32, eps, 1.0, ws.data_ptr(), need,
                 st)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), dl.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the fused kernels
# sl_output_softmax with logits that are known exactly.  Every operand is bf16-exact; every product is a multiple of 2^-10 and
# every partial sum stays below 2^13, so the fp32 accumulators hold it exactly in any order (tests/exact_ints.py, the bit-budget
# argument, with the unit 2^-10 in place of 1), and so is acc + bias.  Channels, at random positions of the cin:
#   nine PATTERN channels, one per integer margin M: the weights over the classes are a logit row -- the top class s, one class
#     s - M, the others s - M - (0 .. 40), |s| <= 10;
#   the FRACTION channel: weight 0 for the top class the patterns of M = 0 and M = 18 share, -1 for every other class;
#   the BIAS channel: weight -bias[c] (the biases are multiples of 2^-10 below 1/4 in magnitude, bf16-exact);
#   every other channel: weights in -3 .. 3.
# Frames, in turn: one pattern channel at 1 and the bias channel at 1 -- the logits are the pattern, the margin M; the pattern of
# M = 0 plus the fraction channel at 2^-10 (the margin the issue calls 1e-3); the pattern of M = 18 plus the fraction channel at
# 205 * 2^-9 (18.400390625); and dense frames: every ordinary channel in {-1, 0, 1}, the bias channel at 0, 1 or 2, in some a
# pattern channel on top.
FUSED_INT_MARGINS = (0, 15, 17, 18, 30, 87, 88, 104, 200)
FUSED_UNIT = 2.0 ** -10
FUSED_MARGINS = tuple(float(m) for m in FUSED_INT_MARGINS) + (FUSED_UNIT, 18 + 205 * 2.0 ** -9)
FUSED_CIN = (64, 256, 512, 2048)
FUSED_K = (2, 5, 16, 17, 29, 32)
FUSED_FRAMES = ((1, 1), (63, 1), (77, 1), (130, 1), (1, 3), (63, 3), (77, 3), (130, 3))  # (t_out, batch)
FUSED_EPS = 1e-8
FUSED_TYPES = len(FUSED_INT_MARGINS) + 2 + 5  # frame kinds in a cycle: the patterns, the two fractions, five dense ones
BIG_BF16 = 1e30  # what the operand elements the kernels must not use hold


def fused_shapes():
    """[(cin, k, t_out, batch)]: every (cin, k) pair with two of the eight (t_out, batch), so that every cin and every k meets
    all eight"""
    out = []
    for ci, cin in enumerate(FUSED_CIN):
        for ki, k in enumerate(FUSED_K):
            for shift in (0, 4):
                t_out, batch = FUSED_FRAMES[(ci + ki + shift) % 8]
                out.append((cin, k, t_out, batch))
    return out


class FusedCase:
    """x (B, t_out, cin), w (k, cin), bias (k,) as float64 holding bf16-exact values (bias: multiples of 2^-10); logits
    (B, t_out, k) float32: the exact result; kinds (B, t_out): the frame kind (index into the cycle of FUSED_TYPES)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def fused_case(cin, k, t_out, batch):
    rng = np.random.RandomState(cin * 1000 + k * 10 + t_out + batch)
    n_pat = len(FUSED_INT_MARGINS)
    ctrl = rng.choice(cin, size=n_pat + 2, replace=False)
    pat, frac_ch, bias_ch = ctrl[:n_pat], int(ctrl[n_pat]), int(ctrl[n_pat + 1])
    ordinary = np.setdiff1d(np.arange(cin), ctrl)
    w = np.zeros((k, cin), dtype=np.float64)
    w[:, ordinary] = rng.randint(-3, 4, size=(k, len(ordinary)))
    shared_top = int(rng.randint(0, k))
    for i, m in enumerate(FUSED_INT_MARGINS):
        top = shared_top if m in (0, 18) else (0, k - 1, int(rng.randint(0, k)))[i % 3]
        others = [c for c in range(k) if c != top]
        second = others[int(rng.randint(0, len(others)))]
        s = int(rng.randint(-10, 11))
        row = s - m - rng.randint(0, 41, size=k)
        row[second] = s - m
        row[top] = s
        w[:, pat[i]] = row
    w[:, frac_ch] = -1.0
    w[shared_top, frac_ch] = 0.0
    bias = rng.randint(-255, 256, size=k) * FUSED_UNIT
    w[:, bias_ch] = -bias
    x = np.zeros((batch, t_out, cin), dtype=np.float64)
    kinds = np.zeros((batch, t_out), dtype=np.int64)
    start = int(rng.randint(0, FUSED_TYPES))
    for b in range(batch):
        for t in range(t_out):
            kind = (start + b * t_out + t) % FUSED_TYPES
            kinds[b, t] = kind
            if kind < n_pat:
                x[b, t, pat[kind]] = 1.0
                x[b, t, bias_ch] = 1.0
            elif kind == n_pat:
                x[b, t, pat[FUSED_INT_MARGINS.index(0)]] = 1.0
                x[b, t, frac_ch] = FUSED_UNIT
                x[b, t, bias_ch] = 1.0
            elif kind == n_pat + 1:
                x[b, t, pat[FUSED_INT_MARGINS.index(18)]] = 1.0
                x[b, t, frac_ch] = 205 * 2.0 ** -9
                x[b, t, bias_ch] = 1.0
            else:
                x[b, t, ordinary] = rng.randint(-1, 2, size=len(ordinary))
                x[b, t, bias_ch] = float(rng.randint(0, 3))
                if kind % 2 == 0:
                    x[b, t, pat[int(rng.randint(0, n_pat))]] = 1.0
    exact = x @ w.T + bias
    logits = exact.astype(np.float32)
    assert np.array_equal(logits.astype(np.float64), exact)
    for a in (x, w, bias, logits):
        a.setflags(write=False)
    return FusedCase(cin=cin, k=k, t_out=t_out, batch=batch, x=x, w=w, bias=bias, logits=logits, kinds=kinds, frac_ch=frac_ch,
                     bias_ch=bias_ch, pattern_chs=pat)


def fused_accumulator_bound(case):
    """the largest sum of |x| |w| (+ |bias|) over the outputs: what bounds every partial sum of any summation order"""
    return float((np.abs(case.x) @ np.abs(case.w).T + np.abs(case.bias)).max())


def run_output_softmax(hip_lib, case, want_logits, eps=FUSED_EPS):
    """sl_output_softmax on a FusedCase under whatever sl_output_softmax_select holds.  x: rows of cin + 8 elements, 64 t_tiles
    rows per utterance (the kernels read whole tiles of 64 rows); w: 32 rows of cin.  Every element of x and w that the result
    must not depend on -- the 8 columns of padding, the rows past t_out, the weight rows >= k -- holds 1e30.  probs / logq:
    B t_out k + GUARD elements, the optional logits rows of k + 3 columns in utterances t_out (k + 3) + 5 apart + GUARD, all
    FILL before the call.  Returns a SoftmaxRun with the whole buffers."""
    import ctypes
    import torch
    from speechless_amd import _lib
    dev = "cuda:0"
    b, t, cin, k = case.batch, case.t_out, case.cin, case.k
    rows, x_rs = (t + 63) // 64 * 64, cin + 8
    xh = torch.full((b, rows, x_rs), BIG_BF16, dtype=torch.float32)
    xh[:, :t, :cin] = torch.from_numpy(np.array(case.x)).to(torch.float32)
    wh = torch.full((32, cin), BIG_BF16, dtype=torch.float32)
    wh[:k] = torch.from_numpy(np.array(case.w)).to(torch.float32)
    x = xh.to(torch.bfloat16).to(dev)
    w = wh.to(torch.bfloat16).to(dev)
    bias = torch.tensor(np.array(case.bias), dtype=torch.float32, device=dev)
    geom = _lib.ConvGeom(batch=b, t_out=t, taps=1, cin=cin, cout=32, x_row0=0, x_row_stride=x_rs, x_batch_stride=rows * x_rs,
                         y_row0=0, y_row_stride=32, y_batch_stride=rows * 32, acc_scale=0.0)
    assert hip_lib.raw("sl_output_softmax_supported")(ctypes.byref(geom), k, _lib.SL_BF16) == 1
    n = b * t * k
    probs = torch.full((n + GUARD,), FILL, dtype=torch.float32, device=dev)
    logq = torch.full((n + GUARD,), FILL, dtype=torch.float32, device=dev)
    ls, lbs = k + 3, t * (k + 3) + 5
    logits = torch.full((b * lbs + GUARD,), FILL, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.call("sl_output_softmax", x.data_ptr(), w.data_ptr(), bias.data_ptr(), probs.data_ptr(), logq.data_ptr(),
                 logits.data_ptr() if want_logits else None, ctypes.byref(geom), k, ls, lbs, eps, _lib.SL_BF16, st)
    torch.cuda.synchronize()
    whole_p, whole_q = probs.cpu().numpy(), logq.cpu().numpy()
    return SoftmaxRun(probs=whole_p[:n].reshape(b, t, k), logq=whole_q[:n].reshape(b, t, k), whole_probs=whole_p,
                      whole_logq=whole_q, whole_logits=logits.cpu().numpy(), logit_stride=ls, logit_batch_stride=lbs)


def expected_logits_buffer(case, written):
    """the whole optional logits buffer after a call: FILL everywhere (written=False: a call with NULL), else the exact logits in
    the first k columns of the first t_out rows of every utterance"""
    ls, lbs = case.k + 3, case.t_out * (case.k + 3) + 5
    buf = np.full(case.batch * lbs + GUARD, FILL, dtype=np.float32)
    if written:
        for b in range(case.batch):
            buf[b * lbs: b * lbs + case.t_out * ls].reshape(case.t_out, ls)[:, :case.k] = case.logits[b]
    return buf
