"""Float64 numpy restatement of sl_asg_segment_scores (include/speechless_hip.h), clamps included, and the brute-force sum over
all frame labelings that the restatement itself is checked against (tests/test_asg_segment.py)."""
import itertools

import numpy as np

from ctc_segment_ref import clamped_segment


def _lse(x, axis=0):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def forward_score(e, g, s, graphemes):
    """N - Z of the header over ALL the rows of e (T, k), float64: g (k, k) [from][to], s (k,) the start scores, graphemes
    already clamped into [0, k).  The edge rules of the header: L = 0 and T = 0 give 0, L = 0 or T < L give -inf, N = -inf or
    Z = -inf give -inf."""
    e = np.asarray(e, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    t_n, n = e.shape[0], len(graphemes)
    if n == 0:
        return 0.0 if t_n == 0 else -np.inf
    if t_n < n:
        return -np.inf
    lab = np.asarray(graphemes, dtype=np.int64)
    gs, ga = g[lab, lab], g[lab[:-1], lab[1:]]
    ninf = np.array([-np.inf])
    with np.errstate(invalid="ignore"):
        a = np.full(n, -np.inf)
        a[0] = s[lab[0]] + e[0, lab[0]]
        d = s + e[0]
        for t in range(1, t_n):
            a = e[t, lab] + np.logaddexp(a + gs, np.concatenate([ninf, a[:-1] + ga]))
            d = e[t] + _lse(d[:, None] + g, 0)
        num, z = a[-1], _lse(d, 0)
    if num == -np.inf or z == -np.inf:
        return -np.inf
    return float(num - z)


def segment_scores(logq, trans, init, labels, input_len, segments, seg_l_max):
    """sl_asg_segment_scores: logq (B, t_out, k), trans (k, k), init (k,), labels (B, l_max) int, input_len (B,), segments (N, 5)
    -> float64 (N,)"""
    logq = np.asarray(logq)
    labels = np.asarray(labels)
    trans = np.asarray(trans, dtype=np.float64)
    assert labels.ndim == 2 and labels.shape[0] == logq.shape[0]
    batch, t_out, k = logq.shape
    out = np.zeros(len(segments), dtype=np.float64)
    for i, seg in enumerate(segments):
        b = int(seg[0])
        if not 0 <= b < batch:
            out[i] = -np.inf
            continue
        f0, t_n, l0, n = clamped_segment(seg, input_len[b], t_out, labels.shape[1], seg_l_max)
        start = np.asarray(init, dtype=np.float64) if l0 == 0 else trans[int(np.clip(labels[b, l0 - 1], 0, k - 1))]
        out[i] = forward_score(logq[b, f0:f0 + t_n], trans, start, [int(c) for c in np.clip(labels[b, l0:l0 + n], 0, k - 1)])
    return out


def segment_frames(segments, input_len, t_out, l_max, seg_l_max, batch):
    """the clamped frame count T of every segment (0 for an utterance out of range): the tolerance's first term"""
    return np.array([clamped_segment(s, input_len[int(s[0])], t_out, l_max, seg_l_max)[1] if 0 <= int(s[0]) < batch else 0
                     for s in segments])


def brute_force_scores(e, g, s):
    """{string: log of the summed probability of every one of the k^T frame labelings that say it}, float64.  A labeling c
    scores s(c_0) + sum_t e_t(c_t) + sum_t g(c_{t-1}, c_t); the probabilities are normalised by their total; the string of a
    labeling is the labeling with adjacent repeats merged."""
    e = np.asarray(e, dtype=np.float64)
    t_n, k = e.shape
    totals = {}
    for c in itertools.product(range(k), repeat=t_n):
        score = s[c[0]] + sum(e[t, c[t]] for t in range(t_n)) + sum(g[c[t - 1], c[t]] for t in range(1, t_n))
        key = tuple(x for i, x in enumerate(c) if i == 0 or x != c[i - 1])
        totals[key] = totals.get(key, 0.0) + float(np.exp(score))
    z = sum(totals.values())
    with np.errstate(divide="ignore"):
        return {key: float(np.log(p / z)) for key, p in totals.items()}
