"""Float64 numpy restatement of sl_ctc_segment_scores (include/speechless_hip.h), and the brute-force sum over all frame labelings
that the restatement itself is checked against (tests/test_ctc_segment.py)."""
import itertools

import numpy as np


def _clamp(v, hi):
    return min(max(int(v), 0), hi)


def clamped_segment(segment, input_len, t_out, l_max, seg_l_max):
    """(frame_begin, T, label_begin, L) of a segment of an utterance in range, as the header clamps them"""
    _, f0, f1, l0, l1 = (int(v) for v in segment)
    tb = _clamp(input_len, t_out)
    f0, f1 = _clamp(f0, tb), _clamp(f1, tb)
    l0, l1 = _clamp(l0, l_max), _clamp(l1, l_max)
    return f0, max(f1 - f0, 0), l0, min(max(l1 - l0, 0), seg_l_max)


def forward_score(logq, letters, k):
    """log of the CTC probability of `letters` over ALL the rows of logq (T, k), float64; blank = k - 1.  The s-2 rule compares
    the letters as given, the emission column of a letter is clamped into [0, k)."""
    logq = np.asarray(logq, dtype=np.float64)
    t_n, n = logq.shape[0], len(letters)
    reps = sum(1 for i in range(1, n) if letters[i] == letters[i - 1])
    if t_n == 0:
        return 0.0 if n == 0 else -np.inf
    if t_n < n + reps:
        return -np.inf
    s_n = 2 * n + 1
    col = np.full(s_n, k - 1, dtype=np.int64)
    col[1::2] = np.clip(np.asarray(letters, dtype=np.int64), 0, k - 1)
    skip = np.zeros(s_n, dtype=bool)
    for s in range(3, s_n, 2):
        skip[s] = letters[(s - 1) // 2] != letters[(s - 1) // 2 - 1]
    a = np.full(s_n, -np.inf)
    a[0] = logq[0, k - 1]
    if s_n > 1:
        a[1] = logq[0, col[1]]
    with np.errstate(invalid="ignore"):
        for t in range(1, t_n):
            one = np.full(s_n, -np.inf)
            one[1:] = a[:-1]
            two = np.full(s_n, -np.inf)
            two[2:] = a[:-2]
            a = np.logaddexp(np.logaddexp(a, one), np.where(skip, two, -np.inf)) + logq[t, col]
    return float(np.logaddexp(a[-1], a[-2])) if s_n > 1 else float(a[-1])


def segment_scores(logq, labels, input_len, segments, seg_l_max):
    """sl_ctc_segment_scores: logq (B, t_out, k), labels (B, l_max) int, input_len (B,), segments (N, 5) -> float64 (N,)"""
    logq = np.asarray(logq)
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.shape[0] == logq.shape[0]
    batch, t_out, k = logq.shape
    out = np.zeros(len(segments), dtype=np.float64)
    for i, seg in enumerate(segments):
        b = int(seg[0])
        if not 0 <= b < batch:
            out[i] = -np.inf
            continue
        f0, t_n, l0, n = clamped_segment(seg, input_len[b], t_out, labels.shape[1], seg_l_max)
        out[i] = forward_score(logq[b, f0:f0 + t_n], [int(c) for c in labels[b, l0:l0 + n]], k)
    return out


def segment_frames(segments, input_len, t_out, l_max, seg_l_max, batch):
    """the clamped frame count T of every segment (0 for an utterance out of range): the tolerance's first term"""
    return np.array([clamped_segment(s, input_len[int(s[0])], t_out, l_max, seg_l_max)[1] if 0 <= int(s[0]) < batch else 0
                     for s in segments])


def collapse(frame_labels, blank):
    """a frame labeling -> the string it says: repeats merged, then blanks dropped"""
    out, previous = [], None
    for c in frame_labels:
        if c != previous and c != blank:
            out.append(c)
        previous = c
    return tuple(out)


def brute_force_scores(logq, k):
    """{string: log of the summed probability of every one of the k^T frame labelings that collapse to it}, float64"""
    logq = np.asarray(logq, dtype=np.float64)
    totals = {}
    for frame_labels in itertools.product(range(k), repeat=logq.shape[0]):
        p = float(np.exp(sum(logq[t, c] for t, c in enumerate(frame_labels))))
        key = collapse(frame_labels, k - 1)
        totals[key] = totals.get(key, 0.0) + p
    with np.errstate(divide="ignore"):
        return {key: float(np.log(p)) for key, p in totals.items()}
