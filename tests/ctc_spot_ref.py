"""Float32 numpy restatement of sl_ctc_spot (include/speechless_hip.h): the per-frame scores and begin tags, and the hit picking;
and the brute force over all frame labelings that the restatement itself is checked against (tests/test_ctc_spot.py)."""
import itertools

import numpy as np

F32 = np.float32
MINUS_INF = F32(-np.inf)


def spot_frames(logq, phrase, t_b):
    """One query over one utterance.  logq: (T', K), blank = K - 1; phrase: the letters as given; t_b: the utterance's frames,
    clamped here.  Returns (frame_score float32 (T',), frame_begin int32 (T',)); every step an exact compare or one rounded
    float32 add."""
    logq = np.asarray(logq, dtype=F32)
    t_out, k = logq.shape
    t_b = min(max(int(t_b), 0), t_out)
    letters = np.array([int(c) for c in phrase], dtype=np.int64)
    n = len(letters)
    score = np.full((t_out,), MINUS_INF, dtype=F32)
    begin = np.full((t_out,), -1, dtype=np.int32)
    if n == 0:
        return score, begin
    s_count = 2 * n - 1
    col = np.full((s_count,), k - 1, dtype=np.int64)
    col[0::2] = np.clip(letters, 0, k - 1)
    skip = np.zeros((s_count,), dtype=bool)
    skip[2::2] = letters[1:] != letters[:-1]
    d = np.full((s_count,), MINUS_INF, dtype=F32)
    g = np.full((s_count,), -1, dtype=np.int64)
    for t in range(t_b):
        p1 = np.empty_like(d)
        g1 = np.empty_like(g)
        p1[0], g1[0] = F32(0), t  # the filler
        p1[1:], g1[1:] = d[:-1], g[:-1]
        p2 = np.full_like(d, MINUS_INF)
        g2 = np.full_like(g, -1)
        p2[2:], g2[2:] = d[:-2], g[:-2]
        p2[~skip] = MINUS_INF
        best, tag = d.copy(), g.copy()
        m = p1 > best  # strict: on a tie the earlier candidate keeps it
        best[m], tag[m] = p1[m], g1[m]
        m = p2 > best
        best[m], tag[m] = p2[m], g2[m]
        d = (best + logq[t, col]).astype(F32)
        g = np.where(d == MINUS_INF, -1, tag)
        score[t], begin[t] = d[-1], g[-1]
    return score, begin


def pick_hits(frame_score, frame_begin, min_score, max_hits):
    """The hit picking of the header on one query's rows.  Returns (hits int32 (max_hits, 2), hit_score float32 (max_hits,),
    n_hits); unused slots -1 / -inf."""
    score = np.asarray(frame_score, dtype=F32)
    begin = np.asarray(frame_begin, dtype=np.int64)
    frames = np.arange(len(score))
    live = (score > MINUS_INF) & (score >= F32(min_score))
    hits = np.full((max_hits, 2), -1, dtype=np.int32)
    hit_score = np.full((max_hits,), MINUS_INF, dtype=F32)
    n = 0
    while n < max_hits and live.any():
        t = int(np.argmax(np.where(live, score, MINUS_INF)))  # (argmax: the first of equal scores)
        hits[n] = (begin[t], t + 1)
        hit_score[n] = score[t]
        live &= ~((begin <= t) & (frames >= begin[t]))
        n += 1
    return hits, hit_score, n


def ctc_spot(logq, input_len, queries, query_len, query_utt, min_score, max_hits):
    """sl_ctc_spot.  logq (B, t_out, k); queries (N, q_max).  Returns (frame_score (N, t_out), frame_begin (N, t_out), hits
    (N, max_hits, 2), hit_score (N, max_hits), n_hits (N,))."""
    logq = np.asarray(logq, dtype=F32)
    queries = np.asarray(queries)
    batch, t_out, _ = logq.shape
    n, q_max = queries.shape
    frame_score = np.full((n, t_out), MINUS_INF, dtype=F32)
    frame_begin = np.full((n, t_out), -1, dtype=np.int32)
    hits = np.full((n, max_hits, 2), -1, dtype=np.int32)
    hit_score = np.full((n, max_hits), MINUS_INF, dtype=F32)
    n_hits = np.zeros((n,), dtype=np.int32)
    for q in range(n):
        b = int(query_utt[q])
        length = min(max(int(query_len[q]), 0), q_max)
        if 0 <= b < batch and length > 0:
            frame_score[q], frame_begin[q] = spot_frames(logq[b], queries[q, :length], input_len[b])
        hits[q], hit_score[q], n_hits[q] = pick_hits(frame_score[q], frame_begin[q], min_score[q], max_hits)
    return frame_score, frame_begin, hits, hit_score, n_hits


def collapses_to(symbols, blank):
    """the letters a frame labeling says: repeats merged, blanks dropped"""
    out, prev = [], None
    for c in symbols:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def brute_force_scores(logq, phrase, t_b):
    """For every end frame t < t_b: the max over begins b <= t and over all k^(t-b+1) labelings of the frames b .. t that start
    and end on a letter and collapse to the phrase, each summed left to right in float32.  Returns float32 (T',)."""
    logq = np.asarray(logq, dtype=F32)
    t_out, k = logq.shape
    blank = k - 1
    phrase = [int(c) for c in phrase]
    out = np.full((t_out,), MINUS_INF, dtype=F32)
    for t in range(min(t_b, t_out)):
        for b in range(t + 1):
            for symbols in itertools.product(range(k), repeat=t - b + 1):
                if symbols[0] == blank or symbols[-1] == blank or collapses_to(symbols, blank) != phrase:
                    continue
                total = logq[b, symbols[0]]
                for i, c in enumerate(symbols[1:]):
                    total = F32(total + logq[b + 1 + i, c])
                if total > out[t]:
                    out[t] = total
    return out
