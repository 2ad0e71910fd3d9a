"""The float32 restatement of sl_asg_align / sl_asg_align_long (include/speechless_hip.h) vectorised per frame, for labels of
thousands of graphemes: the same operations in the same order as the scalar asg_align_reference of tests/test_asg_align.py
(whose bytes it returns: tests/test_asg_align_long.py), one numpy pass over the states per frame, backpointers packed to one
bit per state and frame."""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def asg_align_long_reference(logq, trans, init, labels, label_len, input_len):
    """logq (t_out, k) emissions as they are, trans (k, k) [from][to], init (k,), labels any int sequence of at least
    label_len entries.  Returns (score float32, path int32 (t_out,): the state per frame, -1 past T_b or everywhere when
    infeasible)."""
    logq, trans, init = (np.asarray(x, dtype=F32) for x in (logq, trans, init))
    t_out, k = logq.shape
    L = min(max(int(label_len), 0), len(labels))
    T = min(max(int(input_len), 0), t_out)
    path = np.full(t_out, -1, dtype=np.int32)
    if L == 0 or T == 0 or L > T:
        return NEG_INF, path
    lab = np.clip(np.asarray(labels[:L], dtype=np.int64), 0, k - 1)
    gs = trans[lab, lab]
    ga = np.concatenate([[NEG_INF], trans[lab[:-1], lab[1:]]]).astype(F32)
    d = np.full(L, NEG_INF, dtype=F32)
    d[0] = init[lab[0]] + logq[0, lab[0]]
    moved = np.zeros((T, (L + 7) // 8), dtype=np.uint8)  # np.packbits: state s at bit 7 - (s & 7) of byte s >> 3
    move = np.full(L, NEG_INF, dtype=F32)
    for t in range(1, T):
        stay = d + gs
        move[1:] = d[:-1] + ga[1:]
        mv = move > stay
        d = np.where(mv, move, stay) + logq[t, lab]
        moved[t] = np.packbits(mv)
    assert d.dtype == F32
    score = d[L - 1]
    if score == NEG_INF:
        return NEG_INF, path
    s = L - 1
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= (int(moved[t, s >> 3]) >> (7 - (s & 7))) & 1
    return score, path
