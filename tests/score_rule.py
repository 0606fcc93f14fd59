"""The scoring rule of include/db1_hip.h (db1_score_rows, db1_score_segments) restated in NumPy: the yardstick of the scoring kernels.

A row of logits l[0 .. V) (float32 values as stored), a label y, a window [lo, hi): candidates are the finite logits inside the window;
lse = fp32 log-sum-exp over them (maximum subtracted first); logprob = l[y] - lse; top1 = the largest candidate, lowest column on ties;
rank = the number of candidates strictly above l[y].  status bit 0: the label lies in [0, V) but is no candidate; bit 1: no candidate."""
import numpy as np


def score_row(l, y, lo, hi):
    """-> (lse, logprob, top1, rank, status) of one row"""
    l = np.asarray(l, dtype=np.float32)
    V = l.shape[0]
    assert 0 <= lo < hi <= V
    cols = np.arange(V)
    cand = np.isfinite(l) & (cols >= lo) & (cols < hi)
    y = int(y)
    y_in = 0 <= y < V
    status = 0
    if not cand.any():
        status |= 2
        lse, top1 = np.float32(-np.inf), -1
    else:
        m = l[cand].max()
        e = np.exp((l[cand] - m).astype(np.float32)).astype(np.float32)
        lse = np.float32(m + np.log(np.sum(e, dtype=np.float32), dtype=np.float32))
        top1 = int(cols[cand & (l == m)][0])
    if not y_in:                       # ignored row (torch's ignore_index)
        return lse, np.float32(0.0), top1, -1, status
    if not cand[y]:
        return lse, np.float32(-np.inf), top1, -1, status | 1
    return lse, np.float32(l[y] - lse), top1, int(np.sum(cand & (l > l[y]))), status


def score_rows(logits, labels, lo, hi):
    """logits [T, V] -> lse, logprob (float32 [T]), top1, rank, status (int32 [T])"""
    out = [score_row(l, y, lo, hi) for l, y in zip(np.asarray(logits), np.asarray(labels))]
    return (np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.int32), np.array([o[4] for o in out], np.int32))


def score_segments(logprob, rank, labels, mask, n_seg, V):
    """float64 [n_seg, 3]: sum(mask * logprob), sum(mask), sum(mask * (rank == 0)) over the rows with mask != 0 and a label in [0, V)"""
    lp = np.asarray(logprob, np.float64).reshape(n_seg, -1)
    rk = np.asarray(rank).reshape(n_seg, -1)
    lab = np.asarray(labels).reshape(n_seg, -1)
    mk = np.where((lab >= 0) & (lab < V), np.asarray(mask, np.float64).reshape(n_seg, -1), 0.0)
    on = mk != 0
    out = np.zeros((n_seg, 3))
    for s in range(n_seg):
        out[s, 0] = np.sum(mk[s][on[s]] * lp[s][on[s]])
        out[s, 1] = np.sum(mk[s][on[s]])
        out[s, 2] = np.sum(mk[s][on[s]] * (rk[s][on[s]] == 0))
    return out


def candidate_scores(logprob, cand_len, length_penalty):
    """scores [G, K] float32 and order [G, K] of rank_candidates from logprob [G, K, Lc]: sum over i < len, over len^length_penalty; the order is
    descending with the lower k first on ties"""
    lp = np.asarray(logprob, np.float64)
    n = np.broadcast_to(np.asarray(cand_len), lp.shape[:2])
    keep = np.arange(lp.shape[2])[None, None, :] < n[:, :, None]
    s = np.where(keep, lp, 0.0).sum(-1) / np.power(n.astype(np.float64), float(length_penalty))
    return s.astype(np.float32), np.argsort(-s.astype(np.float32), axis=1, kind="stable")
