"""NumPy restatement of the log-prob rule of db1_select_tokens_lp / db1_select_tokens_slots_lp (include/db1_hip.h) and of the ranking of
``sample_best_of``.

The token is ``select_rule``'s.  Its log-probability is taken over the row's candidates, the finite logits of the columns in [lo, hi), with
NO temperature, top-k or top-p: lp = l[tok] - lse.  Bookkeeping of one launch at token index t: a row that is finished on entry writes 0 and
keeps its sum; a row without a candidate writes 0 and keeps its sum; any other row writes lp and adds it to its sum (the EOS included); with
t outside [0, max_new) nothing is written at all.  Best-of-n: score = sum / L^penalty, L = length + 1 for a row that ended with EOS, -inf for
a row that met a step without a candidate; order by score descending, ties to the lower column."""
from __future__ import annotations

import numpy as np

import select_rule as R


def candidates(l, lo, hi) -> np.ndarray:
    l = np.asarray(l, np.float64)
    c = np.zeros(l.shape[0], bool)
    c[lo:hi] = np.isfinite(l[lo:hi])
    return c


def lse(l, lo, hi) -> float:
    """float64 log-sum-exp over the candidates, the maximum subtracted first; -inf without a candidate"""
    l = np.asarray(l, np.float64)
    c = candidates(l, lo, hi)
    if not c.any():
        return -np.inf
    m = l[c].max()
    return float(m + np.log(np.exp(l[c] - m).sum()))


def logprob(l, tok, lo, hi) -> float:
    """float64 log-probability of column ``tok`` (a candidate) over the window"""
    l = np.asarray(l, np.float64)
    assert lo <= tok < hi and np.isfinite(l[tok])
    return float(l[tok] - lse(l, lo, hi))


def step(logits, t, max_new, finished, logprobs, sums, lo, hi, tokens=None, **sel):
    """one lockstep launch at token index ``t`` on float64 ``logits`` [M, V], in place on ``finished`` (bool [M]), ``logprobs`` ([M, max_new])
    and ``sums`` ([M]) -> the tokens (int64 [M]; -1: no candidate, -2: finished on entry).  ``tokens``: the tokens to score instead of the
    rule's own choice (a kernel's, where a near tie may part the two); ``sel``: what ``select_rule.select_row`` takes after the window.
    EOS is the caller's: it sets ``finished`` from the tokens."""
    M = logits.shape[0]
    out = np.full(M, -2, np.int64)
    for r in range(M):
        if finished[r]:
            if 0 <= t < max_new:
                logprobs[r, t] = 0.0
            continue
        kw = dict(sel)
        if "stream_ids" in kw:
            kw["stream_id"] = int(kw.pop("stream_ids")[r])
        tok = R.select_row(logits[r], lo, hi, **kw)[0] if tokens is None else int(tokens[r])
        if not candidates(logits[r], lo, hi).any():
            tok = -1
        out[r] = tok
        if not 0 <= t < max_new:
            continue
        if tok < 0:
            logprobs[r, t] = 0.0
            finished[r] = True
        else:
            lp = logprob(logits[r], tok, lo, hi)
            logprobs[r, t] = lp
            sums[r] += lp
    return out


def best_of_scores(sums, lengths, ended, no_candidate, length_penalty=1.0) -> np.ndarray:
    """float64 [G, n]: sum / L^penalty with L = lengths + 1 where the row ended with EOS; -inf for a no-candidate row"""
    L = np.asarray(lengths, np.float64) + np.asarray(ended, bool)
    sc = np.asarray(sums, np.float64) / np.maximum(L, 1.0) ** float(length_penalty)
    return np.where(np.asarray(no_candidate, bool), -np.inf, sc)


def best_of_order(scores, R_: int):
    """[G, n] -> a list of G lists: the R_ best columns, best first, ties to the lower column"""
    return [sorted(range(len(row)), key=lambda j: (-row[j], j))[:R_] for row in np.asarray(scores)]
