"""NumPy restatement of the top-n rule of db1_select_tokens_top / db1_select_tokens_slots_top and db1_score_rows_top / db1_lmhead_score_top
(include/db1_hip.h), in float64.

For one row of logits, a window [lo, hi) and 1 <= n <= 16: the candidates are the finite logits of the window (``logprob_rule.candidates``),
as the launch reads them -- in generation after db1_constrain_logits, with no temperature, top-k or top-p.  The alternatives are the
candidates sorted by logit descending, ties by the lower column; the first k = min(n, #candidates) are reported as ``top_ids[i]`` and
``top_logprob[i] = l[top_ids[i]] - lse`` with the lse of ``logprob_rule.lse``; the entries [k, n) are -1 and -inf.  A row with no
candidate, and a lockstep row that was finished on entry, report n unused entries; a vacant slot and a counter outside its range touch neither
buffer (``step`` / ``step_slots`` leave them alone).

Signed zeros: float64 sorts -0.0 and +0.0 as one value, and so do the scoring kernels (``signed_zero=False``).  The generation kernels sort
by the keys their arg-max uses, which put -0.0 below +0.0 (``signed_zero=True``)."""
from __future__ import annotations

import numpy as np

import logprob_rule as L
import select_rule as R  # noqa: F401  (the token of a generation step is select_rule's; callers pass the kernel's own)

MAX_N = 16


def top_row(l, lo, hi, n, signed_zero=False):
    """-> (top_ids int64 [n], top_logprob float64 [n]) of one row"""
    if not 1 <= int(n) <= MAX_N:
        raise ValueError(f"n {n} must lie in [1, {MAX_N}]")
    l = np.asarray(l, np.float64)
    ids, lps = np.full(n, -1, np.int64), np.full(n, -np.inf)
    cols = np.flatnonzero(L.candidates(l, lo, hi))
    if cols.size == 0:
        return ids, lps
    v = l[cols]
    neg0 = (np.signbit(v) & (v == 0.0)) if signed_zero else np.zeros(v.size, bool)
    order = np.lexsort((cols, neg0, -v))          # by -logit, then +0.0 before -0.0 (generation only), then by column
    k = min(int(n), cols.size)
    ids[:k] = cols[order[:k]]
    lps[:k] = l[ids[:k]] - L.lse(l, lo, hi)
    return ids, lps


def top(logits, lo, hi, n, signed_zero=False):
    """all rows -> (int64 [M, n], float64 [M, n])"""
    r = [top_row(row, lo, hi, n, signed_zero) for row in np.asarray(logits, np.float64)]
    return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


def step(logits, t, max_new, finished, top_ids, top_logprob, lo, hi, signed_zero=True):
    """one lockstep launch at token index ``t`` on float64 ``logits`` [M, V], in place on ``top_ids`` / ``top_logprob`` [M, max_new, n]:
    ``finished`` (bool [M]) is the state ON ENTRY; the caller applies EOS and no-candidate endings, as for ``logprob_rule.step``"""
    n = top_ids.shape[2]
    if not 0 <= t < max_new:
        return
    for r in range(logits.shape[0]):
        if finished[r]:
            top_ids[r, t], top_logprob[r, t] = -1, -np.inf
        else:
            top_ids[r, t], top_logprob[r, t] = top_row(logits[r], lo, hi, n, signed_zero)


def step_slots(logits, row_map, t, limit, finished, top_ids, top_logprob, lo, hi, signed_zero=True):
    """one launch of the slot form, in place on ``top_ids`` / ``top_logprob`` [S, max_new, n]: logits row i belongs to slot ``row_map[i]``;
    ``t`` / ``limit`` / ``finished`` ([S]) are the state ON ENTRY and are not advanced here.  A slot that does not exist, a vacant slot and a
    counter outside [0, limit) (or a limit above max_new) touch nothing."""
    S, max_new, n = top_ids.shape
    for i, s in enumerate(row_map):
        if not 0 <= s < S or finished[s]:
            continue
        if not (0 <= t[s] < limit[s] <= max_new):
            continue
        top_ids[s, t[s]], top_logprob[s, t[s]] = top_row(logits[i], lo, hi, n, signed_zero)
