"""NumPy restatement of db1_select_tokens' selection rule (include/db1_hip.h), row by row.

Candidates are the finite logits of the columns in [lo, hi).  Greedy (or top_k == 1): arg-max, lowest column on ties.  Sampling: keep
{l >= k-th largest} (top_k > 0), then p = softmax(l / T) over what is left and keep {l >= tau}, tau = the largest kept logit with
mass{l >= tau} >= top_p; pick arg-max over the kept set of l / T - log(-log u), u = ((x >> 8) + 0.5) * 2^-24, x = word (col % 4) of
Philox4x32-10 on (col // 4, stream id, step, SITE_SAMPLE) under the key (seed lo, seed hi).  The masses here are float64 (the kernel's are
fp32): callers compare with a slack for tokens whose cumulative mass lies within ~1e-5 of top_p."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import db1_oracle as O  # noqa: E402

SITE_SAMPLE = 0xE0000100


def uniforms(n_cols: int, stream_id: int, step: int, seed: int) -> np.ndarray:
    """float64 [n_cols]: the u of every column (exact: the kernel's fp32 value)"""
    g = np.arange((n_cols + 3) // 4, dtype=np.uint64)
    o = O.philox4x32_10(g, np.uint64(stream_id & 0xFFFFFFFF), np.uint64(step & 0xFFFFFFFF), np.uint64(SITE_SAMPLE),
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x = np.stack(o, axis=1).reshape(-1)[:n_cols]
    return ((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def kept_set(l, lo, hi, temperature=1.0, top_k=0, top_p=1.0):
    """-> (kept bool [V], cum, above) after the window, top-k and top-p: cum / above = the mass fraction of {l' >= l} / {l' > l} under the
    softmax the top-p test uses, for every token that survives top-k (nan elsewhere)"""
    l = np.asarray(l, np.float64)
    V = l.shape[0]
    cand = np.zeros(V, bool)
    cand[lo:hi] = np.isfinite(l[lo:hi])
    kept = cand.copy()
    if not cand.any():
        return kept, np.full(V, np.nan), np.full(V, np.nan)
    if top_k > 0:
        vals = np.sort(l[cand])[::-1]
        kth = vals[min(top_k, vals.size) - 1]
        kept &= l >= kth
    m = l[kept].max()
    e = np.where(kept, np.exp((np.where(kept, l, m) - m) / temperature), 0.0)
    z = e.sum()
    cum = np.full(V, np.nan)
    lk = np.where(kept, l, -np.inf)
    order = np.argsort(-lk, kind="stable")
    srt = lk[order]
    cs = np.cumsum(e[order]) / z
    # mass{l' >= l_i}: the cumulative sum up to the LAST token tied with l_i
    last = np.searchsorted(-srt, -srt, side="right") - 1
    first = np.searchsorted(-srt, -srt, side="left")
    cum[order] = cs[last]
    cum[~kept] = np.nan
    above = np.full(V, np.nan)
    above[order] = np.where(first > 0, cs[np.maximum(first - 1, 0)], 0.0)
    above[~kept] = np.nan
    if top_p < 1.0:
        ok = kept & (cum >= top_p)
        tau = l[ok].max()
        kept &= l >= tau
    return kept, cum, above


def select_row(l, lo, hi, greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=0, stream_id=0, step=0):
    """-> (token or -1 when nothing is finite in the window, scores float64 [V] (-inf outside the kept set; greedy: the logits))"""
    l = np.asarray(l, np.float64)
    V = l.shape[0]
    if greedy or top_k == 1:
        sc = np.full(V, -np.inf)
        w = np.isfinite(l[lo:hi])
        sc[lo:hi] = np.where(w, l[lo:hi], -np.inf)
        if not w.any():
            return -1, sc
        return int(np.argmax(sc)), sc
    kept = kept_set(l, lo, hi, temperature, top_k, top_p)[0]
    if not kept.any():
        return -1, np.full(V, -np.inf)
    u = uniforms(V, stream_id, step, seed)
    sc = np.where(kept, l / temperature - np.log(-np.log(u)), -np.inf)
    return int(np.argmax(sc)), sc


def select(logits, lo, hi, greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=0, stream_ids=None, step=0):
    """all rows: -> tokens int64 [M] (-1: nothing finite)"""
    logits = np.asarray(logits, np.float64)
    sid = np.arange(logits.shape[0]) if stream_ids is None else np.asarray(stream_ids)
    return np.array([select_row(r, lo, hi, greedy, temperature, top_k, top_p, seed, int(s), step)[0] for r, s in zip(logits, sid)])
