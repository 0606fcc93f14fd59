"""NumPy restatement of db1_constrain_logits_pen's rule (include/db1_hip.h), row by row: db1_constrain_logits' rule (tests/constraint_rule.py,
whose bf16 helpers and ``banned_columns`` are used as they are) with a frequency penalty, a presence penalty and an additive bias.

For a logits row l[0 .. V) that passed the guard, with the history H = hist[slot, 0 .. t):
  penalties: every distinct c of H with 0 <= c < V and l[c] finite, once; n_c = the occurrences of c in H:
      v = l32;  theta != 1: v = l32 > 0 ? v * inv : v * theta;  freq != 0 or pres != 0: p = fp32(n_c) * freq, p = p + pres, v = v - p
      (np.float32 operations in exactly this order, each rounded, none fused);  l[c] <- round(v), stored once;
  bias: then every (id, b) with 0 <= id < V whose STORED logit is finite: l[id] <- round(widen(l[id]) + b) -- a column in the history and in
      the bias list is rounded twice in bf16;
  bans (n-gram, ``bad``, EOS under ``min_new``) come last: -inf;  everything else keeps its bits.
fp32 logits are np.float32 arrays, bf16 logits their BITS (np.uint16), as in constraint_rule."""
from __future__ import annotations

import numpy as np

from constraint_rule import BF16, F32, NEG_INF_BF16, banned_columns, bf16_bits, bf16_widen, widen  # noqa: F401


def _get(l, c, dtype) -> np.float32:
    return np.float32(bf16_widen(l[c:c + 1])[0] if dtype == BF16 else l[c])


def _put(l, c, v, dtype):
    l[c] = bf16_bits(np.array([v], np.float32))[0] if dtype == BF16 else np.float32(v)


def normalise_bias(bias):
    """a mapping or pairs -> [(int id, np.float32 bias)] (the order does not matter: the ids are distinct)"""
    items = bias.items() if hasattr(bias, "items") else bias
    out = [(int(k), np.float32(b)) for k, b in items]
    assert len({k for k, _ in out}) == len(out), "bias ids must be distinct"
    return out


def apply_row(l, H, t: int, *, V: int, dtype: str, theta: float = 1.0, ngram: int = 0, bad=(), eos_id: int = -1, min_new: int = 0,
              freq: float = 0.0, pres: float = 0.0, bias=()):
    """one row (fp32 array, or uint16 bf16 bits, of >= V entries) that passed the guard -> the edited copy"""
    l = np.array(l, copy=True)
    th, f, p0 = np.float32(theta), np.float32(freq), np.float32(pres)
    inv = np.float32(1.0 / float(th))
    H = [int(c) for c in H[:t]]
    seen = set()
    with np.errstate(over="ignore", invalid="ignore"):
        for c in H:
            if c in seen or not 0 <= c < V:
                continue
            seen.add(c)
            x = _get(l, c, dtype)
            if not np.isfinite(x):
                continue
            v = x
            if th != np.float32(1):
                v = np.float32(x * inv) if x > 0 else np.float32(x * th)
            if f != 0 or p0 != 0:
                p = np.float32(np.float32(H.count(c)) * f)
                p = np.float32(p + p0)
                v = np.float32(v - p)
            _put(l, c, v, dtype)
        for c, b in normalise_bias(bias):
            if not 0 <= c < V:
                continue
            x = _get(l, c, dtype)
            if np.isfinite(x):
                _put(l, c, np.float32(x + b), dtype)
    for c in banned_columns(H, t, ngram, bad, eos_id, min_new):
        if 0 <= c < V:
            l[c] = NEG_INF_BF16 if dtype == BF16 else np.float32(-np.inf)
    return l


def apply(logits, hist, t, *, V: int, dtype: str = F32, finished=None, row_map=None, **kw):
    """logits [M, ld] (np.float32, or np.uint16 bf16 bits), hist int [n_slots, max_new], t an int (one counter for all rows) or an int array
    [n_slots] -> the edited array; the guard and ``row_map`` are constraint_rule.apply's"""
    logits = np.array(logits, copy=True)
    assert logits.dtype == (np.uint16 if dtype == BF16 else np.float32) and logits.ndim == 2
    hist = np.asarray(hist)
    S, mx = hist.shape
    for r in range(logits.shape[0]):
        s = r if row_map is None else int(row_map[r])
        if not 0 <= s < S:
            continue
        if finished is not None and int(finished[s]) != 0:
            continue
        ts = int(t) if np.ndim(t) == 0 else int(np.asarray(t).reshape(-1)[s if np.size(t) > 1 else 0])
        if not 0 <= ts < mx:
            continue
        logits[r] = apply_row(logits[r], hist[s], ts, V=V, dtype=dtype, **kw)
    return logits
