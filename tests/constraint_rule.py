"""NumPy restatement of db1_constrain_logits' rule (include/db1_hip.h), row by row.

For a logits row l[0 .. V) with the history H = hist[slot, 0 .. t) of the tokens its slot has generated:
  1. guard: t outside [0, max_new), finished[slot] != 0 or a row_map entry outside [0, n_slots) -> the row is not touched;
  2. repetition penalty theta: every distinct c in H with 0 <= c < V and l[c] finite, once: l[c] <- round(l32 * inv) if l32 > 0 else
     round(l32 * theta), inv = fp32(1 / theta), ONE fp32 multiplication, round = identity (fp32) / round to nearest even (bf16);
  3. no-repeat n-gram n: every i in [n - 1, t) with H[i - n + 1 .. i - 1] == H[t - n + 1 .. t - 1] bans H[i];
  4. every id of ``bad`` is banned; 5. ``eos_id`` (>= 0) is banned while t < min_new;
  6. a banned column in [0, V) becomes -inf, after the penalty; 7. everything else keeps its bits.
fp32 logits are np.float32 arrays.  bf16 logits are held as their BITS (np.uint16): widening is a shift, rounding is done on the integer."""
from __future__ import annotations

import numpy as np

F32, BF16 = "fp32", "bf16"
NEG_INF_BF16 = np.uint16(0xFF80)


def bf16_bits(x) -> np.ndarray:
    """fp32 -> the bits of the nearest bf16 (ties to even; NaN stays NaN)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def bf16_widen(bits) -> np.ndarray:
    """bf16 bits -> fp32 (exact)"""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def widen(logits, dtype) -> np.ndarray:
    """the logits as fp32 values, whatever they are stored as"""
    return bf16_widen(logits) if dtype == BF16 else np.asarray(logits, np.float32)


def banned_columns(H, t: int, ngram: int, bad, eos_id: int, min_new: int) -> set:
    """the banned ids of a row with history H[0 .. t) (any integer: the caller keeps those in [0, V))"""
    H = [int(c) for c in H[:t]]
    ban = set(int(c) for c in bad)
    if ngram > 0:
        n1 = ngram - 1
        for i in range(n1, t):
            if H[i - n1:i] == H[t - n1:t]:
                ban.add(H[i])
    if eos_id >= 0 and t < min_new:
        ban.add(int(eos_id))
    return ban


def apply_row(l, H, t: int, *, V: int, dtype: str, theta: float = 1.0, ngram: int = 0, bad=(), eos_id: int = -1, min_new: int = 0):
    """one row (fp32 array, or uint16 bf16 bits, of >= V entries) that passed the guard -> the edited copy"""
    l = np.array(l, copy=True)
    th = np.float32(theta)
    inv = np.float32(1.0 / float(th))          # the fp32 nearest to 1 / theta, from a double division
    seen = set()
    for c in (int(c) for c in H[:t]):
        if c in seen or not 0 <= c < V:
            continue
        seen.add(c)
        x = np.float32(bf16_widen(l[c:c + 1])[0] if dtype == BF16 else l[c])
        if not np.isfinite(x):
            continue
        with np.errstate(over="ignore"):
            y = np.float32(x * inv) if x > 0 else np.float32(x * th)
        l[c] = bf16_bits(np.array([y], np.float32))[0] if dtype == BF16 else y
    for c in banned_columns(H, t, ngram, bad, eos_id, min_new):
        if 0 <= c < V:
            l[c] = NEG_INF_BF16 if dtype == BF16 else np.float32(-np.inf)
    return l


def apply(logits, hist, t, *, V: int, dtype: str = F32, theta: float = 1.0, ngram: int = 0, bad=(), eos_id: int = -1, min_new: int = 0,
          finished=None, row_map=None):
    """logits [M, ld] (np.float32, or np.uint16 bf16 bits), hist int [n_slots, max_new], t an int (one counter for all rows) or an int array
    [n_slots] -> the edited array.  ``row_map`` [M]: the slot of every row (None: row i is slot i)."""
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
        logits[r] = apply_row(logits[r], hist[s], ts, V=V, dtype=dtype, theta=theta, ngram=ngram, bad=bad, eos_id=eos_id, min_new=min_new)
    return logits
