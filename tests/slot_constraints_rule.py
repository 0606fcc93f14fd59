"""NumPy restatement of the per-slot rules db1_constrain_logits_slots_per and db1_stop_match_per (include/db1_hip.h), built on the scalar
rules and restating none of them: per slot the guard, the record's invalid / no-op tests, then ``penalty_rule.apply_row`` with the slot's
values and its own list rows; and ``stop_rule.step`` with the slot's own list.

A record is int32 [8], floats as their fp32 bits: 0 theta, 1 inv_theta, 2 ngram, 3 min_new, 4 freq, 5 pres, 6 n_bad, 7 n_bias.  The kernel
multiplies by the record's inv_theta; ``penalty_rule`` computes its own from theta, and the two agree because the host stores the one fp32
division of 1 by theta (``unpack`` keeps the word so a test can say so)."""
from __future__ import annotations

import numpy as np

import penalty_rule as P
import stop_rule as R

WORDS = 8
BAD_RECORD = 8            # status bit 3
MAX_CAP = 1024


def record(theta=1.0, ngram=0, min_new=0, freq=0.0, pres=0.0, n_bad=0, n_bias=0, inv_theta=None) -> np.ndarray:
    """the eight words from values (``inv_theta`` None: the fp32 division); nothing is validated: a test builds bad records with it"""
    w = np.zeros(WORDS, np.uint32)
    with np.errstate(all="ignore"):
        th = np.float32(theta)
        inv = np.float32(1) / th if inv_theta is None else np.float32(inv_theta)
        w[0:2] = np.array([th, inv], np.float32).view(np.uint32)
        w[4:6] = np.array([freq, pres], np.float32).view(np.uint32)
    w[2:4] = np.array([ngram, min_new], np.int64).astype(np.int32).view(np.uint32)
    w[6:8] = np.array([n_bad, n_bias], np.int64).astype(np.int32).view(np.uint32)
    return w.view(np.int32)


def unpack(rec) -> dict:
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    f = rec.view(np.float32)
    return dict(theta=f[0], inv_theta=f[1], ngram=int(rec[2]), min_new=int(rec[3]), freq=f[4], pres=f[5], n_bad=int(rec[6]), n_bias=int(rec[7]))


def invalid(rec, bad_cap: int, bias_cap: int) -> bool:
    p = unpack(rec)
    pos = lambda x: bool(np.isfinite(x) and x > 0)
    return not (pos(p["theta"]) and pos(p["inv_theta"]) and p["ngram"] >= 0 and p["min_new"] >= 0 and np.isfinite(p["freq"]) and
                np.isfinite(p["pres"]) and 0 <= p["n_bad"] <= bad_cap and 0 <= p["n_bias"] <= bias_cap)


def noop(rec, eos_id: int) -> bool:
    p = unpack(rec)
    return bool(p["theta"] == 1 and p["freq"] == 0 and p["pres"] == 0 and p["ngram"] == 0 and p["n_bad"] == 0 and p["n_bias"] == 0 and
                (eos_id < 0 or p["min_new"] == 0))


def scalar_kw(rec, bad_row, bias_ids_row, bias_val_row, eos_id: int) -> dict:
    """a valid record and the slot's list rows -> the keywords of ``penalty_rule.apply_row`` (the scalar rule's own)"""
    p = unpack(rec)
    bias = [(int(bias_ids_row[i]), np.float32(bias_val_row[i])) for i in range(p["n_bias"])]
    return dict(theta=float(p["theta"]), ngram=p["ngram"], bad=[int(v) for v in bad_row[:p["n_bad"]]], eos_id=eos_id, min_new=p["min_new"],
                freq=float(p["freq"]), pres=float(p["pres"]), bias=bias)


def constrain(logits, hist, t, finished, status, cons, bad, bias_ids, bias_val, *, V: int, dtype: str, eos_id: int = -1, row_map=None):
    """one launch -> (logits, finished, status), all copies.  logits [M, ld] (np.float32, or np.uint16 bf16 bits), hist int [S, max_new],
    t / finished / status int [S], cons int32 [S, 8], bad [S, bad_cap], bias_ids / bias_val [S, bias_cap] (None: a capacity of 0)"""
    logits, finished, status = np.array(logits, copy=True), np.array(finished, copy=True), np.array(status, copy=True)
    hist = np.asarray(hist)
    S, mx = hist.shape
    bad = np.zeros((S, 0), np.int32) if bad is None else np.asarray(bad)
    bias_ids = np.zeros((S, 0), np.int32) if bias_ids is None else np.asarray(bias_ids)
    bias_val = np.zeros((S, 0), np.float32) if bias_val is None else np.asarray(bias_val)
    for r in range(logits.shape[0]):
        s = r if row_map is None else int(row_map[r])
        if not 0 <= s < S or int(finished[s]) != 0 or not 0 <= int(t[s]) < mx:
            continue
        if invalid(cons[s], bad.shape[1], bias_ids.shape[1]):
            status[s] |= BAD_RECORD
            finished[s] = 1
            continue
        if noop(cons[s], eos_id):
            continue
        assert unpack(cons[s])["inv_theta"] == np.float32(1.0 / float(unpack(cons[s])["theta"])), "inv_theta must be the fp32 division"
        logits[r] = P.apply_row(logits[r], hist[s], int(t[s]), V=V, dtype=dtype, **scalar_kw(cons[s], bad[s], bias_ids[s], bias_val[s], eos_id))
    return logits, finished, status


def slot_stops(stop_tok, stop_len, s: int):
    """slot s's list as ``stop_rule`` takes it: 16 entries, an entry whose length is outside 1 .. 16 is the empty sequence (it never matches
    and keeps its index, so ``stop_hit`` numbers the table's entries)"""
    out = []
    for k in range(R.MAX_SEQ):
        L = int(stop_len[s][k])
        out.append([int(v) for v in stop_tok[s][k][:L]] if 1 <= L <= R.MAX_LEN else [])
    return out


def stop(state: dict, stop_tok, stop_len, pad_id: int, row_map=None) -> dict:
    """one launch of db1_stop_match_per -> the new state: ``stop_rule.step`` slot by slot, each with its own list"""
    n_slots = np.asarray(state["out"]).shape[0]
    S = state
    for s in (range(n_slots) if row_map is None else (int(v) for v in row_map)):
        if 0 <= s < n_slots:
            S = R.step(S, slot_stops(stop_tok, stop_len, s), pad_id, row_map=[s])
    return S if S is not state else {k: np.array(v, copy=True) for k, v in state.items()}
