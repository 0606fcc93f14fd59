"""NumPy restatement of db1_select_tokens_slots_per's rule (include/db1_hip.h): ``select_rule.select_row`` per slot under the slot's OWN
parameters, plus the guard.

params is int32 [n_slots, 8], indexed by the SLOT, floats as their fp32 bits:
    word 0 greedy (0 / 1)   1 top_k   2 vocab_lo   3 vocab_hi   4 seed low 32 bits   5 seed high 32 bits
    word 6 inv_temperature = fp32 1 / temperature (one fp32 division on the host)   7 top_p
A live slot (not vacant, counter in range) is INVALID if not 0 <= vocab_lo < vocab_hi <= V, or if greedy == 0 and any of: inv_temperature
not finite and positive, top_k < 0, top_p not in (0, 1]: status bit 2 (value 4), finished = 1, pad_id forward, nothing else touched.  A
greedy slot ignores words 1 and 4 .. 7.  Otherwise the slot comes out as db1_select_tokens_slots / _lp / _top leaves it when called with
the slot's parameters as scalars: the Philox counter is (col / 4, stream id, step_base + t[slot], 0xE0000100) under the slot's own seed, and
the candidates of the log-prob and of the alternatives are the finite logits of the slot's own window."""
from __future__ import annotations

import numpy as np

import select_rule as R

WORDS = 8
BAD_PARAMS = 4          # status bit 2


def unpack(rec) -> dict:
    """one record -> greedy, top_k, vocab_lo, vocab_hi, seed, inv_temperature (np.float32), top_p (np.float32)"""
    w = np.asarray(rec, np.int32).reshape(WORDS)
    u = w.view(np.uint32)
    f = w.view(np.float32)
    return dict(greedy=bool(w[0] != 0), top_k=int(w[1]), vocab_lo=int(w[2]), vocab_hi=int(w[3]), seed=int(u[4]) | (int(u[5]) << 32),
                inv_temperature=f[6], top_p=f[7])


def invalid(rec, V: int) -> bool:
    p = unpack(rec)
    if not 0 <= p["vocab_lo"] < p["vocab_hi"] <= V:
        return True
    if p["greedy"]:
        return False
    it, tp = p["inv_temperature"], p["top_p"]
    return bool(not (np.isfinite(it) and it > 0) or p["top_k"] < 0 or not (tp > 0 and tp <= 1))


def select_slot(l, rec, V: int, stream_id: int, step: int):
    """one live slot's logits ``l`` [>= V] under its record -> (status bits, token): (4, None) for an invalid record; (1, -1) when
    nothing in the slot's window is finite; else (0, the token of ``select_rule.select_row`` under the slot's parameters, T = 1 / word 6)"""
    if invalid(rec, V):
        return BAD_PARAMS, None
    p = unpack(rec)
    T = 1.0 if p["greedy"] else 1.0 / float(p["inv_temperature"])
    tok, _ = R.select_row(np.asarray(l, np.float64)[:V], p["vocab_lo"], p["vocab_hi"], p["greedy"], T, p["top_k"], float(p["top_p"]), p["seed"],
                          stream_id, step)
    return (1, -1) if tok < 0 else (0, tok)


def step_slots(logits, row_map, params, t, limit, finished, stream_id, V: int, step_base: int = 0):
    """one launch over the slots: logits row i belongs to slot row_map[i] (None: slot i) -> {slot: (status bits, token or None)} for every
    live slot the launch serves; vacant slots, slots outside [0, n_slots) and counters out of range (status bit 1: the slot form's own rule)
    are left out.  Slot s reads params[s], not params[row]."""
    n = len(t)
    got = {}
    for i in range(len(logits)):
        s = i if row_map is None else int(row_map[i])
        if not 0 <= s < n or finished[s] or not 0 <= t[s] < limit[s]:
            continue
        got[s] = select_slot(logits[i], params[s], V, int(stream_id[s]), step_base + int(t[s]))
    return got
