"""NumPy restatement of db1_stop_match's rule (include/db1_hip.h): one call = one launch after a selection, on a state dict of arrays --
``lengths``, ``checked``, ``finished``, ``stop_hit`` (int32 [S]), ``out`` (int32 [S, max_new]), ``next_ids`` (int64 [S]) and optionally
``logprob`` (float32 [S, max_new]) with ``sum_logprob`` (float32 [S]) and ``top_ids`` (int32) with ``top_logprob`` (float32)
[S, max_new, n].

For logits row i with s = row_map[i] (None: every slot; an s outside [0, S) is skipped):
  1. n = lengths[s]; n == checked[s]: nothing of the slot is touched;
  2. checked[s] = n; n < 1 or n > max_new: nothing else;
  3. sequence k of length L matches if L <= n and out[s, n - L : n] == stops[k]; the longest match wins, then the lowest k;
  4. on a match, m = n - L: out[s, m:n] = pad_id, lengths[s] = checked[s] = m, finished[s] = 1, stop_hit[s] = k + 1, next_ids[s] = pad_id,
     logprob[s, m:n] = 0, sum_logprob[s] = logprob[s, 0] + ... + logprob[s, m - 1] added one by one in fp32 from 0.0, top_ids[s, m:n] = -1,
     top_logprob[s, m:n] = -inf."""
from __future__ import annotations

import numpy as np

MAX_SEQ, MAX_LEN = 16, 16


def pack(stops, fill: int = -1):
    """stop sequences -> (stop_tok int32 [n, 16] (``fill`` after a sequence's tokens), stop_len int32 [n]): the layout the kernel reads"""
    tok = np.full((len(stops), MAX_LEN), fill, np.int32)
    for k, q in enumerate(stops):
        tok[k, :len(q)] = q
    return tok, np.array([len(q) for q in stops], np.int32)


def winner(row, n: int, stops):
    """(k, L) of the sequence that ends row[:n] -- the longest, then the lowest k -- or None"""
    best = None
    for k, q in enumerate(stops):
        L = len(q)
        if 1 <= L <= MAX_LEN and L <= n and [int(v) for v in row[n - L:n]] == [int(v) for v in q]:
            if best is None or L > best[1]:
                best = (k, L)
    return best


def seq_sum(x) -> np.float32:
    s = np.float32(0.0)
    for v in np.asarray(x, np.float32):
        s = np.float32(s + v)
    return s


def step(state: dict, stops, pad_id: int, row_map=None) -> dict:
    """one launch -> the new state (a deep copy; ``state`` is left as it is)"""
    S = {k: np.array(v, copy=True) for k, v in state.items()}
    n_slots, mx = S["out"].shape
    for s in (range(n_slots) if row_map is None else (int(v) for v in row_map)):
        if not 0 <= s < n_slots:
            continue
        n = int(S["lengths"][s])
        if n == int(S["checked"][s]):
            continue
        S["checked"][s] = n
        if n < 1 or n > mx:
            continue
        hit = winner(S["out"][s], n, stops)
        if hit is None:
            continue
        k, L = hit
        m = n - L
        S["out"][s, m:n] = pad_id
        S["lengths"][s] = S["checked"][s] = m
        S["finished"][s] = 1
        S["stop_hit"][s] = k + 1
        S["next_ids"][s] = pad_id
        if "logprob" in S:
            S["logprob"][s, m:n] = 0.0
            S["sum_logprob"][s] = seq_sum(S["logprob"][s, :m])
        if "top_ids" in S:
            S["top_ids"][s, m:n] = -1
            S["top_logprob"][s, m:n] = -np.inf
    return S


def replay_row(ids, length: int, stops, pad_id: int):
    """the rule applied token by token to ONE finished unconstrained row (``ids[:length]`` its tokens before EOS / the limit) -> (the row
    as a generation under ``stops`` returns it, its length, stop_hit): the tokens arrive one per step, the first match ends the row"""
    ids = np.asarray(ids)
    mx = ids.shape[0]
    S = dict(lengths=np.zeros(1, np.int32), checked=np.zeros(1, np.int32), finished=np.zeros(1, np.int32), stop_hit=np.zeros(1, np.int32),
             out=np.full((1, mx), pad_id, np.int32), next_ids=np.zeros(1, np.int64))
    for n in range(1, int(length) + 1):
        S["out"][0, n - 1] = ids[n - 1]
        S["lengths"][0] = n
        S = step(S, stops, pad_id)
        if S["finished"][0]:
            return S["out"][0], int(S["lengths"][0]), int(S["stop_hit"][0])
    return ids.astype(np.int32), int(length), 0
