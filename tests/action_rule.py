"""NumPy restatement of db1_select_actions' rule (include/db1_hip.h), built on select_rule: the choice is select_rule's over the window
[act_lo, act_hi) of a row in which every masked column holds -inf, at the Philox step step_base + env_step * act_len + i; the books are the
bin (token - act_lo), its decoded action value (the action branch of the tokenizer's decode: bin / num_bins * 2 - 1 in float32) and the
next call's input id.  i == act_len (the memorising call) writes nothing; i outside [0, act_len] sets status bit 1 and writes nothing
else; a row without a candidate writes token act_lo, bin 0 and status bit 0."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_rule as R  # noqa: E402


def masked_row(l, act_lo, mask_row):
    """the row ``select_tokens`` would have to see: -inf at every column the mask (1 = allowed, the columns from act_lo on) forbids"""
    l = np.array(l, np.float64)
    if mask_row is not None:
        m = np.asarray(mask_row)
        l[act_lo:act_lo + m.shape[0]][m == 0] = -np.inf
    return l


def decode_action(bins, num_bins):
    """ContinuousScalarTokenizer.decode(is_action=True) in the reference's float32 op order (ids clipped to [0, num_bins - 1])"""
    b = np.clip(np.asarray(bins), 0, num_bins - 1).astype(np.float32)
    return (b / np.float32(num_bins) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def step_of(step_base, env_step, act_len, i):
    return (int(step_base) + int(env_step) * int(act_len) + int(i)) & 0xFFFFFFFF


def select_actions(logits, ctr, bins, values, next_ids, status, *, act_lo, act_hi, mask=None, num_bins=1024, greedy=True, temperature=1.0, top_k=0,
                   top_p=1.0, seed=0, step_base=0, stream_ids=None, ids_col=0):
    """one launch, in place on ``bins`` [M, act_len], ``values`` (or None), ``next_ids`` [M, q] (column ``ids_col``) and ``status`` [M];
    ``ctr`` = (env_step, i) is only read -> the tokens picked (int64 [M]; None when nothing was written)"""
    logits = np.asarray(logits, np.float64)
    M, act_len = bins.shape
    env_step, i = int(ctr[0]), int(ctr[1])
    if i == act_len:
        return None
    if i < 0 or i > act_len:
        status |= 2
        return None
    toks = np.zeros(M, np.int64)
    for r in range(M):
        row = masked_row(logits[r], act_lo, None if mask is None else mask[r])
        sid = r if stream_ids is None else int(stream_ids[r])
        tok = R.select_row(row, act_lo, act_hi, greedy, temperature, top_k, top_p, seed, sid, step_of(step_base, env_step, act_len, i))[0]
        if tok < 0:
            tok = act_lo
            status[r] |= 1
        toks[r] = tok
        bins[r, i] = tok - act_lo
        if values is not None:
            values[r, i] = decode_action(tok - act_lo, num_bins)
        next_ids[r, ids_col] = tok
    return toks


def ambiguous(l, act_lo, act_hi, mask_row, temperature, top_k, top_p, slack=1e-5):
    """whether the fp32 masses of the kernel may cut the top-p set of this row elsewhere than the float64 masses of the rule: some
    surviving token's cumulative mass (with or without its own ties) lies within ``slack`` of top_p -- the slack of the select test"""
    if top_p >= 1.0:
        return False
    _, cum, above = R.kept_set(masked_row(l, act_lo, mask_row), act_lo, act_hi, temperature, top_k, 1.0)
    c = np.concatenate([cum[np.isfinite(cum)], above[np.isfinite(above)]])
    return bool((np.abs(c - top_p) < slack).any())
