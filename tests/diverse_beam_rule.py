"""NumPy restatement of db1_beam_step_diverse's rule (include/db1_hip.h), built on tests/beam_rule.py.

G prompts, W beams each, split into D sub-groups of W' = W / D beams; row b = (g * D + d) * W' + j.  Every state array has the layout of
beam_rule's state for G * D groups of W' beams.  Per step t, per prompt, the sub-groups d = 0 .. D - 1 choose in turn over a list ``chosen``
that starts empty:
  1. a done sub-group, or a counter outside [0, max_new): as in the plain rule; nothing goes to ``chosen``;
  2. candidates: steps 1-2 of the plain rule over the sub-group's W' rows (at t = 0 only beam 0 of EACH sub-group is live);
     s = beam_score + (l - lse);
  3. n(c) = the number of entries of ``chosen`` equal to c; sel = s - fp32(n) * lambda in fp32 (no lower than -FLT_MAX); the candidates sorted by sel descending, ties
     by the lower (j, c); the first 2W' are walked;
  4. the walk of the plain rule with W' for W; every STORED score (beam scores, pool scores s / (t + 1)^alpha) is the unpenalised s;
  5. done when no beam was filled, or the pool holds W' entries and its worst >= (the LARGEST s among the new beams) / (t + 1)^alpha;
  6. at t = max_new - 1 the new beams are offered as in the plain rule;
  7. a sub-group that is not done after the step appends the tokens of its filled beams to ``chosen``, in beam order;
  8. output (host): a prompt's D pools merged, sorted by (score descending, d ascending, position in its pool ascending), the first R.
``step`` takes ``k_row``: None ranks every candidate of a row, an int only the row's best k_row by (logit descending, column ascending) --
what the kernel does with k_row = W' + W.  As in beam_rule the lse is float64 rounded to fp32 and ``step`` reports, per sub-group, whether
a decision hinged on two sel / pool scores closer than ``tol``."""
from __future__ import annotations

import numpy as np

import beam_rule as B

STATE_KEYS = B.STATE_KEYS


def new_state(G: int, W: int, D: int, max_new: int, pad: int = 0) -> dict:
    assert D >= 1 and W % D == 0
    return B.new_state(G * D, W // D, max_new, pad)


def step(S: dict, logits, t: int, W: int, D: int, lam: float, lo: int, hi: int, eos: int = -1, pad: int = 0, alpha: float = 1.0,
         tol: float = 1e-5, k_row=None, walked=None):
    """one step on a copy of ``S`` (new_state layout) and logits [G * W, V] -> (new state, ambiguous bool [G * D]); ``walked`` (a dict):
    receives, per sub-group that chose, the (j, c) pairs of the first 2W' candidates in sel order"""
    return B.step(S, logits, t, W, lo, hi, eos, pad, alpha, tol, D, lam, k_row, walked)


def merge_order(scores, counts):
    """step 8 for one prompt: ``scores`` [D, W'] (sorted pools), ``counts`` [D] -> the (d, k) pairs of every pool entry, best first"""
    ent = [(-float(scores[d][k]), d, k) for d in range(len(counts)) for k in range(int(counts[d]))]
    ent.sort()
    return [(d, k) for _, d, k in ent]


def results(S: dict, W: int, D: int, R: int, pad: int = 0):
    """-> (ids [G, R, max_new], lengths [G, R], scores [G, R], groups [G, R] (-1 where there is no result)) as beam_search returns them"""
    M, mx = S["tokens"].shape
    Wp = W // D
    G = M // W
    ids = np.full((G, R, mx), pad, np.int32)
    lengths = np.zeros((G, R), np.int32)
    scores = np.full((G, R), -np.inf, np.float32)
    groups = np.full((G, R), -1, np.int32)
    for g in range(G):
        qs = slice(g * D, (g + 1) * D)
        for r, (d, k) in enumerate(merge_order(S["pool_score"][qs], S["pool_count"][qs])[:R]):
            q = g * D + d
            ids[g, r] = S["pool_tokens"][q, S["pool_slot"][q, k]]
            lengths[g, r] = S["pool_len"][q, k]
            scores[g, r] = S["pool_score"][q, k]
            groups[g, r] = d
    return ids, lengths, scores, groups


def search(next_logits, G: int, W: int, D: int, lam: float, max_new: int, lo: int, hi: int, eos: int = -1, pad: int = 0, alpha: float = 1.0,
           R: int = 1, tol: float = 1e-5):
    """the whole search with ``next_logits(histories)`` -> logits [G * W, V] of every row given its tokens so far; stops early when every
    sub-group is done.  -> (ids, lengths, scores, groups, final state, ambiguous bool [G]: a sub-group of the prompt was, at some step)"""
    S = new_state(G, W, D, max_new, pad)
    amb = np.zeros(G, bool)
    for t in range(max_new):
        hist = [list(S["tokens"][b, :t]) for b in range(G * W)]
        S, a = step(S, next_logits(hist), t, W, D, lam, lo, hi, eos, pad, alpha, tol)
        amb |= a.reshape(G, D).any(axis=1)
        if S["done"].all():
            break
    return results(S, W, D, R, pad) + (S, amb)
