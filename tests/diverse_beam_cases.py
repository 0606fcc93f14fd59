"""The cases of test_diverse_beam_kernels_gpu.py, shared with test_diverse_beam_cpu.py, which asserts on the very same seeds that they
exercise the penalty (independent random rows almost never collide: the rows of one prompt share a base vector, N(0, 3^2), plus per-row
noise, N(0, 0.3^2), at every step) and stay unambiguous."""
import numpy as np

import diverse_beam_rule as DR

SHAPES = [(1, 4), (2, 2), (4, 1), (16, 1), (3, 5), (5, 3), (4, 4), (2, 8), (8, 2)]       # (D, W')
GS = [1, 3]
VS = [200, 33025]
LAMS = [0.25, 1.0]
STEPS = 5
EOS, ALPHA = 5, 0.8


def window(V):
    return (3, 190) if V == 200 else (0, 32000)


DTYPES = ["float32", "bfloat16"]


def seed(D, Wp, G, V, lam):
    return ((D * 17 + Wp) * 10 + G) * 4 + 2 * (V > 1000) + (lam > 0.5)


def eos_kind(g, G):
    """0: EOS at rank 0 of the prompt's rows; 1: EOS just below the rows' top; 2: EOS wherever the draw put it.  A single prompt is of kind 1
    (with EOS on top its sub-groups of one beam would all end at step 0)."""
    return (g + (G == 1)) % 3


def done_subgroup(G, D):
    """the sub-group planted as already done at t = 2: in the middle of the last prompt (which has no EOS on top)"""
    return (G - 1) * D + (D - 1) // 2


def logits(rng, G, D, Wp, V, t, case=""):
    W = D * Wp
    M = G * W
    base = rng.standard_normal((G, 1, V)).astype(np.float32) * 3.0
    noise = rng.standard_normal((G, W, V)).astype(np.float32) * 0.3
    l = (base + noise).reshape(M, V)
    l[:, 7] = l[:, 8]                                     # planted ties (same row, same logit)
    l[:, 11] = np.nan
    l[:, 12] = np.inf
    l[:, 13] = -np.inf
    l[0, 20:40] = l[0, 20]
    if M >= 2:
        l[1] = l[0] if t == 0 else l[1]
    for g in range(G):
        r = slice(g * W, (g + 1) * W)
        kind = eos_kind(g, G)
        if kind == 0:
            l[r, EOS] = np.nanmax(np.where(np.isfinite(l[r]), l[r], -np.inf), axis=1) + 1.0
        elif kind == 1:
            srt = np.sort(np.where(np.isfinite(l[r]), l[r], -np.inf), axis=1)
            l[r, EOS] = srt[:, -(Wp + 2)] - 1e-3           # a little below the row's top W' + 1
    if case == "norow" and M > 1:
        l[M - 1, :] = np.nan                              # a row without a candidate
    return l


def run(D, Wp, G, V, lam, step_fn, widen=lambda l: l):
    """the five steps of one case: ``step_fn(S, l, t)`` -> (the state the next step starts from, ambiguous [G * D]) is the device (GPU
    test) or the rule (CPU test); yields (t, S before the step, logits as the step saw them, the state after, ambiguous)"""
    W = D * Wp
    lo, hi = window(V)
    rng = np.random.default_rng(seed(D, Wp, G, V, lam))
    S = DR.new_state(G, W, D, STEPS, hi - 1)
    for t in range(STEPS):
        if t == 2:
            S["done"][done_subgroup(G, D)] = 1
        l = widen(logits(rng, G, D, Wp, V, t, "norow" if t == 3 else ""))
        nxt, amb = step_fn(S, l, t)
        yield t, S, l, nxt, amb
        S = nxt


def k_row_case(D, V=64):
    """the case that needs the LAST of a row's W' + W candidates in a stored state: W' = 1 (W = D), t = 0, EOS = token 0, lambda above
    every score difference.  The rows of sub-groups 0 .. D - 2 hold descending logits with EOS far below, so they choose tokens 1, 2, ..,
    D - 1 in turn.  The last sub-group's row holds the same logits with EOS on top: raw rank 0 is EOS (a hypothesis at walk rank 0 < W'),
    raw ranks 1 .. D - 1 are the penalised tokens, and the walk's second candidate, the new beam, is raw rank D = W' + W - 1: token D.
    A list cut to W' + W - 1 = D stores a penalised token (token 1) and its score instead.  -> (state, logits [D, V], EOS, lambda)"""
    l = np.tile(np.arange(V, 0, -1).astype(np.float32)[None], (D, 1))
    l[:D - 1, 0] = -50.0
    return DR.new_state(1, D, D, 3, V - 1), l, 0, 1e4
