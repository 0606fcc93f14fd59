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
    S = {k: np.array(v, copy=True) for k, v in S.items()}
    M, mx = S["tokens"].shape
    Wp = W // D
    Q = M // Wp                                           # sub-groups
    G = Q // D
    amb = np.zeros(Q, bool)
    logits = np.asarray(logits, np.float32)
    lam32 = np.float32(lam)
    if not 0 <= t < mx:
        for q in range(Q):
            S["next_ids"][q * Wp:(q + 1) * Wp] = pad
            if not S["done"][q]:
                S["status"][q] |= 2
        return S, amb
    den = np.float32(np.float32(t + 1) ** np.float32(alpha))
    old_tokens = S["tokens"].copy()
    for g in range(G):
        chosen = []
        for d in range(D):
            q = g * D + d
            b0 = q * Wp
            if S["done"][q]:
                S["next_ids"][b0:b0 + Wp] = pad
                continue
            cs, cj, cc = [], [], []
            for j in range(Wp):
                b = b0 + j
                live = (j == 0) if t == 0 else S["beam_score"][b] > -np.inf
                if not live:
                    continue
                base = np.float32(0.0) if t == 0 else S["beam_score"][b]
                rc = B.row_candidates(logits[b], lo, hi, base, k_row)
                if rc is None:
                    S["status"][q] |= 1
                    continue
                cs.append(rc[0])
                cc.append(rc[1])
                cj.append(np.full(rc[0].size, j))
            ps = [float(x) for x in S["pool_score"][q]]
            pl = [int(x) for x in S["pool_len"][q]]
            pslot = [int(x) for x in S["pool_slot"][q]]
            count = int(S["pool_count"][q])
            src = {}                                      # slot -> (old row, last token)
            if cs:
                s, j_, c_ = np.concatenate(cs), np.concatenate(cj), np.concatenate(cc)
                n = np.zeros(s.size, np.float32)
                for c in chosen:
                    n += (c_ == c)
                with np.errstate(over="ignore"):
                    sel = np.maximum((s - n * lam32).astype(np.float32), -np.finfo(np.float32).max)
                order = np.lexsort((c_, j_, -sel.astype(np.float64)))
                s, sel, j_, c_ = s[order], sel[order], j_[order], c_[order]
                scale = max(1.0, float(np.abs(sel[:2 * Wp + 1]).max()))
                gaps = np.abs(np.diff(sel[:2 * Wp + 1].astype(np.float64)))
                if ((gaps > 0) & (gaps <= tol * scale)).any():
                    amb[q] = True
                s, j_, c_ = s[:2 * Wp], j_[:2 * Wp], c_[:2 * Wp]
            else:
                s = j_ = c_ = np.zeros(0)
                scale = 1.0
            if walked is not None:
                walked[q] = [(int(j), int(c)) for j, c in zip(j_, c_)]

            def offer(h, row, last, n_tok):
                nonlocal count
                h = float(h)
                if any(0 < abs(h - p) <= tol * scale for p in ps[:count]):
                    amb[q] = True
                pos = count
                while pos > 0 and ps[pos - 1] < h:
                    pos -= 1
                if pos >= Wp:
                    return
                if count < Wp:
                    slot = count
                    count += 1
                else:
                    slot = pslot[Wp - 1]
                for k in range(count - 1, pos, -1):
                    ps[k], pl[k], pslot[k] = ps[k - 1], pl[k - 1], pslot[k - 1]
                ps[pos], pl[pos], pslot[pos] = h, n_tok, slot
                src[slot] = (row, last)

            new = []                                      # (j, c, s)
            for r in range(len(s)):
                if len(new) == Wp:
                    break
                if int(c_[r]) == eos:
                    if r < Wp:
                        offer(np.float32(s[r] / den), b0 + int(j_[r]), eos, t)
                    continue
                new.append((int(j_[r]), int(c_[r]), np.float32(s[r])))
            if t == mx - 1:
                for j, c, sc in new:
                    offer(np.float32(sc / den), b0 + j, c, t + 1)
            if new:
                best = float(np.float32(max(sc for _, _, sc in new) / den))
                if count == Wp and 0 < abs(ps[Wp - 1] - best) <= tol * scale:
                    amb[q] = True
                done = count == Wp and ps[Wp - 1] >= best
            else:
                done = True
            S["pool_count"][q] = count
            S["done"][q] = int(done)
            if t > 0:
                S["switches"][q] += sum(1 for k, (j, _, _) in enumerate(new) if j != k)
            for k in range(Wp):
                b = b0 + k
                if k < len(new):
                    j, c, sc = new[k]
                    S["beam_score"][b] = sc
                    S["parent"][b] = b0 + j
                    S["tokens"][b, :t] = old_tokens[b0 + j, :t]
                    S["tokens"][b, t] = c
                    S["next_ids"][b] = pad if done else c
                else:
                    S["beam_score"][b] = -np.inf
                    S["parent"][b] = b
                    S["tokens"][b, t] = pad
                    S["next_ids"][b] = pad
            S["pool_score"][q] = ps
            S["pool_len"][q] = pl
            S["pool_slot"][q] = pslot
            for slot, (row, last) in src.items():
                S["pool_tokens"][q, slot] = pad
                S["pool_tokens"][q, slot, :t] = old_tokens[row, :t]
                S["pool_tokens"][q, slot, t] = last
            if not done:
                chosen.extend(c for _, c, _ in new)
    return S, amb


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
