"""NumPy restatement of db1_beam_step's rule (include/db1_hip.h), on the device layout of the state.

G groups of W beams, M = G * W rows, row b = g * W + j; step t chooses token t.  Per step:
  1. row candidates: columns c in [lo, hi) with a finite logit (fp32); lse_b = fp32 log-sum-exp over them; s = beam_score[b] + (l - lse_b);
  2. at t = 0 only j = 0 is live (beam_score not read); later the rows with beam_score > -inf; a live row without candidates sets status bit 0;
  3. the group's candidates sorted by s descending, ties by the lower (j, c); the first 2W are walked:
  4. EOS at rank < W -> a hypothesis (parent's tokens + EOS, n = t, score s / (t + 1)^alpha) offered to the pool; EOS at rank >= W dropped;
     any other candidate -> the next beam until W are filled; unfilled beams: score -inf, parent = themselves;
     the pool keeps its W best, sorted, equal scores: the earlier offer stays ahead (slots: a new slot while the pool is not full, else the
     evicted entry's slot);
  5. done when no beam was filled, or the pool is full and its worst score >= best new beam_score / (t + 1)^alpha;
  6. at t = max_new - 1 every new beam is offered with n = t + 1 and score beam_score / (t + 1)^alpha;
  7. output: the first R pool entries.
The lse here is float64 rounded to fp32 (the kernel's is an fp32 sum): scores agree to a few ulp, and ``step`` reports, per group, whether a
decision hinged on two scores closer than ``tol`` (relative to the scale of the scores) -- callers compare such groups with a slack."""
from __future__ import annotations

import numpy as np

STATE_KEYS = ("beam_score", "parent", "tokens", "pool_tokens", "pool_len", "pool_score", "pool_slot", "pool_count", "done", "switches",
              "status", "next_ids")


def new_state(G: int, W: int, max_new: int, pad: int = 0) -> dict:
    """the state before step 0 (what beam_search's start() writes on the device)"""
    M = G * W
    return dict(beam_score=np.zeros(M, np.float32), parent=np.arange(M, dtype=np.int32), tokens=np.full((M, max_new), pad, np.int32),
                pool_tokens=np.full((G, W, max_new), pad, np.int32), pool_len=np.zeros((G, W), np.int32),
                pool_score=np.full((G, W), -np.inf, np.float32), pool_slot=np.tile(np.arange(W, dtype=np.int32), (G, 1)),
                pool_count=np.zeros(G, np.int32), done=np.zeros(G, np.int32), switches=np.zeros(G, np.int32), status=np.zeros(G, np.int32),
                next_ids=np.zeros(M, np.int64))


def _lse32(x) -> np.float32:
    x = np.asarray(x, np.float64)
    m = x.max()
    return np.float32(m + np.log(np.exp(x - m).sum()))


def row_candidates(l, lo, hi, base, k=None):
    """-> (s float32 [<= k], c int [<= k]): the row's best k candidates (None: all of them) by (logit desc, column asc) and their scores"""
    l = np.asarray(l, np.float32)
    cols = np.arange(lo, hi)
    lw = l[lo:hi]
    fin = np.isfinite(lw)
    if not fin.any():
        return None
    cols, lw = cols[fin], lw[fin]
    lse = _lse32(lw)
    order = np.lexsort((cols, -lw.astype(np.float64)))[:k]
    s = (np.float32(base) + (lw[order] - lse).astype(np.float32)).astype(np.float32)
    return s, cols[order]


def step(S: dict, logits, t: int, W: int, lo: int, hi: int, eos: int = -1, pad: int = 0, alpha: float = 1.0, tol: float = 1e-5, D: int = 1,
         lam: float = 0.0, k_row=None, walked=None):
    """one step on a copy of the state ``S`` (new_state layout) and logits [M, V] (fp32; bf16 widened) -> (new state, ambiguous bool [G D]).
    The only restatement of the step: with ``D`` > 1 and ``lam`` the rule of tests/diverse_beam_rule.py over D sub-groups of W / D beams per
    prompt (``S``: G * D groups of W / D beams), of which the plain rule above is the case D = 1, lam = 0 (sel = s; the largest new score is
    the first).  ``k_row``: None ranks every candidate of a row, an int only the row's best k_row; ``walked`` (a dict) receives, per
    (sub-)group that chose, the (j, c) pairs of the first 2 W / D candidates in sel order"""
    S = {k: np.array(v, copy=True) for k, v in S.items()}
    M, mx = S["tokens"].shape
    Wp = W // D
    Q = M // Wp                                           # (sub-)groups
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
    chosen = []
    for q in range(Q):
        if q % D == 0:
            chosen = []                                   # the tokens the earlier sub-groups of this prompt chose
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
            rc = row_candidates(logits[b], lo, hi, base, k_row)
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
        src = {}                                          # slot -> (old row, last token)
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

        new = []                                          # (j, c, s)
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


def results(S: dict, W: int, R: int, pad: int = 0):
    """-> (ids [G, R, max_new], lengths [G, R], scores [G, R]) as beam_search returns them"""
    M, mx = S["tokens"].shape
    G = M // W
    ids = np.full((G, R, mx), pad, np.int32)
    lengths = np.zeros((G, R), np.int32)
    scores = np.full((G, R), -np.inf, np.float32)
    for g in range(G):
        k = min(R, int(S["pool_count"][g]))
        ids[g, :k] = S["pool_tokens"][g, S["pool_slot"][g, :k]]
        lengths[g, :k] = S["pool_len"][g, :k]
        scores[g, :k] = S["pool_score"][g, :k]
    return ids, lengths, scores


def search(next_logits, G: int, W: int, max_new: int, lo: int, hi: int, eos: int = -1, pad: int = 0, alpha: float = 1.0, R: int = 1):
    """the whole search with ``next_logits(histories)`` -> logits [M, V] of every row given its tokens so far (list of M int lists);
    stops early when every group is done.  -> (ids, lengths, scores, final state)"""
    S = new_state(G, W, max_new, pad)
    for t in range(max_new):
        hist = [list(S["tokens"][b, :t]) for b in range(G * W)]
        S, _ = step(S, next_logits(hist), t, W, lo, hi, eos, pad, alpha)
        if S["done"].all():
            break
    return results(S, W, R, pad) + (S,)
