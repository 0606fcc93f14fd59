"""NumPy restatement of the speculative-decoding rule (include/db1_hip.h: db1_spec_pick, db1_spec_accept, db1_spec_commit), on top of
``select_rule`` (which token a logits row picks) and ``logprob_rule`` (how likely it was).

A step feeds every row Q = 1 + k tokens: column 0 of ``ids`` is the last emitted token, columns 1 .. k are guesses for the token indices
t .. t + k - 1.  ``pick`` chooses for every position what the plain selection chooses there; ``accept`` keeps each row's choices up to its
first wrong guess, cuts every row to the shortest such run (one token counter, one ring origin), commits, and proposes the next guesses
from a script or by n-gram lookup over the row's history; ``commit`` advances the counter and takes the ring's origin back over what was
not kept.  ``State`` holds what the device holds; every function works in place on it."""
from __future__ import annotations

import numpy as np

import logprob_rule as L
import select_rule as R

SKIP, NONE = -2, -1
MAX_Q, MAX_HIST, MAX_NGRAM = 16, 4096, 8


class State:
    def __init__(self, M, Q, max_new, pad_id=0, logprobs=False, ring_state=None, cap=0):
        self.M, self.Q, self.max_new, self.pad = M, Q, max_new, pad_id
        self.t = 0
        self.finished = np.zeros(M, bool)
        self.lengths = np.zeros(M, np.int64)
        self.status = np.zeros(M, np.int64)
        self.out = np.full((M, max_new), pad_id, np.int64)
        self.logprob = np.zeros((M, max_new), np.float32) if logprobs else None
        self.sums = np.zeros(M, np.float32) if logprobs else None
        self.ids = np.zeros((M, Q), np.int64)
        self.sel = np.zeros((M, Q), np.int64)
        self.hit = np.zeros((M, Q), np.int64)
        self.lp = np.zeros((M, Q), np.float32)
        self.n_acc = 0
        self.hist = np.zeros(Q + 1, np.int64)
        self.ring_state, self.cap = ring_state, cap


def pick(st: State, logits, q_in, lo, hi, step_base=0, stream_ids=None, **sel):
    """launch 1: ``logits`` float64 [M * q_in, V] -> st.sel / st.hit / st.lp [:, :q_in]; nothing else of the state is written.  ``sel``:
    what ``select_rule.select_row`` takes after the window (greedy, temperature, top_k, top_p, seed)."""
    logits = np.asarray(logits, np.float64)
    for r in range(st.M):
        sid = r if stream_ids is None else int(stream_ids[r])
        for i in range(q_in):
            tau = st.t + i
            st.hit[r, i] = 0
            st.lp[r, i] = 0.0
            if st.finished[r] or not 0 <= tau < st.max_new:
                st.sel[r, i] = SKIP
                continue
            row = logits[r * q_in + i]
            tok = R.select_row(row, lo, hi, stream_id=sid, step=step_base + tau, **sel)[0]
            if not L.candidates(row, lo, hi).any():
                tok = NONE
            st.sel[r, i] = tok
            if tok >= 0:
                st.lp[r, i] = np.float32(L.logprob(row, tok, lo, hi))
            st.hit[r, i] = int(i + 1 < q_in and st.ids[r, i + 1] == tok)


def row_emits(st: State, r, q_in, eos_id):
    """the emissions of a live row: it stops after position i when the row ends there, at the last token index, at the call's last position
    or at a wrong guess"""
    i = 0
    while True:
        v = st.sel[r, i]
        if v == NONE or v == eos_id or st.t + i + 1 == st.max_new or i == q_in - 1 or st.hit[r, i] == 0:
            return i + 1
        i += 1


def find_ngram(h, ng_min, ng_max):
    """-> (p, g): the longest n-gram length g in [ng_min, ng_max] (n > g) whose copy of the history's last g tokens starts at some
    p <= n - g - 1, and the LARGEST such p; None without a match"""
    n = len(h)
    for g in range(ng_max, ng_min - 1, -1):
        if n <= g:
            continue
        for p in range(n - g - 1, -1, -1):
            if list(h[p:p + g]) == list(h[n - g:n]):
                return p, g
    return None


def drafts(h, k, V, pad_id, finished=False, script_row=None, t2=0, max_new=0, ng_min=1, ng_max=3):
    """the k guesses after the history ``h`` (the prompt's text tokens, then the row's output up to the new counter ``t2``)"""
    n = len(h)
    if finished or n == 0:
        return [pad_id] * k
    if script_row is not None:
        return [int(script_row[t2 + j]) if t2 + j < max_new and 0 <= int(script_row[t2 + j]) < V else int(h[n - 1]) for j in range(k)]
    m = find_ngram(h, ng_min, ng_max)
    if m is None:
        return [int(h[n - 1])] * k
    p, g = m
    Lp = n - (p + g)
    return [int(h[p + g + j % Lp]) for j in range(k)]


def accept(st: State, q_in, V, eos_id=-1, ctx=None, ctx_len=None, script=None, ng_min=1, ng_max=3):
    """launch 2: st.n_acc, the rows' books, column 0 of st.ids and the next guesses"""
    t, mx = st.t, st.max_new
    if not 0 <= t <= mx:
        st.status |= 2
        st.n_acc = 0
        return
    if t == mx:
        st.n_acc = 0
        return
    live = [r for r in range(st.M) if st.sel[r, 0] != SKIP]
    n_acc = min((row_emits(st, r, q_in, eos_id) for r in live), default=0)
    st.n_acc = n_acc
    for r in range(st.M):
        if r not in live:
            for i in range(n_acc):
                st.out[r, t + i] = st.pad
                if st.logprob is not None:
                    st.logprob[r, t + i] = 0.0
        else:
            for i in range(n_acc):
                v = int(st.sel[r, i])
                if v == NONE:
                    st.out[r, t + i] = st.pad
                    if st.logprob is not None:
                        st.logprob[r, t + i] = 0.0
                    st.status[r] |= 1
                    st.finished[r] = True
                else:
                    st.out[r, t + i] = v
                    if st.logprob is not None:
                        st.logprob[r, t + i] = st.lp[r, i]
                        st.sums[r] = np.float32(st.sums[r] + st.lp[r, i])     # (one fp32 add per token, in token order)
                    if v == eos_id:
                        st.finished[r] = True
                    else:
                        st.lengths[r] += 1
        if n_acc > 0:
            st.ids[r, 0] = st.pad if st.finished[r] else st.sel[r, n_acc - 1]
        t2 = t + n_acc
        nc = 0 if ctx is None else min(max(int(ctx_len[r]), 0), ctx.shape[1])
        h = ([] if ctx is None else [int(v) for v in ctx[r, :nc]]) + [int(v) for v in st.out[r, :t2]]
        st.ids[r, 1:] = drafts(h, st.Q - 1, V, st.pad, bool(st.finished[r]), None if script is None else script[r], t2, mx, ng_min, ng_max)


def commit(st: State, q_in, count=True):
    """launch 3"""
    n = min(max(int(st.n_acc), 0), q_in)
    st.t += n
    if st.ring_state is not None:
        st.ring_state = (st.ring_state + st.cap - (q_in - n)) % st.cap
    if count:
        st.hist[n] += 1


def step(st: State, logits, q_in, lo, hi, V, eos_id=-1, ctx=None, ctx_len=None, script=None, ng_min=1, ng_max=3, count=True, **sel):
    pick(st, logits, q_in, lo, hi, **sel)
    accept(st, q_in, V, eos_id, ctx, ctx_len, script, ng_min, ng_max)
    commit(st, q_in, count)


def generate(model, M, Q, max_new, lo, hi, V, eos_id=-1, pad_id=0, ctx=None, ctx_len=None, script=None, ng_min=1, ng_max=3, logprobs=False,
             max_steps=None, **sel):
    """the whole loop over ``model(r, prefix) -> logits float64 [V]`` (``prefix``: the tokens row r has been fed after its prompt): token 0
    from the prefill (q_in = 1, not counted in hist), then steps of Q positions until every row has finished or the counter is at the end
    -> the state.  The forward of a step sees, per row, its committed output followed by the guesses in st.ids[:, 1:]."""
    st = State(M, Q, max_new, pad_id, logprobs)
    logits = np.stack([model(r, []) for r in range(M)])
    step(st, logits, 1, lo, hi, V, eos_id, ctx, ctx_len, script, ng_min, ng_max, count=False, **sel)
    steps = 0
    while st.t < max_new and not st.finished.all() and (max_steps is None or steps < max_steps):
        rows = []
        for r in range(M):
            fed = [int(v) for v in st.out[r, :st.t - 1]] + [int(v) for v in st.ids[r]]
            rows += [model(r, fed[:st.t + i]) for i in range(Q)]
        step(st, np.stack(rows), Q, lo, hi, V, eos_id, ctx, ctx_len, script, ng_min, ng_max, **sel)
        steps += 1
    return st


def generate_plain(model, M, max_new, lo, hi, eos_id=-1, pad_id=0, **sel):
    """the one-token loop of db1_select_tokens_lp over the same model -> (out, lengths, logprob float32, sums float32, status)"""
    out = np.full((M, max_new), pad_id, np.int64)
    lengths, status = np.zeros(M, np.int64), np.zeros(M, np.int64)
    finished = np.zeros(M, bool)
    logprob, sums = np.zeros((M, max_new), np.float32), np.zeros(M, np.float32)
    for t in range(max_new):
        for r in range(M):
            if finished[r]:
                continue
            row = model(r, [int(v) for v in out[r, :t]])
            tok = R.select_row(row, lo, hi, stream_id=r, step=t, **sel)[0]
            if not L.candidates(row, lo, hi).any():
                status[r] |= 1
                finished[r] = True
                continue
            out[r, t] = tok
            lp = np.float32(L.logprob(row, tok, lo, hi))
            logprob[r, t] = lp
            sums[r] = np.float32(sums[r] + lp)
            if tok == eos_id:
                finished[r] = True
            else:
                lengths[r] += 1
    return out, lengths, logprob, sums, status


def step_counts(n, Q):
    """(accepted histogram of a perfect script, of an always-wrong one) for n new tokens: the GPU generation test expects them of the device"""
    perfect, wrong = np.zeros(Q + 1, np.int64), np.zeros(Q + 1, np.int64)
    perfect[Q] = (n - 1) // Q
    if (n - 1) % Q:
        perfect[(n - 1) % Q] += 1
    wrong[1] = n - 1
    return perfect, wrong



# the histories of the draft rule: (history, ngram_min, ngram_max, k, the drafts); the CPU test checks the rule on them, the GPU test the kernel
DRAFT_CASES = [
    ([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 1, 3, 4, [8, 1, 2, 3]),                  # the latest match of [1 2 3] wins (p = 4, not 0)
    ([5, 6, 7, 1, 9, 7, 2, 9, 5, 6, 7], 1, 3, 3, [1, 9, 7]),                     # the 3-gram at p = 0 beats the more recent 1-gram [7] at p = 5
    ([5, 6, 7, 1, 9, 7, 2, 9, 5, 6, 7], 1, 1, 3, [2, 9, 5]),                     # ... which wins once only 1-grams are looked at
    ([4, 4], 1, 3, 5, [4, 4, 4, 4, 4]),                                          # L = 1: the loop [4] goes on
    ([3, 7, 3, 7, 3], 2, 3, 5, [7, 3, 7, 3, 7]),                                 # L = 2 (p = 0, g = 3: continue at 3 with [7, 3], periodically)
    ([1, 2, 3, 4], 1, 3, 3, [4, 4, 4]),                                          # no match: the last token
    ([6], 1, 3, 2, [6, 6]),                                                      # n <= g for every g: no match
]
