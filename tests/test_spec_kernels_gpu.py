"""db1_spec_pick / db1_spec_accept / db1_spec_commit on synthetic logits, without a model.

The pick: sel[r, i] and lp[r, i] are, bit for bit, what db1_select_tokens[_lp] writes for that logits row with *t = t + i (the device's own
sibling: no float64 slack at a top-p threshold).  The rest -- hit, the accepted count, the books, the next ids and drafts, the counter, the
ring origin and the histogram -- against tests/spec_rule.py fed with the device's picks: one step from a planted state (full accept, a miss
at position 0 and in the middle, rows that stop at different positions, EOS inside an accepted run, a finished row among live ones, all
rows finished, the end of the output inside the call, the counter at the end and out of range; ties, NaN, +-inf and a row without a
candidate in the logits), then five steps from the device's own state with lookup drafts.  Every buffer starts filled with a sentinel.
Then the draft histories of tests/test_spec_cpu.py and one of 4096 tokens, the commit's wrap-around, determinism and every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401
import spec_rule as S  # noqa: E402
DRAFT_CASES = S.DRAFT_CASES

MAXNEW, PAD, SENT, FSENT, STEP_BASE, CAP = 24, 31, -7, -7.5, 3, 104
SHAPES = [(200, 208, 3, 190), (5000, 5000, 0, 5000), (33025, 33280, 0, 32000)]     # V, ld, window: NG 1 / 3 / 9
DTYPES = [torch.float32, torch.bfloat16]
SAMPLING = {"greedy": dict(greedy=True), "top_p": dict(greedy=False, temperature=0.8, top_k=0, top_p=0.9, seed=(1 << 40) + 12345)}
SID = [11, 7, 300]


def _logits(rng, M, q_in, V, ld, lo, hi, dtype, special=True):
    lg = (rng.standard_normal((M * q_in, ld)) * 3).astype(np.float32)
    if special:
        lg[0, lo + 5] = np.inf                          # never a candidate
        lg[0, lo + 9] = np.nan
        lg[0, lo + 11] = -np.inf
        lg[0, [lo + 20, lo + 40]] = 50.0                # a tie at the top of row 0, position 0: the lower column
        if hi < V:
            lg[0, hi + 2] = 1e9                         # outside the window
        if M > 1:                                       # row 1 has no candidate at position min(2, q_in - 1)
            lg[q_in + min(2, q_in - 1), lo:hi] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, hi - lo)]
    return _tdev(lg).to(dtype)


class _Dev:
    """the device state of a speculative generation, sentinel-filled where a launch must not write, and its mirror in the rule"""

    def __init__(self, M, Q, t0=0, fin=None, lp=True, ring=50, ctx=None, ctx_len=None, script=None):
        i32 = lambda a: _tdev(np.asarray(a, np.int32))
        self.M, self.Q, self.has_lp = M, Q, lp
        fin = [0] * M if fin is None else fin
        self.t, self.finished, self.lengths, self.status = i32([t0]), i32(fin), i32([max(t0, 0)] * M), i32([0] * M)
        self.sid = i32(SID[:M])
        self.out = torch.full((M, MAXNEW), SENT, dtype=torch.int32, device=DEV)
        self.ids = torch.full((M, Q), 1, dtype=torch.int64, device=DEV)
        self.sel, self.hit = (torch.full((M, Q), SENT, dtype=torch.int32, device=DEV) for _ in range(2))
        self.lp = torch.full((M, Q), FSENT, dtype=torch.float32, device=DEV) if lp else None
        self.logprob = torch.full((M, MAXNEW), FSENT, dtype=torch.float32, device=DEV) if lp else None
        self.sum_logprob = _tdev(np.linspace(-1, -2, M).astype(np.float32)) if lp else None
        self.n_acc, self.hist, self.ring = i32([SENT]), i32([0] * (Q + 1)), i32([ring])
        self.ctx = None if ctx is None else i32(ctx)
        self.ctx_len = None if ctx is None else i32(ctx_len)
        self.script = None if script is None else i32(script)
        st = self.st = S.State(M, Q, MAXNEW, PAD, lp, ring_state=ring, cap=CAP)
        st.t, st.finished[:], st.lengths[:] = t0, np.asarray(fin, bool), max(t0, 0)
        st.out[:], st.ids[:] = SENT, 1
        if lp:
            st.logprob[:], st.sums[:] = FSENT, self.sum_logprob.cpu().numpy()
        self.np_ctx, self.np_ctx_len, self.np_script = ctx, ctx_len, script

    def set_ids(self, ids):
        self.ids.copy_(_tdev(np.asarray(ids, np.int64)))
        self.st.ids[:] = ids

    def pick(self, lg, q_in, V, lo, hi, kw):
        from bdm_db1_amd import ops
        ops.spec_pick(lg, self.t, self.finished, self.ids, self.sel, self.hit, q_in=q_in, V=V, vocab_lo=lo, vocab_hi=hi, pad_id=PAD,
                      step_base=STEP_BASE, stream_id=self.sid, lp=self.lp, max_new=MAXNEW, **kw)

    def expected_pick(self, lg, q_in, V, lo, hi, kw):
        """what db1_select_tokens[_lp] writes for every position's logits row at *t = t + i, on copies of the state -> (sel, lp)"""
        from bdm_db1_amd import ops
        M, t0 = self.M, int(self.t.cpu())
        sel, lp = np.full((M, q_in), S.SKIP, np.int64), np.zeros((M, q_in), np.float32)
        rows = lg.view(M, q_in, lg.shape[1])
        for i in range(q_in):
            if not 0 <= t0 + i < MAXNEW:
                continue
            fin, lens, status = self.finished.clone(), self.lengths.clone(), torch.zeros_like(self.status)
            out = torch.full((M, MAXNEW), SENT, dtype=torch.int32, device=DEV)
            nxt = torch.zeros(M, dtype=torch.int64, device=DEV)
            extra = {}
            if self.has_lp:
                extra = dict(logprob=torch.zeros(M, MAXNEW, dtype=torch.float32, device=DEV), sum_logprob=torch.zeros(M, dtype=torch.float32, device=DEV))
            ops.select_tokens(rows[:, i], _tdev(np.array([t0 + i], np.int32)), fin, lens, out, nxt, status, V=V, vocab_lo=lo, vocab_hi=hi, pad_id=PAD,
                              step_base=STEP_BASE, stream_id=self.sid, eos_id=-1, **extra, **kw)
            o, stt, was = out[:, t0 + i].cpu().numpy(), status.cpu().numpy(), self.finished.cpu().numpy()
            for r in range(M):
                if was[r]:
                    continue
                sel[r, i] = S.NONE if stt[r] & 1 else o[r]
                if self.has_lp:
                    lp[r, i] = extra["logprob"][r, t0 + i].item()
        return sel, lp

    def step(self, lg, q_in, V, lo, hi, kw, eos=-1, ng=(1, 3), check_pick=True):
        """pick (checked against the sibling), accept and commit on the device; the rule on the mirror; every buffer compared"""
        from bdm_db1_amd import ops
        st = self.st
        self.sel.fill_(SENT); self.hit.fill_(SENT)
        if self.has_lp:
            self.lp.fill_(FSENT)
        self.pick(lg, q_in, V, lo, hi, kw)
        sel, hit = self.sel.cpu().numpy(), self.hit.cpu().numpy()
        lp = self.lp.cpu().numpy() if self.has_lp else np.zeros((self.M, self.Q), np.float32)
        assert (sel[:, q_in:] == SENT).all() and (hit[:, q_in:] == SENT).all() and (not self.has_lp or (lp[:, q_in:] == FSENT).all())
        if check_pick:
            want_sel, want_lp = self.expected_pick(lg, q_in, V, lo, hi, kw)
            assert np.array_equal(sel[:, :q_in], want_sel), (sel[:, :q_in], want_sel)
            if self.has_lp:
                assert np.array_equal(lp[:, :q_in].view(np.int32), want_lp.view(np.int32))
        st.sel[:, :q_in], st.lp[:, :q_in] = sel[:, :q_in], lp[:, :q_in]
        for r in range(self.M):
            for i in range(q_in):
                st.hit[r, i] = int(i + 1 < q_in and st.ids[r, i + 1] == st.sel[r, i])
        assert np.array_equal(hit[:, :q_in], st.hit[:, :q_in])
        lpkw = dict(lp=self.lp, logprob=self.logprob, sum_logprob=self.sum_logprob) if self.has_lp else {}
        ops.spec_accept(self.t, self.sel, self.hit, self.finished, self.lengths, self.out, self.status, self.ids, self.n_acc, q_in=q_in, V=V, eos_id=eos,
                        pad_id=PAD, ctx=self.ctx, ctx_len=self.ctx_len, script=self.script, ngram_min=ng[0], ngram_max=ng[1], **lpkw)
        ops.spec_commit(self.t, self.n_acc, q_in=q_in, Q=self.Q, hist=self.hist, ring_state=self.ring, cap=CAP)
        S.accept(st, q_in, V, eos, self.np_ctx, self.np_ctx_len, self.np_script, ng[0], ng[1])
        S.commit(st, q_in)
        self.compare()

    def snap(self):
        torch.cuda.synchronize()
        keys = ("t", "finished", "lengths", "status", "out", "ids", "n_acc", "hist", "ring", "sel", "hit") + (("lp", "logprob", "sum_logprob") if self.has_lp else ())
        return {k: getattr(self, k).cpu().numpy().copy() for k in keys}

    def compare(self):
        g, st = self.snap(), self.st
        assert int(g["n_acc"][0]) == st.n_acc and int(g["t"][0]) == st.t and int(g["ring"][0]) == st.ring_state
        assert np.array_equal(g["hist"], st.hist)
        assert np.array_equal(g["finished"] != 0, st.finished) and np.array_equal(g["lengths"], st.lengths) and np.array_equal(g["status"], st.status)
        assert np.array_equal(g["out"], st.out), (g["out"], st.out)
        assert np.array_equal(g["ids"], st.ids), (g["ids"], st.ids)
        if self.has_lp:
            assert np.array_equal(g["logprob"].view(np.int32), st.logprob.view(np.int32))
            assert np.array_equal(g["sum_logprob"].view(np.int32), st.sums.view(np.int32))


def _plant(d, lg, q_in, V, lo, hi, kw, miss):
    """drafts that are right (the device's own picks) except at each row's position ``miss[r]`` (None: nowhere)"""
    d.pick(lg, q_in, V, lo, hi, kw)
    sel = d.sel.cpu().numpy()
    ids = d.st.ids.copy()
    for r in range(d.M):
        for i in range(q_in - 1):
            ids[r, i + 1] = sel[r, i] if sel[r, i] >= 0 else 1
            if miss[r] is not None and i == miss[r]:
                ids[r, i + 1] = (sel[r, i] + 1) if sel[r, i] + 1 < hi else lo
    d.set_ids(ids)
    return sel


@pytest.mark.parametrize("lp", [False, True], ids=["plain", "lp"])
@pytest.mark.parametrize("sampling", sorted(SAMPLING))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"V{s[0]}" for s in SHAPES])
def test_one_planted_step_then_five_from_the_devices_own_state(shape, dtype, sampling, lp):
    V, ld, lo, hi = shape
    kw = SAMPLING[sampling]
    rng = np.random.default_rng(V + 7)
    for M in (1, 3):
        for q_in in (1, 2, 5, 16):
            Q = max(q_in, 2)
            lg = _logits(rng, M, q_in, V, ld, lo, hi, dtype)
            none = [None] * M
            scenarios = [("full", dict(), none, False), ("miss0", dict(), [0] * M, False), ("missmid", dict(), [q_in // 2] * M, False),
                         ("ragged", dict(), [(r + 1) % q_in for r in range(M)], False), ("eos", dict(), none, True),
                         ("onefin", dict(fin=[0] * (M - 1) + [1]), none, False), ("allfin", dict(fin=[1] * M), none, False),
                         ("tail", dict(t0=MAXNEW - 2), none, False), ("end", dict(t0=MAXNEW), none, False),
                         ("below", dict(t0=-1), none, False), ("above", dict(t0=MAXNEW + 1), none, False)]
            for name, init, miss, with_eos in scenarios:
                d = _Dev(M, Q, lp=lp, ring=2 if name in ("miss0", "allfin") else 50, **init)
                sel0 = _plant(d, lg, q_in, V, lo, hi, kw, miss)
                eos = int(sel0[0, min(1, q_in - 1)]) if with_eos and sel0[0, min(1, q_in - 1)] >= 0 else -1
                before = int(d.ring.cpu())
                d.step(lg, q_in, V, lo, hi, kw, eos=eos)
                g = d.snap()
                n = int(g["n_acc"][0])
                if name in ("allfin", "end", "below", "above"):
                    assert n == 0 and int(g["ring"][0]) == (before + CAP - q_in) % CAP and g["hist"][0] == 1
                    assert ((g["status"] == 2).all() if name in ("below", "above") else not g["status"].any())
                if name == "full" and M == 1:
                    assert n == q_in
                if name == "miss0":
                    assert n == 1
                if name == "tail":
                    assert n == min(2, q_in) and int(g["t"][0]) <= MAXNEW
                if name == "eos" and eos >= 0 and q_in > 1 and M == 1:
                    assert n == 2 and g["finished"][0] == 1 and g["lengths"][0] == 1
            # five steps from the device's own state: lookup drafts over a ragged prompt text, a small window so that n-grams recur
            ctx = rng.integers(lo, lo + 6, size=(M, 9))
            d = _Dev(M, Q, lp=lp, ctx=ctx, ctx_len=[9, 0, 4][:M])
            for s in range(5):
                lg2 = _logits(rng, M, q_in, V, ld, lo, lo + 6, dtype, special=False)
                d.step(lg2, q_in, V, lo, lo + 6, kw, ng=(1, 3), check_pick=s == 0)
            assert d.st.hist.sum() == 5


def _accept_alone(hist_rows, nc, Q, V, ng, max_new, script=None, pad=PAD):
    """db1_spec_accept on hand-made picks: every row's history is ctx[:nc] + out[:t] + the one token this step commits"""
    from bdm_db1_amd import ops
    M, n = len(hist_rows), len(hist_rows[0])
    t0 = n - nc - 1
    i32 = lambda a: _tdev(np.ascontiguousarray(a, np.int32))
    h = np.asarray(hist_rows, np.int64)
    out = np.full((M, max_new), SENT, np.int32)
    out[:, :t0] = h[:, nc:n - 1]
    sel = np.full((M, Q), S.SKIP, np.int32)
    sel[:, 0] = h[:, n - 1]
    ids = torch.full((M, Q), 1, dtype=torch.int64, device=DEV)
    n_acc = i32([SENT])
    dv_out = i32(out)
    ops.spec_accept(i32([t0]), i32(sel), i32(np.zeros((M, Q))), i32([0] * M), i32([t0] * M), dv_out, i32([0] * M), ids, n_acc, q_in=1, V=V, pad_id=pad,
                    ctx=i32(h[:, :nc]) if nc else None, ctx_len=i32([nc] * M) if nc else None, script=None if script is None else i32(script),
                    ngram_min=ng[0], ngram_max=ng[1])
    torch.cuda.synchronize()
    assert int(n_acc.cpu()) == 1 and np.array_equal(dv_out.cpu().numpy()[:, :t0 + 1], h[:, nc:])
    return ids.cpu().numpy()


@pytest.mark.parametrize("case", range(len(DRAFT_CASES)))
def test_draft_histories_of_the_cpu_test(case):
    h, lo, hi, k, want = DRAFT_CASES[case]
    for nc in sorted({0, 2, len(h) - 1} & set(range(len(h)))):         # the seam between the prompt text and the output at three places
        got = _accept_alone([h, h[::-1]], nc, k + 1, 48, (lo, hi), 16)
        assert list(got[0]) == [h[-1]] + want, (nc, got)
        assert list(got[1, 1:]) == S.drafts(h[::-1], k, 48, PAD, ng_min=lo, ng_max=hi)


def test_a_history_of_4096_tokens_and_the_script():
    rng = np.random.default_rng(5)
    h = [list(rng.integers(0, 6, 4096)), list(rng.integers(0, 3000, 4096))]
    h[1][100:104] = h[1][-4:]                                        # one planted 4-gram early in a history that hardly repeats
    for ng in ((1, 8), (5, 8), (1, 1)):
        got = _accept_alone(h, 4000, 16, 3000, ng, 96)
        for r in range(2):
            assert list(got[r, 1:]) == S.drafts(h[r], 15, 3000, PAD, ng_min=ng[0], ng_max=ng[1]), (ng, r)
    assert _accept_alone(h, 4000, 16, 3000, (3, 8), 96)[1, 1] == h[1][104]          # the planted 4-gram, continued
    # script mode: values outside [0, V) and indices past the end fall back to the history's last token
    hs = [[9, 1, 4], [9, 1, 4]]
    sc = np.array([[3, 4, 5, -1, 48, 7, 8, 9], [0] * 8])
    got = _accept_alone(hs, 1, 8, 48, (1, 3), 8, script=sc)           # t' = 2: script[2:] = 5, -1, 48, 7, 8, 9, then past the end
    assert list(got[0]) == [4, 5, 4, 4, 7, 8, 9, 4] and list(got[1]) == [4] + [0] * 6 + [4]


def test_commit_wraps_and_counts():
    from bdm_db1_amd import ops
    i32 = lambda a: _tdev(np.asarray(a, np.int32))
    for ring, n, q_in, want in ((2, 1, 5, 102), (0, 0, 16, 88), (103, 5, 5, 103), (3, 2, 5, 0)):
        t, hist, state = i32([4]), i32([0] * 17), i32([ring])
        ops.spec_commit(t, i32([n]), q_in=q_in, Q=16, hist=hist, ring_state=state, cap=CAP)
        ops.spec_commit(t, i32([n]), q_in=q_in, Q=16)                   # (neither a ring nor a histogram: the prefill's form)
        assert int(state.cpu()) == want and int(t.cpu()) == 4 + 2 * n
        assert int(hist.cpu()[n]) == 1 and int(hist.sum().cpu()) == 1


def test_two_runs_give_the_same_bits():
    V, ld, lo, hi = SHAPES[1]
    snaps = []
    for _ in range(2):
        rng = np.random.default_rng(99)
        d = _Dev(3, 5, lp=True, ctx=rng.integers(0, 6, size=(3, 9)), ctx_len=[9, 0, 4])
        for s in range(4):
            d.step(_logits(rng, 3, 5, V, ld, 0, 6, torch.bfloat16, special=False), 5, V, 0, 6, SAMPLING["top_p"], check_pick=False)
        snaps.append(d.snap())
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k].view(np.int32) if snaps[0][k].dtype == np.float32 else snaps[0][k],
                              snaps[1][k].view(np.int32) if snaps[1][k].dtype == np.float32 else snaps[1][k]), k


def test_every_refusal_with_its_code_and_nothing_launched():
    from bdm_db1_amd import lib, ops
    L = lib.load()
    BAD, UNSUP, DT = -1, -6, -3
    vp = ctypes.c_void_p
    M, Q, V, ld = 2, 5, 200, 208
    d = _Dev(M, Q, lp=True, ctx=np.zeros((M, 6), np.int64), ctx_len=[6, 6])
    lg = _logits(np.random.default_rng(1), M, Q, V, ld, 0, V, torch.float32)
    before = d.snap()
    p = lambda x: vp(0) if x is None else vp(x.data_ptr())

    def pick(**kw):
        a = dict(logits=p(lg), M=M, q_in=Q, Q=Q, V=V, ld=ld, dt=0, lo=0, hi=V, temp=1.0, top_k=0, top_p=1.0, greedy=1, t=p(d.t), fin=p(d.finished),
                 mx=MAXNEW, ids=p(d.ids), sel=p(d.sel), hit=p(d.hit), lp=p(d.lp))
        a.update(kw)
        return L.db1_spec_pick(a["logits"], a["M"], a["q_in"], a["Q"], a["V"], a["ld"], a["dt"], a["lo"], a["hi"], a["temp"], a["top_k"], a["top_p"],
                               a["greedy"], 0, 0, PAD, 0, a["t"], p(d.sid), a["fin"], a["mx"], a["ids"], a["sel"], a["hit"], a["lp"], ops.stream())

    for kw, code in ((dict(dt=7), DT), (dict(logits=vp(0)), BAD), (dict(t=vp(0)), BAD), (dict(fin=vp(0)), BAD), (dict(ids=vp(0)), BAD), (dict(sel=vp(0)), BAD),
                     (dict(hit=vp(0)), BAD), (dict(q_in=0), BAD), (dict(q_in=6), BAD), (dict(Q=1, q_in=1), BAD), (dict(Q=17), BAD), (dict(M=0), BAD),
                     (dict(M=13108), BAD), (dict(lo=5, hi=5), BAD), (dict(hi=V + 1), BAD), (dict(lo=-1), BAD), (dict(ld=V - 1), BAD), (dict(mx=0), BAD),
                     (dict(V=40000, ld=40000, hi=40000), UNSUP), (dict(greedy=0, temp=0.0), BAD), (dict(greedy=0, top_p=0.0), BAD), (dict(greedy=0, top_k=-1), BAD)):
        assert pick(**kw) == code, kw

    def accept(**kw):
        a = dict(M=M, q_in=Q, Q=Q, V=V, mx=MAXNEW, t=p(d.t), sel=p(d.sel), hit=p(d.hit), lp=p(d.lp), fin=p(d.finished), lens=p(d.lengths), out=p(d.out),
                 status=p(d.status), logprob=p(d.logprob), sums=p(d.sum_logprob), ids=p(d.ids), ctx=p(d.ctx), ctx_len=p(d.ctx_len), ctx_cap=6,
                 script=vp(0), ng_min=1, ng_max=3, n_acc=p(d.n_acc))
        a.update(kw)
        return L.db1_spec_accept(a["M"], a["q_in"], a["Q"], -1, PAD, a["V"], a["mx"], a["t"], a["sel"], a["hit"], a["lp"], a["fin"], a["lens"], a["out"],
                                 a["status"], a["logprob"], a["sums"], a["ids"], a["ctx"], a["ctx_len"], a["ctx_cap"], a["script"], a["ng_min"], a["ng_max"],
                                 a["n_acc"], ops.stream())

    for kw, code in ((dict(t=vp(0)), BAD), (dict(sel=vp(0)), BAD), (dict(hit=vp(0)), BAD), (dict(fin=vp(0)), BAD), (dict(lens=vp(0)), BAD), (dict(out=vp(0)), BAD),
                     (dict(status=vp(0)), BAD), (dict(ids=vp(0)), BAD), (dict(n_acc=vp(0)), BAD), (dict(lp=vp(0)), BAD), (dict(logprob=vp(0)), BAD),
                     (dict(sums=vp(0)), BAD), (dict(ctx=vp(0)), BAD), (dict(ctx_len=vp(0)), BAD), (dict(ctx_cap=0), BAD), (dict(ctx_cap=-1), BAD),
                     (dict(q_in=0), BAD), (dict(q_in=6), BAD), (dict(Q=1, q_in=1), BAD), (dict(Q=17), BAD), (dict(M=0), BAD), (dict(M=13108), BAD), (dict(V=0), BAD),
                     (dict(mx=0), BAD), (dict(ng_min=0), BAD), (dict(ng_max=9), BAD), (dict(ng_min=3, ng_max=2), BAD),
                     (dict(ctx_cap=4096 - MAXNEW + 1), UNSUP), (dict(mx=4091), UNSUP)):
        assert accept(**kw) == code, kw
    commit = lambda t=p(d.t), n=p(d.n_acc), q_in=Q, QQ=Q, ring=p(d.ring), cap=CAP: L.db1_spec_commit(t, n, p(d.hist), q_in, QQ, ring, cap, ops.stream())
    for kw in (dict(t=vp(0)), dict(n=vp(0)), dict(q_in=0), dict(q_in=6), dict(QQ=1, q_in=1), dict(QQ=17), dict(cap=0), dict(cap=-5), dict(cap=4)):
        assert commit(**kw) == BAD, kw
    after = d.snap()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=before[k].dtype == np.float32), k          # nothing was launched
    assert L.db1_spec_pick_supported(33025, 33280, 1, 16) and not L.db1_spec_pick_supported(33025, 33280, 1, 17)
    assert not L.db1_spec_pick_supported(36865, 36865, 1, 5) and L.db1_spec_accept_supported(16, 4000, 96, 1, 8)
    assert not L.db1_spec_accept_supported(16, 4001, 96, 1, 8) and not L.db1_spec_accept_supported(16, 0, 96, 2, 1)
    assert L.db1_spec_commit_supported(2, 1) and not L.db1_spec_commit_supported(2, 0)
    assert ops.spec_supported(33025, 33280, torch.bfloat16, 5, 4066, 30, 1, 3, 1088)
