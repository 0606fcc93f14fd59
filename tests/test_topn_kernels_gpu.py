"""db1_select_tokens_top / db1_select_tokens_slots_top and db1_score_rows_top / db1_lmhead_score_top through ``ops``: the alternatives against
the float64 rule of tests/topn_rule.py (ids exactly, log-probs within the bound of the log-prob and score kernel tests), the exact
consequences of the rule as bit comparisons, every other output bit-equal to the parent entry point on clones of the same inputs, and
sentinels where a launch must not write.  One case per NG branch of the selection and per thread count of the fp32 row kernel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import score_rule as SR  # noqa: E402
import topn_rule as T  # noqa: E402
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

# the bound of tests/test_select_logprob_gpu.py and tests/test_score_kernels_gpu.py: both sides subtract the same maximum and sum at most
# 2^16 positive terms in different orders, good to ~2e-6 absolute after the log
TOL = 1e-5
MAXNEW, PAD, SENT, SUM0 = 3, 0, -7, 1.5
NS = [1, 5, 16]
SEL_SHAPES = [(4096, 4096), (4097, 4160), (12289, 12352), (33025, 33280)]       # NG 1 (full), 3, 9, 9 (DB1-1.3B's vocabulary and row stride)
MODES = {"greedy": dict(greedy=True), "top_p": dict(greedy=False, top_p=0.9, seed=78)}
FEW = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32)                    # exact in bf16; no zero: its sign is a rule of its own
M_ROWS = 6
_CACHE = {}


def _case(V, ld, dtype):
    """(device logits [6, ld], their values as stored in float64 [6, V]) -- made once per shape and dtype, never changed.  Row 0: normal; row
    1: six distinct values, so ties span threads and waves; row 2: all -inf; row 3: normal with the -inf holes db1_constrain_logits leaves,
    a +inf and NaNs; row 4: six distinct values with holes; row 5: a copy of row 0, the caller's to mark finished.  Column 18 is NaN
    (row 2 aside): the window [17, 20) has two candidates.  The padding columns hold 1e9 and must never be read as candidates."""
    key = (V, ld, dtype)
    if key not in _CACHE:
        rng = np.random.default_rng(V)
        x = np.full((M_ROWS, ld), 1e9, np.float32)
        x[0, :V] = rng.standard_normal(V) * 3
        x[1, :V] = FEW[rng.integers(0, FEW.size, V)]
        x[3, :V] = rng.standard_normal(V) * 3
        x[3, rng.choice(V, V // 3, replace=False)] = -np.inf
        x[3, [1, 40, V - 2]] = [np.nan, np.inf, np.nan]
        x[4, :V] = FEW[rng.integers(0, FEW.size, V)]
        x[4, rng.choice(V, V // 2, replace=False)] = -np.inf
        x[5, :V] = x[0, :V]
        x[:, 18] = np.nan
        x[:, [17, 19]] = [[0.25, 0.75]]                    # (finite, whatever the holes did)
        x[2, :V] = -np.inf
        lg = _tdev(x).to(dtype)
        _CACHE[key] = (lg, lg[:, :V].float().cpu().numpy().astype(np.float64))
    return _CACHE[key]


def _windows(V):
    return [(0, V), (5, V - 3), (17, 20)]


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _check_alternatives(got_ids, got_lp, want_ids, want_lp, what):
    """ids exactly (sentinels and -1 included); log-probs: NaN sentinels and -inf where the rule has them, else within TOL of float64;
    never increasing along the alternatives"""
    assert np.array_equal(got_ids, want_ids), (what, np.argwhere(got_ids != want_ids)[:5])
    assert np.array_equal(np.isnan(got_lp), np.isnan(want_lp)), what
    inf = np.isneginf(want_lp)
    assert np.array_equal(np.isneginf(got_lp), inf) and not np.isposinf(got_lp).any(), what
    fin = ~inf & ~np.isnan(want_lp)
    err = np.abs(got_lp[fin].astype(np.float64) - want_lp[fin]).max() if fin.any() else 0.0
    print(f"{what}: max |top_logprob - float64| = {err:.3e}")
    assert err <= TOL, (what, err)
    written = got_lp[~np.isnan(got_lp).any(-1)]
    assert (written[:, 1:] <= written[:, :-1]).all(), what                          # consequence 1 (-inf tails included)


class _State:
    def __init__(self, M, n=None, finished=()):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.t = torch.ones(1, **i32)                                               # token index 1 of MAXNEW = 3
        self.finished = torch.zeros(M, **i32)
        for r in finished:
            self.finished[r] = 1
        self.lengths, self.status = torch.ones(M, **i32), torch.zeros(M, **i32)
        self.out = torch.full((M, MAXNEW), SENT, **i32)
        self.ids = torch.full((M, 2), SENT, dtype=torch.int64, device=DEV)
        self.sid = torch.arange(40, 40 + M, **i32)
        self.logprob = torch.full((M, MAXNEW), float("nan"), dtype=torch.float32, device=DEV)
        self.sum_logprob = torch.full((M,), SUM0, dtype=torch.float32, device=DEV)
        self.kw = dict(logprob=self.logprob, sum_logprob=self.sum_logprob)
        if n:
            self.top_ids = torch.full((M, MAXNEW, n), SENT, **i32)
            self.top_logprob = torch.full((M, MAXNEW, n), float("nan"), dtype=torch.float32, device=DEV)
            self.kw.update(top_n=n, top_ids=self.top_ids, top_logprob=self.top_logprob)

    def call(self, lg, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens(lg, self.t, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, stream_id=self.sid, pad_id=PAD,
                          **self.kw, **kw)

    def host(self):
        h = {k: getattr(self, k).cpu().numpy().copy() for k in ("t", "finished", "lengths", "status", "out", "ids")}
        h.update(logprob=_bits(self.logprob), sum_logprob=_bits(self.sum_logprob))
        return h


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V,ld", SEL_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_select_tokens_top_follows_the_rule_and_changes_nothing_else(dtype, V, ld, n):
    lg, x = _case(V, ld, dtype)
    eos = V - 5
    for lo, hi in _windows(V):
        for mode, sel in MODES.items():
            kw = dict(V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, **sel)
            lp, top = _State(M_ROWS, finished=(5,)), _State(M_ROWS, n, finished=(5,))
            for s in (lp, top):
                s.call(lg, **kw)
            h = top.host()
            _same(lp.host(), h)                              # tokens, logprob, sum_logprob, finished, lengths, status, next_ids: bit-equal
            fin = np.zeros(M_ROWS, bool)
            fin[5] = True
            want_ids, want_lp = np.full((M_ROWS, MAXNEW, n), SENT, np.int64), np.full((M_ROWS, MAXNEW, n), np.nan)
            T.step(x, 1, MAXNEW, fin, want_ids, want_lp, lo, hi)
            got_ids, got_lp = top.top_ids.cpu().numpy(), top.top_logprob.cpu().numpy()
            what = f"V={V} [{lo}, {hi}) n={n} {mode}"
            _check_alternatives(got_ids, got_lp, want_ids, want_lp, what)
            assert (got_ids[2, 1] == -1).all() and (got_ids[5, 1] == -1).all()      # no candidate; finished on entry
            if (lo, hi) == (17, 20):
                assert (got_ids[[0, 1, 3, 4], 1, :2] == [19, 17][:n]).all()        # 0.75 at column 19, 0.25 at column 17
                assert (got_ids[[0, 1, 3, 4], 1, 2:] == -1).all()                   # two candidates
            tok = h["out"][:, 1]
            for r in (0, 1, 3, 4):
                hit = np.flatnonzero(got_ids[r, 1] == tok[r])
                if mode == "greedy":
                    assert hit.size == 1 and hit[0] == 0, (what, r)                 # the arg-max leads its alternatives
                if hit.size:                                                        # consequence 2: the chosen token's own bits
                    assert _bits(top.top_logprob)[r, 1, hit[0]] == h["logprob"][r, 1], (what, r)
    # t out of range: status bit 1, neither buffer is touched
    ids0, lp0 = _bits(top.top_ids), _bits(top.top_logprob)
    top.t.fill_(MAXNEW)
    top.finished.zero_()
    top.call(lg, **kw)
    assert (top.status.cpu().numpy() & 2).all()
    assert np.array_equal(_bits(top.top_ids), ids0) and np.array_equal(_bits(top.top_logprob), lp0)


# ------------------------------------------------------------------------------------------------------------------------------ the slot form
S = 6
T0 = [0, 2, 1, 3, 5, 0]
LIMIT = [4, 4, 4, 4, 6, 4]            # slot 4 sits at limit - 1
FIN = [0, 0, 0, 1, 0, 0]              # slot 3 is vacant
MAXNEW_S = 6


class _Slots:
    def __init__(self, n=None):
        i32 = lambda a: _tdev(np.asarray(a, np.int32))
        self.t, self.limit, self.finished, self.sid = i32(T0), i32(LIMIT), i32(FIN), i32([9, 8, 7, 6, 5, 4])
        self.lengths, self.status = i32(T0), i32([0] * S)
        self.out = torch.full((S, MAXNEW_S), SENT, dtype=torch.int32, device=DEV)
        self.ids = torch.full((S, 2), SENT, dtype=torch.int64, device=DEV)
        self.logprob = torch.full((S, MAXNEW_S), float("nan"), dtype=torch.float32, device=DEV)
        self.sum_logprob = torch.full((S,), SUM0, dtype=torch.float32, device=DEV)
        self.kw = dict(logprob=self.logprob, sum_logprob=self.sum_logprob)
        if n:
            self.top_ids = torch.full((S, MAXNEW_S, n), SENT, dtype=torch.int32, device=DEV)
            self.top_logprob = torch.full((S, MAXNEW_S, n), float("nan"), dtype=torch.float32, device=DEV)
            self.kw.update(top_n=n, top_ids=self.top_ids, top_logprob=self.top_logprob)

    def call(self, lg, row_map, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens_slots(lg, self.t, self.limit, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, stream_id=self.sid,
                                pad_id=PAD, row_map=_tdev(np.asarray(row_map, np.int32)), **self.kw, **kw)

    host = _State.host


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slot_form_writes_every_live_slot_at_its_own_counter(dtype, n):
    V, ld = 12289, 12352
    lg6, x6 = _case(V, ld, dtype)
    lg, x = lg6[[0, 1, 3]].contiguous(), x6[[0, 1, 3]]
    lo, hi = 5, V - 3
    kw = dict(V=V, vocab_lo=lo, vocab_hi=hi, eos_id=V - 5, greedy=True)
    a, b = _Slots(), _Slots(n)
    want_ids, want_lp = np.full((S, MAXNEW_S, n), SENT, np.int64), np.full((S, MAXNEW_S, n), np.nan)
    for row_map in ([4, 6, 1], [3, -1, 0]):                           # 6 and -1: no such slot; slot 3 is vacant; slot 4 at limit - 1
        hb = b.host()
        T.step_slots(x, row_map, hb["t"], np.asarray(LIMIT), hb["finished"], want_ids, want_lp, lo, hi)
        for st in (a, b):
            st.call(lg, row_map, **kw)
        _same(a.host(), b.host())
    got_ids, got_lp = b.top_ids.cpu().numpy(), b.top_logprob.cpu().numpy()
    _check_alternatives(got_ids, got_lp, want_ids, want_lp, f"slots n={n}")
    written = {(s, t) for s, t in np.argwhere(got_ids[:, :, 0] != SENT).tolist()}
    assert written == {(4, 5), (1, 2), (0, 0)}                        # vacant and unmapped slots, and every other column, keep their sentinels
    hb = b.host()
    for s, t in written:
        assert got_ids[s, t, 0] == hb["out"][s, t] and _bits(b.top_logprob)[s, t, 0] == hb["logprob"][s, t]
    assert hb["finished"][4] == 1
    # slot 0 reopened with its counter at its limit: status bit 1, nothing written
    b.t[0] = LIMIT[0]
    b.finished[0] = 0
    ids0, lp0 = _bits(b.top_ids), _bits(b.top_logprob)
    b.call(lg, [0, 6, 6], **kw)
    assert int(b.status[0]) & 2 and np.array_equal(_bits(b.top_ids), ids0) and np.array_equal(_bits(b.top_logprob), lp0)


def test_top_arguments_are_checked_before_a_launch():
    from bdm_db1_amd import lib, ops
    s = _State(2, 4)
    lg = torch.randn(2, 100, device=DEV)
    base = (lg, s.t, s.finished, s.lengths, s.out, s.ids[:, 1], s.status)
    lp = dict(logprob=s.logprob, sum_logprob=s.sum_logprob)
    for kw in (dict(top_n=4, top_ids=s.top_ids, top_logprob=s.top_logprob),                                # without the log-prob buffers
               dict(**lp, top_n=4, top_ids=s.top_ids), dict(**lp, top_n=17, top_ids=s.top_ids, top_logprob=s.top_logprob),
               dict(**lp, top_n=3, top_ids=s.top_ids, top_logprob=s.top_logprob),
               dict(**lp, top_n=4, top_ids=s.top_ids.long(), top_logprob=s.top_logprob)):
        with pytest.raises(ValueError):
            ops.select_tokens(*base, **kw)
    Lb = lib.load()
    P = lambda x: x.data_ptr()
    args = lambda n, ti, tl: (P(lg), 2, 100, 100, 0, 0, 100, 1.0, 0, 1.0, 1, 0, 0, -1, 0, 0, P(s.t), None, P(s.finished), P(s.lengths), P(s.out),
                              MAXNEW, P(s.ids), 2, P(s.status), P(s.logprob), P(s.sum_logprob), n, ti, tl, None, 0, None)
    for n, ti, tl in ((0, P(s.top_ids), P(s.top_logprob)), (17, P(s.top_ids), P(s.top_logprob)), (4, None, P(s.top_logprob)),
                      (4, P(s.top_ids), None)):
        assert Lb.db1_select_tokens_top(*args(n, ti, tl)) == ops.DB1_ERR_BAD_SHAPE
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    o = _outs(2)
    assert Lb.db1_score_rows_top(P(lg), P(lab), *[P(t) for t in o], 2, 100, 100, 0, 17, P(s.top_ids), P(s.top_logprob), 0, 100, None) == \
        ops.DB1_ERR_BAD_SHAPE
    assert Lb.db1_score_rows_top(P(lg), P(lab), *[P(t) for t in o], 2, 100, 100, 0, 4, None, P(s.top_logprob), 0, 100, None) == ops.DB1_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (s.out == SENT).all() and (s.top_ids == SENT).all() and torch.isnan(s.top_logprob).all()       # nothing was launched


# ------------------------------------------------------------------------------------------------------------------------------------ scoring
# (V, ld): bf16 at DB1-1.3B's row and at a short one; fp32 at the last row the 256-thread form takes (256 * 4 * 17) and the first of the 512 one
SCORE_SHAPES = {torch.bfloat16: [(33025, 33280), (365, 512)], torch.float32: [(17401, 17408), (17409, 17412), (365, 512)]}


def _outs(Tn):
    f = torch.full((Tn,), float("nan"), device=DEV)
    return [f.clone(), f.clone()] + [torch.full((Tn,), -12345, dtype=torch.int32, device=DEV) for _ in range(3)]


def _score_case(V, ld, dtype):
    """the rows of ``_case`` plus two with signed zeros at the top (scoring ranks -0.0 and +0.0 as one value) and a single -0.0 candidate;
    labels: the arg-max, a tied value, an ignored row, a non-candidate"""
    key = ("score", V, ld, dtype)
    if key not in _CACHE:
        lg6, _ = _case(V, ld, dtype)
        z = torch.full((2, ld), 1e9, device=DEV).to(dtype)
        z[:, :V] = -1.0
        z[0, [30, 7, 50]] = torch.tensor([0.0, -0.0, 0.0], device=DEV).to(dtype)     # the maximum: -0.0 at the lowest column
        z[1, :V] = float("-inf")
        z[1, 33] = -0.0                                                              # one candidate, -0.0: lse = 0
        lg = torch.cat([lg6, z]).contiguous()
        x = lg[:, :V].float().cpu().numpy().astype(np.float64)
        rng = np.random.default_rng(V + 1)
        labels = rng.integers(20, V - 3, lg.shape[0])
        labels[0] = int(np.nanargmax(np.where(np.isfinite(x[0]), x[0], np.nan)))
        labels[3] = -100
        labels[4] = 18
        labels[6], labels[7] = 7, 33
        _CACHE[key] = (lg, x, _tdev(labels.astype(np.int64)), labels)
    return _CACHE[key]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype,V,ld", [(dt, V, ld) for dt, shapes in SCORE_SHAPES.items() for V, ld in shapes])
def test_score_rows_top_follows_the_rule_and_changes_nothing_else(dtype, V, ld, n):
    from bdm_db1_amd import ops
    lg, x, labels, lab = _score_case(V, ld, dtype)
    Tn = lg.shape[0]
    for lo, hi in _windows(V):
        ref, got = _outs(Tn), _outs(Tn)
        ops.score_rows(lg, labels, *ref, V=V, vocab_lo=lo, vocab_hi=hi)
        ti = torch.full((Tn, n), SENT, dtype=torch.int32, device=DEV)
        tl = torch.full((Tn, n), float("nan"), dtype=torch.float32, device=DEV)
        ops.score_rows(lg, labels, *got, V=V, vocab_lo=lo, vocab_hi=hi, top_n=n, top_ids=ti, top_logprob=tl)
        for g, r in zip(got, ref):                                                  # lse, logprob, top1, rank, status: bit-equal
            assert np.array_equal(_bits(g), _bits(r))
        want_ids, want_lp = T.top(x, lo, hi, n)
        got_ids, got_lp = ti.cpu().numpy(), tl.cpu().numpy()
        what = f"score V={V} ld={ld} [{lo}, {hi}) n={n}"
        _check_alternatives(got_ids, got_lp, want_ids, want_lp, what)
        lse, lp, top1, rank, status = (g.cpu().numpy() for g in got)
        assert np.array_equal(got_ids[:, 0], top1), what                            # consequence 3 (-1 where there is no candidate)
        for r in range(Tn):
            y = int(lab[r])
            if rank[r] < 0:
                continue
            cand = np.zeros(V, bool)
            cand[lo:hi] = np.isfinite(x[r, lo:hi])
            if rank[r] < n and (x[r][cand] == x[r, y]).sum() == 1:
                assert got_ids[r, rank[r]] == y, (what, r)
            hit = np.flatnonzero(got_ids[r] == y)
            if hit.size:                                                            # consequence 2
                assert _bits(tl)[r, hit[0]] == _bits(got[1])[r], (what, r)
        if lo == 0:
            assert got_ids[6, 0] == 7 and got_ids[6, 1:3].tolist() == [30, 50][:max(0, min(2, n - 1))]      # signed zeros: by column
            assert got_ids[7, 0] == 33 and (got_ids[7, 1:] == -1).all() and _bits(tl)[7, 0] == _bits(got[1])[7]
    ref = SR.score_rows(x, lab, lo, hi)                                              # (the parent's outputs are the score rule's)
    assert np.array_equal(top1, ref[2]) and np.array_equal(rank, ref[3])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_lmhead_score_top_equals_gemm_then_score_rows_top(dtype):
    from bdm_db1_amd import ops
    V, rows, d, Tn, n = 1000, 1024, 256, 200, 5
    rng = np.random.default_rng(7)
    h = torch.from_numpy(rng.standard_normal((Tn, d)).astype(np.float32)).to(DEV).to(dtype)
    W = torch.from_numpy((rng.standard_normal((rows, d)) * 0.3).astype(np.float32)).to(DEV).to(dtype)
    labels = torch.from_numpy(rng.integers(0, V, Tn)).to(DEV)
    labels[3] = -100
    logits = torch.empty(Tn, rows, device=DEV, dtype=dtype)
    ops.gemm(h, W.t(), logits)
    lo, hi = 10, 900
    mk = lambda: (torch.full((Tn, n), SENT, dtype=torch.int32, device=DEV), torch.full((Tn, n), float("nan"), dtype=torch.float32, device=DEV))
    ref, (ri, rl) = _outs(Tn), mk()
    ops.score_rows(logits, labels, *ref, V=V, vocab_lo=lo, vocab_hi=hi, top_n=n, top_ids=ri, top_logprob=rl)
    plain = _outs(Tn)
    ops.reserve_workspace(64 << 20)
    ops.lmhead_score(h, W, labels, *plain, V=V, vocab_lo=lo, vocab_hi=hi, chunk_rows=96)
    for chunk in (96, 4096):                                                        # Tn is no multiple of 96; 4096 > Tn
        got, (gi, gl) = _outs(Tn), mk()
        ops.lmhead_score(h, W, labels, *got, V=V, vocab_lo=lo, vocab_hi=hi, chunk_rows=chunk, top_n=n, top_ids=gi, top_logprob=gl)
        for g, p in zip(got, plain):                                                # db1_lmhead_score's outputs: bit-equal
            assert np.array_equal(_bits(g), _bits(p))
        assert torch.equal(gi, ri) and torch.equal(gi[:, 0], got[2])
        err = float((gl.double() - rl.double()).abs().max())
        print(f"sweep vs materialised: {err:.2e}")
        assert err <= TOL
    want_ids, want_lp = T.top(logits.float().cpu().numpy()[:, :V].astype(np.float64), lo, hi, n)
    _check_alternatives(ri.cpu().numpy(), rl.cpu().numpy(), want_ids, want_lp, "sweep")
