"""db1_select_tokens_lp / db1_select_tokens_slots_lp through ``ops``: the choice and its bookkeeping bit-equal to the plain entry points on
clones of the same inputs, the log-probs against the float64 rule of tests/logprob_rule.py, the running sum bit for bit, sentinels where the
launch must not write, the slot form at every slot's own counter, a captured graph against eager calls, and determinism."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import logprob_rule as L  # noqa: E402
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

MAXNEW, PAD, SENT, SUM0, TOL = 4, 0, -7, 1.5, 1e-5
MODES = {"greedy": dict(greedy=True), "top_k": dict(greedy=False, top_k=40, seed=77), "top_p": dict(greedy=False, top_p=0.9, seed=78),
         "temperature": dict(greedy=False, temperature=0.7, seed=79)}
SHAPES = [(1, 7), (5, 5000), (5, 33025)]          # one per NG branch (1, 3, 9 groups of 4096 columns)
_CACHE = {}


def _case(M, V, dtype):
    """(device logits [M, ld] with NaN padding, their float64 values [M, V], lo, hi, eos) -- made once per shape and dtype, never changed.
    M = 5: row 1 holds NaN and +-inf inside the window, row 2 nothing finite inside it, row 3 is the caller's to mark finished, row 4 picks
    ``eos`` (a logit far above the rest)."""
    key = (M, V, dtype)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + V)
        ld = V + (64 - V % 64) + 64
        x = np.full((M, ld), np.nan, np.float32)
        x[:, :V] = rng.standard_normal((M, V)).astype(np.float32) * 3.0
        lo, hi = 1, V - 1
        eos = V - 3
        if M >= 5:
            c = rng.choice(np.arange(lo, hi), size=min(30, hi - lo), replace=False)
            x[1, c] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, c.size)]
            x[2, lo:hi] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, hi - lo)]
            x[4, eos] = 24.0
        lg = _tdev(x).to(dtype)
        _CACHE[key] = (lg, lg[:, :V].float().cpu().numpy().astype(np.float64), lo, hi, eos)
    return _CACHE[key]


class _State:
    def __init__(self, M, lp: bool, finished=()):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.t = torch.zeros(1, **i32)
        self.finished = torch.zeros(M, **i32)
        for r in finished:
            self.finished[r] = 1
        self.lengths = torch.zeros(M, **i32)
        self.status = torch.zeros(M, **i32)
        self.out = torch.full((M, MAXNEW), SENT, **i32)
        self.ids = torch.full((M, 2), SENT, dtype=torch.int64, device=DEV)
        self.sid = torch.arange(40, 40 + M, **i32)
        self.lp = {}
        if lp:
            self.logprob = torch.full((M, MAXNEW), float("nan"), dtype=torch.float32, device=DEV)
            self.sum_logprob = torch.full((M,), SUM0, dtype=torch.float32, device=DEV)
            self.lp = dict(logprob=self.logprob, sum_logprob=self.sum_logprob)

    def call(self, lg, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens(lg, self.t, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, stream_id=self.sid, pad_id=PAD,
                          **self.lp, **kw)

    def host(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("t", "finished", "lengths", "status", "out", "ids")}


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _run3(lg, M, V, lo, hi, eos, mode, lp):
    s = _State(M, lp, finished=(3,) if M >= 5 else ())
    steps = []
    for _ in range(3):
        s.call(lg, V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, **MODES[mode])
        steps.append(s.host())
        s.t.add_(1)
    return s, steps


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,V", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lp_call_chooses_like_the_plain_call_and_scores_by_the_rule(dtype, M, V, mode):
    lg, x, lo, hi, eos = _case(M, V, dtype)
    plain, p_steps = _run3(lg, M, V, lo, hi, eos, mode, lp=False)
    s, steps = _run3(lg, M, V, lo, hi, eos, mode, lp=True)
    for a, b in zip(p_steps, steps):
        _same(a, b)                                                    # token, out, lengths, finished, status, next_ids: bit-equal
    out = steps[-1]["out"]
    got, sums = s.logprob.cpu().numpy(), s.sum_logprob.cpu().numpy()
    # the rule, on the kernel's own tokens
    fin = np.zeros(M, bool)
    if M >= 5:
        fin[3] = True
    want = np.full((M, MAXNEW), np.nan)
    want_sum = np.full(M, SUM0)
    run = np.full(M, np.float32(SUM0))
    for t in range(3):
        live = ~fin
        toks = L.step(x, t, MAXNEW, fin, want, want_sum, lo, hi, tokens=out[:, t])
        fin |= toks == eos
        for r in range(M):
            if live[r] and toks[r] >= 0:
                run[r] = np.float32(run[r] + got[r, t])                # the fp32 sum, in launch order
    assert np.array_equal(np.isnan(got), np.isnan(want))               # column 3 and nothing else keeps the sentinel
    err = np.nanmax(np.abs(got.astype(np.float64) - want))
    print(f"max |lp - lp64| = {err:.3e}  (min lp {np.nanmin(want):.2f})")
    assert np.nanmin(want) > -32.0 and err <= TOL, err
    assert np.array_equal(_bits(s.sum_logprob), run.view(np.int32)), (sums, run)
    # against the float64 sum: three terms within TOL each, three fp32 additions below 128 in magnitude (half an ulp, 2^-18, each)
    assert np.abs(sums - want_sum).max() <= 3 * TOL + 3 * 2.0 ** -18
    if M >= 5:
        assert (_bits(s.logprob)[[2, 3], :3] == 0).all()               # no candidate / finished on entry: +0.0f written
        assert (sums[[2, 3]] == np.float32(SUM0)).all()                # and the sum left alone
        assert steps[0]["status"][2] & 1 and steps[0]["finished"][2] == 1
        assert out[4, 0] == eos and got[4, 0] != 0.0 and (got[4, 1:3] == 0.0).all()      # the EOS is scored, the steps after it are not
        assert sums[4] == np.float32(np.float32(SUM0) + got[4, 0])
    # t == max_new: status bit 1, both buffers keep their bits
    s.t.fill_(MAXNEW)
    plain.t.fill_(MAXNEW)
    lp0, sum0 = _bits(s.logprob), _bits(s.sum_logprob)
    for st in (s, plain):
        st.call(lg, V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, **MODES[mode])
    _same(plain.host(), s.host())
    assert (s.status.cpu().numpy() & 2).all()
    assert np.array_equal(_bits(s.logprob), lp0) and np.array_equal(_bits(s.sum_logprob), sum0)
    # the same calls again: the same bits
    again, _ = _run3(lg, M, V, lo, hi, eos, mode, lp=True)
    assert np.array_equal(_bits(again.logprob), _bits(torch.from_numpy(got))) and np.array_equal(_bits(again.sum_logprob), run.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------------ the slot form
S = 6
T0 = [0, 2, 1, 3, 5, 0]
LIMIT = [4, 4, 4, 4, 6, 4]            # slot 4 sits at limit - 1
FIN = [0, 0, 0, 1, 0, 0]              # slot 3 is vacant
MAXNEW_S = 6


class _Slots:
    def __init__(self, lp: bool):
        i32 = lambda a: _tdev(np.asarray(a, np.int32))
        self.t, self.limit, self.finished, self.sid = i32(T0), i32(LIMIT), i32(FIN), i32([9, 8, 7, 6, 5, 4])
        self.lengths, self.status = i32(T0), i32([0] * S)
        self.out = torch.full((S, MAXNEW_S), SENT, dtype=torch.int32, device=DEV)
        self.ids = torch.full((S, 2), SENT, dtype=torch.int64, device=DEV)
        self.lp = {}
        if lp:
            self.logprob = torch.full((S, MAXNEW_S), float("nan"), dtype=torch.float32, device=DEV)
            self.sum_logprob = torch.full((S,), SUM0, dtype=torch.float32, device=DEV)
            self.lp = dict(logprob=self.logprob, sum_logprob=self.sum_logprob)

    def call(self, lg, row_map, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens_slots(lg, self.t, self.limit, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, stream_id=self.sid,
                                pad_id=PAD, row_map=_tdev(np.asarray(row_map, np.int32)), **self.lp, **kw)

    host = _State.host


@pytest.mark.parametrize("mode", ["greedy", "top_p"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slot_form_scores_every_live_slot_at_its_own_counter(dtype, mode):
    V = 5000
    lg5, x5, lo, hi, eos = _case(5, V, dtype)
    lg, x = lg5[[0, 1, 4]].contiguous(), x5[[0, 1, 4]]                  # three rows: plain, with non-finite entries, picking EOS
    kw = dict(V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, **MODES[mode])
    a, b = _Slots(False), _Slots(True)
    want = np.full((S, MAXNEW_S), np.nan)
    want_sum = np.full(S, np.float32(SUM0))
    touched = set()
    for row_map in ([4, 6, 1], [3, -1, 0]):                           # 6 and -1: no such slot; slot 3 is vacant; slot 4 at limit - 1
        t_before = b.t.cpu().numpy().copy()
        for st in (a, b):
            st.call(lg, row_map, **kw)
        ha, hb = a.host(), b.host()
        _same(ha, hb)
        got = b.logprob.cpu().numpy()
        for i, slot in enumerate(row_map):
            if not 0 <= slot < S or FIN[slot]:
                continue
            t = int(t_before[slot])
            tok = int(hb["out"][slot, t])
            assert hb["t"][slot] == t + 1 and tok == hb["ids"][slot, 1]
            want[slot, t] = L.logprob(x[i], tok, lo, hi)
            want_sum[slot] = np.float32(want_sum[slot] + got[slot, t])
            touched.add(slot)
    got = b.logprob.cpu().numpy()
    assert touched == {4, 1, 0} and np.array_equal(np.isnan(got), np.isnan(want))      # vacant and unmapped slots keep their sentinels
    assert np.nanmax(np.abs(got - want)) <= TOL
    assert np.array_equal(_bits(b.sum_logprob), want_sum.view(np.int32))
    assert (b.sum_logprob.cpu().numpy()[[2, 3, 5]] == np.float32(SUM0)).all()
    assert hb["finished"][4] == 1 and hb["ids"][3, 1] == PAD             # the limit closes slot 4; the vacant slot only hands pad_id on
    # slot 0 reopened with its counter at its limit: status bit 1, nothing scored
    b.t[0] = LIMIT[0]
    b.finished[0] = 0
    lp0, sum0 = _bits(b.logprob), _bits(b.sum_logprob)
    b.call(lg, [0, 6, 6], **kw)
    assert int(b.status[0]) & 2 and np.array_equal(_bits(b.logprob), lp0) and np.array_equal(_bits(b.sum_logprob), sum0)


def test_graph_captured_lp_call_equals_the_eager_calls():
    from bdm_db1_amd.decode import graph_capture
    M, V = 5, 33025
    lg, _, lo, hi, eos = _case(M, V, torch.bfloat16)
    kw = dict(V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, greedy=False, top_p=0.9, top_k=200, seed=8)
    eager = _State(M, True)
    for _ in range(3):
        eager.call(lg, **kw)
        eager.t.add_(1)
    gs = _State(M, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the capture
        gs.call(lg, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for x in (gs.lengths, gs.finished, gs.status):
        x.zero_()
    gs.out.fill_(SENT)
    gs.logprob.fill_(float("nan"))
    gs.sum_logprob.fill_(SUM0)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):      # (the cyclic collector held off: bdm_db1_amd.decode.graph_capture)
        gs.call(lg, **kw)
        gs.t.add_(1)
    for x in (gs.lengths, gs.finished, gs.status, gs.t):      # (whatever the capture itself may have run)
        x.zero_()
    gs.out.fill_(SENT)
    gs.logprob.fill_(float("nan"))
    gs.sum_logprob.fill_(SUM0)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    _same(eager.host(), gs.host())
    assert np.array_equal(_bits(gs.logprob), _bits(eager.logprob)) and np.array_equal(_bits(gs.sum_logprob), _bits(eager.sum_logprob))
    assert not np.isnan(eager.logprob.cpu().numpy()[:, :3]).any()


def test_lp_buffers_are_checked_before_a_launch():
    from bdm_db1_amd import lib, ops
    s = _State(2, True)
    lg = torch.randn(2, 100, device=DEV)
    with pytest.raises(ValueError):
        ops.select_tokens(lg, s.t, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, logprob=s.logprob)
    with pytest.raises(ValueError):
        ops.select_tokens(lg, s.t, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, logprob=s.logprob, sum_logprob=s.sum_logprob.double())
    with pytest.raises(ValueError):
        ops.select_tokens(lg, s.t, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, logprob=s.logprob[:, :3], sum_logprob=s.sum_logprob)
    Lb = lib.load()
    P = lambda x: x.data_ptr()
    args = lambda lp, sm: (P(lg), 2, 100, 100, 0, 0, 100, 1.0, 0, 1.0, 1, 0, 0, -1, 0, 0, P(s.t), None, P(s.finished), P(s.lengths), P(s.out),
                           MAXNEW, P(s.ids), 2, P(s.status), lp, sm, None, 0, None)
    assert Lb.db1_select_tokens_lp(*args(None, P(s.sum_logprob))) == ops.DB1_ERR_BAD_SHAPE
    assert Lb.db1_select_tokens_lp(*args(P(s.logprob), None)) == ops.DB1_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (s.out == SENT).all() and torch.isnan(s.logprob).all()       # nothing was launched
