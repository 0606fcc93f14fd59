"""db1_constrain_logits_slots_per and db1_stop_match_per against their NumPy rule (tests/slot_constraints_rule.py), bit for bit over the
WHOLE logits buffer (NaN-prefilled padding columns and untouched rows included), fp32 and bf16, and -- rule-free -- against the scalar entry
points launched for one slot alone with that slot's values.  One launch mixes a no-op record, each single constraint alone, everything at
once (a column in the history, biased and banned), full lists, a vacant slot, a finished slot and a counter at max_new; then the row_map
form, a capacity of 0, a history across the 256-thread stride, the three-roundings tie, every kind of invalid record, and the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import constraint_rule as C  # noqa: E402
import slot_constraints_rule as Q  # noqa: E402
import stop_rule as R  # noqa: E402
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

S, V, LD, EOS, PAD = 6, 67, 72, 3, 9
DTYPES = [C.F32, C.BF16]


def _logits(rng, M, dtype, ld=LD):
    x = (rng.standard_normal((M, ld)) * 4).astype(np.float32)
    x[:, V:] = np.nan                                   # the padding columns: NaN before, NaN after
    return C.bf16_bits(x) if dtype == C.BF16 else x


def _up(l, dtype):
    return _tdev(l.view(np.int16)).view(torch.bfloat16) if dtype == C.BF16 else _tdev(l)


def _down(lg, dtype):
    return lg.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == C.BF16 else lg.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _history(rng, mx):
    """[S, mx]: half of the tokens from a few columns (so they repeat), some entries outside [0, V)"""
    h = rng.integers(0, V, (S, mx))
    often = rng.random((S, mx)) < 0.5
    h[often] = np.array([0, 5, 11, V - 1])[rng.integers(0, 4, int(often.sum()))]
    out = rng.random((S, mx)) < 0.08
    h[out] = np.array([-1, V, V + 5])[rng.integers(0, 3, int(out.sum()))]
    return h.astype(np.int32)


def _tables(slots, bad_cap, bias_cap, eos=EOS):
    """a list of DecodingConstraints (or None) -> the stacked tables of ops.pack_slot_constraints"""
    from bdm_db1_amd import ops
    rows = [ops.pack_slot_constraints(c, eos, bad_cap, bias_cap) for c in slots]
    return [np.stack([r[k] for r in rows]) for k in range(6)]


def _launch(l, dtype, t, hist, finished, cons, bad, bias_ids, bias_val, eos=EOS, row_map=None):
    """-> (logits, finished, status) after one launch (status starts at 0)"""
    from bdm_db1_amd import ops
    lg, fin, st = _up(l, dtype), _tdev(np.asarray(finished, np.int32)), torch.zeros(len(finished), dtype=torch.int32, device=DEV)
    lists = {k: (_tdev(v) if v.shape[1] else None) for k, v in (("bad", bad), ("bias_ids", bias_ids), ("bias_val", bias_val))}
    ops.constrain_logits_slots_per(lg, _tdev(cons), _tdev(np.asarray(t, np.int32)), _tdev(hist), fin, st, V=V, eos_id=eos,
                                   row_map=None if row_map is None else _tdev(np.asarray(row_map, np.int32)), **lists)
    torch.cuda.synchronize()
    return _down(lg, dtype), fin.cpu().numpy(), st.cpu().numpy()


def _scalar(l_row, dtype, t, hist_row, c, eos=EOS):
    """the existing entry point launched for ONE slot alone with its values (``c``: a DecodingConstraints) -> the row"""
    from bdm_db1_amd import ops
    lg = _up(l_row[None], dtype)
    kw = dict(repetition_penalty=c.repetition_penalty, no_repeat_ngram_size=c.no_repeat_ngram_size, eos_id=eos, min_new=c.min_new_tokens,
              frequency_penalty=c.frequency_penalty, presence_penalty=c.presence_penalty,
              bad=_tdev(np.array(c.bad_token_ids, np.int32)) if c.bad_token_ids else None)
    if c.logit_bias:
        kw.update(bias_ids=_tdev(np.array([k for k, _ in c.logit_bias], np.int32)), bias_val=_tdev(np.array([b for _, b in c.logit_bias], np.float32)))
    ops.constrain_logits(lg, _tdev(np.array([t], np.int32)), _tdev(hist_row[None]), V=V, **kw)
    torch.cuda.synchronize()
    return _down(lg, dtype)[0]


def _same(got, want, where=""):
    d = _bits(got) != _bits(want)
    assert not d.any(), (where, np.argwhere(d)[:4], _bits(got)[d][:4], _bits(want)[d][:4])


def _mixed(bad_cap=4, bias_cap=3):
    """one constraint set per launch; the slots of the mixed launch take six of them at a time"""
    from bdm_db1_amd import DecodingConstraints as D
    singles = [None, D(repetition_penalty=1.3), D(no_repeat_ngram_size=2), D(min_new_tokens=39), D(bad_token_ids=(5, V + 1)),
               D(frequency_penalty=0.4), D(presence_penalty=-0.6), D(logit_bias={11: 1.5, 66: -2.0}), D(stop_sequences=((1, 2),))]
    # everything at once: column 5 is in every history, biased and banned; both lists full
    full = D(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=39, bad_token_ids=(5, 0, 66, V)[:bad_cap], frequency_penalty=0.25,
             presence_penalty=0.5, logit_bias=tuple({5: 2.0, 11: -1.0, 40: 0.75}.items())[:bias_cap])
    return singles, full


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mx,t_hi", [(40, 37), (300, 290)])
def test_one_launch_of_mixed_slots_equals_the_rule_and_the_scalar_kernels(dtype, mx, t_hi):
    rng = np.random.default_rng(mx + (dtype == C.BF16))
    singles, full = _mixed()
    hist = _history(rng, mx)
    hist[:, 1] = 5
    groups = [[None, singles[1], singles[2], singles[3], singles[4], full],            # every slot live
              [singles[5], singles[6], singles[7], singles[8], full, None],            # slot 5: finished, under a no-op record
              [full, full, singles[1], None, singles[4], singles[3]]]                  # slot 0: vacant; slot 1: its counter at max_new
    edited = 0
    for g, slots in enumerate(groups):
        cons, bad, bi, bv, _, _ = _tables(slots, 4, 3)
        assert cons[slots.index(full)][6] == 4 and cons[slots.index(full)][7] == 3            # n_bad == bad_cap, n_bias == bias_cap
        t = np.array([t_hi, 5, t_hi - 1, 2, 7, t_hi], np.int32)
        finished = np.zeros(S, np.int32)
        if g == 1:
            finished[5] = 1
        if g == 2:
            finished[0], t[1] = 1, mx
        l = _logits(rng, S, dtype)
        want = Q.constrain(l, hist, t, finished, np.zeros(S, np.int32), cons, bad, bi, bv, V=V, dtype=dtype, eos_id=EOS)
        got = _launch(l, dtype, t, hist, finished, cons, bad, bi, bv)
        _same(got[0], want[0], (g, "logits"))
        assert (got[1] == want[1]).all() and (got[1] == finished).all() and (got[2] == 0).all()
        assert np.isnan(C.widen(got[0][:, V:], dtype)).all()
        for s, c in enumerate(slots):                                                # rule-free: the scalar entry point, slot by slot
            live = not finished[s] and t[s] < mx
            if c is None or not live or not c.edits_logits(EOS):
                _same(got[0][s], l[s], (g, s, "untouched"))
            else:
                _same(got[0][s], _scalar(l[s], dtype, int(t[s]), hist[s], c), (g, s, "scalar"))
                edited += int((_bits(got[0][s]) != _bits(l[s])).any())
    assert edited >= 11


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_map_form_and_a_capacity_of_zero(dtype):
    from bdm_db1_amd import DecodingConstraints as D
    rng = np.random.default_rng(7)
    mx = 40
    hist = _history(rng, mx)
    singles, full = _mixed()
    slots = [full, singles[1], None, singles[4], singles[7], singles[2]]
    cons, bad, bi, bv, _, _ = _tables(slots, 4, 3)
    t = np.array([9, 20, 3, 12, 0, 30], np.int32)
    finished = np.array([0, 0, 0, 0, 0, 1], np.int32)
    row_map = [4, 0, 9, 3, 5]                                    # rows in another order than slots; 9: no such slot; slot 5 is finished
    l = _logits(rng, 5, dtype)
    want = Q.constrain(l, hist, t, finished, np.zeros(S, np.int32), cons, bad, bi, bv, V=V, dtype=dtype, eos_id=EOS, row_map=row_map)
    got = _launch(l, dtype, t, hist, finished, cons, bad, bi, bv, row_map=row_map)
    _same(got[0], want[0])
    _same(got[0][[2, 4]], l[[2, 4]])
    _same(got[0][1], _scalar(l[1], dtype, 9, hist[0], full))
    _same(got[0][0], _scalar(l[0], dtype, 0, hist[4], singles[7]))
    assert (got[2] == 0).all() and (got[1] == finished).all()
    # capacities of 0: NULL lists; the records that need no list still edit, and no EOS (eos_id -1) makes a minimum length a no-op
    slots0 = [D(repetition_penalty=1.3, frequency_penalty=0.2), D(no_repeat_ngram_size=2), None, D(min_new_tokens=30), D(presence_penalty=1.0), None]
    for eos in (EOS, -1):
        cons, bad, bi, bv, _, _ = _tables(slots0, 0, 0, eos=eos)
        assert bad.shape == (S, 0) and bi.shape == (S, 0)
        l = _logits(rng, S, dtype)
        t = np.full(S, 20, np.int32)
        want = Q.constrain(l, hist, t, np.zeros(S, np.int32), np.zeros(S, np.int32), cons, None, None, None, V=V, dtype=dtype, eos_id=eos)
        got = _launch(l, dtype, t, hist, np.zeros(S, np.int32), cons, bad, bi, bv, eos=eos)
        _same(got[0], want[0], eos)
        _same(got[0][[2, 5]], l[[2, 5]])
        assert (_bits(got[0][3]) != _bits(l[3])).any() == (eos == EOS)


def test_bf16_tie_three_roundings_not_a_fused_multiply_add():
    """150 copies of token 5: p = fp32(150 * 0.01) + 0.5 and v = fp32(l * inv) - p must each round (tests/test_penalty_kernels_gpu.py's case)"""
    from bdm_db1_amd import DecodingConstraints as D
    mx, t = 300, 299
    rng = np.random.default_rng(3)
    c = D(repetition_penalty=1.3, frequency_penalty=0.01, presence_penalty=0.5)
    for dtype in DTYPES:
        l = _logits(rng, S, dtype)
        hist = rng.integers(6, V, (S, mx)).astype(np.int32)
        hist[:, ::2] = 5
        for r, v in enumerate((3.0, -3.0, 1.0, -1.0, 0.3330078125, 7.0)):
            l[r, 5] = C.bf16_bits(np.array([v], np.float32))[0] if dtype == C.BF16 else np.float32(v)
        cons, bad, bi, bv, _, _ = _tables([c] * S, 0, 0)
        got = _launch(l, dtype, np.full(S, t, np.int32), hist, np.zeros(S, np.int32), cons, bad, bi, bv)
        th, inv = np.float32(1.3), np.float32(1) / np.float32(1.3)
        p = np.float32(np.float32(np.float32(150) * np.float32(0.01)) + np.float32(0.5))
        for r, v in enumerate((3.0, -3.0)):
            w = np.float32(np.float32(np.float32(v) * (inv if v > 0 else th)) - p)
            w = C.bf16_widen(C.bf16_bits(np.array([w])))[0] if dtype == C.BF16 else w
            assert C.widen(got[0][r:r + 1, 5:6], dtype)[0, 0] == w
        want = Q.constrain(l, hist, np.full(S, t), np.zeros(S, np.int32), np.zeros(S, np.int32), cons, None, None, None, V=V, dtype=dtype, eos_id=EOS)
        _same(got[0], want[0], dtype)
        _same(got[0][0], _scalar(l[0], dtype, t, hist[0], c))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_kind_of_invalid_record_ends_the_slot_and_touches_no_logit(dtype):
    from bdm_db1_amd import DecodingConstraints as D
    rng = np.random.default_rng(21)
    mx, bad_cap, bias_cap = 40, 4, 3
    hist = _history(rng, mx)
    good = D(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_token_ids=(5,), logit_bias={11: 1.0})
    nan, inf = float("nan"), float("inf")
    kinds = [dict(theta=0.0), dict(theta=-1.3), dict(theta=nan), dict(theta=inf), dict(inv_theta=0.0), dict(inv_theta=nan), dict(inv_theta=inf),
             dict(inv_theta=-1.0), dict(ngram=-1), dict(min_new=-1), dict(freq=nan), dict(freq=inf), dict(pres=-inf), dict(pres=nan),
             dict(n_bad=-1), dict(n_bad=bad_cap + 1), dict(n_bias=-1), dict(n_bias=bias_cap + 1)]
    base = dict(theta=1.3, ngram=2, n_bad=1, n_bias=1)
    for i in range(0, len(kinds), 3):
        cons, bad, bi, bv, _, _ = _tables([good] * S, bad_cap, bias_cap)
        where = {1 + 2 * j: k for j, k in enumerate(kinds[i:i + 3])}              # slots 1, 3, 5 invalid; 0, 2, 4 valid neighbours
        for s, k in where.items():
            cons[s] = Q.record(**{**base, **k})
            assert Q.invalid(cons[s], bad_cap, bias_cap), k
        t = np.full(S, 17, np.int32)
        l = _logits(rng, S, dtype)
        zero = np.zeros(S, np.int32)
        want = Q.constrain(l, hist, t, zero, zero, cons, bad, bi, bv, V=V, dtype=dtype, eos_id=EOS)
        got = _launch(l, dtype, t, hist, zero, cons, bad, bi, bv)
        _same(got[0], want[0], where)
        for s in range(S):
            if s in where:
                assert got[2][s] == 8 and got[1][s] == 1, where[s]
                _same(got[0][s], l[s], where[s])                                 # the row and its padding keep their bits
            else:
                assert got[2][s] == 0 and got[1][s] == 0
                _same(got[0][s], _scalar(l[s], dtype, 17, hist[s], good))
    # an invalid record behind the guard is never looked at: vacant, counter out of range
    cons, bad, bi, bv, _, _ = _tables([good] * S, bad_cap, bias_cap)
    cons[1] = cons[2] = Q.record(theta=nan)
    l = _logits(rng, S, dtype)
    got = _launch(l, dtype, np.array([3, 3, mx, 3, 3, 3], np.int32), hist, np.array([0, 1, 0, 0, 0, 0], np.int32), cons, bad, bi, bv)
    assert (got[2] == 0).all() and got[1].tolist() == [0, 1, 0, 0, 0, 0]
    _same(got[0][[1, 2]], l[[1, 2]])
    # status bits 0 .. 2 already set stay: bit 3 is or-ed in
    from bdm_db1_amd import ops
    st, fin = _tdev(np.array([7, 1, 0, 0, 0, 0], np.int32)), torch.zeros(S, dtype=torch.int32, device=DEV)
    cons[0] = Q.record(theta=nan)
    cons[1] = Q.record(theta=1.3)
    ops.constrain_logits_slots_per(_up(l, dtype), _tdev(cons), _tdev(np.full(S, 3, np.int32)), _tdev(hist), fin, st, V=V, bad=_tdev(bad),
                                   bias_ids=_tdev(bi), bias_val=_tdev(bv), eos_id=EOS)
    assert st.cpu().tolist() == [15, 1, 8, 0, 0, 0] and fin.cpu().tolist() == [1, 0, 1, 0, 0, 0]


def test_refusals_before_a_launch():
    from bdm_db1_amd import lib, ops
    mx = 8
    lg = torch.full((S, LD), 7.5, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    t, hist, fin, st = torch.ones(S, **i32), torch.zeros(S, mx, **i32), torch.zeros(S, **i32), torch.zeros(S, **i32)
    cons = _tdev(np.tile(Q.record(theta=1.3), (S, 1)))
    bad, bi, bv = torch.zeros(S, 4, **i32), torch.zeros(S, 3, **i32), torch.zeros(S, 3, device=DEV)
    ok = dict(V=V, bad=bad, bias_ids=bi, bias_val=bv, eos_id=EOS)
    for a, kw in (((lg, None, t, hist, fin, st), ok), ((lg, cons[:, :7], t, hist, fin, st), ok), ((lg, cons.long(), t, hist, fin, st), ok),
                  ((lg, cons, t[:3], hist, fin, st), ok), ((lg, cons, t, hist, None, st), ok), ((lg, cons, t, hist, fin, None), ok),
                  ((lg, cons, t, hist, fin, st), dict(ok, bias_val=None)), ((lg, cons, t, hist, fin, st), dict(ok, bad=torch.zeros(S, 1025, **i32))),
                  ((lg, cons, t, hist, fin, st), dict(ok, bias_val=torch.zeros(S, 4, device=DEV))),
                  ((lg.half(), cons, t, hist, fin, st), ok), ((lg, cons, t, torch.zeros(S, 4097, **i32), fin, st), ok),
                  ((lg, cons, t, hist, fin, st), dict(ok, V=LD + 1))):
        with pytest.raises(ValueError):
            ops.constrain_logits_slots_per(*a, **kw)
    assert ops.constrain_logits_slots_supported(V, LD, 4096, 1024, 1024, torch.bfloat16)
    assert not ops.constrain_logits_slots_supported(V, LD, 4096, 1025, 0, torch.float32)
    assert not ops.constrain_logits_slots_supported(V, LD, 4096, 0, 1025, torch.float32)
    assert not ops.constrain_logits_slots_supported(V, LD, 4097, 0, 0, torch.float32)
    L = lib.load()
    P_ = lambda x: x.data_ptr()
    args = lambda **o: tuple({**dict(lg=P_(lg), M=S, V=V, ld=LD, dt=0, t=P_(t), hist=P_(hist), mx=mx, fin=P_(fin), st=P_(st), rm=None, S=S,
                                     cons=P_(cons), bad=P_(bad), bc=4, bi=P_(bi), bv=P_(bv), bic=3, eos=EOS, ws=None, wsn=0, stream=None),
                                **o}.values())
    for o in (dict(cons=None), dict(fin=None), dict(st=None), dict(cons=P_(cons) + 16), dict(bc=1025), dict(bic=1025), dict(bad=None),
              dict(bi=None), dict(bv=None), dict(bc=-1), dict(dt=5), dict(M=0), dict(ld=V - 1), dict(mx=4097), dict(S=S + 1), dict(lg=None)):
        assert L.db1_constrain_logits_slots_per(*args(**o)) != 0, o
        assert L.db1_last_error()
    assert L.db1_constrain_logits_slots_workspace_bytes(S, V, mx, 4, 3, 0) == 0
    torch.cuda.synchronize()
    assert (lg == 7.5).all() and (st == 0).all() and (fin == 0).all()
    assert L.db1_constrain_logits_slots_per(*args(bad=None, bc=0, bi=None, bv=None, bic=0)) == 0          # (capacity 0 allows NULL lists)


# ------------------------------------------------------------------------------------------------------------------ db1_stop_match_per
def _stop_state(rng, mx, lp, n_top):
    st = dict(lengths=np.zeros(S, np.int32), checked=np.zeros(S, np.int32), finished=np.zeros(S, np.int32), stop_hit=np.zeros(S, np.int32),
              out=rng.integers(0, 4, (S, mx)).astype(np.int32), next_ids=rng.integers(0, 4, S).astype(np.int64))
    if lp:
        st["logprob"] = -rng.random((S, mx)).astype(np.float32) * 5
        st["sum_logprob"] = -rng.random(S).astype(np.float32)
    if n_top:
        st["top_ids"] = rng.integers(0, 4, (S, mx, n_top)).astype(np.int32)
        st["top_logprob"] = -rng.random((S, mx, n_top)).astype(np.float32)
    return st


def _stop_run(st, tok, n, row_map=None, per=True, slot=None):
    from bdm_db1_amd import ops
    dev = {k: _tdev(v) for k, v in st.items()}
    opt = {k: dev[k] for k in ("logprob", "sum_logprob", "top_ids", "top_logprob") if k in dev}
    if "top_ids" in dev:
        opt["top_n"] = int(dev["top_ids"].shape[2])
    rm = None if row_map is None else _tdev(np.asarray(row_map, np.int32))
    a = (dev["lengths"], dev["checked"], dev["finished"], dev["stop_hit"], dev["out"], dev["next_ids"])
    if per:
        ops.stop_match_per(_tdev(tok), _tdev(n), *a, pad_id=PAD, row_map=rm, **opt)
    else:           # the scalar entry point for ONE slot with its own list (its used entries)
        ops.stop_match(_tdev(tok[slot]), _tdev(n[slot]), *a, pad_id=PAD, row_map=_tdev(np.array([slot], np.int32)), **opt)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}


def _state_same(got, want, where=""):
    for k in want:
        a, b = got[k], want[k]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert (a == b).all(), (where, k, np.argwhere(a != b)[:4])


@pytest.mark.parametrize("bufs", ["plain", "lp", "top"])
def test_stop_match_per_equals_the_rule_and_the_scalar_kernel(bufs):
    from bdm_db1_amd import DecodingConstraints as D
    rng = np.random.default_rng(len(bufs))
    mx = 40
    lists = [((5, 6, 7),), (), ((7,), (6, 7), (5, 6, 7)), ((6, 7), (7, 7), (6, 7)), ((4, 5, 6, 7),), tuple((4 + k % 4, 7) for k in range(16))]
    tables = _tables([D(stop_sequences=q) if q else None for q in lists], 0, 0)
    tok, n = tables[4], tables[5]
    assert tok.shape == (S, 16, 16) and n.shape == (S, 16) and n[1].tolist() == [0] * 16 and n[5].tolist() == [2] * 16
    st = _stop_state(rng, mx, bufs != "plain", 3 if bufs == "top" else 0)
    for s in range(S):                                   # every slot's output ends in 4 5 6 7
        st["lengths"][s] = 10 + s
        st["out"][s, 6 + s:10 + s] = (4, 5, 6, 7)
    st["lengths"][4] = 4                                 # slot 4: a match at n == len, the whole output goes
    st["out"][4, :4] = (4, 5, 6, 7)
    want = Q.stop(st, tok, n, PAD)
    got = _stop_run(st, tok, n)
    _state_same(got, want)
    # slot 0 stops on its own list, slot 1 (the empty list) goes on though its tail matches its neighbours' lists; slot 2: the longest wins;
    # slot 3: the longest-match tie goes to the lowest index; slot 5: entry 2 of 16 is (6, 7)
    assert want["stop_hit"].tolist() == [1, 0, 3, 1, 1, 3] and want["finished"].tolist() == [1, 0, 1, 1, 1, 1]
    assert want["lengths"].tolist() == [7, 11, 9, 11, 0, 13] and want["checked"][1] == 11
    for s in range(S):                                   # rule-free: db1_stop_match for that slot alone with its own list
        if lists[s]:
            one = _stop_run(st, tok[:, :len(lists[s])], n[:, :len(lists[s])], per=False, slot=s)
            for k in one:
                a, b = got[k][s], one[k][s]
                assert (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all(), (s, k)
    # the row_map form: rows in another order, an entry out of range, a slot not served keeps everything
    rm = [5, 9, 0, 2]
    want = Q.stop(st, tok, n, PAD, row_map=rm)
    got = _stop_run(st, tok, n, row_map=rm)
    _state_same(got, want, "row_map")
    assert want["finished"].tolist() == [1, 0, 1, 0, 0, 1] and want["checked"].tolist()[3:5] == [0, 0]
    # the same launch again changes nothing
    _state_same(_stop_run(want, tok, n, row_map=rm), want, "again")


def test_stop_match_per_refusals():
    from bdm_db1_amd import ops
    i32 = dict(dtype=torch.int32, device=DEV)
    z = lambda *s: torch.zeros(*s, **i32)
    tok, n, out, ids = z(S, 16, 16), z(S, 16), z(S, 8), torch.zeros(S, dtype=torch.int64, device=DEV)
    for a in ((tok[:, :15], n), (tok, n[:, :15]), (tok[:5], n), (tok.long(), n), (None, n)):
        with pytest.raises(ValueError):
            ops.stop_match_per(a[0], a[1], z(S), z(S), z(S), z(S), out, ids)
    with pytest.raises(ValueError):
        ops.stop_match_per(tok, n, z(S), z(S), z(S), z(S), out, ids, logprob=torch.zeros(S, 8, device=DEV))
    ops.stop_match_per(tok, n, z(S), z(S), z(S), z(S), out, ids)
