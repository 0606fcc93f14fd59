"""db1_select_tokens_slots_per (every slot's sampling parameters read from a device record) against its siblings: with one parameter set in
every record, db1_select_tokens_slots / _lp / _top on the same inputs, every output bit for bit; with six different records, the lockstep
db1_select_tokens_top run on each live row alone under the slot's scalars.  Then the guard, the row map, determinism and the refusals.
The conventions are those of tests/test_select_slots_gpu.py: 6 slots, MAXNEW 8, sentinel-filled buffers, and its row layout (live,
last-token, vacant, limit-1 and no-candidate rows); the shapes are both sides of each NG boundary of the kernel and the model's own."""
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

M, MAXNEW, PAD, SENT, FSENT, TOPN, STEP_BASE = 6, 8, 31, -7, -7.5, 3, 3
T0 = [0, 3, 5, 2, 0, 1]            # row 2: t = limit - 1; row 3: finished (vacant); row 4: limit 1; row 5: no finite logit in [0, hi(V))
LIMIT = [8, 8, 6, 8, 1, 8]
FIN = [0, 0, 0, 1, 0, 0]
SID = [11, 7, 300, 5, 2, 9]
LEN0 = [0, 3, 5, 2, 0, 1]
SUM0 = [0.0, -1.25, -2.5, -3.75, 0.0, -6.25]
LIVE = [0, 1, 2, 4, 5]
SHAPES = [(4096, 4096), (4097, 4104), (12289, 12296), (33025, 33280)]      # V / ld: NG 1 | 3, 3 | 9, 9 (the model's)
DTYPES = [torch.float32, torch.bfloat16]
MODES = ["plain", "lp", "top"]
KEYS = ("t", "finished", "lengths", "status", "out", "ids", "logprob", "sum_logprob", "top_ids", "top_logprob")


def hi_of(V):
    """the end of the 'text' window of a vocabulary of V: 32 000 of the model's 33 025; never a multiple of 4 below it"""
    return 32000 if V == 33025 else V - 97


_LOGITS = {}


def _logits(V, ld, dtype):
    if (V, ld) not in _LOGITS:
        rng = np.random.default_rng(17 + V)
        lg = (rng.standard_normal((M, ld)) * 3).astype(np.float32)
        HI = hi_of(V)
        lg[5, :HI] = np.array([np.nan, np.inf, -np.inf, np.nan], np.float32)[rng.integers(0, 4, HI)]
        lg[0, 100] = np.inf                # (never a candidate)
        lg[1, HI + 5] = 1e9                # (outside the text window, inside the tail window)
        _LOGITS[(V, ld)] = _tdev(lg)
    return _LOGITS[(V, ld)].to(dtype)


def _same(V, greedy):
    """ONE parameter set (test 1): greedy over the text window, or the sampling set of tests/test_select_slots_gpu.py"""
    kw = dict(greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=0) if greedy else \
        dict(greedy=False, temperature=0.8, top_k=50, top_p=0.9, seed=(1 << 40) + 12345)
    return dict(kw, vocab_lo=0, vocab_hi=hi_of(V))


def _kinds(V):
    """six records that differ in every field: two greedy ones with different windows, top_k = 1, top-k only, top-p only, both"""
    HI = hi_of(V)
    return [dict(greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=0, vocab_lo=0, vocab_hi=HI),
            dict(greedy=True, temperature=5.0, top_k=9, top_p=0.3, seed=77, vocab_lo=V - 1025, vocab_hi=V),              # [32000, V) of the model
            dict(greedy=False, temperature=0.7, top_k=1, top_p=0.5, seed=(1 << 33) + 5, vocab_lo=1000, vocab_hi=3000),    # inside the text range
            dict(greedy=False, temperature=1.3, top_k=40, top_p=1.0, seed=(1 << 40) + 12345, vocab_lo=5, vocab_hi=HI - 3),
            dict(greedy=False, temperature=0.8, top_k=0, top_p=0.9, seed=4321, vocab_lo=0, vocab_hi=V),
            dict(greedy=False, temperature=2.0, top_k=50, top_p=0.9, seed=2 ** 64 - 3, vocab_lo=0, vocab_hi=HI)]


def _records(kws):
    from bdm_db1_amd import ops
    return np.stack([ops.pack_slot_params(**kw) for kw in kws])


class _Slots:
    def __init__(self, t=T0, limit=LIMIT, fin=FIN):
        i32 = lambda a: _tdev(np.asarray(a, np.int32))
        self.t, self.limit, self.finished, self.stream_id = i32(t), i32(limit), i32(fin), i32(SID)
        self.lengths = i32(LEN0)
        self.status = i32([0] * M)
        self.out = torch.full((M, MAXNEW), SENT, dtype=torch.int32, device=DEV)
        self.ids = torch.full((M, 2), SENT, dtype=torch.int64, device=DEV)
        self.logprob = torch.full((M, MAXNEW), FSENT, dtype=torch.float32, device=DEV)
        self.sum_logprob = _tdev(np.asarray(SUM0, np.float32))
        self.top_ids = torch.full((M, MAXNEW, TOPN), SENT, dtype=torch.int32, device=DEV)
        self.top_logprob = torch.full((M, MAXNEW, TOPN), FSENT, dtype=torch.float32, device=DEV)

    def _extra(self, mode):
        kw = {}
        if mode in ("lp", "top"):
            kw.update(logprob=self.logprob, sum_logprob=self.sum_logprob)
        if mode == "top":
            kw.update(top_n=TOPN, top_ids=self.top_ids, top_logprob=self.top_logprob)
        return kw

    def snap(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in KEYS}

    def run_per(self, lg, V, params, mode="top", row_map=None):
        from bdm_db1_amd import ops
        ops.select_tokens_slots_per(lg, _tdev(np.ascontiguousarray(params, np.int32)), self.t, self.limit, self.finished, self.lengths, self.out,
                                    self.ids[:, 1], self.status, V=V, pad_id=PAD, step_base=STEP_BASE, stream_id=self.stream_id, row_map=row_map,
                                    **self._extra(mode))
        return self.snap()

    def run_slots(self, lg, V, kw, mode="top", row_map=None):
        from bdm_db1_amd import ops
        ops.select_tokens_slots(lg, self.t, self.limit, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, V=V, pad_id=PAD,
                                step_base=STEP_BASE, stream_id=self.stream_id, row_map=row_map, **kw, **self._extra(mode))
        return self.snap()


def _equal(a, b):
    """bit for bit (NaN-safe: floats are compared as their bits)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _sibling_top(lg, V, row, kw):
    """db1_select_tokens_top on row ``row`` alone, *t = T0[row], the row's stream id, the scalars ``kw`` ->
    dict(tok, fin, n, st, lp, top_ids, top_logprob)"""
    from bdm_db1_amd import ops
    i32 = lambda a: _tdev(np.asarray(a, np.int32))
    t, fin, n, st, sid = i32([T0[row]]), i32([0]), i32([0]), i32([0]), i32([SID[row]])
    out = torch.full((1, MAXNEW), SENT, dtype=torch.int32, device=DEV)
    ids = torch.full((1,), SENT, dtype=torch.int64, device=DEV)
    lp = torch.full((1, MAXNEW), FSENT, dtype=torch.float32, device=DEV)
    sm = torch.zeros(1, dtype=torch.float32, device=DEV)
    ti = torch.full((1, MAXNEW, TOPN), SENT, dtype=torch.int32, device=DEV)
    tl = torch.full((1, MAXNEW, TOPN), FSENT, dtype=torch.float32, device=DEV)
    ops.select_tokens(lg[row:row + 1], t, fin, n, out, ids, st, V=V, pad_id=PAD, step_base=STEP_BASE, stream_id=sid, logprob=lp, sum_logprob=sm,
                      top_n=TOPN, top_ids=ti, top_logprob=tl, **kw)
    torch.cuda.synchronize()
    assert int(out[0, T0[row]]) == int(ids[0])
    return dict(tok=int(ids[0]), fin=int(fin[0]), n=int(n[0]), st=int(st[0]), lp=lp[0, T0[row]].cpu().numpy(),
                top_ids=ti[0, T0[row]].cpu().numpy(), top_logprob=tl[0, T0[row]].cpu().numpy())


def _check_against_siblings(lg, V, kws, got, slots=LIVE):
    """every slot of ``slots`` (live) as the lockstep _top sibling leaves its row under the slot's own scalars; bookkeeping as in
    tests/test_select_slots_gpu.py"""
    for r in slots:
        kw = kws[r]
        sib = _sibling_top(lg, V, r, kw)
        assert got["ids"][r, 1] == sib["tok"] == got["out"][r, T0[r]], (r, kw)                  # bit-equal token
        assert _equal(got["logprob"][r, T0[r]], sib["lp"]), (r, kw)
        assert _equal(got["top_ids"][r, T0[r]], sib["top_ids"]) and _equal(got["top_logprob"][r, T0[r]], sib["top_logprob"]), (r, kw)
        want_sum = np.float32(SUM0[r]) + sib["lp"] if sib["st"] == 0 else np.float32(SUM0[r])
        assert _equal(got["sum_logprob"][r], np.float32(want_sum)), r
        assert got["t"][r] == T0[r] + 1
        assert got["lengths"][r] == LEN0[r] + sib["n"]
        assert got["status"][r] == sib["st"]
        assert got["finished"][r] == int(bool(sib["fin"]) or T0[r] + 1 == LIMIT[r]), r
        if sib["st"] == 0:                                                                     # the slot's OWN window
            assert kw["vocab_lo"] <= sib["tok"] < kw["vocab_hi"], (r, kw)
            k = sib["top_ids"][sib["top_ids"] >= 0]
            assert ((k >= kw["vocab_lo"]) & (k < kw["vocab_hi"])).all(), (r, kw)
        # written at [slot, t[slot]] only
        rest = np.delete(np.arange(MAXNEW), T0[r])
        assert (got["out"][r, rest] == SENT).all() and (got["logprob"][r, rest] == FSENT).all()
        assert (got["top_ids"][r, rest] == SENT).all() and (got["top_logprob"][r, rest] == FSENT).all()


def _check_vacant(got, r=3):
    """pad_id forward, nothing else"""
    assert got["ids"][r, 1] == PAD and got["t"][r] == T0[r] and got["lengths"][r] == LEN0[r] and got["status"][r] == 0 and got["finished"][r] == 1
    assert (got["out"][r] == SENT).all() and (got["logprob"][r] == FSENT).all() and got["sum_logprob"][r] == np.float32(SUM0[r])
    assert (got["top_ids"][r] == SENT).all() and (got["top_logprob"][r] == FSENT).all()


def _check_refused(got, r, t=T0):
    """status bit 2, finished, pad_id forward; out / t / lengths / logprob / sum / top_* as they were"""
    assert got["status"][r] == 4 and got["finished"][r] == 1 and got["ids"][r, 1] == PAD, r
    assert got["t"][r] == t[r] and got["lengths"][r] == LEN0[r] and got["sum_logprob"][r] == np.float32(SUM0[r]), r
    assert (got["out"][r] == SENT).all() and (got["logprob"][r] == FSENT).all(), r
    assert (got["top_ids"][r] == SENT).all() and (got["top_logprob"][r] == FSENT).all(), r


# ------------------------------------------------------------------------------------------------ 1. the same parameters everywhere
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_one_parameter_set_in_every_record_is_the_slot_form(V, ld, dtype, sampling):
    lg = _logits(V, ld, dtype)
    kw = _same(V, not sampling)
    params = _records([kw] * M)
    for mode in MODES:
        want = _Slots().run_slots(lg, V, kw, mode)
        got = _Slots().run_per(lg, V, params, mode)
        for k in KEYS:
            assert _equal(got[k], want[k]), (mode, k)
        # (the comparison is not of two launches that did nothing)
        assert (got["t"][LIVE] == np.asarray(T0)[LIVE] + 1).all() and got["status"][5] == 1 and (got["status"][:5] == 0).all()
        assert (got["ids"][[0, 1, 2, 4], 1] < hi_of(V)).all() and (got["ids"][[0, 1, 2, 4], 1] >= 0).all()


# ------------------------------------------------------------------------------------------------ 2. different parameters per slot
@pytest.mark.parametrize("rot", [0, 3])        # kind k sits in slot (k + rot) % 6: every kind meets a live row that has candidates
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_every_slot_is_decoded_under_its_own_record(V, ld, dtype, rot):
    lg = _logits(V, ld, dtype)
    kinds = _kinds(V)
    kws = [kinds[(s - rot) % M] for s in range(M)]
    got = _Slots().run_per(lg, V, _records(kws), "top")
    _check_against_siblings(lg, V, kws, got)
    _check_vacant(got)
    assert got["finished"][2] == 1 and got["finished"][4] == 1                                # t = limit - 1, limit 1
    assert got["finished"][5] == 1 and got["status"][5] == 1 and got["ids"][5, 1] == PAD      # nothing finite in the slot's window
    assert (got["ids"][:, 0] == SENT).all()
    tail = kws.index(kinds[1])
    assert got["ids"][tail, 1] >= V - 1025                                                    # the greedy slot of the tail window
    if tail == 1:
        assert got["ids"][1, 1] == hi_of(V) + 5                                               # (the 1e9 the text window must not see)
    # 5. determinism: identical calls, identical bits
    again = _Slots().run_per(lg, V, _records(kws), "top")
    for k in KEYS:
        assert _equal(got[k], again[k]), k


# ------------------------------------------------------------------------------------------------ 3. the guard
def _garbage_greedy(kw):
    rec = _records([kw])[0].copy()
    rec[1], rec[4:] = -5, np.array([-1, 0x12345678, 0x7FC00000, 0], np.int32)                 # top_k -5, a seed, NaN, top_p 0
    return rec


@pytest.mark.parametrize("mode", ["plain", "top"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_invalid_records_close_their_slot_and_nothing_else(V, ld, dtype, mode):
    lg = _logits(V, ld, dtype)
    kws = _kinds(V)
    base_rec = _records(kws)
    base = _Slots().run_per(lg, V, base_rec, mode)
    sampled = kws[5]
    bad = lambda **kw: _records([dict(sampled, **kw)])[0]
    nan_t, zero_t = bad(), bad()
    nan_t[6], zero_t[6] = 0x7FC00000, 0
    # launch A: an empty window, vocab_hi > V, top_p = 0 while sampling; slots 1 and 5 are the neighbours
    recA = base_rec.copy()
    recA[0], recA[2], recA[4] = bad(vocab_lo=700, vocab_hi=700), bad(vocab_hi=V + 1), bad(top_p=0.0)
    # launch B: NaN and zero inv_temperature and top_k = -1 while sampling; slot 4 greedy with garbage in words 1 and 4 .. 7; neighbour 5
    recB = base_rec.copy()
    recB[0], recB[1], recB[2], recB[4] = nan_t, zero_t, bad(top_k=-1), _garbage_greedy(kws[1])
    for rec, refused, served in ((recA, (0, 2, 4), (1, 5)), (recB, (0, 1, 2), (5,))):
        rec[3] = bad(vocab_lo=9, vocab_hi=3, top_k=-1)                                        # the vacant slot's record is never looked at
        got = _Slots().run_per(lg, V, rec, mode)
        for r in refused:
            _check_refused(got, r)
        _check_vacant(got)
        for r in served:                                                                       # the neighbours: as in test 2
            for k in KEYS:
                assert _equal(got[k][r], base[k][r]), (r, k)
    # the greedy slot with garbage: served as the greedy sibling under its window serves the row
    if mode == "top":
        _check_against_siblings(lg, V, {4: kws[1]}, got, slots=[4])
    else:
        assert got["status"][4] == 0 and got["t"][4] == 1 and got["ids"][4, 1] >= V - 1025 and got["out"][4, 0] == got["ids"][4, 1]
    # a counter out of range comes first: bit 1, and the record (invalid here) is not read
    t = list(T0)
    t[0] = LIMIT[0]
    got = _Slots(t=t).run_per(lg, V, recA, mode)
    assert got["status"][0] == 2 and got["finished"][0] == 1 and got["ids"][0, 1] == PAD and got["t"][0] == t[0]


# ------------------------------------------------------------------------------------------------ 3b. the kernel against the NumPy rule
@pytest.mark.parametrize("V,ld", [SHAPES[1], SHAPES[3]])
def test_the_kernel_follows_the_numpy_rule(V, ld):
    """tests/slot_params_rule.py (the statement the header, the README and the ops docstring share) against the kernel on fp32 logits: the
    status of every served slot, the token of the greedy and top_k = 1 slots exactly, a sampled slot's token inside the rule's kept set (the
    rule's masses are float64: a token whose cumulative mass lies within 1e-4 of top_p may fall on either side)"""
    import select_rule as R
    import slot_params_rule as S
    lg = _logits(V, ld, torch.float32)
    host = lg.cpu().numpy().astype(np.float64)
    for rot in (0, 3):
        kinds = _kinds(V)
        kws = [kinds[(s - rot) % M] for s in range(M)]
        rec = _records(kws)
        rec[0 if rot else 4] = _records([dict(kinds[5], top_p=0.0)])[0]                        # one record the guard refuses
        got = _Slots().run_per(lg, V, rec, "plain")
        want = S.step_slots(host, None, rec, T0, LIMIT, FIN, SID, V, STEP_BASE)
        assert sorted(want) == LIVE
        for s_, (st, tok) in want.items():
            assert got["status"][s_] == st, (rot, s_)
            if st == S.BAD_PARAMS:
                _check_refused(got, s_)
            elif st == 1:
                assert got["ids"][s_, 1] == PAD
            else:
                p = S.unpack(rec[s_])
                mine = int(got["ids"][s_, 1])
                if p["greedy"] or p["top_k"] == 1:
                    assert mine == tok, (rot, s_)
                else:
                    kept, cum, above = R.kept_set(host[s_, :V], p["vocab_lo"], p["vocab_hi"], 1.0 / float(p["inv_temperature"]), p["top_k"],
                                                  float(p["top_p"]))
                    assert kept[mine] or above[mine] < float(p["top_p"]) + 1e-4, (rot, s_)
        _check_vacant(got)


# ------------------------------------------------------------------------------------------------ 4. the row map
@pytest.mark.parametrize("V,ld", [SHAPES[1], SHAPES[3]])
def test_row_map_moves_the_logits_not_the_records(V, ld):
    lg = _logits(V, ld, torch.bfloat16)
    kws = _kinds(V)
    rec = _records(kws)
    base = _Slots().run_per(lg, V, rec, "top")
    perm = np.array([4, 2, 5, 0, 3, 1])                          # logits row i belongs to slot perm[i]; slot s still reads params[s]
    shuffled = torch.empty_like(lg)
    shuffled[torch.arange(M, device=DEV)] = lg[_tdev(perm.astype(np.int64))]
    got = _Slots().run_per(shuffled, V, rec, "top", row_map=_tdev(perm.astype(np.int32)))
    for k in KEYS:
        assert _equal(base[k], got[k]), k
    # a subset of the slots (an admission): the other slots are not touched at all
    sub = np.array([4, 1], np.int32)
    got = _Slots().run_per(lg[_tdev(sub.astype(np.int64))].contiguous(), V, rec, "top", row_map=_tdev(sub))
    fresh = _Slots().snap()
    for r in range(M):
        for k in KEYS:
            assert _equal(got[k][r], (base if r in sub else fresh)[k][r]), (r, k)
    # (had slot 4, fed by logits row 0, read params[0], it would have chosen greedily in the text window, not as ``base`` did under record 4)


# ------------------------------------------------------------------------------------------------ 5. the refusals
def test_bad_arguments_raise_before_a_launch():
    from bdm_db1_amd import lib, ops
    V, ld = SHAPES[3]
    lg = _logits(V, ld, torch.float32)
    rec = _tdev(_records(_kinds(V)))
    s = _Slots()
    call = lambda params=rec, **kw: ops.select_tokens_slots_per(lg, params, s.t, s.limit, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, V=V,
                                                                pad_id=PAD, **kw)
    shifted = torch.zeros(M * 8 + 4, dtype=torch.int32, device=DEV)[4:].view(M, 8)            # 16 bytes past a 32-byte boundary
    assert rec.data_ptr() % 32 == 0 and shifted.data_ptr() % 32 == 16
    lp, top = dict(logprob=s.logprob, sum_logprob=s.sum_logprob), dict(top_ids=s.top_ids, top_logprob=s.top_logprob)
    for kw in (dict(params=None), dict(params=shifted), dict(params=rec[:5]), dict(params=rec.long()), dict(params=rec.t().contiguous().t()),
               dict(params=rec.cpu()), dict(logprob=s.logprob), dict(sum_logprob=s.sum_logprob), dict(top_n=TOPN, **top), dict(top_n=TOPN, **lp),
               dict(top_n=TOPN, top_ids=s.top_ids, **lp), dict(**lp, **top), dict(top_n=17, **lp, **top), dict(top_n=0, **lp, **top),
               dict(row_map=s.t[:2])):
        with pytest.raises(ValueError):
            call(**kw)
    # the library's own checks, through the C ABI (what a caller without ops meets): DB1_ERR_BAD_SHAPE, nothing launched
    vp = ctypes.c_void_p
    ptr = lambda x: vp(0) if x is None else vp(x.data_ptr())

    def raw(s, params, logprob=None, sum_logprob=None, top_n=0, top_ids=None, top_logprob=None):
        lib.call("db1_select_tokens_slots_per", ptr(lg), M, V, ld, ops.dt_code(lg), params, -1, PAD, 0, ptr(s.t), ptr(s.limit), ptr(s.stream_id),
                 ptr(s.finished), ptr(s.lengths), ptr(s.out), MAXNEW, vp(s.ids[:, 1].data_ptr()), 2, ptr(s.status), vp(0), M, ptr(logprob),
                 ptr(sum_logprob), top_n, ptr(top_ids), ptr(top_logprob), vp(0), 0, ops.stream())

    good = ptr(rec)
    for args in (dict(params=vp(0)), dict(params=ptr(shifted)), dict(params=good, logprob=s.logprob),
                 dict(params=good, top_n=TOPN, **top), dict(params=good, top_n=TOPN, **lp), dict(params=good, top_n=0, **lp, **top),
                 dict(params=good, top_n=17, **lp, **top), dict(params=good, top_n=-1, **lp, **top)):
        with pytest.raises(lib.Db1Error, match="status"):
            raw(s, **args)
    fresh = _Slots().snap()
    got = s.snap()
    for k in KEYS:
        assert _equal(got[k], fresh[k]), k                                                     # nothing was launched
    # and the three accepted combinations do launch
    for mode in MODES:
        s2 = _Slots()
        raw(s2, good, **s2._extra(mode))
        assert (s2.snap()["t"][LIVE] == np.asarray(T0)[LIVE] + 1).all(), mode
    assert ops.select_tokens_slots_supported(V, ld, torch.bfloat16) and lib.load().db1_select_tokens_slots_workspace_bytes(64, V, 1) == 0
