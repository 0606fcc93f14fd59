"""db1_constrain_logits_pen against its NumPy rule (tests/penalty_rule.py): the WHOLE logits buffer is compared bit for bit, padding columns
and untouched rows included.  fp32 and bf16; history lengths across the 256-thread stride; every penalty mode with and without theta,
negative penalties, a bias list that overlaps the history, the banned ids and EOS under the minimum length; NaN / +-inf logits; the count of
a token that fills half the history; history entries outside [0, V); the slot form; a captured launch; the old entry point; the refusals."""
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
import penalty_rule as P  # noqa: E402
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

MODES = [dict(freq=0.4), dict(pres=0.7), dict(freq=0.25, pres=-0.6), dict(freq=-0.3, pres=0.45, theta=1.3)]


def _host_logits(rng, M, ld, dtype, scale=4.0):
    x = (rng.standard_normal((M, ld)) * scale).astype(np.float32)
    return C.bf16_bits(x) if dtype == C.BF16 else x


def _up(l, dtype):
    return _tdev(l.view(np.int16)).view(torch.bfloat16) if dtype == C.BF16 else _tdev(l)


def _down(lg, dtype):
    return lg.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == C.BF16 else lg.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _put(l, r, c, v, dtype):
    l[r, c] = C.bf16_bits(np.array([v], np.float32))[0] if dtype == C.BF16 else np.float32(v)


def _history(rng, S, mx, V):
    """[S, mx]: tokens from a handful of columns plus a spread of others (so some repeat often, some once), and entries outside [0, V);
    -> (hist, the frequent columns)"""
    cols = np.unique(np.concatenate([[0, V - 1], rng.integers(0, V, 3)]))
    h = rng.integers(0, V, (S, mx))
    often = rng.random((S, mx)) < 0.5
    h[often] = cols[rng.integers(0, cols.size, int(often.sum()))]
    out = rng.random((S, mx)) < 0.1
    h[out] = np.array([-1, -7, V, V + 5])[rng.integers(0, 4, int(out.sum()))]
    return h.astype(np.int32), cols


def _kernel_kw(theta=1.0, ngram=0, bad=(), eos_id=-1, min_new=0, freq=0.0, pres=0.0, bias=()):
    """the rule's keywords -> ops.constrain_logits' (device lists)"""
    bias = P.normalise_bias(bias)
    kw = dict(repetition_penalty=theta, no_repeat_ngram_size=ngram, eos_id=eos_id, min_new=min_new, frequency_penalty=freq, presence_penalty=pres,
              bad=_tdev(np.asarray(bad, np.int32)) if len(bad) else None)
    if bias:
        kw.update(bias_ids=_tdev(np.array([k for k, _ in bias], np.int32)), bias_val=_tdev(np.array([b for _, b in bias], np.float32)))
    return kw


def _run(l, dtype, t, hist, V, finished=None, row_map=None, **rule_kw):
    from bdm_db1_amd import ops
    lg = _up(l, dtype)
    dev = {k: (None if v is None else _tdev(np.asarray(v, np.int32))) for k, v in (("finished", finished), ("row_map", row_map))}
    ops.constrain_logits(lg, _tdev(np.atleast_1d(np.asarray(t, np.int32))), _tdev(hist), V=V, **dev, **_kernel_kw(**rule_kw))
    return _down(lg, dtype)


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
@pytest.mark.parametrize("M,V,ld", [(1, 7, 7), (3, 67, 80), (4, 33025, 33280)])
def test_kernel_equals_the_rule_bit_for_bit(dtype, M, V, ld):
    rng = np.random.default_rng(V + (dtype == C.BF16))
    mx = 300
    k = edited = twice = 0
    for t in (0, 1, 255, 256, 257):
        hist, cols = _history(rng, M, mx, V)
        for mode in MODES:
            for with_bias in (False, True):
                k += 1
                l = _host_logits(rng, M, ld, dtype)
                for r in range(M):          # non-finite logits at penalised (and, with a bias, biased) columns: they come back as stored
                    for c, v in zip(cols[:3], (np.nan, np.inf, -np.inf)):
                        if (k + r + c) % 3 == 0:
                            _put(l, r, c, v, dtype)
                kw = dict(mode)
                if with_bias:       # the bias overlaps the history's columns, the banned ids, EOS under min_new, and leaves [0, V)
                    eos = int(cols[1])
                    bad = (V, V + 3, int(cols[-1]), int(rng.integers(0, V)))
                    ids = sorted({int(cols[0]), int(cols[2 % cols.size]), int(cols[-1]), eos, bad[3], int(rng.integers(0, V)), V, V + 9, 3 % V})
                    kw.update(bias={c: float(rng.standard_normal() * 3) for c in ids}, bad=bad, eos_id=eos, min_new=t + (k % 2), ngram=(0, 2)[k % 2])
                want = P.apply(l, hist, t, V=V, dtype=dtype, **kw)
                got = _run(l, dtype, t, hist, V, **kw)
                diff = _bits(got) != _bits(want)
                assert not diff.any(), (t, kw, np.argwhere(diff)[:4], _bits(got)[diff][:4], _bits(want)[diff][:4], _bits(l)[diff][:4])
                edited += int((_bits(want) != _bits(l)).any())
                if with_bias and t > 1:     # (a column both penalised and biased exists: the double rounding is exercised)
                    twice += int(any(0 <= c < V and c in set(hist[0, :t].tolist()) for c in kw["bias"]))
    assert k == 40 and edited >= 32 and twice >= 8


def test_one_token_filling_half_the_history_is_written_once_with_its_count():
    V, mx, t = 67, 300, 299
    rng = np.random.default_rng(3)
    for dtype in (C.F32, C.BF16):
        l = _host_logits(rng, 2, 80, dtype)
        hist = rng.integers(6, V, (2, mx)).astype(np.int32)
        hist[:, ::2] = 5                                    # positions 0, 2, .., 298: 150 copies among the first 299
        _put(l, 0, 5, 3.0, dtype)
        _put(l, 1, 5, -3.0, dtype)
        got = _run(l, dtype, t, hist, V, theta=1.3, freq=0.01, pres=0.5)
        th, inv = np.float32(1.3), np.float32(1.0 / float(np.float32(1.3)))
        p = np.float32(np.float32(np.float32(150) * np.float32(0.01)) + np.float32(0.5))
        want = [np.float32(np.float32(np.float32(3.0) * inv) - p), np.float32(np.float32(np.float32(-3.0) * th) - p)]
        for r in range(2):
            g = C.widen(got[r:r + 1, 5:6], dtype)[0, 0]
            w = C.widen(C.bf16_bits(np.array([want[r]])), dtype)[0] if dtype == C.BF16 else want[r]
            assert g == w, (dtype, r, g, w)
        assert (_bits(got) == _bits(P.apply(l, hist, t, V=V, dtype=dtype, theta=1.3, freq=0.01, pres=0.5))).all()


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_history_entries_outside_the_vocabulary_and_untouched_memory(dtype):
    V, ld, mx, t = 67, 80, 20, 18
    rng = np.random.default_rng(13)
    l = _host_logits(rng, 3, ld, dtype)
    hist = np.tile(np.array([-1, V, V + 5, -9, 2 ** 31 - 1, 4, -1, V], np.int32), (3, 3))[:, :mx]     # one token in range: 4
    got = _run(l, dtype, t, hist, V, freq=1.0, pres=1.0, finished=[0, 1, 0])
    want = P.apply(l, hist, t, V=V, dtype=dtype, freq=1.0, pres=1.0, finished=[0, 1, 0])
    assert (_bits(got) == _bits(want)).all()
    changed = np.argwhere(_bits(got) != _bits(l))
    assert sorted(map(tuple, changed.tolist())) == [(0, 4), (2, 4)]                      # column 4 of the two live rows, nothing else
    n4 = np.float32(np.float32(np.float32(2) * np.float32(1.0)) + np.float32(1.0))       # token 4 at positions 5 and 13: counted twice
    x = C.widen(l, dtype)[0, 4]
    w = np.float32(x - n4)
    assert C.widen(got, dtype)[0, 4] == (C.bf16_widen(C.bf16_bits(np.array([w])))[0] if dtype == C.BF16 else w)
    assert (_bits(got[:, V:]) == _bits(l[:, V:])).all() and (_bits(got[1]) == _bits(l[1])).all()


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_slot_form_row_map_per_slot_counters_and_vacant_slots(dtype):
    V, ld, mx, S = 67, 80, 12, 6
    rng = np.random.default_rng(11)
    hist, cols = _history(rng, S, mx, V)
    l = _host_logits(rng, 4, ld, dtype)
    row_map = [4, 0, 9, 2]                     # a permutation of a subset of the slots; 9: no such slot
    t = [7, 3, 0, 11, 5, 2]
    finished = [0, 1, 1, 0, 0, 1]              # slot 2 (row 3) is vacant
    kw = dict(theta=1.3, ngram=2, bad=(1, V + 1), eos_id=3, min_new=6, freq=0.3, pres=-0.2, bias={int(cols[0]): 1.5, 3: 2.0, 1: -1.0, 66: 0.25})
    want = P.apply(l, hist, np.array(t), V=V, dtype=dtype, finished=finished, row_map=row_map, **kw)
    got = _run(l, dtype, t, hist, V, finished=finished, row_map=row_map, **kw)
    assert (_bits(got) == _bits(want)).all()
    assert (_bits(got[2:]) == _bits(l[2:])).all() and (_bits(got[:2]) != _bits(l[:2])).any()
    # no row_map: row i is slot i, per-slot counters, two of them outside [0, max_new), one slot vacant
    l6 = _host_logits(rng, S, ld, dtype)
    t6 = [7, 3, 12, 11, -1, 2]
    want = P.apply(l6, hist, np.array(t6), V=V, dtype=dtype, finished=[0, 0, 0, 0, 0, 1], **kw)
    got = _run(l6, dtype, t6, hist, V, finished=[0, 0, 0, 0, 0, 1], **kw)
    assert (_bits(got) == _bits(want)).all() and (_bits(got[[2, 4, 5]]) == _bits(l6[[2, 4, 5]])).all()
    # t = 0: no history, the bias alone (and the bans) edits the row
    got = _run(l6, dtype, 0, hist, V, **kw)
    assert (_bits(got) == _bits(P.apply(l6, hist, 0, V=V, dtype=dtype, **kw))).all() and (_bits(got) != _bits(l6)).any()


def test_graph_captured_launch_replays_over_changing_t_and_history():
    from bdm_db1_amd.decode import graph_capture
    from bdm_db1_amd import ops
    dtype, M, V, ld, mx = C.BF16, 8, 33025, 33280, 300
    rng = np.random.default_rng(5)
    l = _host_logits(rng, M, ld, dtype)
    hists = [_history(rng, M, mx, V)[0] for _ in range(3)]
    ts = [4, 257, 29]
    rule = dict(theta=1.2, ngram=3, bad=(7, V, 33000), eos_id=2, min_new=20, freq=0.2, pres=0.1, bias={7: 1.0, 2: -2.0, 100: 0.5, 33024: 3.0})
    kw = dict(V=V, **_kernel_kw(**rule))
    ref = [P.apply(l, h, t, V=V, dtype=dtype, **rule) for h, t in zip(hists, ts)]
    src, lg = _up(l, dtype), _up(l, dtype)
    t_dev, h_dev = _tdev(np.array([0], np.int32)), _tdev(hists[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the capture
        ops.constrain_logits(lg, t_dev, h_dev, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):      # (the cyclic collector held off: bdm_db1_amd.decode.graph_capture)
        ops.constrain_logits(lg, t_dev, h_dev, **kw)
    for i in range(3):
        lg.copy_(src)
        t_dev.fill_(ts[i])
        h_dev.copy_(_tdev(hists[i]))
        graph.replay()
        assert (_down(lg, dtype) == ref[i]).all(), i


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_new_entry_point_with_everything_off_equals_the_old_one(dtype):
    from bdm_db1_amd import lib, ops
    M, V, ld, mx, t = 3, 67, 80, 300, 257
    rng = np.random.default_rng(17)
    l = _host_logits(rng, M, ld, dtype)
    hist, _ = _history(rng, M, mx, V)
    old = _run(l, dtype, t, hist, V, theta=1.3, ngram=2, bad=(1, V + 1), eos_id=3, min_new=300)
    assert (_bits(old) == _bits(C.apply(l, hist, t, V=V, dtype=dtype, theta=1.3, ngram=2, bad=(1, V + 1), eos_id=3, min_new=300))).all()
    L = lib.load()
    lg, tt, hh, bad = _up(l, dtype), _tdev(np.array([t], np.int32)), _tdev(hist), _tdev(np.array([1, V + 1], np.int32))
    th = float(np.float32(1.3))
    st = L.db1_constrain_logits_pen(lg.data_ptr(), M, V, ld, ops.dt_code(lg), tt.data_ptr(), 0, hh.data_ptr(), mx, None, None, M, th,
                                    float(np.float32(1.0 / th)), 2, bad.data_ptr(), 2, 3, 300, 0.0, 0.0, None, None, 0, None, 0, None)
    assert st == 0
    torch.cuda.synchronize()
    assert (_bits(_down(lg, dtype)) == _bits(old)).all() and (_bits(old) != _bits(l)).any()
    # ... and with nothing at all to do it launches nothing
    lg = _up(l, dtype)
    assert L.db1_constrain_logits_pen(lg.data_ptr(), M, V, ld, ops.dt_code(lg), tt.data_ptr(), 0, hh.data_ptr(), mx, None, None, M, 1.0, 1.0, 0,
                                      None, 0, -1, 0, 0.0, 0.0, None, None, 0, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (_bits(_down(lg, dtype)) == _bits(l)).all()


def test_invalid_arguments_raise_and_leave_the_logits_alone():
    from bdm_db1_amd import lib, ops
    M, V, mx = 2, 100, 8
    lg = torch.full((M, V), 7.5, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    t, hist, fin = torch.ones(1, **i32), torch.zeros(M, mx, **i32), torch.zeros(M, **i32)
    ids, val = torch.arange(3, **i32), torch.ones(3, device=DEV)
    ok = dict(frequency_penalty=0.5, presence_penalty=0.5, bias_ids=ids, bias_val=val, finished=fin)
    for kw in (dict(ok, frequency_penalty=float("nan")), dict(ok, frequency_penalty=float("inf")), dict(ok, presence_penalty=float("-inf")),
               dict(ok, presence_penalty=1e39), dict(ok, bias_val=None), dict(ok, bias_ids=None), dict(ok, bias_ids=ids.long()),
               dict(ok, bias_val=val.double()), dict(ok, bias_val=torch.ones(4, device=DEV)), dict(ok, bias_ids=[0, 1, 2]),
               dict(ok, bias_ids=torch.arange(1025, **i32), bias_val=torch.ones(1025, device=DEV)), dict(ok, bias_ids=ids.cpu()),
               dict(ok, repetition_penalty=0.0), dict(ok, V=V + 1)):
        with pytest.raises(ValueError):
            ops.constrain_logits(lg, t, hist, **kw)
    for a, b, c in ((lg.half(), t, hist), (lg, t, torch.zeros(M, 4097, **i32)), (lg, torch.zeros(3, **i32), hist)):
        with pytest.raises(ValueError):
            ops.constrain_logits(a, b, c, **ok)
    assert not ops.constrain_logits_pen_supported(V, V, mx, 0, 1025, torch.float32) and not ops.constrain_logits_pen_supported(V, V, 4097, 0, 0, torch.float32)
    assert ops.constrain_logits_pen_supported(V, V, 4096, 1024, 1024, torch.bfloat16)
    # the C entry point itself: the library's error codes, before any launch
    L = lib.load()
    P_ = lambda x: x.data_ptr()
    args = lambda **o: tuple({**dict(lg=P_(lg), M=M, V=V, ld=V, dt=0, t=P_(t), per=0, hist=P_(hist), mx=mx, fin=P_(fin), rm=None, S=M, th=1.3,
                                     inv=1 / 1.3, n=2, bad=None, nb=0, eos=1, mn=4, fr=0.5, pr=0.5, bi=P_(ids), bv=P_(val), nbias=3, ws=None,
                                     wsn=0, st=None), **o}.values())
    for o in (dict(dt=5), dict(M=0), dict(ld=V - 1), dict(mx=4097), dict(nbias=1025), dict(nbias=-1), dict(bi=None), dict(bv=None),
              dict(fr=float("nan")), dict(pr=float("inf")), dict(th=0.0), dict(S=M + 1), dict(lg=None), dict(hist=None)):
        assert L.db1_constrain_logits_pen(*args(**o)) != 0, o
        assert L.db1_last_error()
    assert L.db1_constrain_logits_pen_workspace_bytes(M, V, mx, 0, 3, 0) == 0
    torch.cuda.synchronize()
    assert (lg == 7.5).all()
    assert L.db1_constrain_logits_pen(*args()) == 0        # (and the valid call does edit)
    torch.cuda.synchronize()
    assert not (lg == 7.5).all()
