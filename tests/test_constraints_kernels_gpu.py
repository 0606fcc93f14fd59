"""db1_constrain_logits against its NumPy rule (tests/constraint_rule.py): the WHOLE logits buffer is compared bit for bit, padding columns
and untouched rows included.  fp32 and bf16; histories with heavy duplication and entries outside [0, V); NaN / +-inf logits at history
columns; the slot form (row_map, per-slot counters, vacant slots); the guard; a captured launch; the refusals."""
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
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

DTYPES = {C.F32: torch.float32, C.BF16: torch.bfloat16}


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
    """[S, mx]: tokens from a handful of columns (so tokens and n-grams repeat), one token on every second position, and entries outside
    [0, V); -> (hist, the columns it uses)"""
    cols = np.unique(np.concatenate([[0, V - 1], rng.integers(0, V, 3)]))
    pool = np.concatenate([cols, [-1, -7, V, V + 5]])
    h = pool[rng.integers(0, pool.size, (S, mx))]
    h[:, ::2] = cols[rng.integers(0, cols.size, (S, 1))]
    return h.astype(np.int32), cols


def _run(l, dtype, t, hist, V, **kw):
    from bdm_db1_amd import ops
    lg = _up(l, dtype)
    bad = kw.pop("bad", ())
    dev = {k: (None if v is None else _tdev(np.asarray(v, np.int32))) for k, v in
           (("finished", kw.pop("finished", None)), ("row_map", kw.pop("row_map", None)))}
    ops.constrain_logits(lg, _tdev(np.atleast_1d(np.asarray(t, np.int32))), _tdev(hist), V=V,
                         bad=_tdev(np.asarray(bad, np.int32)) if len(bad) else None, **dev, **kw)
    return _down(lg, dtype)


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
@pytest.mark.parametrize("M,V,ld", [(1, 7, 7), (3, 67, 80), (4, 33025, 33280)])
def test_kernel_equals_the_rule_bit_for_bit(dtype, M, V, ld):
    rng = np.random.default_rng(V + (dtype == C.BF16))
    thetas = (1.0, 1.3, 0.7)
    k = edited = 0
    for mx in (1, 5, 300):
        hist, cols = _history(rng, M, mx, V)
        for n in (0, 1, 2, 3):
            for t in sorted({0, 1, n - 1, n, mx - 1}):
                if not 0 <= t < mx:
                    continue
                k += 1
                theta = thetas[k % 3]
                l = _host_logits(rng, M, ld, dtype)
                for r in range(M):          # non-finite logits at history columns: they come back as stored unless banned
                    for c, v in zip(cols[:3], (np.nan, np.inf, -np.inf)):
                        if (k + r + c) % 3 == 0:
                            _put(l, r, c, v, dtype)
                bad = (V, V + 3, int(cols[-1]), int(rng.integers(0, V))) if k % 2 else ()
                eos, min_new = ((-1, mx) if k % 4 == 0 else (int(rng.integers(0, V)), t + (k % 3)))
                kw = dict(theta=theta, ngram=n, bad=bad, eos_id=eos, min_new=min_new)
                want = C.apply(l, hist, t, V=V, dtype=dtype, **kw)
                got = _run(l, dtype, t, hist, V, repetition_penalty=theta, no_repeat_ngram_size=n, bad=bad, eos_id=eos, min_new=min_new)
                assert (_bits(got) == _bits(want)).all(), (mx, n, t, theta, np.argwhere(_bits(got) != _bits(want))[:4])
                edited += int((_bits(want) != _bits(l)).any())
    assert k > 30 and edited >= k // 3         # (the cases do edit)


def test_one_token_filling_half_the_history_is_penalised_once():
    V, mx, t = 67, 300, 299
    rng = np.random.default_rng(3)
    for dtype in (C.F32, C.BF16):
        l = _host_logits(rng, 2, 80, dtype)
        hist = rng.integers(0, V, (2, mx)).astype(np.int32)
        hist[:, ::2] = 5
        _put(l, 0, 5, 3.0, dtype)
        _put(l, 1, 5, -3.0, dtype)
        got = _run(l, dtype, t, hist, V, repetition_penalty=1.3)
        th, inv = np.float32(1.3), np.float32(1.0 / float(np.float32(1.3)))
        want = [np.float32(3.0) * inv, np.float32(-3.0) * th]
        for r in range(2):
            g = C.widen(got[r:r + 1, 5:6], dtype)[0, 0]
            w = C.widen(C.bf16_bits(np.array([want[r]])), dtype)[0] if dtype == C.BF16 else want[r]
            assert g == w, (dtype, r, g, w)
        assert (_bits(got) == _bits(C.apply(l, hist, t, V=V, dtype=dtype, theta=1.3))).all()


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_slot_form_row_map_per_slot_counters_and_vacant_slots(dtype):
    V, ld, mx, S = 67, 80, 12, 6
    rng = np.random.default_rng(11)
    hist, _ = _history(rng, S, mx, V)
    l = _host_logits(rng, 4, ld, dtype)
    row_map = [4, 0, 9, 2]                     # a permutation of a subset of the slots; 9: no such slot
    t = [7, 3, 0, 11, 5, 2]
    finished = [0, 1, 1, 0, 0, 1]              # slot 2 (row 3) is vacant
    kw = dict(theta=1.3, ngram=2, bad=(1, V + 1), eos_id=3, min_new=6)
    want = C.apply(l, hist, np.array(t), V=V, dtype=dtype, finished=finished, row_map=row_map, **kw)
    got = _run(l, dtype, t, hist, V, finished=finished, row_map=row_map, repetition_penalty=1.3, no_repeat_ngram_size=2, bad=(1, V + 1),
               eos_id=3, min_new=6)
    assert (_bits(got) == _bits(want)).all()
    assert (_bits(got[2:]) == _bits(l[2:])).all() and (_bits(got[:2]) != _bits(l[:2])).any()
    assert np.isneginf(C.widen(got, dtype)[0, 3]) and not np.isneginf(C.widen(got, dtype)[1, 3])      # min_new 6: slot 4 (t 5) yes, slot 0 (t 7) no
    # no row_map: row i is slot i, per-slot counters, one of them outside [0, max_new)
    l6 = _host_logits(rng, S, ld, dtype)
    t6 = [7, 3, 12, 11, -1, 2]
    want = C.apply(l6, hist, np.array(t6), V=V, dtype=dtype, finished=[0, 0, 0, 0, 0, 1], **kw)
    got = _run(l6, dtype, t6, hist, V, finished=[0, 0, 0, 0, 0, 1], repetition_penalty=1.3, no_repeat_ngram_size=2, bad=(1, V + 1), eos_id=3,
               min_new=6)
    assert (_bits(got) == _bits(want)).all()
    assert (_bits(got[[2, 4, 5]]) == _bits(l6[[2, 4, 5]])).all()
    # one shared counter: finished rows stay untouched; the counter outside [0, max_new): the buffer is unchanged
    want = C.apply(l6, hist, 9, V=V, dtype=dtype, finished=[0, 1, 0, 0, 1, 0], **kw)
    got = _run(l6, dtype, 9, hist, V, finished=[0, 1, 0, 0, 1, 0], repetition_penalty=1.3, no_repeat_ngram_size=2, bad=(1, V + 1), eos_id=3,
               min_new=6)
    assert (_bits(got) == _bits(want)).all() and (_bits(got[[1, 4]]) == _bits(l6[[1, 4]])).all()
    for t_out in (-1, mx, mx + 100):
        got = _run(l6, dtype, t_out, hist, V, repetition_penalty=1.3, no_repeat_ngram_size=1, bad=(1,), eos_id=3, min_new=10 ** 6)
        assert (_bits(got) == _bits(l6)).all(), t_out


def test_graph_captured_launch_replays_over_changing_t_and_history():
    from bdm_db1_amd.decode import graph_capture
    from bdm_db1_amd import ops
    dtype, M, V, ld, mx = C.BF16, 64, 33025, 33280, 30
    rng = np.random.default_rng(5)
    l = _host_logits(rng, M, ld, dtype)
    hists = [_history(rng, M, mx, V)[0] for _ in range(3)]
    ts = [4, 17, 29]
    bad = _tdev(np.array([7, V, 33000], np.int32))
    kw = dict(V=V, repetition_penalty=1.2, no_repeat_ngram_size=3, bad=bad, eos_id=2, min_new=20)
    ref = []
    for h, t in zip(hists, ts):
        lg = _up(l, dtype)
        ops.constrain_logits(lg, _tdev(np.array([t], np.int32)), _tdev(h), **kw)
        ref.append(_down(lg, dtype))
        assert (ref[-1] == C.apply(l, h, t, V=V, dtype=dtype, theta=1.2, ngram=3, bad=(7, V, 33000), eos_id=2, min_new=20)).all()
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


def test_invalid_arguments_raise_and_leave_the_logits_alone():
    from bdm_db1_amd import lib, ops
    M, V, mx = 2, 100, 8
    lg = torch.full((M, V), 7.5, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    t, hist, fin = torch.ones(1, **i32), torch.zeros(M, mx, **i32), torch.zeros(M, **i32)
    bad = torch.zeros(3, **i32)
    ok = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad=bad, eos_id=1, min_new=4, finished=fin)
    cases = [
        (lg.half(), t, hist, ok),                                                     # logits dtype
        (lg.t(), t, hist, ok),                                                        # column stride
        (lg, t, hist.long(), ok),                                                     # history dtype
        (lg, t, torch.zeros(M + 1, mx, **i32), ok),                                   # no row_map: one history row per logits row
        (lg, t, torch.zeros(M, 4097, **i32), ok),                                     # max_new beyond the LDS staging
        (lg, torch.zeros(3, **i32), hist, ok),                                        # t: 1 or one per slot
        (lg, t.long(), hist, ok),
        (lg, t, hist, dict(ok, repetition_penalty=0.0)),
        (lg, t, hist, dict(ok, repetition_penalty=float("nan"))),
        (lg, t, hist, dict(ok, repetition_penalty=float("inf"))),
        (lg, t, hist, dict(ok, no_repeat_ngram_size=-1)),
        (lg, t, hist, dict(ok, min_new=-1)),
        (lg, t, hist, dict(ok, bad=torch.zeros(1025, **i32))),
        (lg, t, hist, dict(ok, bad=bad.long())),
        (lg, t, hist, dict(ok, finished=torch.zeros(M + 1, **i32))),
        (lg, t, hist, dict(ok, row_map=torch.zeros(M + 1, **i32))),
        (lg, t, hist, dict(ok, V=V + 1)),
    ]
    for a, b, c, kw in cases:
        with pytest.raises(ValueError):
            ops.constrain_logits(a, b, c, **kw)
    for a, b, c, kw, word in ((lg, t, torch.zeros(M, 4097, **i32), ok, "max_new 4097"), (lg, t, hist, dict(ok, bad=torch.zeros(1025, **i32)), "1025 banned"),
                              (lg, 1, hist, ok, "t and bad"), (lg, t, hist, dict(ok, bad=[1, 2]), "t and bad")):
        with pytest.raises(ValueError, match=word):          # (the limits and the argument kinds are named in the message)
            ops.constrain_logits(a, b, c, **kw)
    assert not ops.constrain_logits_supported(V, V, 4097, 0, torch.float32) and not ops.constrain_logits_supported(V, V, mx, 1025, torch.float32)
    assert ops.constrain_logits_supported(V, V, 4096, 1024, torch.bfloat16)
    # the C entry point itself: the library's error codes, before any launch
    L = lib.load()
    P = lambda x: x.data_ptr()
    args = lambda **o: tuple({**dict(lg=P(lg), M=M, V=V, ld=V, dt=0, t=P(t), per=0, hist=P(hist), mx=mx, fin=P(fin), rm=None, S=M, th=1.3,
                                     inv=1 / 1.3, n=2, bad=P(bad), nb=3, eos=1, mn=4, ws=None, wsn=0, st=None), **o}.values())
    for o in (dict(dt=5), dict(M=0), dict(ld=V - 1), dict(mx=0), dict(mx=4097), dict(nb=1025), dict(nb=-1), dict(S=M + 1), dict(lg=None),
              dict(t=None), dict(hist=None), dict(bad=None), dict(th=0.0), dict(inv=float("inf")), dict(n=-1), dict(mn=-1)):
        assert L.db1_constrain_logits(*args(**o)) != 0, o
        assert L.db1_last_error()
    assert L.db1_constrain_logits_workspace_bytes(M, V, mx, 3, 0) == 0
    torch.cuda.synchronize()
    assert (lg == 7.5).all()
    assert L.db1_constrain_logits(*args()) == 0        # (and the valid call does edit)
    torch.cuda.synchronize()
    assert not (lg == 7.5).all()
