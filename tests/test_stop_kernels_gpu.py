"""db1_stop_match against its NumPy rule (tests/stop_rule.py): every integer output, and logprob / sum_logprob bit for bit.  1, 3 and 16
sequences of 1, 2 and 16 tokens; a match that removes the whole output; n < L; a match ending at max_new; two sequences matching at once;
lengths == checked; a trimmed slot launched again; a stale ``checked``; row_map with entries out of range; with and without the log-prob and
top-n buffers; a captured launch replayed over state the host changes; the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stop_rule as S  # noqa: E402
from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

PAD = 9


def _state(rng, n_slots, mx, lp=False, n_top=0, vocab=4):
    st = dict(lengths=rng.integers(0, mx + 1, n_slots).astype(np.int32), checked=np.zeros(n_slots, np.int32),
              finished=np.zeros(n_slots, np.int32), stop_hit=np.zeros(n_slots, np.int32),
              out=rng.integers(0, vocab, (n_slots, mx)).astype(np.int32), next_ids=rng.integers(0, vocab, n_slots).astype(np.int64))
    if lp:
        st["logprob"] = -rng.random((n_slots, mx)).astype(np.float32) * 5
        st["sum_logprob"] = -rng.random(n_slots).astype(np.float32)
    if n_top:
        st["top_ids"] = rng.integers(0, vocab, (n_slots, mx, n_top)).astype(np.int32)
        st["top_logprob"] = -rng.random((n_slots, mx, n_top)).astype(np.float32)
    return st


def _launch(dev, stops, row_map=None, fill=-1):
    from bdm_db1_amd import ops
    tok, n = S.pack(stops, fill)
    opt = {k: dev[k] for k in ("logprob", "sum_logprob", "top_ids", "top_logprob") if k in dev}
    if "top_ids" in dev:
        opt["top_n"] = int(dev["top_ids"].shape[2])
    ops.stop_match(_tdev(tok), _tdev(n), dev["lengths"], dev["checked"], dev["finished"], dev["stop_hit"], dev["out"], dev["next_ids"], pad_id=PAD,
                   row_map=None if row_map is None else _tdev(np.asarray(row_map, np.int32)), **opt)


def _run(st, stops, row_map=None, fill=-1):
    dev = {k: _tdev(v) for k, v in st.items()}
    _launch(dev, stops, row_map, fill)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}


def _same(got, want, where=""):
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = got[k], want[k]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert (a == b).all(), (where, k, np.argwhere(a != b)[:4])


def _plant(st, s, n, seq):
    """slot s: n tokens, the last len(seq) of them ``seq``"""
    st["lengths"][s] = n
    st["out"][s, n - len(seq):n] = seq


@pytest.mark.parametrize("bufs", ["plain", "lp", "top"])
@pytest.mark.parametrize("n_stop,L", [(1, 1), (1, 2), (1, 16), (3, 1), (3, 2), (3, 16), (16, 1), (16, 2), (16, 16)])
def test_kernel_equals_the_rule(n_stop, L, bufs):
    rng = np.random.default_rng(100 * n_stop + L)
    n_slots, mx = 70, 40                                             # (more than one wave's worth of rows; tokens 0 .. 3, sequences from 4 up)
    stops = [tuple(int(v) for v in rng.integers(4, 8, L)) for _ in range(n_stop)]
    st = _state(rng, n_slots, mx, lp=bufs != "plain", n_top=3 if bufs == "top" else 0)
    st["checked"][:] = rng.integers(0, mx + 1, n_slots)
    for s in range(0, n_slots, 2):                                    # every second slot ends in one of the sequences ...
        _plant(st, s, int(rng.integers(L, mx + 1)), stops[int(rng.integers(0, n_stop))])
    _plant(st, 0, L, stops[n_stop - 1])                              # ... slot 0 at n == L: the whole output goes, lengths = 0
    _plant(st, 2, mx, stops[0])                                      # ... slot 2 at n == max_new
    st["checked"][[0, 2]] = 0
    if L > 1:                                                        # n < L: the tail of a sequence alone at the start of a row matches nothing
        st["lengths"][4], st["checked"][4] = L - 1, 0
        st["out"][4, :L - 1] = stops[0][1:]
    _plant(st, 6, max(L, 5), stops[0])
    st["checked"][6] = st["lengths"][6]                              # a matching tail that was looked at already: not touched
    want = S.step(st, stops, PAD)
    got = _run(st, stops)
    _same(got, want, (n_stop, L))
    assert want["lengths"][0] == 0 and (want["out"][0, :L] == PAD).all() and want["stop_hit"][0] >= 1
    assert want["lengths"][2] == mx - L and want["finished"][2] == 1
    assert (L == 1 or want["finished"][4] == 0) and all((want[k][6] == st[k][6]).all() for k in st)
    assert (want["stop_hit"] > 0).sum() >= 20 and (want["stop_hit"] == 0).sum() >= 20
    # the same launch again changes nothing: lengths == checked everywhere now
    _same(_run(want, stops), want, "again")


def test_longest_match_wins_then_the_lowest_index():
    st = _state(np.random.default_rng(1), 4, 12, lp=True, n_top=2)
    st["checked"][:] = 0
    for s in range(4):
        _plant(st, s, 8, (5, 6, 7))
    cases = [[(7,), (6, 7), (5, 6, 7)], [(5, 6, 7), (7,), (6, 7)], [(6, 7), (7,), (6, 7)], [(7,), (7,), (4, 7)]]
    for stops, hit, L in zip(cases, (3, 1, 1, 1), (3, 3, 2, 1)):
        want = S.step(st, stops, PAD)
        assert want["stop_hit"].tolist() == [hit] * 4 and want["lengths"].tolist() == [8 - L] * 4
        _same(_run(st, stops), want, stops)
    # the columns of stop_tok after a sequence's length are never compared: whatever they hold
    _same(_run(st, cases[0], fill=7), S.step(st, cases[0], PAD), "fill")


def test_a_trimmed_slot_is_not_trimmed_twice_and_a_stale_checked_heals():
    st = _state(np.random.default_rng(2), 3, 6, lp=True)
    st["out"][0] = [1, 2, 5, 5, 0, 0]                                # stop [5] on a tail 5 5
    st["lengths"][:], st["checked"][:] = [4, 0, 3], [3, 5, 3]
    one = _run(st, [(5,)])
    _same(one, S.step(st, [(5,)], PAD), "first")
    assert one["out"][0].tolist() == [1, 2, 5, PAD, 0, 0] and one["lengths"][0] == 3 and one["checked"][0] == 3 and one["finished"][0] == 1
    # slot 1: a stale checked = 5 over a fresh lengths = 0 heals, and nothing else of the slot is written
    assert one["checked"][1] == 0 and (one["out"][1] == st["out"][1]).all() and one["next_ids"][1] == st["next_ids"][1] and one["finished"][1] == 0
    two = _run(one, [(5,)])
    _same(two, one, "second")                                        # the tail is still a 5: the slot is not trimmed again


@pytest.mark.parametrize("bufs", ["plain", "top"])
def test_row_map_with_entries_out_of_range(bufs):
    rng = np.random.default_rng(3)
    st = _state(rng, 8, 10, lp=bufs == "top", n_top=2 if bufs == "top" else 0)
    for s in range(8):
        _plant(st, s, 3 + s % 4, (6, 5))
    row_map = [5, -1, 0, 8, 7, 2 ** 31 - 1, 3]
    want = S.step(st, [(6, 5)], PAD, row_map)
    _same(_run(st, [(6, 5)], row_map), want, "row_map")
    assert want["finished"].tolist() == [1, 0, 0, 1, 0, 1, 0, 1]


def test_graph_captured_launch_replays_over_state_the_host_changes():
    from bdm_db1_amd.decode import graph_capture
    from bdm_db1_amd import ops
    rng = np.random.default_rng(4)
    n_slots, mx = 16, 24
    stops = [(5, 6), (6,), (7, 5, 6)]
    base = _state(rng, n_slots, mx, lp=True, n_top=2, vocab=8)
    base["lengths"][:] = 0
    dev = {k: _tdev(v) for k, v in base.items()}
    tok, n = S.pack(stops)
    args = (_tdev(tok), _tdev(n), dev["lengths"], dev["checked"], dev["finished"], dev["stop_hit"], dev["out"], dev["next_ids"])
    kw = dict(pad_id=PAD, logprob=dev["logprob"], sum_logprob=dev["sum_logprob"], top_n=2, top_ids=dev["top_ids"], top_logprob=dev["top_logprob"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the capture (lengths == checked == 0: it touches nothing)
        ops.stop_match(*args, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):      # (the cyclic collector held off: bdm_db1_amd.decode.graph_capture)
        ops.stop_match(*args, **kw)
    host = {k: v.copy() for k, v in base.items()}
    hits = 0
    for step in range(mx):       # the host plays the selection: every live row gets one more token, then the replay looks at it
        live = host["finished"] == 0
        host["lengths"][live] += 1
        dev["lengths"].copy_(_tdev(host["lengths"]))
        host = S.step(host, stops, PAD)
        graph.replay()
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in dev.items()}, host, step)
        hits = int((host["stop_hit"] > 0).sum())
    assert hits >= 4


def test_invalid_arguments_raise():
    from bdm_db1_amd import lib, ops
    i32 = dict(dtype=torch.int32, device=DEV)
    n_slots, mx = 4, 8
    tok, n = torch.zeros(2, 16, **i32), torch.ones(2, **i32)
    v = lambda: torch.zeros(n_slots, **i32)
    out, nxt = torch.zeros(n_slots, mx, **i32), torch.zeros(n_slots, dtype=torch.long, device=DEV)
    lp, sm = torch.zeros(n_slots, mx, device=DEV), torch.zeros(n_slots, device=DEV)
    ti, tl = torch.zeros(n_slots, mx, 2, **i32), torch.zeros(n_slots, mx, 2, device=DEV)
    good = dict(stop_tok=tok, stop_len=n, lengths=v(), checked=v(), finished=v(), stop_hit=v(), out=out, next_ids=nxt)
    ops.stop_match(**good)
    ops.stop_match(**good, logprob=lp, sum_logprob=sm, top_n=2, top_ids=ti, top_logprob=tl)
    for kw in (dict(good, stop_tok=torch.zeros(17, 16, **i32), stop_len=torch.ones(17, **i32)), dict(good, stop_tok=torch.zeros(2, 8, **i32)),
               dict(good, stop_tok=torch.zeros(0, 16, **i32), stop_len=torch.ones(0, **i32)), dict(good, stop_len=torch.ones(3, **i32)),
               dict(good, stop_tok=tok.long()), dict(good, lengths=torch.zeros(n_slots + 1, **i32)), dict(good, checked=v().long()),
               dict(good, out=out[0]), dict(good, next_ids=nxt.int()), dict(good, row_map=torch.zeros(n_slots + 1, **i32)),
               dict(good, logprob=lp), dict(good, sum_logprob=sm), dict(good, top_n=2, top_ids=ti, top_logprob=tl),
               dict(good, logprob=lp, sum_logprob=sm, top_n=2, top_ids=ti), dict(good, logprob=lp, sum_logprob=sm, top_n=17, top_ids=ti, top_logprob=tl),
               dict(good, logprob=lp, sum_logprob=sm, top_n=3, top_ids=ti, top_logprob=tl)):
        with pytest.raises(ValueError):
            ops.stop_match(**kw)
    assert ops.stop_match_supported(16, 4096) and not ops.stop_match_supported(17, 30)
    # the C entry point itself
    L = lib.load()
    P_ = lambda x: x.data_ptr()
    g = good
    args = lambda **o: tuple({**dict(tok=P_(tok), n=P_(n), ns=2, pad=0, le=P_(g["lengths"]), ch=P_(g["checked"]), fi=P_(g["finished"]),
                                     hit=P_(g["stop_hit"]), out=P_(out), mx=mx, nxt=P_(nxt), stride=1, rm=None, M=n_slots, S=n_slots, lp=None,
                                     sm=None, tn=0, ti=None, tl=None, st=None), **o}.values())
    for o in (dict(ns=0), dict(ns=17), dict(M=0), dict(S=n_slots + 1), dict(mx=0), dict(tok=None), dict(le=None), dict(ch=None), dict(hit=None),
              dict(nxt=None), dict(lp=P_(lp)), dict(sm=P_(sm)), dict(tn=2), dict(tn=2, ti=P_(ti), tl=P_(tl)),
              dict(lp=P_(lp), sm=P_(sm), tn=17, ti=P_(ti), tl=P_(tl)), dict(lp=P_(lp), sm=P_(sm), ti=P_(ti), tl=P_(tl))):
        assert L.db1_stop_match(*args(**o)) != 0, o
        assert L.db1_last_error()
    assert L.db1_stop_match(*args()) == 0
    torch.cuda.synchronize()
