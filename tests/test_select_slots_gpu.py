"""db1_select_tokens_slots (per-slot token counters, limits and the row map) against its sibling db1_select_tokens called on every live row
alone with the scalar counter t[row]: the tokens must be bit-equal, and the bookkeeping must be the slot's own."""
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

M, V, LD, HI, MAXNEW, PAD, SENT = 6, 33025, 33280, 32000, 8, 31999, -7
T0 = [0, 3, 5, 2, 0, 1]            # row 2: t = limit - 1; row 3: finished (vacant); row 4: limit 1; row 5: no finite logit in the window
LIMIT = [8, 8, 6, 8, 1, 8]
FIN = [0, 0, 0, 1, 0, 0]
SID = [11, 7, 300, 5, 2, 9]
LIVE = [0, 1, 2, 4, 5]
SAMPLING = dict(greedy=False, top_k=50, top_p=0.9, temperature=0.8, seed=(1 << 40) + 12345, step_base=3)


@pytest.fixture(scope="module")
def logits32():
    rng = np.random.default_rng(17)
    lg = (rng.standard_normal((M, LD)) * 3).astype(np.float32)
    lg[5, :HI] = np.array([np.nan, np.inf, -np.inf, np.nan], np.float32)[rng.integers(0, 4, HI)]
    lg[0, 100] = np.inf                # (never a candidate)
    lg[1, HI + 5] = 1e9                # (outside the window)
    return lg


def _logits(logits32, dtype):
    return _tdev(logits32).to(dtype)


class _Slots:
    def __init__(self, t=T0, limit=LIMIT, fin=FIN):
        i32 = lambda a: _tdev(np.asarray(a, np.int32))
        self.t, self.limit, self.finished, self.stream_id = i32(t), i32(limit), i32(fin), i32(SID)
        self.lengths = i32([0, 3, 5, 2, 0, 1])
        self.status = i32([0] * M)
        self.out = torch.full((M, MAXNEW), SENT, dtype=torch.int32, device=DEV)
        self.ids = torch.full((M, 2), SENT, dtype=torch.int64, device=DEV)

    def run(self, lg, row_map=None, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens_slots(lg, self.t, self.limit, self.finished, self.lengths, self.out, self.ids[:, 1], self.status, V=V, vocab_hi=HI,
                                pad_id=PAD, stream_id=self.stream_id, row_map=row_map, **kw)
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("t", "finished", "lengths", "status", "out", "ids")}


def _sibling(lg, row, **kw):
    """db1_select_tokens on row ``row`` alone, *t = T0[row], the row's stream id -> (token, finished, length, status)"""
    from bdm_db1_amd import ops
    i32 = lambda a: _tdev(np.asarray(a, np.int32))
    t, fin, n, st, sid = i32([T0[row]]), i32([0]), i32([0]), i32([0]), i32([SID[row]])
    out = torch.full((1, MAXNEW), SENT, dtype=torch.int32, device=DEV)
    ids = torch.full((1,), SENT, dtype=torch.int64, device=DEV)
    ops.select_tokens(lg[row:row + 1], t, fin, n, out, ids, st, V=V, vocab_hi=HI, pad_id=PAD, stream_id=sid, **kw)
    assert int(out[0, T0[row]]) == int(ids[0])
    return int(ids[0]), int(fin[0]), int(n[0]), int(st[0])


@pytest.mark.parametrize("mode", ["greedy", "sampling"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slots_match_the_sibling_row_by_row(logits32, dtype, mode):
    kw = {} if mode == "greedy" else SAMPLING
    lg = _logits(logits32, dtype)
    got = _Slots().run(lg, **kw)
    before = _Slots()
    len0 = before.lengths.cpu().numpy()
    want_out = np.full((M, MAXNEW), SENT, np.int32)
    for r in LIVE:
        tok, fin, n, st = _sibling(lg, r, **kw)
        want_out[r, T0[r]] = tok
        assert got["ids"][r, 1] == tok, r                         # bit-equal token
        assert got["t"][r] == T0[r] + 1
        assert got["lengths"][r] == len0[r] + n
        assert got["status"][r] == st
        assert got["finished"][r] == int(bool(fin) or T0[r] + 1 == LIMIT[r]), r
    assert np.array_equal(got["out"], want_out)                   # written at [row, t[row]] only
    assert got["finished"][2] == 1 and got["finished"][4] == 1
    assert got["finished"][5] == 1 and got["status"][5] & 1 and got["ids"][5, 1] == PAD
    assert got["finished"][0] == 0 and got["finished"][1] == 0
    # the vacant row: pad_id forward, nothing else
    assert got["ids"][3, 1] == PAD and got["t"][3] == T0[3] and got["lengths"][3] == len0[3] and got["status"][3] == 0
    assert (got["out"][3] == SENT).all() and got["finished"][3] == 1
    assert (got["ids"][:, 0] == SENT).all()                       # (the ids' other column is not the kernel's)
    if mode == "sampling":     # the draw follows the slot's own counter: another t gives another Philox step for the same logits
        assert 0 <= got["ids"][0, 1] < HI
    again = _Slots().run(lg, **kw)
    for k in got:
        assert np.array_equal(got[k], again[k]), k                # identical calls, identical bits


@pytest.mark.parametrize("mode", ["greedy", "sampling"])
def test_row_map_places_logits_rows_into_slots(logits32, mode):
    kw = {} if mode == "greedy" else SAMPLING
    lg = _logits(logits32, torch.bfloat16)
    base = _Slots().run(lg, **kw)
    perm = np.array([4, 2, 5, 0, 3, 1])                          # logits row i belongs to slot perm[i]
    shuffled = torch.empty_like(lg)
    shuffled[torch.arange(M, device=DEV)] = lg[_tdev(perm)]
    got = _Slots().run(shuffled, row_map=_tdev(perm.astype(np.int32)), **kw)
    for k in base:
        assert np.array_equal(base[k], got[k]), k
    # a subset of the slots (an admission): the other slots are not touched at all
    sub = np.array([4, 1], np.int32)
    s = _Slots()
    got = s.run(lg[_tdev(sub.astype(np.int64))].contiguous(), row_map=_tdev(sub), **kw)
    for r in range(M):
        if r in sub:
            assert got["ids"][r, 1] == base["ids"][r, 1] and got["t"][r] == T0[r] + 1 and np.array_equal(got["out"][r], base["out"][r])
        else:
            assert got["ids"][r, 1] == SENT and got["t"][r] == T0[r] and (got["out"][r] == SENT).all() and got["finished"][r] == FIN[r]


def test_counter_at_the_limit_is_reported(logits32):
    lg = _logits(logits32, torch.float32)
    t = list(T0)
    t[1], t[0] = LIMIT[1], -1
    got = _Slots(t=t).run(lg)
    for r in (0, 1):
        assert got["status"][r] & 2 and got["finished"][r] == 1 and got["ids"][r, 1] == PAD
        assert (got["out"][r] == SENT).all() and got["t"][r] == t[r]
    assert got["status"][2] == 0 and got["t"][2] == T0[2] + 1


def test_bad_arguments_raise_before_a_launch(logits32):
    from bdm_db1_amd import ops
    lg = _logits(logits32, torch.float32)
    s = _Slots()
    with pytest.raises(ValueError):
        ops.select_tokens_slots(lg, s.t[:1], s.limit, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, V=V)       # ONE counter
    with pytest.raises(ValueError):
        ops.select_tokens_slots(lg, s.t, s.limit, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, V=V, row_map=s.t[:2])
    with pytest.raises(ValueError):
        ops.select_tokens_slots(lg, s.t, s.limit, s.finished, s.lengths, s.out, s.ids[:, 1], s.status, V=V, greedy=False, top_p=0.0)
    assert ops.select_tokens_slots_supported(V, LD, torch.bfloat16) and not ops.select_tokens_slots_supported(40000, 40000, torch.bfloat16)
    from bdm_db1_amd import lib
    assert lib.load().db1_select_tokens_slots_workspace_bytes(64, V, 1) == 0
