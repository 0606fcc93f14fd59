"""db1_ring_load_rows against a NumPy scatter, bit for bit, and RingMemory.load_rows against RingMemory.load after a list-form prefill."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_common import DEV, _bf16_model, _need_gpu, _tdev  # noqa: E402,F401

L, M, MLEN, CAP, H, D = 2, 4, 100, 164, 2, 128      # (the slot of the test model: 2 * H * D bf16 = 1024 bytes)


def _bits(rng, *shape):
    """random bit patterns as int16 (viewed as bf16 on the device: a pure copy must keep NaN payloads too)"""
    return rng.integers(-32768, 32768, shape, dtype=np.int16)


def _run(ring_bits, src_bits, rows, origin):
    from bdm_db1_amd import ops
    rings = [_tdev(r).view(torch.bfloat16) for r in ring_bits]
    src = [_tdev(s).view(torch.bfloat16) for s in src_bits]
    state = _tdev(np.array([origin], np.int32))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.ring_load_rows(rings, ops.ring_pointers(rings), src, state, MLEN, _tdev(np.asarray(rows, np.int32)), status)
    torch.cuda.synchronize()
    assert int(state[0]) == origin                       # the origin is only read
    return [r.view(torch.int16).cpu().numpy() for r in rings], int(status[0])


@pytest.mark.parametrize("origin", [0, 150])
def test_ring_load_rows_is_a_scatter(origin):
    rng = np.random.default_rng(origin + 1)
    rows = [2, 0]
    ring = [_bits(rng, M, CAP, 2, H, D) for _ in range(L)]
    src = [_bits(rng, len(rows), MLEN, 2, H, D) for _ in range(L)]
    got, status = _run(ring, src, rows, origin)
    slots = (origin + np.arange(MLEN)) % CAP
    outside = np.setdiff1d(np.arange(CAP), slots)
    assert outside.size == CAP - MLEN == 64
    for l in range(L):
        want = ring[l].copy()
        for i, r in enumerate(rows):
            want[r, slots] = src[l][i]
        assert np.array_equal(got[l], want)
        assert np.array_equal(got[l][[1, 3]], ring[l][[1, 3]])                               # the other rows
        assert np.array_equal(got[l][[0, 2]][:, outside], ring[l][[0, 2]][:, outside])       # outside the loaded rows' window
    assert status == 0


def test_no_rows_is_a_no_op_and_a_bad_row_is_skipped():
    rng = np.random.default_rng(5)
    ring = [_bits(rng, M, CAP, 2, H, D) for _ in range(L)]
    got, status = _run(ring, [_bits(rng, 0, MLEN, 2, H, D) for _ in range(L)], [], 7)
    assert status == 0 and all(np.array_equal(g, r) for g, r in zip(got, ring))
    for bad in (M, -1, 1 << 20):
        src = [_bits(rng, 2, MLEN, 2, H, D) for _ in range(L)]
        got, status = _run(ring, src, [bad, 3], 150)
        slots = (150 + np.arange(MLEN)) % CAP
        for l in range(L):
            want = ring[l].copy()
            want[3, slots] = src[l][1]
            assert np.array_equal(got[l], want)          # nothing written for the bad entry, the good one loaded
        assert status & 1


def test_unsupported_shapes_are_refused():
    from bdm_db1_amd import lib, ops
    Lb = lib.load()
    assert Lb.db1_ring_load_rows_supported(1024, 100, 164) and not Lb.db1_ring_load_rows_supported(1000, 100, 164)
    assert not Lb.db1_ring_load_rows_supported(1024, 164, 164) and not Lb.db1_ring_load_rows_supported(1024, 0, 164)
    null = lambda: __import__("ctypes").c_void_p(0)
    assert Lb.db1_ring_load_rows(null(), null(), 2, 4, 2, 164, 1000, null(), 100, null(), null(), null()) == ops.DB1_ERR_UNSUPPORTED
    assert Lb.db1_ring_load_rows(null(), null(), 2, 4, 2, 100, 1024, null(), 100, null(), null(), null()) == ops.DB1_ERR_UNSUPPORTED
    rings = [torch.zeros(M, CAP, 2, H, D, dtype=torch.bfloat16, device=DEV) for _ in range(L)]
    ptrs = ops.ring_pointers(rings)
    i1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows = torch.zeros(2, dtype=torch.int32, device=DEV)
    src = [torch.zeros(2, MLEN, 2, H, D, dtype=torch.bfloat16, device=DEV) for _ in range(L)]
    with pytest.raises(ValueError):
        ops.ring_load_rows(rings, ptrs, src, i1, CAP, rows, i1)                      # mlen >= cap (and the sources' shape)
    with pytest.raises(ValueError):
        ops.ring_load_rows(rings, ptrs, src[:1], i1, MLEN, rows, i1)
    with pytest.raises(ValueError):
        ops.ring_load_rows(rings, ptrs, src, i1, MLEN, rows[:1], i1)
    with pytest.raises(ValueError):
        ops.ring_load_rows(rings, ptrs, [s[:, :, :1] for s in src], i1, MLEN, rows, i1)


def test_ring_memory_load_rows_continues_a_prefill():
    """RingMemory.load_rows into rows [2, 0] of a ring that has already advanced, after a 70-token list-form prefill, then one token call:
    the next-token logits against the same call over RingMemory.load (the bound of test_ring_memory_load_continues_a_prefill)"""
    from bdm_db1_amd import RingMemory
    from bdm_db1_amd.data import NLPTaskInput
    cfg, model = _bf16_model(mem_len=MLEN)
    rng = np.random.default_rng(3)
    n = 2
    ids = rng.integers(0, 32000, (n, 70))
    nxt = rng.integers(0, 32000, (n, 1))
    mk = lambda a: NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(a), text_len=None)
    with torch.no_grad():
        model._dec_state = None
        _, _, mems = model([mk(ids)], compute_loss=False, mems=model.init_mem(n))
        loaded = RingMemory(model, n)
        loaded.load(mems)
        want = model([mk(nxt)], compute_loss=False, mems=loaded)[0].float().cpu().numpy()
        ring = RingMemory(model, M)
        for _ in range(3):          # the ring has moved on: its origin is not 0 and rows 1, 3 hold other requests
            model([mk(rng.integers(0, 32000, (M, 50)))], compute_loss=False, mems=ring)
        origin = int(ring.state[0])
        assert origin == 150
        rows = [2, 0]
        ring.load_rows(mems, _tdev(np.asarray(rows, np.int32)))
        assert int(ring.state[0]) == origin and int(ring.load_status[0]) == 0
        tok = rng.integers(0, 32000, (M, 1))
        tok[rows] = nxt
        got = model([mk(tok)], compute_loss=False, mems=ring)[0].float().cpu().numpy()[rows]
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err < 1e-2, err
    with pytest.raises(ValueError):
        ring.load_rows(mems[:1], _tdev(np.asarray(rows, np.int32)))
    with pytest.raises(ValueError):
        ring.load_rows(mems, _tdev(np.asarray([1], np.int32)))


def test_load_and_load_rows_share_one_projection():
    """RingMemory.load against load_rows of all rows at origin 0, bit for bit; the model's decode state survives both, and a refused load"""
    from bdm_db1_amd import RingMemory
    from bdm_db1_amd.data import NLPTaskInput
    cfg, model = _bf16_model()
    B, mlen = 3, int(model.mem_len)
    ids = np.random.default_rng(11).integers(0, 32000, (B, 50))
    x = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(ids), text_len=None)
    with torch.no_grad():
        model._dec_state = None
        _, _, mems = model([x], compute_loss=False, mems=model.init_mem(B))
    a, b = RingMemory(model, B), RingMemory(model, B)
    state = model._dec_state = object()
    a.load(mems)
    assert model._dec_state is state
    b.load_rows(mems, torch.arange(B, dtype=torch.int32, device=DEV))
    assert model._dec_state is state
    assert int(a.state[0]) == int(b.state[0]) == 0 and int(a.load_status[0]) == int(b.load_status[0]) == 0
    assert len(a.kv) == len(b.kv) == 2
    for u, v in zip(a.kv, b.kv):
        assert torch.equal(u[:, :mlen].view(torch.int16), v[:, :mlen].view(torch.int16))
        assert bool(u[:, :mlen].any())
    with pytest.raises(ValueError):
        a.load([m[:, :-1] for m in mems])
    assert model._dec_state is state
    model._dec_state = None
