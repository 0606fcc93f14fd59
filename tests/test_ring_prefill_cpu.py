"""The ring-prefill rule (tests/ring_prefill_rule.py) against a second formulation -- concatenate, keep the last mlen rows, roll them to the
origin -- on q < mlen, q == mlen, q > mlen, a wrapping origin, a broadcast memory, repeated sources and out-of-range rows / sources; its fp8
form against the host-side ops.kv8_pack; RingPrefill's host refusals that need no device; the new prototypes.  No GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kv8_rule as K8  # noqa: E402
import ring_prefill_rule as RP  # noqa: E402

H, D = 2, 128
MLEN, CAP, M = 12, 20, 5
PATTERN = 0x5A5A


def _bf16_values(rng, *shape):
    """random bf16 values as float32 (the low 16 bits cleared)"""
    a = rng.standard_normal(shape).astype(np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _second_way(ring, mem_kv, new_kv, mlen, origin, rows, src, enc):
    """the same result from whole-array operations: cat, the last mlen rows, one roll"""
    out = np.array(ring, copy=True)
    M_, cap = ring.shape[:2]
    status = 0
    for i, row in enumerate(rows):
        s = i if src is None else src[i]
        if not 0 <= row < M_:
            status |= 1
        if not 0 <= origin < cap:
            status |= 2
        if not 0 <= s < new_kv.shape[0]:
            status |= 4
        if not (0 <= row < M_ and 0 <= origin < cap and 0 <= s < new_kv.shape[0]):
            continue
        mem = np.broadcast_to(mem_kv[min(s, mem_kv.shape[0] - 1)], (mlen,) + mem_kv.shape[2:])
        last = np.concatenate([mem, new_kv[s]], 0)[-mlen:]
        slots = (origin + np.arange(mlen)) % cap
        out[row, slots] = enc(last)
    return out, status


CASES = [
    # (q, origin, broadcast memory, rows, src)
    (5, 0, False, [3, 1], None),                      # q < mlen
    (MLEN, 0, False, [0, 4], None),                   # q == mlen: everything from the call
    (17, 3, False, [2, 0], None),                     # q > mlen
    (5, 15, False, [3, 1], None),                     # the origin wraps: slots 15 .. 19, 0 .. 6
    (1, 19, True, [4, 2], None),                      # one new row over the broadcast memory row, wrapping
    (7, 9, True, [0, 1, 2, 3], [0, 0, 1, 1]),         # repeated sources: the W-fold expansion
    (7, 9, False, [0, 9, 2, -1], [1, 0, 1, 0]),       # rows outside [0, M): skipped, status bit 0
    (7, 9, False, [0, 1, 2], [1, 2, -1]),             # sources outside [0, n_src): skipped, status bit 2
    (7, CAP, False, [0, 1], None),                    # an origin outside [0, cap): nothing written, status bit 1
]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("q,origin,bcast,rows,src", CASES)
def test_rule_against_the_second_formulation(q, origin, bcast, rows, src, fp8):
    rng = np.random.default_rng([q, origin, int(bcast), len(rows)])
    n_src = 2
    new_kv = _bf16_values(rng, n_src, q, 2, H, D)
    mem_kv = _bf16_values(rng, 1, 1, 2, H, D) if bcast else _bf16_values(rng, n_src, MLEN, 2, H, D)
    if fp8:
        ring = np.full((M, CAP, K8.slot_bytes(H)), 0x5A, np.uint8)
        enc = K8.pack
    else:
        ring = np.full((M, CAP, 2, H, D), np.float32(-7.5), np.float32)
        enc = lambda a: a
    got, st = RP.prefill_rows(ring, mem_kv, new_kv, MLEN, origin, rows, src, fp8=fp8)
    want, st2 = _second_way(ring, mem_kv, new_kv, MLEN, origin, rows, src, enc)
    assert st == st2 and np.array_equal(got, want)
    expect = (1 if any(not 0 <= r < M for r in rows) else 0) | (2 if origin >= CAP else 0) | \
             (4 if src is not None and any(not 0 <= s < n_src for s in src) else 0)
    assert st == expect
    # every slot outside the window of a written row, and every other row, keeps the pattern
    ok_rows = [r for i, r in enumerate(rows) if 0 <= r < M and origin < CAP and (src is None or 0 <= src[i] < n_src)]
    keep = np.ones((M, CAP), bool)
    for r in ok_rows:
        keep[r, (origin + np.arange(MLEN)) % CAP] = False
    assert np.array_equal(got[keep], ring[keep])
    assert not np.array_equal(got[~keep], ring[~keep]) or not ok_rows


def test_the_window_is_the_last_mlen_rows():
    """position j reads memory row j + q while that is a memory row, then the call's rows in order; the newest row lands on slot origin + mlen - 1"""
    q, origin = 5, 15
    mem = np.arange(MLEN, dtype=np.float32).reshape(1, MLEN, 1, 1, 1) * np.ones((1, 1, 2, H, D), np.float32)
    new = (100 + np.arange(q, dtype=np.float32)).reshape(1, q, 1, 1, 1) * np.ones((1, 1, 2, H, D), np.float32)
    got, st = RP.prefill_rows(np.full((1, CAP, 2, H, D), -1.0, np.float32), mem, new, MLEN, origin, [0])
    assert st == 0
    seq = [got[0, (origin + j) % CAP, 0, 0, 0] for j in range(MLEN)]
    assert seq == [float(v) for v in range(q, MLEN)] + [100.0 + v for v in range(q)]


def test_fp8_form_agrees_with_ops_kv8_pack():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd import ops
    rng = np.random.default_rng(88)
    q, origin, rows, src = 5, 15, [3, 1, 0], [1, 1, 0]
    new_kv = _bf16_values(rng, 2, q, 2, H, D) * np.float32(16.0)
    mem_kv = _bf16_values(rng, 2, MLEN, 2, H, D)
    new_kv[0, 1, 0, 1, 7] = np.inf                     # a non-finite element: the NaN byte, its block's scale unchanged
    mem_kv[1, 8, 1, 0] = 0.0                           # a block of zeros: scale 1
    ring = np.full((M, CAP, K8.slot_bytes(H)), 0x5A, np.uint8)
    got, st = RP.prefill_rows(ring, mem_kv, new_kv, MLEN, origin, rows, src, fp8=True)
    assert st == 0
    for i, r in enumerate(rows):
        last = np.concatenate([mem_kv[src[i]], new_kv[src[i]]], 0)[-MLEN:]
        slots = ops.kv8_pack(torch.from_numpy(last)).numpy()
        assert np.array_equal(got[r, (origin + np.arange(MLEN)) % CAP], slots)


def _fake_ring(B=4):
    torch = pytest.importorskip("torch")
    from bdm_db1_amd.decode import RingMemory
    ring = object.__new__(RingMemory)           # (no device: the attributes RingPrefill's host checks read)
    ring.B, ring.model, ring.state = B, SimpleNamespace(dev=torch.device("cpu")), torch.zeros(1, dtype=torch.int32)
    return torch, ring


def test_ring_prefill_host_refusals():
    torch, ring = _fake_ring(4)
    from bdm_db1_amd.decode import RingPrefill
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    ok = RingPrefill(ring, i32(3, 1))
    assert ok.n_dst == 2 and ok.src is None and ok.rows.tolist() == [3, 1] and ok.is_ring_prefill
    assert RingPrefill(ring).rows.tolist() == [0, 1, 2, 3]
    assert RingPrefill(ring, None, i32(0, 0, 1, 1)).n_dst == 4
    for bad in (dict(rows=torch.tensor([3, 1])), dict(rows=i32(3, 1).float()), dict(rows=[3, 1]), dict(rows=i32(3, 1).view(1, 2)),
                dict(rows=i32(0, 1, 2, 3, 3)), dict(src=torch.tensor([0, 0, 1, 1])), dict(src=i32(0, 0, 1)), dict(rows=i32(0, 1), src=i32(0, 0, 0)),
                dict(rows=i32(0, 1, 2, 3)[::2])):
        with pytest.raises(ValueError):
            RingPrefill(ring, **bad)
    with pytest.raises(ValueError):
        RingPrefill("not a ring")
    ok.check_batch(2)
    ok.check_batch(3)
    with pytest.raises(ValueError):
        ok.check_batch(1)                       # two destinations, one call row, no src map
    RingPrefill(ring, None, i32(0, 0, 0, 0)).check_batch(1)


def test_flag_defaults_and_exports():
    import inspect
    import bdm_db1_amd as pkg
    from bdm_db1_amd import decode, generation
    from bdm_db1_amd.model import transformer_xl as T
    assert "self.use_ring_prefill = False" in inspect.getsource(T.TransformerXL.__init__)
    assert isinstance(T.TransformerXL.ring_prefill_supported, property)
    assert decode.RingPrefill is generation.RingPrefill
    assert "RingPrefill" in pkg.__all__ and pkg.RingPrefill is decode.RingPrefill
    off = SimpleNamespace(use_ring_prefill=False, ring_prefill_supported=True)
    unsupported = SimpleNamespace(use_ring_prefill=True, ring_prefill_supported=False)
    on = SimpleNamespace(use_ring_prefill=True, ring_prefill_supported=True)
    assert [generation._use_ring_prefill(m) for m in (off, unsupported, on, SimpleNamespace())] == [False, False, True, False]


def test_prototypes_are_declared():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for n in ("db1_relattn_mem_kv_supported", "db1_relattn_mem_kv_workspace_bytes", "db1_relattn_mem_kv_fwd", "db1_ring_prefill_rows_supported",
              "db1_ring_prefill_rows"):
        assert n in names
    protos = lib.parse_header()
    # the two-place attention: db1_relattn_mem_fwd's arguments with (k, v, 2 strides) twice and no klen
    assert len(protos["db1_relattn_mem_kv_fwd"][1]) == len(protos["db1_relattn_mem_fwd"][1]) + 3
    assert len(protos["db1_ring_prefill_rows"][1]) == 23 and len(protos["db1_ring_prefill_rows_supported"][1]) == 6
