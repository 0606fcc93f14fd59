"""The two kernels of the prefix cache.
db1_relattn_mem_ring_fwd (attention over a memory that lives in the slots of a K/V ring, plus the call's own K/V): bit for bit
db1_relattn_mem_kv_fwd over the unpacked, linearised memory at every case of tests/mem_attn_cases.py with a memory, on a 3-row base ring, bf16
(H = 3) and fp8 (H = 4), at origin 0, an origin that wraps, one that is no multiple of 32 and cap = mlen + 1, with base_rows [1, 1] and [2, 0];
unused rows and slots hold NaN (fp8: the byte 0x7f); NaN-filled guarded outputs; two launches; the guard's status bit; the refusals.
db1_ring_fork_rows: ring bytes and status against tests/ring_fork_rule.py at mlen = 96, q in {1, 40, 96, 130}, both formats, both src maps,
rings pre-filled with a byte pattern, the base ring unchanged; every status bit; the refusals, overlapping buffers among them."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ring_fork_rule as RF  # noqa: E402
from gpu_common import DEV, Guarded, _need_gpu  # noqa: E402,F401
from mem_attn_cases import MEM_CASES  # noqa: E402

D = 128
KV_CASES = [c for c in MEM_CASES if c[1] >= 1]
BF = torch.bfloat16
M_BASE = 3


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen, device="cpu").to(BF).to(DEV)


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _slots(kv):
    """bf16 keys / values [..., 2, H, D] on the device -> their fp8 slots uint8 [..., 264 H] (ops.kv8_quantize)"""
    from bdm_db1_amd import ops
    H = kv.shape[-2]
    flat = kv.reshape(1, -1, 2, H, D).contiguous()
    out = torch.empty(1, flat.shape[1], ops.kv8_slot_bytes(H, D), device=DEV, dtype=torch.uint8)
    ops.kv8_quantize(flat, out)
    return out.view(*kv.shape[:-3], out.shape[-1])


def _base_ring(gen, fp8, H, mlen, cap, origin, used):
    """a 3-row base ring whose rows ``used`` hold a memory of mlen slots from ``origin`` (wrapping at cap) and NaN everywhere else
    -> (the ring, {row: the memory's values bf16 [mlen, 2, H, D]})"""
    from bdm_db1_amd import ops
    if fp8:
        ring = torch.full((M_BASE, cap, ops.kv8_slot_bytes(H, D)), 0x7F, device=DEV, dtype=torch.uint8)
    else:
        ring = torch.full((M_BASE, cap, 2, H, D), float("nan"), device=DEV, dtype=BF)
    idx = ((origin + torch.arange(mlen)) % cap).to(DEV)
    lin = {}
    for r in used:
        kv = _rand(gen, mlen, 2, H, D)
        if fp8:
            sl = _slots(kv * 4.0)
            ring[r, idx] = sl
            kv = ops.kv8_unpack(sl, H)[0].to(DEV)        # the slots' value: payload * scale, exact in bf16
            assert bool(torch.isfinite(kv.float()).all())
        else:
            ring[r, idx] = kv
        lin[r] = kv
    return ring, lin


def _attn_once(fp8, q, mlen, shift, nd, cap, origin, base_rows, seed=0, state_value=None, rows_value=None):
    """one configuration: relattn_mem_kv_fwd over the linear memory against two relattn_mem_ring_fwd launches -> the status word.
    ``state_value`` / ``rows_value``: what the device vectors hold instead (the guard), the ring being built for origin / base_rows."""
    from bdm_db1_amd import ops
    B, H = 2, (4 if fp8 else 3)
    gen = torch.Generator().manual_seed(1000 * q + mlen + 7 * origin + seed)
    klen = mlen + q
    ndr = klen if nd is None else nd
    ring, lin = _base_ring(gen, fp8, H, mlen, cap, origin, sorted(set(base_rows)))
    mem = torch.stack([lin[r] for r in base_rows]).contiguous()
    nbuf = torch.full((B, q + 1, 3, H, D), float("nan"), device=DEV, dtype=BF)
    nbuf[:, 1:] = _rand(gen, B, q, 3, H, D)
    new = nbuf[:, 1:]
    qu, qv, R = _rand(gen, B, q, H, D), _rand(gen, B, q, H, D), _rand(gen, ndr, H * D)
    scale = 1.0 / math.sqrt(D)
    ref_out = torch.full((B, q, H, D), float("nan"), device=DEV, dtype=BF)
    ref_lse = torch.full((B, H, q), float("nan"), device=DEV, dtype=torch.float32)
    ops.relattn_mem_kv_fwd(qu, qv, new[:, :, 1], new[:, :, 2], mem[:, :, 0], mem[:, :, 1], R, ref_out, ref_lse, B, q, mlen, H, D, shift, scale)
    assert ops.relattn_mem_ring_supported(B, q, mlen, cap, fp8, H, D, shift, BF)
    state = _i32([origin if state_value is None else state_value])
    rows = _i32(list(base_rows) if rows_value is None else rows_value)
    status = _i32([0])
    before = ring.clone()
    runs = []
    for _ in range(2):
        out, lse = Guarded(B * q, H * D, "bf16"), Guarded(B * H, q, "f32")
        out.t.fill_(float("nan"))
        lse.t.fill_(float("nan"))
        ops.relattn_mem_ring_fwd(qu, qv, new[:, :, 1], new[:, :, 2], ring, state, rows, status, R, out.t.view(B, q, H, D), lse.t.view(B, H, q),
                                 B, q, mlen, H, D, shift, scale)
        torch.cuda.synchronize()
        out.intact("out")
        lse.intact("lse")
        runs.append((out.t.view(B, q, H, D).clone(), lse.t.view(B, H, q).clone()))
    case = (fp8, q, mlen, shift, nd, cap, origin, base_rows)
    (o0, l0), (o1, l1) = runs
    assert bool(torch.isfinite(ref_out.float()).all()) and bool(torch.isfinite(ref_lse).all()), (case, "the reference itself")
    assert bool(torch.isfinite(o0.float()).all()) and bool(torch.isfinite(l0).all()), (case, "an unused slot or a guard row reached the output")
    assert torch.equal(o0.view(torch.int16), ref_out.view(torch.int16)), (case, "out differs from relattn_mem_kv_fwd over the linear memory")
    assert torch.equal(l0.view(torch.int32), ref_lse.view(torch.int32)), (case, "lse differs from relattn_mem_kv_fwd over the linear memory")
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), (case, "two launches")
    assert torch.equal(ring.view(torch.uint8), before.view(torch.uint8)), (case, "the base ring was written")
    return int(status.cpu())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("q,mlen,shift,nd", KV_CASES)
def test_ring_attention_is_bit_equal_to_the_linear_memory(q, mlen, shift, nd, fp8):
    cap = mlen + 37
    # origin 0; an origin whose window wraps; an origin that is no multiple of 32 (with mlen >= 5 the second is none either)
    for origin, base_rows in ((0, [1, 1]), (cap - min(mlen, 5), [2, 0]), (45 % cap, [2, 0])):
        assert _attn_once(fp8, q, mlen, shift, nd, cap, origin, base_rows) == 0


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_ring_attention_with_one_spare_slot(fp8):
    """cap = mlen + 1: the smallest ring that is supported, at an origin in its middle"""
    q, mlen, shift, nd = 100, 129, 32, None
    assert _attn_once(fp8, q, mlen, shift, nd, mlen + 1, 77, [1, 1]) == 0
    assert _attn_once(fp8, q, mlen, shift, nd, mlen + 1, mlen, [2, 0]) == 0


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_ring_attention_guard_clamps_and_sets_bit_3(fp8):
    """a base row outside [0, M_base) is read as row 0, an origin outside [0, cap) as 0: the output is the rule's for the clamped values"""
    q, mlen, shift, nd = 80, 40, 120, None
    assert _attn_once(fp8, q, mlen, shift, nd, 77, 30, [1, 0], rows_value=[1, M_BASE]) == 8
    assert _attn_once(fp8, q, mlen, shift, nd, 77, 30, [0, 2], rows_value=[-1, 2]) == 8
    assert _attn_once(fp8, q, mlen, shift, nd, 77, 0, [2, 1], state_value=77) == 8
    assert _attn_once(fp8, q, mlen, shift, nd, 77, 0, [2, 1], state_value=-3) == 8


def test_ring_attention_without_base_rows_is_the_identity():
    from bdm_db1_amd import ops
    gen = torch.Generator().manual_seed(5)
    B, H, q, mlen, cap, shift = 2, 3, 70, 33, 50, 0
    ring, lin = _base_ring(gen, False, H, mlen, cap, 40, [0, 1])
    mem = torch.stack([lin[0], lin[1]])
    new, qu, qv, R = _rand(gen, B, q, 3, H, D), _rand(gen, B, q, H, D), _rand(gen, B, q, H, D), _rand(gen, mlen + q, H * D)
    outs = [torch.full((B, q, H, D), float("nan"), device=DEV, dtype=BF) for _ in range(2)]
    status = _i32([0])
    ops.relattn_mem_kv_fwd(qu, qv, new[:, :, 1], new[:, :, 2], mem[:, :, 0], mem[:, :, 1], R, outs[0], None, B, q, mlen, H, D, shift, 0.1)
    ops.relattn_mem_ring_fwd(qu, qv, new[:, :, 1], new[:, :, 2], ring, _i32([40]), None, status, R, outs[1], None, B, q, mlen, H, D, shift, 0.1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0].float()).all()) and torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and int(status.cpu()) == 0


def test_ring_attention_refusals_launch_nothing():
    from bdm_db1_amd import lib, ops
    B, H, q, mlen, cap, shift = 2, 2, 70, 10, 20, 80
    mk = lambda *s: torch.zeros(*s, device=DEV, dtype=BF)
    qkv, qu, qv, R = mk(B, q, 3, H, D), mk(B, q, H, D), mk(B, q, H, D), mk(mlen + q, H * D)
    ring = mk(M_BASE, cap, 2, H, D)
    good = dict(qu=qu, qv=qv, k_new=qkv[:, :, 1], v_new=qkv[:, :, 2], base=ring, state_base=_i32([0]), base_rows=_i32([0, 1]), status=_i32([0]), R=R,
                lse=None, B=B, q=q, mlen=mlen, H=H, D=D, shift=shift, scale=1.0)
    odd8 = torch.zeros(M_BASE, cap, 264 * 3, device=DEV, dtype=torch.uint8)
    q3 = mk(B, q, 3, 3, D)
    for bad in (dict(mlen=cap), dict(mlen=0), dict(base=ring[:, :, :1]), dict(base=ring.float()), dict(base=ring[:, :, :, :, :64]),
                dict(base_rows=_i32([0])), dict(base_rows=torch.tensor([0, 1], device=DEV)), dict(state_base=_i32([0]).long()), dict(status=_i32([0, 0])),
                dict(B=M_BASE + 1, base_rows=None), dict(k_new=qkv[:, :, 1].float()), dict(v_new=qkv[:, :, 2, :, :64]),
                dict(base=odd8, H=3, qu=mk(B, q, 3, D), qv=mk(B, q, 3, D), k_new=q3[:, :, 1], v_new=q3[:, :, 2], R=mk(mlen + q, 3 * D))):
        out = torch.full((B, q, bad.get("H", H), D), float("nan"), device=DEV, dtype=BF)
        with pytest.raises((lib.Db1Error, ValueError)):
            ops.relattn_mem_ring_fwd(out=out, **dict(good, **bad))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), bad.keys()
    assert int(good["status"].cpu()) == 0
    sup = ops.relattn_mem_ring_supported
    assert sup(B, q, mlen, cap, False, H, D, shift, BF) and sup(B, q, mlen, cap, True, H, D, shift, BF) and sup(B, q, mlen, mlen + 1, False, 3, D, shift, BF)
    assert not sup(B, q, mlen, mlen, False, H, D, shift, BF) and not sup(B, q, 0, cap, False, H, D, shift, BF)
    assert not sup(B, q, mlen, cap, True, 3, D, shift, BF) and not sup(B, q, mlen, cap, False, H, 64, shift, BF)
    assert not sup(B, 8193, mlen, cap, False, H, D, shift, BF) and not sup(B, q, mlen, cap, False, H, D, shift, torch.float32)
    assert int(lib.load().db1_relattn_mem_ring_workspace_bytes(B, q, mlen, H)) == 0


# ------------------------------------------------------------------------------------------------------------------ db1_ring_fork_rows
MLEN, CAP, M, H2, CAP_BASE = 96, 160, 5, 2, 130


def _bits(t):
    """a bf16 tensor as uint16 bit patterns, a uint8 tensor as it is (NumPy)"""
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == BF else t.cpu().numpy()


def _new_ring(fp8):
    from bdm_db1_amd import ops
    if fp8:
        return torch.full((M, CAP, ops.kv8_slot_bytes(H2, D)), 0x5A, device=DEV, dtype=torch.uint8)
    ring = torch.empty(M, CAP, 2, H2, D, device=DEV, dtype=BF)
    ring.view(torch.int16).fill_(0x5A5A)
    return ring


def _fork_once(fp8, q, origin, origin_base, rows, src, base_rows, gen):
    """one launch against the rule, bit for bit: the destination ring, the status word, the untouched bytes and the base ring"""
    from bdm_db1_amd import ops
    n_src = 2
    qkv = _rand(gen, n_src, q, 3, H2, D)
    basekv = _rand(gen, M_BASE, CAP_BASE, 2, H2, D)
    if fp8:
        qkv = qkv * 8.0                                     # (other scales for the call's rows and the memory's)
        base = _slots(basekv * 0.25)
    else:
        base = basekv
    ring = _new_ring(fp8)
    before, base_before = ring.clone(), base.clone()
    state, state_base, status = _i32([origin]), _i32([origin_base]), _i32([0])
    ops.ring_fork_rows(ring, base, state_base, _i32(base_rows), qkv[:, :, 1], qkv[:, :, 2], state, MLEN, _i32(rows), _i32(src), status)
    torch.cuda.synchronize()
    assert int(state.cpu()) == origin and int(state_base.cpu()) == origin_base
    conv = (lambda t: t.float().cpu().numpy()) if fp8 else _bits
    want, st = RF.fork_rows(_bits(before), _bits(base_before), conv(qkv[:, :, 1:3]), MLEN, origin, origin_base, rows, src, base_rows, fp8=fp8)
    case = (fp8, q, origin, origin_base, rows, src, base_rows)
    assert int(status.cpu()) == st, case
    got = _bits(ring)
    assert np.array_equal(got, want), (case, "ring bytes differ from the rule", np.argwhere(got != want)[:3])
    assert torch.equal(base, base_before), (case, "the base ring was written")
    ok = [r for i, r in enumerate(rows) if 0 <= r < M and 0 <= origin < CAP and 0 <= origin_base < CAP_BASE and
          0 <= (i if src is None else src[i]) < n_src and
          0 <= ((i if src is None else src[i]) if base_rows is None else base_rows[i if src is None else src[i]]) < M_BASE]
    keep = np.ones((M, CAP), bool)
    for r in ok:
        keep[r, (origin + np.arange(MLEN)) % CAP] = False
    assert keep.sum() == M * CAP - len(ok) * MLEN and np.array_equal(got[keep], _bits(before)[keep]), case
    if fp8 and q < MLEN and ok:     # a forked memory slot is the base slot, byte for byte: nothing was requantised
        i = next(i for i, r in enumerate(rows) if r == ok[0])
        s = i if src is None else src[i]
        r = s if base_rows is None else base_rows[s]
        assert np.array_equal(got[ok[0], (origin + np.arange(MLEN - q)) % CAP], _bits(base)[r, (origin_base + q + np.arange(MLEN - q)) % CAP_BASE]), case
    return st


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("q", [1, 40, 96, 130])
def test_ring_fork_rows_against_the_rule(q, fp8):
    gen = torch.Generator().manual_seed(96130 + q)
    for origin, origin_base in ((0, 0), (100, 100), (100, 7)):        # (100 + 96 > 160, 100 + 96 > 130: both windows wrap)
        assert _fork_once(fp8, q, origin, origin_base, [3, 1, 4, 0], [0, 0, 1, 1], [2, 0], gen) == 0
        assert _fork_once(fp8, q, origin, origin_base, [3, 1], None, [1, 1], gen) == 0
    assert _fork_once(fp8, q, 100, 100, [0, 2], None, None, gen) == 0


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_ring_fork_rows_skips_what_is_out_of_range(fp8):
    gen = torch.Generator().manual_seed(7)
    assert _fork_once(fp8, 40, 100, 100, [3, M, 4, 0], [0, 0, 2, 1], [2, 0], gen) == 5       # row 5 of 5: bit 0; source 2 of 2: bit 2
    assert _fork_once(fp8, 40, CAP, 100, [3, 1], None, [2, 0], gen) == 2                      # the origin outside [0, cap): nothing written
    assert _fork_once(fp8, 40, 100, 100, [3, 1], None, [M_BASE, 0], gen) == 8                 # a base row outside [0, M_base): that one skipped
    assert _fork_once(fp8, 40, 100, CAP_BASE, [3, 1], None, [2, 0], gen) == 8                 # the base origin outside [0, cap_base)
    assert _fork_once(fp8, 40, -1, -1, [-1, 2], [1, -1], [-1, 0], gen) == 15


def test_ring_fork_rows_refusals_launch_nothing():
    from bdm_db1_amd import lib, ops
    gen = torch.Generator().manual_seed(3)
    qkv = _rand(gen, 2, 40, 3, H2, D)
    state, status = _i32([0]), _i32([0])
    ring = _new_ring(False)
    before = ring.clone()
    base = _rand(gen, M_BASE, CAP_BASE, 2, H2, D)
    both = torch.zeros(M + M_BASE, CAP, 2, H2, D, device=DEV, dtype=BF)
    k, v = qkv[:, :, 1], qkv[:, :, 2]
    good = dict(ring=ring, base=base, state_base=_i32([0]), base_rows=_i32([2, 0]), k_new=k, v_new=v, state=state, mlen=MLEN, rows=_i32([3, 1]), src=None,
                status=status)
    base8 = torch.zeros(M_BASE, CAP_BASE, 264 * H2, device=DEV, dtype=torch.uint8)
    for bad in (dict(ring=both[:M], base=both[M - 1:]), dict(ring=both[:M], base=both[:M]), dict(base=base[:, :MLEN].contiguous()), dict(mlen=CAP), dict(mlen=0),
                dict(base=base8), dict(base=base.float()), dict(base=base[:, :, :, :1]), dict(base_rows=_i32([0])), dict(base_rows=_i32([0, 1]).long()),
                dict(state_base=_i32([0, 0])), dict(rows=_i32([0, 1, 2, 3, 4, 0])), dict(rows=_i32([0, 1, 2])), dict(src=_i32([0])), dict(k_new=k.float()),
                dict(v_new=qkv[:, :, 2, :, :64]), dict(base_rows=None, k_new=_rand(gen, 4, 40, 3, H2, D)[:, :, 1], v_new=_rand(gen, 4, 40, 3, H2, D)[:, :, 2])):
        with pytest.raises(ValueError):
            ops.ring_fork_rows(**dict(good, **bad))
    # the entry point's own refusals: overlapping buffers, a NULL buffer, a misaligned one (DB1_ERR_BAD_SHAPE / BAD_SHAPE / BAD_ALIGN)
    P, st = ops.P, ops.stream()
    tail = lambda kn: (P(kn), P(v), k.stride(1), k.stride(0), P(state), P(good["rows"]), P(None), 2, 2, 40, MLEN, H2, D, P(status), st)
    for args in ((P(both), 0, M, CAP, P(both[M - 1:]), M_BASE, CAP, P(state), P(None)) + tail(k),
                 (P(ring), 0, M, CAP, P(None), M_BASE, CAP_BASE, P(state), P(None)) + tail(k),
                 (P(ring), 0, M, CAP, P(base), M_BASE, CAP_BASE, P(state), P(None)) + tail(k.reshape(-1)[4:])):
        with pytest.raises(lib.Db1Error):
            lib.call("db1_ring_fork_rows", *args)
    torch.cuda.synchronize()
    assert torch.equal(ring, before) and int(status.cpu()) == 0 and not bool(both.any())
    assert ops.ring_fork_rows_supported(False, 40, MLEN, MLEN + 1, CAP, H2, D) and not ops.ring_fork_rows_supported(False, 40, MLEN, MLEN, CAP, H2, D)
    assert not ops.ring_fork_rows_supported(True, 40, MLEN, CAP_BASE, CAP, 3, D) and not ops.ring_fork_rows_supported(False, 0, MLEN, CAP_BASE, CAP, H2, D)
