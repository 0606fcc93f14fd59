"""The two kernels of the prefill straight into the K/V ring.
db1_relattn_mem_kv_fwd (attention over a K/V memory plus the call's own K/V): bit for bit db1_relattn_mem_fwd over the concatenation at every
case of tests/mem_attn_cases.py with a memory -- the seam falls at 1, 31, 32, 33, 40, 64, 96, 127, 128, 129 and 300 relative to the 32-key
steps --, the two halves in separate buffers with other strides and a NaN guard row on each side of the seam; NaN-filled guarded outputs;
two launches; the memory broadcast over the batch and over the positions; float64 for one case; the refusals.
db1_ring_prefill_rows: ring bytes and status against tests/ring_prefill_rule.py and against the chain it replaces (torch.cat ->
ops.kv8_quantize -> ops.ring_load_rows), on bf16 and fp8 rings pre-filled with a byte pattern."""
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

import ring_prefill_rule as RP  # noqa: E402
from gpu_common import DEV, Guarded, _need_gpu  # noqa: E402,F401
from mem_attn_cases import MEM_CASES  # noqa: E402

D = 128
KV_CASES = [c for c in MEM_CASES if c[1] >= 1]
BF = torch.bfloat16


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen, device="cpu").to(BF).to(DEV)


def _halves(gen, B, H, q, mlen, mem_b=None, mem_rows=None):
    """(memory view [mem_b, mem_rows, 2, H, D] inside a buffer whose row after the last is NaN; the call's qkv [B, q, 3, H, D] inside a buffer
    whose row before the first is NaN; the concatenation [B, mlen + q, 2, H, D] with the memory expanded)"""
    mem_b, mem_rows = B if mem_b is None else mem_b, mlen if mem_rows is None else mem_rows
    mbuf = torch.full((mem_b, mem_rows + 1, 2, H, D), float("nan"), device=DEV, dtype=BF)
    mbuf[:, :mem_rows] = _rand(gen, mem_b, mem_rows, 2, H, D)
    nbuf = torch.full((B, q + 1, 3, H, D), float("nan"), device=DEV, dtype=BF)
    nbuf[:, 1:] = _rand(gen, B, q, 3, H, D)
    mem, new = mbuf[:, :mem_rows], nbuf[:, 1:]
    cat = torch.cat([mem.expand(B, mlen, 2, H, D), new[:, :, 1:3]], 1).contiguous()
    return mem, new, cat


def _run_pair(B, H, q, mlen, shift, nd, mem_b=None, mem_rows=None, seed=0):
    """-> (out, lse) of relattn_mem_fwd over the concatenation, [(out, lse)] of two relattn_mem_kv_fwd launches on the halves, the inputs"""
    from bdm_db1_amd import ops
    gen = torch.Generator().manual_seed(1000 * q + mlen + seed)
    klen = mlen + q
    ndr = klen if nd is None else nd
    mem, new, cat = _halves(gen, B, H, q, mlen, mem_b, mem_rows)
    qu, qv, R = _rand(gen, B, q, H, D), _rand(gen, B, q, H, D), _rand(gen, ndr, H * D)
    scale = 1.0 / math.sqrt(D)
    ref_out = torch.full((B, q, H, D), float("nan"), device=DEV, dtype=BF)
    ref_lse = torch.full((B, H, q), float("nan"), device=DEV, dtype=torch.float32)
    ops.relattn_mem_fwd(qu, qv, cat[:, :, 0], cat[:, :, 1], R, ref_out, ref_lse, B, q, klen, mlen, H, D, shift, scale)
    assert ops.relattn_mem_kv_supported(B, q, mlen, H, D, shift, BF)
    runs = []
    for _ in range(2):
        out, lse = Guarded(B * q, H * D, "bf16"), Guarded(B * H, q, "f32")
        out.t.fill_(float("nan"))
        lse.t.fill_(float("nan"))
        ops.relattn_mem_kv_fwd(qu, qv, new[:, :, 1], new[:, :, 2], mem[:, :, 0], mem[:, :, 1], R, out.t.view(B, q, H, D), lse.t.view(B, H, q),
                               B, q, mlen, H, D, shift, scale)
        torch.cuda.synchronize()
        out.intact("out")
        lse.intact("lse")
        runs.append((out.t.view(B, q, H, D).clone(), lse.t.view(B, H, q).clone()))
    return (ref_out, ref_lse), runs, dict(qu=qu, qv=qv, R=R, cat=cat, scale=scale)


def _assert_bits(case, ref, runs):
    (ro, rl), (o0, l0), (o1, l1) = ref, runs[0], runs[1]
    assert bool(torch.isfinite(ro.float()).all()) and bool(torch.isfinite(rl).all()), (case, "the reference itself")
    assert bool(torch.isfinite(o0.float()).all()) and bool(torch.isfinite(l0).all()), (case, "a guard row reached the output")
    assert torch.equal(o0.view(torch.int16), ro.view(torch.int16)), (case, "out differs from relattn_mem_fwd over the concatenation")
    assert torch.equal(l0.view(torch.int32), rl.view(torch.int32)), (case, "lse differs from relattn_mem_fwd over the concatenation")
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), (case, "two launches")


@pytest.mark.parametrize("q,mlen,shift,nd", KV_CASES)
def test_kv_attention_is_bit_equal_to_the_concatenation(q, mlen, shift, nd):
    B, H = 2, 3
    ref, runs, _ = _run_pair(B, H, q, mlen, shift, nd)
    _assert_bits(("kv", q, mlen, shift, nd), ref, runs)


@pytest.mark.parametrize("q,mlen,shift,nd", [(80, 40, 120, None), (96, 300, 97, None), (130, 129, 0, None)])
def test_kv_attention_with_a_broadcast_memory(q, mlen, shift, nd):
    """mem_batch_stride = 0 (one memory for every sequence), then both memory strides 0 (one row), against the expanded concatenation"""
    B, H = 3, 2
    ref, runs, _ = _run_pair(B, H, q, mlen, shift, nd, mem_b=1, seed=1)
    _assert_bits(("batch stride 0", q, mlen, shift), ref, runs)
    ref, runs, x = _run_pair(B, H, q, mlen, shift, nd, mem_b=1, mem_rows=1, seed=2)
    _assert_bits(("both strides 0", q, mlen, shift), ref, runs)
    if (q, mlen) != (80, 40):
        return
    # per element against float64: the bounds of tests/test_mem_attn_kernels_gpu.py::test_mem_attention_random_data_other_strides
    f = lambda t: t.double().cpu().numpy()
    qu, qv, R, cat, klen = f(x["qu"]), f(x["qv"]), f(x["R"]).reshape(-1, H, D), f(x["cat"]), mlen + q
    i, j = np.arange(q)[:, None], np.arange(klen)[None, :]
    AC = np.einsum("bihd,bjhd->bhij", qu, cat[:, :, 0])
    T = np.einsum("bihd,rhd->bhir", qv, R)
    BD = np.take_along_axis(T, np.broadcast_to(np.clip(mlen + i - j, 0, R.shape[0] - 1)[None, None], AC.shape), axis=3)
    S = np.where(((j <= i + mlen) & (j > i - shift))[None, None], (AC + BD) * x["scale"], -np.inf)
    mx = S.max(-1, keepdims=True)
    Pm = np.exp(S - mx)
    ref_lse = mx[..., 0] + np.log(Pm.sum(-1))
    ref_out = np.einsum("bhij,bjhd->bihd", Pm / Pm.sum(-1, keepdims=True), cat[:, :, 1])
    err = np.abs(f(runs[0][0]) - ref_out).max() / np.abs(ref_out).max()
    lerr = np.abs(f(runs[0][1]) - ref_lse).max()
    print(f"kv attention, one memory row for all: out rel err {err:.3e}, lse abs err {lerr:.3e}")
    assert err < 2e-2 and lerr < 1e-3


def test_kv_attention_refusals_launch_nothing():
    from bdm_db1_amd import lib, ops
    B, H, q, mlen, shift = 2, 2, 70, 10, 80
    mk = lambda *s: torch.zeros(*s, device=DEV, dtype=BF)

    def attempt(Dn=D, mlen_=mlen, pad=0, off=0):
        qu, qv = mk(B, q, H, Dn), mk(B, q, H, Dn)
        rs = 3 * H * Dn + pad
        nbuf = mk(B * q * rs + 16)
        kn = nbuf.as_strided((B, q, H, Dn), (q * rs, rs, Dn, 1), H * Dn)
        vn = nbuf.as_strided((B, q, H, Dn), (q * rs, rs, Dn, 1), 2 * H * Dn)
        mbuf = mk(B * max(mlen_, 1) * 2 * H * Dn + 16)
        km = mbuf.as_strided((B, mlen_, H, Dn), (max(mlen_, 1) * 2 * H * Dn, 2 * H * Dn, Dn, 1), off)
        vm = mbuf.as_strided((B, mlen_, H, Dn), (max(mlen_, 1) * 2 * H * Dn, 2 * H * Dn, Dn, 1), off + H * Dn)
        R = mk(mlen_ + q, H * Dn)
        out = torch.full((B, q, H, Dn), float("nan"), device=DEV, dtype=BF)
        with pytest.raises((lib.Db1Error, ValueError)):
            ops.relattn_mem_kv_fwd(qu, qv, kn, vn, km, vm, R, out, None, B, q, mlen_, H, Dn, shift, 1.0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())

    attempt(mlen_=0)
    attempt(pad=4)                 # a row stride that is no multiple of 8 elements
    attempt(off=4)                 # a memory pointer 8 bytes past a 16-byte boundary
    attempt(Dn=64)
    assert not ops.relattn_mem_kv_supported(B, q, 0, H, D, shift, BF) and not ops.relattn_mem_kv_supported(B, q, mlen, H, 64, shift, BF)
    assert not ops.relattn_mem_kv_supported(B, 8193, mlen, H, D, shift, BF) and not ops.relattn_mem_kv_supported(B, q, mlen, H, D, shift, torch.float32)
    assert ops.relattn_mem_kv_supported(B, q, mlen, H, D, shift, BF)
    assert int(lib.load().db1_relattn_mem_kv_workspace_bytes(B, q, mlen, H)) == 0


# ------------------------------------------------------------------------------------------------------------------ db1_ring_prefill_rows
MLEN, CAP, M, H2 = 96, 160, 5, 2


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


def _kernel_b_once(fp8, q, origin, bcast, rows, src, gen):
    """one launch against the rule (bit for bit, ring and status) and, for the entries in range, against cat -> (kv8_quantize) -> ring_load_rows"""
    from bdm_db1_amd import ops
    n_src = 2
    qkv = _rand(gen, n_src, q, 3, H2, D)
    mem = _rand(gen, 1, 1, 2, H2, D) if bcast else _rand(gen, n_src, MLEN, 2, H2, D)
    if fp8:
        qkv, mem = qkv * 8.0, mem * 0.25          # (other scales for the call's rows and the memory's)
    ring = _new_ring(fp8)
    before = ring.clone()
    state = torch.tensor([origin], dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)
    ops.ring_prefill_rows(ring, qkv[:, :, 1], qkv[:, :, 2], mem[:, :, 0], mem[:, :, 1], state, MLEN, i32(rows), i32(src), status)
    torch.cuda.synchronize()
    assert int(state.cpu()) == origin
    conv = (lambda t: t.float().cpu().numpy()) if fp8 else _bits
    want, st = RP.prefill_rows(_bits(before), conv(mem), conv(qkv[:, :, 1:3]), MLEN, origin, rows, src, fp8=fp8)
    case = (fp8, q, origin, bcast, rows, src)
    assert int(status.cpu()) == st, case
    got = _bits(ring)
    assert np.array_equal(got, want), (case, "ring bytes differ from the rule", np.argwhere(got != want)[:3])
    # every byte outside the target slots of the target rows keeps the pattern (the 64 slots the window does not cover among them)
    ok = [(i, r) for i, r in enumerate(rows) if 0 <= r < M and 0 <= origin < CAP and (src is None or 0 <= src[i] < n_src)]
    keep = np.ones((M, CAP), bool)
    for _, r in ok:
        keep[r, (origin + np.arange(MLEN)) % CAP] = False
    assert keep.sum() == M * CAP - len(ok) * MLEN and np.array_equal(got[keep], _bits(before)[keep]), case
    # the chain this launch replaces
    if ok:
        memx = mem.expand(n_src, MLEN, 2, H2, D)
        srcs = torch.stack([torch.cat([memx[i if src is None else src[i]], qkv[i if src is None else src[i], :, 1:3]], 0)[-MLEN:] for i, _ in ok]).contiguous()
        ring2 = before.clone()
        if fp8:
            slots = torch.empty(len(ok), MLEN, ring.shape[2], device=DEV, dtype=torch.uint8)
            ops.kv8_quantize(srcs, slots)
            srcs = slots
        st2 = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.ring_load_rows([ring2], ops.ring_pointers([ring2]), [srcs], state, MLEN, i32([r for _, r in ok]), st2)
        torch.cuda.synchronize()
        assert int(st2.cpu()) == 0 and torch.equal(ring2, ring), (case, "ring bytes differ from cat -> quantize -> ring_load_rows")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("q", [1, 40, 96, 130])
def test_ring_prefill_rows_against_the_rule_and_the_chain(q, fp8):
    gen = torch.Generator().manual_seed(96160 + q)
    for origin in (0, 100):                                   # (100 + 96 > 160: the window wraps)
        for bcast in (True, False):
            _kernel_b_once(fp8, q, origin, bcast, [3, 1, 4, 0], [0, 0, 1, 1], gen)
            _kernel_b_once(fp8, q, origin, bcast, [3, 1], None, gen)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_ring_prefill_rows_skips_what_is_out_of_range(fp8):
    gen = torch.Generator().manual_seed(7)
    _kernel_b_once(fp8, 40, 100, False, [3, M, 4, 0], [0, 0, 2, 1], gen)       # row 5 of 5: bit 0; source 2 of 2: bit 2
    _kernel_b_once(fp8, 40, 100, True, [-1, 2], [1, -1], gen)                  # nothing in range: nothing written
    _kernel_b_once(fp8, 40, CAP, False, [3, 1], None, gen)                     # the origin outside [0, cap): bit 1, nothing written


def test_ring_prefill_rows_refusals_launch_nothing():
    from bdm_db1_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(3)
    qkv, mem = _rand(gen, 2, 40, 3, H2, D), _rand(gen, 2, MLEN, 2, H2, D)
    state, status = i32(0), i32(0)
    ring = _new_ring(False)
    before = ring.clone()
    k, v, km, vm = qkv[:, :, 1], qkv[:, :, 2], mem[:, :, 0], mem[:, :, 1]
    good = dict(ring=ring, k_new=k, v_new=v, k_mem=km, v_mem=vm, state=state, mlen=MLEN, rows=i32(3, 1), src=None, status=status)
    odd = torch.zeros(M, CAP, 264 * 3, device=DEV, dtype=torch.uint8)
    q3 = _rand(gen, 2, 40, 3, 3, D)
    m64 = _rand(gen, 2, 40, 3, H2, 64)
    for bad in (dict(mlen=CAP), dict(mlen=0), dict(rows=torch.tensor([3, 1], device=DEV)), dict(rows=i32(0, 1, 2, 3, 4, 0)), dict(rows=i32(0, 1, 2)),
                dict(src=i32(0)), dict(ring=ring[:, :, :1]), dict(ring=ring.float()), dict(k_new=k.float()), dict(v_new=qkv[:, :, 2, :, :64]),
                dict(ring=odd, k_new=q3[:, :, 1], v_new=q3[:, :, 2], k_mem=q3[:1, :1, 1], v_mem=q3[:1, :1, 2]),     # an odd H on an fp8 ring
                dict(ring=torch.zeros(M, CAP, 2, H2, 64, device=DEV, dtype=BF), k_new=m64[:, :, 1], v_new=m64[:, :, 2], k_mem=m64[:1, :1, 1],
                     v_mem=m64[:1, :1, 2]),                                                                         # D != 128
                dict(k_mem=mem[:, :50, 0], v_mem=mem[:, :50, 1]), dict(state=state.long())):
        with pytest.raises(ValueError):
            ops.ring_prefill_rows(**dict(good, **bad))
    torch.cuda.synchronize()
    assert torch.equal(ring, before) and int(status.cpu()) == 0
