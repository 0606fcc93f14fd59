"""The fp8 K/V ring kernels (include/db1_hip.h, "fp8 K/V ring"): db1_relattn_decode_ring_kv8_fwd on the attention probes over rings with
crafted scales (tests/test_kv8_rule_cpu.py proves that a wrong scale exceeds the tolerance ten times) and, on random data, bit for bit against
db1_relattn_decode_ring_fwd over the dequantised ring; db1_kv8_quantize and the appended slots byte for byte against tests/kv8_rule.py; the
ring copies on fp8 slots; the refusals."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probe as A  # noqa: E402
import kv8_rule as K8  # noqa: E402

DEV = "cuda"
B, H, D = A.B, A.H, A.D
SLOT = K8.slot_bytes(H)
GUARD = 4096
BAD_ALIGN = -2          # DB1_ERR_BAD_ALIGN (include/db1_hip.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)


def guarded(slots):
    """a device copy of the slot image [B, cap, SLOT] with GUARD bytes of 0xA5 behind it -> (the ring view, the whole buffer)"""
    buf = torch.full((slots.size + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    buf[:slots.size] = torch.from_numpy(np.ascontiguousarray(slots).reshape(-1)).to(DEV)
    return buf[:slots.size].view(slots.shape), buf


@functools.lru_cache(maxsize=None)
def probe(q, mlen, shift, nd):
    p, _ = A.build(q, mlen, shift, nd)
    ref = A.reference(p)
    tol = A.tolerances(ref, A.reference(p, rounded=True))
    for x in list(p.values()) + list(ref.values()):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return p, ref, tol


def run_forms(fwd, qkv_new, U, VB, ring_of, state_of, Rd, q, mlen, shift, scale, forms):
    """{form: (out, part or None, ring after, buffer after)} -- every output buffer starts as NaN"""
    from bdm_db1_amd import ops
    klen, d = mlen + q, H * D
    eye = torch.eye(d, device=DEV, dtype=torch.bfloat16)
    res = {}
    for form in forms:
        ring, buf = ring_of()
        state = state_of()
        out = torch.full((B, q, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
        part = None
        if form == "partials":
            part = torch.full((ops.relattn_decode_ring_part_numel(B, q, klen, H),), float("nan"), device=DEV, dtype=torch.float32)
            fwd(qkv_new, U, VB, ring, state, Rd, None, B, q, mlen, H, D, shift, scale, part=part)
            ops.linear_decode_attn(part, klen, B, q, H, D, eye, out.view(B * q, d))
        else:
            fwd(qkv_new, U, VB, ring, state, Rd, out, B, q, mlen, H, D, shift, scale, fused_merge=form == "in-launch")
        torch.cuda.synchronize()
        assert int(ops.decode_tickets(qkv_new.device).abs().sum().item()) == 0, form
        res[form] = (out, part, ring, buf, state)
    return res


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_kv8_ring_probe(q, mlen, shift, nd):
    """the three forms at every ring capacity and origin of the case, over a ring packed on the host under crafted scales (exact for the
    probe's values, so the bf16 kernel's tolerances hold): the output per element against the float64 closed form, the ring after the call
    byte for byte -- the new rows packed by the canonical rule, every other byte as it was -- the guard bytes, the origin, the tickets"""
    from bdm_db1_amd import ops
    p, ref, tol = probe(q, mlen, shift, nd)
    klen, ndr, d = mlen + q, p["R"].shape[0], H * D
    qkv_new = dev16(np.stack([p["q"], p["k"][:, mlen:], p["v"][:, mlen:]], axis=2))      # [B, q, 3, H, D]
    U, VB, Rd = dev16(p["u"]), dev16(p["vb"]), dev16(p["R"]).view(ndr, d)
    assert ops.relattn_decode_ring_kv8_supported(B, q, klen, H, D)
    forms = ["in-launch", "separate"] + (["partials"] if ops.linear_decode_attn_supported(B, q, H, D, klen, d) else [])
    new_slots = K8.pack(np.stack([p["k"][:, mlen:], p["v"][:, mlen:]], axis=2))           # [B, q, SLOT], canonical scales
    for cap in A.ring_caps(q, mlen):
        scales = K8.crafted_scales(cap)
        for start in A.ring_origins(q, mlen, cap):
            ring0 = A.ring_initial(p, cap, start)
            slots0 = ops.kv8_pack(torch.from_numpy(ring0), scales=torch.from_numpy(scales)).numpy()
            assert np.array_equal(slots0, K8.pack(ring0, scales))
            want = slots0.copy()
            want[:, A.ring_rows(start, mlen, q, cap, append=True)] = new_slots
            img = A.ring_expected(p, ring0, start)                                         # (the same rows, as values)
            assert np.array_equal(K8.dequantize(*K8.unpack(want, H)), img)
            res = run_forms(ops.relattn_decode_ring_kv8_fwd, qkv_new, U, VB, lambda: guarded(slots0),
                            lambda: torch.tensor([start], dtype=torch.int32, device=DEV), Rd, q, mlen, shift, p["scale"], forms)
            for form, (out, _, ring, buf, state) in res.items():
                case = ("kv8 ring", q, mlen, shift, nd, cap, start, form)
                got = out.to(torch.float64).cpu().numpy()
                err = np.abs(got - ref["out"])
                print(f"kv8_probe {case}: max|got - ref| = {err.max():.3e}, tol = {tol['out']:.3e}")
                assert np.isfinite(got).all(), case
                assert err.max() <= tol["out"], (case, float(err.max()), tol["out"], np.unravel_index(err.argmax(), err.shape))
                assert np.array_equal(ring.cpu().numpy(), want), (case, "ring image")
                assert bool((buf[want.size:] == 0xA5).all()), (case, "guard")
                assert int(state.item()) == start, case


def _random_case(rng, q, mlen, cap, start):
    """random keys / values whose magnitude varies per (row, position, K or V, head) over many binades; the ring holds them quantised"""
    mag = lambda *s: np.exp2(rng.integers(-9, 5, s + (1,)).astype(np.float64))
    ring_kv = A.bf16(rng.standard_normal((B, cap, 2, H, D)) * mag(B, cap, 2, H))
    ring_kv[0, (start + 3) % cap, 1, 1] = 0.0                                             # a zero block in the memory
    new_kv = A.bf16(rng.standard_normal((B, q, 2, H, D)) * mag(B, q, 2, H))
    if q > 2:
        new_kv[1, 2, 0, 0] = 0.0                                                          # ... and among the appended ones
    new_q = A.bf16(rng.standard_normal((B, q, 1, H, D)) * 0.5)
    qkv_new = dev16(np.concatenate([new_q, new_kv], axis=2))
    nd = mlen + q
    U, VB, Rd = dev16(rng.standard_normal((H, D)) * 0.25), dev16(rng.standard_normal((H, D)) * 0.25), dev16(rng.standard_normal((nd, H * D)) * 0.5)
    return K8.pack(ring_kv), new_kv, qkv_new, U, VB, Rd


@pytest.mark.parametrize("q,mlen,cap,start,shift", [(1, 300, 364, 100, 301), (2, 127, 129, 128, 129), (17, 129, 160, 150, 32), (64, 200, 267, 5, 264),
                                                    (16, 96, 112, 111, 112)])
def test_kv8_ring_is_the_bf16_kernel_over_the_dequantised_ring(q, mlen, cap, start, shift):
    """out and the partials bit for bit against ops.relattn_decode_ring_fwd over the kv8_unpack'ed ring; the appended slots byte for byte
    against the rule; a second launch gives the same bits"""
    from bdm_db1_amd import ops
    rng = np.random.default_rng([q, mlen, cap, start])
    slots0, new_kv, qkv_new, U, VB, Rd = _random_case(rng, q, mlen, cap, start)
    klen, d, scale = mlen + q, H * D, 1.0 / np.sqrt(D)
    deq = ops.kv8_unpack(torch.from_numpy(slots0), H)[0]                                  # bf16 [B, cap, 2, H, D]
    forms = ["in-launch", "separate"] + (["partials"] if ops.linear_decode_attn_supported(B, q, H, D, klen, d) else [])
    state_of = lambda: torch.tensor([start], dtype=torch.int32, device=DEV)
    got = run_forms(ops.relattn_decode_ring_kv8_fwd, qkv_new, U, VB, lambda: guarded(slots0), state_of, Rd, q, mlen, shift, scale, forms)
    again = run_forms(ops.relattn_decode_ring_kv8_fwd, qkv_new, U, VB, lambda: guarded(slots0), state_of, Rd, q, mlen, shift, scale, forms)
    ref = run_forms(ops.relattn_decode_ring_fwd, qkv_new, U, VB, lambda: (deq.to(DEV), None), state_of, Rd, q, mlen, shift, scale, forms)
    want = slots0.copy()
    want[:, A.ring_rows(start, mlen, q, cap, append=True)] = K8.pack(new_kv)
    for form in forms:
        out, part, ring, buf, _ = got[form]
        case = ("kv8 random", q, mlen, cap, start, form)
        assert bool(torch.isfinite(out.float()).all()), case
        assert torch.equal(out.view(torch.int16), ref[form][0].view(torch.int16)), (case, "out")
        assert torch.equal(out.view(torch.int16), again[form][0].view(torch.int16)), (case, "second launch")
        if part is not None:
            assert torch.equal(part.view(torch.int32), ref[form][1].view(torch.int32)), (case, "partials")
            assert torch.equal(part.view(torch.int32), again[form][1].view(torch.int32)), (case, "partials, second launch")
        assert np.array_equal(ring.cpu().numpy(), want), (case, "ring image")
        assert torch.equal(ring, again[form][2]) and bool((buf[want.size:] == 0xA5).all()), case
        # the bf16 kernel appended the same rows unquantised: the fp8 ring holds their quantisation
        rows = A.ring_rows(start, mlen, q, cap, append=True)
        assert np.array_equal(ref[form][2][:, rows].float().cpu().numpy(), new_kv.astype(np.float32)), case


def test_kv8_quantize_is_the_rule():
    """db1_kv8_quantize byte for byte: many binades, a zero block, -0, subnormals, the largest values, non-finite elements; into a strided
    destination (rows 2 .. 6 of a 9-row ring) whose other bytes stay"""
    from bdm_db1_amd import ops
    rng = np.random.default_rng(11)
    n, mlen, Hn, cap, first = 3, 5, 4, 9, 2
    x = A.bf16(rng.standard_normal((n, mlen, 2, Hn, D)) * np.exp2(rng.integers(-30, 30, (n, mlen, 2, Hn, 1)).astype(np.float64)))
    x[0, 1, 0, 2] = 0.0
    x[0, 1, 1, 2] = 0.0
    x[0, 1, 1, 2, 7] = -0.0
    x[1, 0, 0, 0] = A.bf16(rng.standard_normal(D) * 2.0 ** -130)                           # subnormal bf16: the scale stays 2^-126
    x[1, 0, 1, 0] = A.bf16(rng.standard_normal(D) * 2.0 ** -124)
    x[2, 4, 0, 3] = A.bf16(rng.standard_normal(D) * 2.0 ** 124)                            # near the top of the format
    x[2, 2, 1, 1, [3, 50, 127]] = [np.inf, -np.inf, np.nan]
    x[1, 3, 0, 1] = A.bf16(rng.standard_normal(D) * 2.0)
    x[1, 3, 0, 1, 0] = 446.0 * 2.0 ** -3                                                   # amax / s = 446, the last bf16 below 448
    x[1, 3, 1, 1] = A.bf16(rng.standard_normal(D) * 2.0)
    x[1, 3, 1, 1, 5] = -450.0 * 2.0 ** -3                                                  # ... and the first above it: the scale doubles
    x[0, 0, 0, 0] = A.bf16(rng.standard_normal(D) * 2.0)
    x[0, 0, 0, 0, 9] = 448.0 * 2.0 ** -3                                                   # ... and 448 itself
    src = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(np.nan_to_num(src.to(torch.float64).numpy(), nan=3.0), np.nan_to_num(x, nan=3.0))
    slot = K8.slot_bytes(Hn)
    buf = torch.full((n, cap, slot), 0xCD, dtype=torch.uint8, device=DEV)
    assert ops.kv8_slot_bytes(Hn, D) == slot
    ops.kv8_quantize(src.to(DEV), buf[:, first:first + mlen])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = np.full((n, cap, slot), 0xCD, np.uint8)
    want[:, first:first + mlen] = K8.pack(x)
    gp, gs = K8.unpack(got[:, first:first + mlen], Hn)
    wp, ws = K8.unpack(want[:, first:first + mlen], Hn)
    assert np.array_equal(gs, ws), "scales"
    assert np.array_equal(gp, wp), np.argwhere(gp != wp)[:8]
    assert np.array_equal(got, want)
    # a contiguous destination too
    flat = torch.full((n, mlen, slot), 0xCD, dtype=torch.uint8, device=DEV)
    ops.kv8_quantize(src.to(DEV), flat)
    assert np.array_equal(flat.cpu().numpy(), K8.pack(x))
    with pytest.raises(ValueError):
        ops.kv8_quantize(src.to(DEV), flat[:, :, :-8])
    with pytest.raises(ValueError):
        ops.kv8_quantize(src.to(DEV)[:, :, :, :3].contiguous(), flat)


def test_ring_copies_move_fp8_slots_as_bytes():
    """ops.ring_reorder and ops.ring_load_rows on uint8 [M, cap, 264 H] rings against a NumPy gather"""
    from bdm_db1_amd import ops
    rng = np.random.default_rng(3)
    L, M, W, cap, mlen, s0, t = 2, 4, 2, 84, 20, 75, 12
    rings_np = [rng.integers(0, 256, (M, cap, SLOT), dtype=np.uint8) for _ in range(L)]
    rings = [torch.from_numpy(r).to(DEV) for r in rings_np]
    parent = [1, 1, 2, 2]
    ops.ring_reorder(rings, ops.ring_pointers(rings), torch.tensor([s0], dtype=torch.int32, device=DEV), mlen,
                     torch.tensor([t], dtype=torch.int32, device=DEV), 12, torch.tensor(parent, dtype=torch.int32, device=DEV), W=W)
    torch.cuda.synchronize()
    slots = (s0 + mlen - t + np.arange(t)) % cap
    for r_np, r in zip(rings_np, rings):
        want = r_np.copy()
        for b in range(M):
            want[b, slots] = r_np[parent[b], slots]
        assert np.array_equal(r.cpu().numpy(), want)
    # load_rows: two new requests into rows [3, 0], relative to the origin 75 (the window wraps)
    rings_np = [r.cpu().numpy() for r in rings]
    src_np = [rng.integers(0, 256, (2, mlen, SLOT), dtype=np.uint8) for _ in range(L)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.ring_load_rows(rings, ops.ring_pointers(rings), [torch.from_numpy(s).to(DEV) for s in src_np], torch.tensor([s0], dtype=torch.int32, device=DEV),
                       mlen, torch.tensor([3, 0], dtype=torch.int32, device=DEV), status)
    torch.cuda.synchronize()
    slots = (s0 + np.arange(mlen)) % cap
    for r_np, s_np, r in zip(rings_np, src_np, rings):
        want = r_np.copy()
        want[3, slots], want[0, slots] = s_np[0], s_np[1]
        assert np.array_equal(r.cpu().numpy(), want)
    assert int(status.item()) == 0


def test_kv8_refusals():
    """DB1_ERR_UNSUPPORTED (another d_head, an odd number of heads, klen > 2048), DB1_ERR_BAD_SHAPE (cap < klen, a NULL operand),
    DB1_ERR_BAD_ALIGN -- all before a launch"""
    from bdm_db1_amd import lib, ops
    Lb = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    q, mlen, cap = 2, 30, 40
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    part = torch.zeros(ops.relattn_decode_ring_part_numel(B, 64, 2048, H), dtype=torch.float32, device=DEV)
    state = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(qkv=buf, u=buf, vb=buf, ring=buf, st=state, cap=cap, R=buf, out=buf, q=q, mlen=mlen, Hn=H, Dn=D):
        ptr = lambda x: null if x is None else (x if isinstance(x, ctypes.c_void_p) else P(x))
        return Lb.db1_relattn_decode_ring_kv8_fwd(ptr(qkv), ptr(u), ptr(vb), ptr(ring), ptr(st), cap, ptr(R), 64, ptr(out), B, q, mlen, Hn, Dn, 64,
                                                  0.1, P(part), part.numel() * 4, null, null)

    assert Lb.db1_relattn_decode_ring_kv8_supported(B, q, mlen + q, H, D) == 1
    for kw in (dict(Dn=64), dict(Hn=3), dict(mlen=2047, cap=4096), dict(q=65, cap=128), dict(q=0)):
        assert call(**kw) == ops.DB1_ERR_UNSUPPORTED, kw
        assert Lb.db1_relattn_decode_ring_kv8_supported(B, kw.get("q", q), kw.get("mlen", mlen) + kw.get("q", q), kw.get("Hn", H), kw.get("Dn", D)) == 0
    for kw in (dict(cap=mlen + q - 1), dict(ring=None), dict(qkv=None), dict(u=None), dict(vb=None), dict(R=None), dict(st=None)):
        assert call(**kw) == ops.DB1_ERR_BAD_SHAPE, kw
    off = ctypes.c_void_p(buf.data_ptr() + 8)
    for kw in (dict(ring=off), dict(qkv=off), dict(R=off), dict(out=off), dict(u=off), dict(vb=off)):
        assert call(**kw) == BAD_ALIGN, kw
    assert Lb.db1_kv8_slot_bytes(16, 128) == 4224 and Lb.db1_kv8_slot_bytes(2, 128) == SLOT and Lb.db1_kv8_slot_bytes(3, 128) == 0
    # db1_kv8_quantize
    qz = lambda src=P(buf), dst=P(buf), n=2, ml=4, Hn=H, Dn=D, stride=4 * SLOT: Lb.db1_kv8_quantize(src, dst, n, ml, Hn, Dn, stride, null)
    assert Lb.db1_kv8_quantize_supported(H, D) == 1 and Lb.db1_kv8_quantize_supported(3, D) == 0 and Lb.db1_kv8_quantize_supported(H, 64) == 0
    assert qz(Hn=3) == ops.DB1_ERR_UNSUPPORTED and qz(Dn=64) == ops.DB1_ERR_UNSUPPORTED
    assert qz(src=null) == ops.DB1_ERR_BAD_SHAPE and qz(dst=null) == ops.DB1_ERR_BAD_SHAPE and qz(stride=3 * SLOT) == ops.DB1_ERR_BAD_SHAPE
    assert qz(src=off) == BAD_ALIGN and qz(dst=off) == BAD_ALIGN and qz(stride=4 * SLOT + 8) == BAD_ALIGN
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                            # nothing was launched
    with pytest.raises(ValueError):                                                       # the wrapper: a ring of another shape
        ops.relattn_decode_ring_kv8_fwd(buf, buf, buf, buf.view(B, -1, 2, H, D // 2)[:, :cap], state, buf.view(-1, H * D)[:64], None, B, q, mlen, H, D, 64, 0.1)
