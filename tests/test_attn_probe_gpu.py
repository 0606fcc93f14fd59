"""The attention kernels against the float64 closed form on the index-revealing probes of tests/attn_probe.py: per element, under the tolerance
derived from the rounded model (tests/test_attn_probe_cpu.py proves that every one-off index or mask error exceeds it ten times).
Every buffer a kernel has to write -- outputs, lse, delta, gradients, kept probabilities, workspaces -- is pre-filled with NaN, and check() demands a
finite result: an element that was never written cannot land inside a tolerance by coincidence."""
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

DEV = "cuda"
B, H, D = A.B, A.H, A.D
SENTINEL = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)


def host(t):
    return t.detach().to(torch.float64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def probe(q, mlen, shift, nd, backward):
    """inputs, float64 reference and tolerances of one case: computed once, shared by the tests, never written to"""
    p, dout = A.build(q, mlen, shift, nd)
    d = dout if backward else None
    ref = A.reference(p, d)
    tol = A.tolerances(ref, A.reference(p, d, rounded=True))
    for x in list(p.values()) + [dout] + list(ref.values()):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return p, dout, ref, tol


def check(what, got, ref, tol, case):
    got = host(got) if hasattr(got, "detach") else np.asarray(got, np.float64)
    err = np.abs(got - ref)
    worst = float(err.max())
    print(f"attn_probe {case} {what}: max|got - ref| = {worst:.3e}, tol = {tol:.3e}, ratio = {worst / tol if tol > 0 else (0.0 if worst == 0 else float('inf')):.3f}")
    assert np.isfinite(got).all(), (case, what)
    assert worst <= tol, (case, what, worst, tol, np.unravel_index(err.argmax(), err.shape))


def flash_inputs(p, L):
    from bdm_db1_amd import ops
    qkv = dev16(np.stack([p["q"], p["k"], p["v"]], axis=2))                   # [B, L, 3, H, D]
    Rd, U, VB = dev16(p["R"]), dev16(p["u"]), dev16(p["vb"])
    qu, qv = torch.empty(B, L, H, D, device=DEV, dtype=torch.bfloat16), torch.empty(B, L, H, D, device=DEV, dtype=torch.bfloat16)
    ops.relattn_add_head_bias(qkv, U, VB, qu, qv, B, L, L, H, D)
    assert torch.equal(qu, dev16(p["q"] + p["u"])) and torch.equal(qv, dev16(p["q"] + p["vb"]))      # exact by construction
    return qkv, Rd, qu, qv


def flash_forward(p, L, shift, qkv, Rd, qu, qv, keep):
    from bdm_db1_amd import ops
    assert ops.relattn_flash_supported(B, L, H, D, torch.bfloat16)
    out = torch.full((B, L, H, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, L), SENTINEL, device=DEV, dtype=torch.float32)
    probs = mblk = None
    if keep:
        probs = torch.full((B * H, ops.relattn_flash_probs_tiles(L), 512), float("nan"), device=DEV, dtype=torch.bfloat16)
        mblk = torch.full((B * H, L // 32, L), float("nan"), device=DEV, dtype=torch.float32)
    ops.relattn_flash_fwd(qu, qv, qkv, Rd, out, lse, B, L, H, D, shift, p["scale"], probs=probs, mblk=mblk)
    torch.cuda.synchronize()
    return out, lse, probs, mblk


@pytest.mark.parametrize("L,shift", A.FLASH_FWD_CASES)
def test_flash_forward_probe(L, shift):
    from bdm_db1_amd import ops
    p, _, ref, tol = probe(L, 0, shift, None, False)
    qkv, Rd, qu, qv = flash_inputs(p, L)
    runs = [("plain", False, None), ("kept", True, None)]
    if shift >= L:
        runs += [(f"kept, loop {m}", True, m) for m in (0, 1, 2)]              # the compiled loop and the two hand-scheduled ones
    for name, keep, loop in runs:
        try:
            if loop is not None:
                ops.flash_fwd2(loop)
            out, lse, _, _ = flash_forward(p, L, shift, qkv, Rd, qu, qv, keep)
        finally:
            if loop is not None:
                ops.flash_fwd2(1)
        check("out", out, ref["out"], tol["out"], ("flash_fwd", L, shift, name))
        check("lse", lse, ref["lse"], tol["lse"], ("flash_fwd", L, shift, name))


@pytest.mark.parametrize("L,shift", A.FLASH_BWD_CASES)
@pytest.mark.parametrize("mode", A.FLASH_BWD_MODES)
def test_flash_backward_probe(L, shift, mode):
    from bdm_db1_amd import lib, ops
    p, dout, ref, tol = probe(L, 0, shift, None, True)
    qkv, Rd, qu, qv = flash_inputs(p, L)
    out, lse, probs, mblk = flash_forward(p, L, shift, qkv, Rd, qu, qv, mode == "fwd_probs")
    for kv3 in ((1, 0) if (mode == "fwd_probs" and L % 256 == 0) else (None,)):
        case = ("flash_bwd", L, shift, mode, kv3)
        dqkv = torch.full((B, L, 3, H, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
        dT = torch.zeros(H, B, L, L, device=DEV, dtype=torch.bfloat16)
        delta = torch.full((B, H, L), SENTINEL, device=DEV, dtype=torch.float32)
        if mode != "recompute":
            ops.reserve_workspace(int(lib.load().db1_relattn_flash_bwd_workspace_bytes(B, L, H, int(mode == "fwd_probs"))))
            for buf in ops._workspace.bufs.values():
                buf.fill_(0xFF)
        try:
            if kv3 is not None:
                lib.set_knob("flash_kv3", kv3)
            ops.relattn_flash_bwd(qu, qv, qkv, Rd, out, dev16(dout), lse, delta, dqkv, dT, B, L, H, D, shift, p["scale"], store_probs=mode != "recompute",
                                  probs=probs, mblk=mblk)
            torch.cuda.synchronize()
        finally:
            if kv3 is not None:
                lib.set_knob("flash_kv3", -1)
        g, dTn = host(dqkv), host(dT)
        check("dv", g[:, :, 2], ref["dv"], tol["dv"], case)
        check("dk", g[:, :, 1], ref["dk"], tol["dk"], case)
        dqr = np.einsum("nbir,rnd->bind", dTn, p["R"])
        check("dq", g[:, :, 0] + dqr, ref["dq"], tol["dq"], case)
        check("dR", np.einsum("nbir,bind->rnd", dTn, p["q"] + p["vb"]), ref["dR"], tol["dR"], case)
        check("du", g[:, :, 0].sum((0, 1)), ref["du"], tol["du"], case)
        check("dv_bias", dqr.sum((0, 1)), ref["dv_bias"], tol["dv_bias"], case)
        check("delta", delta, ref["delta"], tol["delta"], case)
        ii, dd = np.arange(L)[:, None], np.arange(L)[None, :]
        seen = (dd <= ii) & (dd < shift)                                       # the visible keys j = i - dist: the producer judged directly
        check("dT", dTn[:, :, seen], ref["dT"].transpose(1, 0, 2, 3)[:, :, seen], tol["dT"], case)


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_decode_probe(q, mlen, shift, nd):
    from bdm_db1_amd import ops
    p, _, ref, tol = probe(q, mlen, shift, nd, False)
    klen, ndr = mlen + q, p["R"].shape[0]
    kv = dev16(np.stack([p["k"], p["v"]], axis=2))                            # [B, klen, 2, H, D]
    out = torch.full((B, q, H, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    assert ops.relattn_decode_supported(B, q, klen, H, D, torch.bfloat16)
    ops.relattn_decode_fwd(dev16(p["q"] + p["u"]), dev16(p["q"] + p["vb"]), kv[:, :, 0], kv[:, :, 1], dev16(p["R"]).view(ndr, H * D), out,
                           B, q, klen, mlen, H, D, shift, p["scale"])
    torch.cuda.synchronize()
    check("out", out, ref["out"], tol["out"], ("decode", q, mlen, shift, nd))


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_decode_ring_probe(q, mlen, shift, nd):
    """the three forms of db1_relattn_decode_ring_fwd at every ring capacity and origin of the case: the output per element, the ring after the
    call bit-equal to the expected image (every untouched row included), the ticket counters zero"""
    from bdm_db1_amd import ops
    p, _, ref, tol = probe(q, mlen, shift, nd, False)
    klen, ndr, d = mlen + q, p["R"].shape[0], H * D
    qkv_new = dev16(np.stack([p["q"], p["k"][:, mlen:], p["v"][:, mlen:]], axis=2))      # [B, q, 3, H, D]
    U, VB, Rd = dev16(p["u"]), dev16(p["vb"]), dev16(p["R"]).view(ndr, d)
    eye = torch.eye(d, device=DEV, dtype=torch.bfloat16)
    assert ops.relattn_decode_supported(B, q, klen, H, D, torch.bfloat16) and klen <= 2048
    forms = ["in-launch", "separate"] + (["partials"] if ops.linear_decode_attn_supported(B, q, H, D, klen, d) else [])
    for cap in A.ring_caps(q, mlen):
        for start in A.ring_origins(q, mlen, cap):
            ring0 = A.ring_initial(p, cap, start)
            want = dev16(A.ring_expected(p, ring0, start))
            for form in forms:
                case = ("ring", q, mlen, shift, nd, cap, start, form)
                ring = dev16(ring0)
                state = torch.tensor([start], dtype=torch.int32, device=DEV)
                out = torch.full((B, q, H, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
                if form == "partials":
                    part = torch.full((ops.relattn_decode_ring_part_numel(B, q, klen, H),), float("nan"), device=DEV, dtype=torch.float32)
                    ops.relattn_decode_ring_fwd(qkv_new, U, VB, ring, state, Rd, None, B, q, mlen, H, D, shift, p["scale"], part=part)
                    ops.linear_decode_attn(part, klen, B, q, H, D, eye, out.view(B * q, d))
                else:
                    ops.relattn_decode_ring_fwd(qkv_new, U, VB, ring, state, Rd, out, B, q, mlen, H, D, shift, p["scale"], fused_merge=form == "in-launch")
                torch.cuda.synchronize()
                check("out", out, ref["out"], tol["out"], case)
                assert torch.equal(ring.view(torch.int16), want.view(torch.int16)), (case, "ring image")
                assert int(state.item()) == start, case
                assert int(ops.decode_tickets(qkv_new.device).abs().sum().item()) == 0, case


@pytest.mark.parametrize("start,q,cap", [(3, 5, 64), (59, 5, 64), (60, 5, 64), (0, 64, 64), (63, 1, 64), (6, 1, 7)])
def test_ring_advance_wraps(start, q, cap):
    """start + q below, equal to and above cap"""
    from bdm_db1_amd import ops
    state = torch.tensor([start], dtype=torch.int32, device=DEV)
    ops.ring_advance(state, q, cap)
    torch.cuda.synchronize()
    assert int(state.item()) == (start + q) % cap
