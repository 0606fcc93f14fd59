"""The tail of the attention backward on the GPU.

Part 1: the dq_r stream kernel (relattn_dqr.hip) in its four entry points against the float64 closed form of tests/dqr_rule.py on the two integer
probes -- every comparison BITWISE (bf16 as int16, the float32 sums as int32), every output pre-filled with NaN inside a guarded allocation,
the workspace filled with 0xFF bytes before each call (R^T and the partial table must be written before they are read) and every k-tile of
dT that the kernel has no business reading filled with NaN.  tests/test_dqr_rule_cpu.py proves that a misplaced term changes the bits.  A
failure names the first wrong element: its sequence, row (and 64-row item), head and column -- or the row of the partial table.

Part 2: the dT contract between its producers (relattn_flash_bwd; relattn_softmax_bwd of the fp32 parity path) and its consumers (the stream
kernel and the two tri-hinted batched GEMMs of TransformerXL._attention_bwd): what the producers write and leave, the reuse of one zeroed
buffer, and the chain from the kernels' own dT to dq, du, dv_bias and dR, per element against tests/attn_probe.py's closed form."""
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
import dqr_rule as Q  # noqa: E402
from gpu_common import Guarded, _need_gpu  # noqa: E402,F401

DEV = "cuda"
D = Q.D
NAN = float("nan")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def host(t):
    return t.detach().to(torch.float64).cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(what, got, want, case):
    """got == want bit for bit; a failure names the first wrong element (for a [B, L, H, D] tensor: sequence, row, head, column)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (case, what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    n = int(bad.sum())
    if n:
        idx = tuple(bad.nonzero()[0].tolist())
        where = f"64-row item {idx[1] // Q.ROWS} of sequence {idx[0]}, head {idx[2]}" if got.dim() == 4 else ""
        raise AssertionError(f"{case} {what}: {n} of {bad.numel()} elements differ in bits, the first at {idx} {where}: "
                             f"got {float(got[idx])}, want {float(want[idx])}")


def scrub(nbytes):
    """the workspace holds 0xFF bytes (NaN as bf16 and as float32) before the call"""
    from bdm_db1_amd import ops
    ops.reserve_workspace(int(nbytes))
    for buf in ops._workspace.bufs.values():
        buf.fill_(0xFF)


def ws_bytes(L, H, ng=1):
    from bdm_db1_amd import lib
    return int(lib.load().db1_relattn_dqr_groups_workspace_bytes(L, H, ng))


class Packed:
    """a guarded [B, L, 3, H, D] gradient like the model's dqkv, NaN everywhere but (fused mode) the q slot, which holds dq_k"""

    def __init__(self, B, L, H, dq_k=None):
        self.g = Guarded(B * L, 3 * H * D, "bf16")
        self.g.t.fill_(NAN)
        self.t = self.g.t.view(B, L, 3, H, D)
        self.q = self.t[:, :, 0]
        if dq_k is not None:
            self.q.copy_(dq_k)
        self.rest = self.t[:, :, 1:].clone()

    def check(self, what, want, case):
        same_bits(what, self.q, want, case)
        same_bits(what + ": the k and v slots", self.t[:, :, 1:], self.rest, case)
        self.g.intact(f"{case} {what}")


def acc0(H):
    return torch.full((H * D,), Q.ACC0[0], device=DEV), torch.full((H * D,), Q.ACC0[1], device=DEV)


def upload(kind, H, B, L, ng):
    pr = (Q.build_index if kind == "index" else Q.build_dense)(H, B, L, ng, poison=True)
    ref = Q.closed_form(pr)
    assert kind != "index" or Q.index_is_exact(ref)
    assert np.isnan(pr["dT"]).sum() == H * B * int(Q.poison_mask(L).sum())
    # R of group g inside a larger [ng, 3, L, H D] tensor (the model's batched r_net output): a strided [ng, L, H D] view; NaN around it
    Rall = torch.full((ng, 3, L, H * D), NAN, device=DEV, dtype=torch.bfloat16)
    Rall[:, 1] = dev16(pr["R"].reshape(ng, L, H * D))
    want = dict(dq_r=dev16(Q.bf16(ref["dq_r"])), dq=dev16(ref["dq"]), du=dev32(ref["du"]), dv=dev32(ref["dv"]))
    return pr, ref, dev16(pr["dT"]), Rall[:, 1], dev16(pr["dq_k"]), want


@pytest.mark.parametrize("kind", ["index", "dense"])
@pytest.mark.parametrize("H,B,L,ng", [c for c in Q.CASES if c[3] == 1])
def test_stream_kernel_probe(H, B, L, ng, kind):
    from bdm_db1_amd import ops
    case = ("dqr", H, B, L, kind)
    pr, ref, dT, Rg, dq_k, want = upload(kind, H, B, L, 1)
    R, nws = Rg[0], ws_bytes(L, H)
    assert ops.relattn_dqr_supported(B, L, H, D, torch.bfloat16)
    # ---- relattn_dqr into a contiguous output, and into the q slot of a packed gradient
    out = Guarded(B * L, H * D, "bf16")
    out.t.fill_(NAN)
    scrub(nws)
    ops.relattn_dqr(dT, R, out.t.view(B, L, H, D))
    same_bits("relattn_dqr", out.t.view(B, L, H, D), want["dq_r"], case)
    out.intact(f"{case} relattn_dqr")
    pk = Packed(B, L, H)
    scrub(nws)
    ops.relattn_dqr(dT, R, pk.q)
    pk.check("relattn_dqr into the q slot", want["dq_r"], case)
    # ---- relattn_dqr_fused, twice
    fused = []
    for rep in range(2):
        pk, (du, dv) = Packed(B, L, H, dq_k), acc0(H)
        scrub(nws)
        ops.relattn_dqr_fused(dT, R, pk.q, du, dv)
        pk.check(f"relattn_dqr_fused dq (launch {rep})", want["dq"], case)
        same_bits(f"relattn_dqr_fused du (launch {rep})", du, want["du"], case)
        same_bits(f"relattn_dqr_fused dv (launch {rep})", dv, want["dv"], case)
        fused.append(pk.q.clone())
    same_bits("relattn_dqr_fused, second launch against the first", fused[1], fused[0], case)
    # ---- relattn_dqr_fused_parts: the table per workgroup row, its sum, the idle rows
    rows = ops.relattn_dqr_parts_rows(H)
    assert rows == Q.wph(H)
    pk, parts = Packed(B, L, H, dq_k), Guarded(2 * rows, H * D, "f32")
    parts.t.fill_(NAN)
    scrub(nws)
    ops.relattn_dqr_fused_parts(dT, R, pk.q, parts.t.view(2, rows, H * D))
    pk.check("relattn_dqr_fused_parts dq", want["dq"], case)
    same_bits("relattn_dqr_fused_parts dq against relattn_dqr_fused", pk.q, fused[0], case)
    parts.intact(f"{case} parts")
    table = host(parts.t).reshape(2, rows, H * D)
    assert np.isfinite(table).all(), (case, "parts: rows never written", np.argwhere(~np.isfinite(table))[:4].tolist())
    tiles = [x.reshape(B, L // Q.ROWS, Q.ROWS, H * D).sum(2) for x in (pr["dq_k"], ref["dq_r"])]          # [B, NT, H D] per half
    exp = np.zeros_like(table)
    for j in range(rows):
        for b, i0 in Q.workgroup(j, H, B, L)[1]:
            exp[0, j] += tiles[0][b, i0 // Q.ROWS]
            exp[1, j] += tiles[1][b, i0 // Q.ROWS]
    for half, name in enumerate(("dq_k", "dq_r")):
        wrong = np.argwhere((table[half] != exp[half]).any(1)).ravel()
        assert wrong.size == 0, (case, f"parts[{name}]: the rows of workgroups {wrong[:8].tolist()} differ", [Q.workgroup(int(j), H, B, L)[1] for j in wrong[:2]])
    idle = [j for j in range(rows) if Q.idle(j, H, B, L)]
    assert (bits(parts.t.view(2, rows, H * D)[:, idle]) == 0).all(), (case, "idle rows are not +0")
    assert np.array_equal(table.sum(1), ref["sums"]), (case, "parts summed over rows")


@pytest.mark.parametrize("kind", ["index", "dense"])
@pytest.mark.parametrize("H,B,L,ng", [c for c in Q.CASES if c[3] > 1])
def test_stream_kernel_probe_with_groups(H, B, L, ng, kind):
    from bdm_db1_amd import ops
    case = ("dqr groups", H, B, L, ng, kind)
    pr, ref, dT, Rg, dq_k, want = upload(kind, H, B, L, ng)
    assert ops.relattn_dqr_groups_supported(B, L, H, D, torch.bfloat16, ng) and not Rg.is_contiguous()
    pk, (du, dv) = Packed(B, L, H, dq_k), acc0(H)
    scrub(ws_bytes(L, H, ng))
    ops.relattn_dqr_fused_groups(dT, Rg, pk.q, du, dv)
    pk.check("relattn_dqr_fused_groups dq", want["dq"], case)
    same_bits("relattn_dqr_fused_groups du", du, want["du"], case)
    same_bits("relattn_dqr_fused_groups dv", dv, want["dv"], case)
    # ng launches of the one-R form on the blocks: the same dq, and -- the integer sums are exact -- the same sums
    pk2, (du2, dv2) = Packed(B, L, H, dq_k), acc0(H)
    Bm = B // ng
    for g in range(ng):
        scrub(ws_bytes(L, H))
        ops.relattn_dqr_fused(dT[:, g * Bm:(g + 1) * Bm].contiguous(), Rg[g], pk2.q[g * Bm:(g + 1) * Bm], du2, dv2)
    pk2.check("one relattn_dqr_fused per group", want["dq"], case)
    same_bits("groups against one launch per group: dq", pk.q, pk2.q, case)
    same_bits("groups against one launch per group: du", du, du2, case)
    same_bits("groups against one launch per group: dv", dv, dv2, case)


def test_stream_kernel_replays_from_a_graph():
    from bdm_db1_amd import ops
    from bdm_db1_amd.decode import graph_capture
    H, B, L = 2, 2, 256
    case = ("dqr graph", H, B, L)
    pr, ref, dT, Rg, dq_k, want = upload("index", H, B, L, 1)
    R = Rg[0]
    pk, (du, dv) = Packed(B, L, H), acc0(H)

    def run():
        pk.q.copy_(dq_k)
        du.fill_(Q.ACC0[0])
        dv.fill_(Q.ACC0[1])
        ops.relattn_dqr_fused(dT, R, pk.q, du, dv)

    def forget():
        pk.q.fill_(NAN)
        du.fill_(NAN)
        dv.fill_(NAN)
        scrub(ws_bytes(L, H))
        torch.cuda.synchronize()

    scrub(ws_bytes(L, H))
    run()
    torch.cuda.synchronize()
    pk.check("eager", want["dq"], case)
    eager = (pk.q.clone(), du.clone(), dv.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):       # warm-up off the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):
        run()
    for rep in range(2):
        forget()
        graph.replay()
        torch.cuda.synchronize()
        pk.check(f"replay {rep}", want["dq"], case)
        for name, got, e in zip(("dq", "du", "dv"), (pk.q, du, dv), eager):
            same_bits(f"replay {rep} against eager: {name}", got, e, case)
    same_bits("du", du, want["du"], case)
    same_bits("dv", dv, want["dv"], case)


# ------------------------------------------------------------------------------------------------------------------ refusals
OK_SHAPE = dict(B=1, L=128, H=1, D=128)


def _refusal_buffers(B, L, H, Dh):
    """real buffers of the full size, so that an entry point that fails to refuse still stays inside its allocations"""
    n = max(H * Dh, 8)
    dT = torch.zeros(H * B * L * L + 8, device=DEV, dtype=torch.bfloat16)
    R = torch.zeros(L * n + 64, device=DEV, dtype=torch.bfloat16)
    out = torch.full((B * L * 3 * n + 64,), NAN, device=DEV, dtype=torch.bfloat16)
    acc = torch.full((2, max(H, 1) * max(Dh, 128)), NAN, device=DEV)
    parts = torch.full((2 * 256 * max(H, 1) * max(Dh, 128),), NAN, device=DEV)
    ws = torch.full((int(1.25 * ws_bytes(max(L, 128), H, 4)) + 4096,), 0xFF, device=DEV, dtype=torch.uint8)
    return dT, R, out, acc, parts, ws


REFUSALS = [
    # (name, entry, shape overrides, argument overrides, status)
    ("L = 64", "plain", dict(L=64), {}, -6), ("L = 192", "plain", dict(L=192), {}, -6), ("L = 1152", "plain", dict(L=1152), {}, -6),
    ("L = 192, fused", "fused", dict(L=192), {}, -6), ("L = 1152, parts", "parts", dict(L=1152), {}, -6), ("L = 64, groups", "groups", dict(L=64, B=2), dict(ng=2), -6),
    ("D = 64", "plain", dict(D=64), {}, -6), ("D = 64, fused", "fused", dict(D=64), {}, -6),
    ("H = 257", "plain", dict(H=257), {}, -6), ("H = 257, fused", "fused", dict(H=257), {}, -6),
    ("null du", "fused", {}, dict(du=None), -1), ("null dv", "fused", {}, dict(dv=None), -1), ("null du, groups", "groups", dict(B=2), dict(ng=2, du=None), -1),
    ("null parts", "parts", {}, dict(parts=None), -2),
    ("dq row stride 3 H D + 4", "fused", {}, dict(o_rs=3 * 128 + 4), -2), ("dq batch stride + 4", "parts", {}, dict(o_bs=128 * 3 * 128 + 4), -2),
    ("dq row stride + 4, groups", "groups", dict(B=2), dict(ng=2, o_rs=3 * 128 + 4), -2),
    ("out row stride H D + 2", "plain", {}, dict(o_rs=128 + 2), -2), ("out batch stride + 2", "plain", {}, dict(o_bs=128 * 128 + 2), -2),
    ("out base + 2 bytes", "plain", {}, dict(out_off=1), -2),
    ("R base + 2 bytes", "plain", {}, dict(r_off=1), -2), ("R base + 4 bytes, fused", "fused", {}, dict(r_off=2), -2),
    ("R row stride H D + 2", "plain", {}, dict(r_rs=128 + 2), -2), ("R group stride + 2", "groups", dict(B=2), dict(ng=2, r_gs=128 * 128 + 2), -2),
    ("workspace one byte short", "plain", {}, dict(ws_short=1), -4), ("workspace one byte short, fused", "fused", {}, dict(ws_short=1), -4),
    ("workspace one byte short, groups", "groups", dict(B=2), dict(ng=2, ws_short=1), -4), ("no workspace", "parts", {}, dict(ws_none=True), -4),
    ("ngroups = 3 divides neither B = 4 nor 128", "groups", dict(B=4, H=2), dict(ng=3), -6),
    ("ngroups = 0", "groups", dict(B=4, H=2), dict(ng=0), -6),
]


@pytest.mark.parametrize("name,entry,shape,args,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(name, entry, shape, args, status):
    from bdm_db1_amd import lib, ops
    s = dict(OK_SHAPE, **shape)
    B, L, H, Dh = s["B"], s["L"], s["H"], s["D"]
    dT, R, out, acc, parts, ws = _refusal_buffers(B, L, H, Dh)
    ng = args.get("ng", 1)
    r_rs, o_rs = args.get("r_rs", H * Dh), args.get("o_rs", 3 * H * Dh)
    o_bs, r_gs = args.get("o_bs", L * o_rs), args.get("r_gs", L * r_rs)
    need = int(lib.load().db1_relattn_dqr_groups_workspace_bytes(L, H, max(ng, 1)))
    wsp, wsn = (ops.P(None), 0) if args.get("ws_none") else (ops.P(ws), need - args.get("ws_short", 0))
    Rp, outp = ops.P(R[args.get("r_off", 0):]), ops.P(out[args.get("out_off", 0):])
    du = ops.P(None) if "du" in args else ops.P(acc[0])
    dv = ops.P(None) if "dv" in args else ops.P(acc[1])
    tail = (B, L, H, Dh, wsp, wsn, ops.stream())
    call = {"plain": ("db1_relattn_dqr", ops.P(dT), Rp, r_rs, outp, o_rs, o_bs) + tail,
            "fused": ("db1_relattn_dqr_fused", ops.P(dT), Rp, r_rs, outp, o_rs, o_bs, du, dv) + tail,
            "parts": ("db1_relattn_dqr_fused_parts", ops.P(dT), Rp, r_rs, outp, o_rs, o_bs, ops.P(None) if "parts" in args else ops.P(parts)) + tail,
            "groups": ("db1_relattn_dqr_fused_groups", ops.P(dT), Rp, r_rs, r_gs, ng, outp, o_rs, o_bs, du, dv) + tail}[entry]
    with pytest.raises(lib.Db1Error, match=rf"failed with status {status}:"):
        lib.call(*call)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(acc).all()) and bool(torch.isnan(parts).all()), name
    assert bool((ws == 0xFF).all()), (name, "the workspace was written")


def test_refusals_of_the_wrappers():
    """float32 operands (the entry points take no dtype: the wrappers refuse), a shape the support query rejects"""
    from bdm_db1_amd import lib, ops
    B, L, H = 1, 128, 1
    assert not ops.relattn_dqr_supported(B, L, H, D, torch.float32) and not ops.relattn_dqr_groups_supported(2, L, H, D, torch.float32, 2)
    assert not ops.relattn_dqr_groups_supported(4, 256, 2, D, torch.bfloat16, 3) and ops.relattn_dqr_groups_supported(4, 256, 2, D, torch.bfloat16, 2)
    for L_bad in (64, 192, 1152):
        assert not ops.relattn_dqr_supported(B, L_bad, H, D, torch.bfloat16)
    assert not ops.relattn_dqr_supported(B, L, 257, D, torch.bfloat16) and not ops.relattn_dqr_supported(B, L, H, 64, torch.bfloat16)
    dT, R = torch.zeros(H, B, L, L, device=DEV), torch.zeros(L, H * D, device=DEV)
    out = torch.full((B, L, H, D), NAN, device=DEV)
    du, dv = torch.full((H * D,), NAN, device=DEV), torch.full((H * D,), NAN, device=DEV)
    parts = torch.full((2, ops.relattn_dqr_parts_rows(H), H * D), NAN, device=DEV)
    scrub(ws_bytes(L, H, 1))
    for f in (lambda: ops.relattn_dqr(dT, R, out), lambda: ops.relattn_dqr_fused(dT, R, out, du, dv),
              lambda: ops.relattn_dqr_fused_parts(dT, R, out, parts), lambda: ops.relattn_dqr_fused_groups(dT, R[None], out, du, dv),
              lambda: ops.relattn_dqr(dT.bfloat16(), R, out), lambda: ops.relattn_dqr(dT.bfloat16(), R.bfloat16(), out)):
        with pytest.raises(lib.Db1Error, match="bf16"):
            f()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x).all()) for x in (out, du, dv, parts))
    assert all(bool((buf == 0xFF).all()) for buf in ops._workspace.bufs.values())


# ------------------------------------------------------------------------------------------------------------------ the dT contract
SENT = 7.0
BH = (A.B, A.H)


@functools.lru_cache(maxsize=None)
def probe(L, shift, seed=0):
    """inputs, float64 reference and tolerances of one training geometry (B = H = 2); tol["dq"] is the chain's (one more rounding: bf16(dq_k + dq_r))"""
    p, dout = A.build(L, 0, shift, None, seed)
    ref = A.reference(p, dout)
    tol = A.tolerances(ref, A.reference(p, dout, rounded=True))
    tol_chain = A.tolerances(ref, A.reference(p, dout, rounded=True, round_dq=True))
    for x in list(p.values()) + [dout] + list(ref.values()):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return p, dout, ref, tol, tol_chain


def visible_dist(L, shift):
    """[L, L] bool over (i, dist): the keys max(0, i - shift + 1) <= j <= i re-indexed by dist = i - j"""
    i, dist = np.arange(L)[:, None], np.arange(L)[None, :]
    return (dist <= i) & (dist < shift)


def check(what, got, ref, tol, case, ratios=None):
    got = host(got) if hasattr(got, "detach") else np.asarray(got, np.float64)
    err = np.abs(got - ref)
    worst = float(err.max())
    ratio = worst / tol if tol > 0 else (0.0 if worst == 0 else float("inf"))
    print(f"dT contract {case} {what}: max|got - ref| = {worst:.3e}, tol = {tol:.3e}, ratio = {ratio:.3f}")
    assert np.isfinite(got).all(), (case, what, "not finite at", np.argwhere(~np.isfinite(got))[:4].tolist())
    assert worst <= tol, (case, what, worst, tol, np.unravel_index(err.argmax(), err.shape))


def flash_backward(L, shift, mode, dT, seed=0):
    """relattn_flash_fwd + relattn_flash_bwd on the probe of (L, shift, seed) into the given dT buffer; returns dqkv [B, L, 3, H, D] and the inputs"""
    from bdm_db1_amd import lib, ops
    B, H = BH
    p, dout, _, _, _ = probe(L, shift, seed)
    qkv = dev16(np.stack([p["q"], p["k"], p["v"]], axis=2))
    Rd, U, VB = dev16(p["R"]), dev16(p["u"]), dev16(p["vb"])
    qu, qv = torch.empty(B, L, H, D, device=DEV, dtype=torch.bfloat16), torch.empty(B, L, H, D, device=DEV, dtype=torch.bfloat16)
    ops.relattn_add_head_bias(qkv, U, VB, qu, qv, B, L, L, H, D)
    out = torch.full((B, L, H, D), NAN, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, L), NAN, device=DEV, dtype=torch.float32)
    probs = mblk = None
    if mode == "fwd_probs":
        probs = torch.full((B * H, ops.relattn_flash_probs_tiles(L), 512), NAN, device=DEV, dtype=torch.bfloat16)
        mblk = torch.full((B * H, L // 32, L), NAN, device=DEV, dtype=torch.float32)
    ops.relattn_flash_fwd(qu, qv, qkv, Rd, out, lse, B, L, H, D, shift, p["scale"], probs=probs, mblk=mblk)
    dqkv = torch.full((B, L, 3, H, D), NAN, device=DEV, dtype=torch.bfloat16)
    delta = torch.full((B, H, L), NAN, device=DEV, dtype=torch.float32)
    if mode != "recompute":
        scrub(int(lib.load().db1_relattn_flash_bwd_workspace_bytes(B, L, H, int(mode == "fwd_probs"))))
    ops.relattn_flash_bwd(qu, qv, qkv, Rd, out, dev16(dout), lse, delta, dqkv, dT, B, L, H, D, shift, p["scale"], store_probs=mode != "recompute",
                          probs=probs, mblk=mblk)
    torch.cuda.synchronize()
    return dqkv, Rd, qv


@pytest.mark.parametrize("L,shift", A.FLASH_BWD_CASES)
@pytest.mark.parametrize("mode", A.FLASH_BWD_MODES)
def test_flash_producer_writes_the_visible_set_and_nothing_else(L, shift, mode):
    B, H = BH
    case = ("flash dT", L, shift, mode)
    _, _, ref, tol, _ = probe(L, shift)
    vis = visible_dist(L, shift)
    dT = dev16(np.broadcast_to(np.where(vis, np.nan, SENT), (H, B, L, L)))
    flash_backward(L, shift, mode, dT)
    got, want = host(dT), ref["dT"].transpose(1, 0, 2, 3)
    assert not want[:, :, ~vis].any()
    check("dT on the visible set", got[:, :, vis], want[:, :, vis], tol["dT"], case)
    rest = bits(dT).cpu().numpy()[:, :, ~vis]
    sent, zero = rest == int(bits(torch.tensor([SENT], dtype=torch.bfloat16))[0]), (rest & 0x7FFF) == 0
    print(f"dT contract {case}: outside the visible set {int(sent.sum())} entries left as they were, {int(zero.sum())} zeroed, of {rest.size}")
    assert (sent | zero).all(), (case, "entries outside the visible set that are neither left nor zero", int((~(sent | zero)).sum()))


@pytest.mark.parametrize("L", A.FLASH_LENGTHS)
@pytest.mark.parametrize("mode", A.FLASH_BWD_MODES)
def test_one_zeroed_dT_buffer_serves_every_call(L, mode):
    """shift >= L: the second backward into the buffer the first one used gives the dT of a fresh zeroed buffer, bit for bit (the model's _dT_buf)"""
    B, H = BH
    used = torch.zeros(H, B, L, L, device=DEV, dtype=torch.bfloat16)
    flash_backward(L, L, mode, used, seed=0)
    first = used.clone()
    flash_backward(L, L, mode, used, seed=1)
    fresh = torch.zeros(H, B, L, L, device=DEV, dtype=torch.bfloat16)
    flash_backward(L, L, mode, fresh, seed=1)
    assert not torch.equal(first, fresh)                                    # the two probes differ, or the reuse would show nothing
    same_bits("the reused buffer against a fresh one", used, fresh, ("dT reuse", L, mode))
    i = np.arange(L)
    assert not bool(used[:, :, torch.from_numpy(i[None, :] > i[:, None]).to(DEV)].any())


MAT_CASES = [(L, 0, s, None) for L, s in A.FLASH_BWD_CASES] + [(1, 127, 128, None), (16, 32, 48, None), (17, 128, 145, None)]
assert all(c in A.DECODE_CASES for c in MAT_CASES[-3:])


def _materialised(AC, T, dP, mlen, shift, scale, case, empty_rows=0):
    """relattn_softmax_fwd + relattn_softmax_bwd on float32 operands against A.materialised, per element"""
    from bdm_db1_amd import ops
    H, B, Lq, Lk = AC.shape
    nd = T.shape[3]
    ref, written = A.materialised(AC, T, dP, mlen, shift, scale)
    rnd, _ = A.materialised(AC, T, dP, mlen, shift, scale, rounded=True)
    i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    empty = ~((j > i - shift) & (j <= i + mlen)).any(1)
    assert int(empty.sum()) == empty_rows
    Pd, Td, dPd = dev32(AC), dev32(T), dev32(dP)
    assert np.array_equal(host(Pd), AC) and np.array_equal(host(Td), T) and np.array_equal(host(dPd), dP)       # float32 holds the operands exactly
    lse = torch.full((H, B, Lq), NAN, device=DEV)
    ops.relattn_softmax_fwd(Pd, Td, lse, H, B, Lq, Lk, nd, mlen, shift, scale)
    dT = torch.full((H, B, Lq, nd), NAN, device=DEV)
    ops.relattn_softmax_bwd(Pd, dPd, dT, H, B, Lq, Lk, nd, mlen, shift, scale)
    torch.cuda.synchronize()
    lse_ref, lse_rnd = np.where(empty, -np.inf, ref["lse"]), np.where(empty, -np.inf, rnd["lse"])     # the -1e30 rows: compared exactly below
    tol = {k: A.tolerance(ref[k], rnd[k], bits=24) for k in ("P", "dS", "dT")}
    with np.errstate(invalid="ignore"):
        tol["lse"] = A.tolerance(lse_ref, lse_rnd, bits=24)
    check("P", Pd, ref["P"], tol["P"], case)
    check("lse", host(lse)[:, :, ~empty], ref["lse"][:, :, ~empty], tol["lse"], case)
    check("dS", dPd, ref["dS"], tol["dS"], case)
    check("dT", dT, ref["dT"], tol["dT"], case)
    assert (bits(dT).cpu().numpy()[:, :, ~written] == 0).all(), (case, "dT outside the written set is not +0")
    if empty_rows:
        e = torch.from_numpy(empty).to(DEV)
        assert (bits(lse[:, :, e]) == bits(torch.tensor([np.float32(-1e30) + np.float32(np.log(np.float32(Lk)))], device=DEV))).all(), case
        assert (bits(Pd[:, :, e]) == bits(torch.tensor([np.float32(1.0) / np.float32(Lk)], device=DEV))).all(), case
        assert (bits(dPd[:, :, e]) == 0).all() and (bits(dT[:, :, e]) == 0).all(), case


@pytest.mark.parametrize("q,mlen,shift,nd", MAT_CASES)
def test_materialised_producer_probe(q, mlen, shift, nd):
    p, dout = A.build(q, mlen, shift, nd)
    T_ = lambda x: x.transpose(2, 0, 1, 3)                                            # [B, n, H, D] -> [H, B, n, D]
    qu, qv, k, v, do = T_(p["q"] + p["u"]), T_(p["q"] + p["vb"]), T_(p["k"]), T_(p["v"]), T_(dout)
    AC, T, dP = qu @ k.transpose(0, 1, 3, 2), qv @ p["R"].transpose(1, 2, 0)[:, None], do @ v.transpose(0, 1, 3, 2)
    _materialised(AC, T, dP, mlen, shift, p["scale"], ("materialised", q, mlen, shift))


def test_materialised_producer_rows_without_a_visible_key():
    """Lq = 8 rows over Lk = 4 keys, shift = 2: rows 5, 6, 7 see no key -- P = 1 / Lk, lse = -1e30 + log Lk, dS = dT = 0"""
    rng = np.random.default_rng(11)
    H, B, Lq, Lk, nd = 2, 2, 8, 4, 8
    AC, T, dP = (rng.integers(-64, 65, s) / 16.0 for s in ((H, B, Lq, Lk), (H, B, Lq, nd), (H, B, Lq, Lk)))
    _materialised(AC, T, dP, 0, 2, 0.25, ("materialised, empty rows",), empty_rows=3)


@pytest.mark.parametrize("L,shift", [c for c in A.FLASH_BWD_CASES if c[0] % 128 == 0])
def test_chain_from_the_kernels_own_dT(L, shift):
    """the calls of TransformerXL._attention_bwd behind relattn_flash_bwd, on the dT the kernel wrote: the stream kernel into dqkv5[:, :, 0], the
    tri = (1, 0) GEMM + add2d_colsums as the non-stream path, the tri = (2, L) GEMM for dR"""
    from bdm_db1_amd import ops
    B, H = BH
    d = H * D
    p, _, ref, tol, tol_chain = probe(L, shift)
    assert all(tol_chain[k] == tol[k] for k in tol if k != "dq")                 # the extra rounding point moves the tolerance of dq alone
    for mode in A.FLASH_BWD_MODES:
        case = ("chain", L, shift, mode)
        dT = torch.zeros(H, B, L, L, device=DEV, dtype=torch.bfloat16)
        dqkv, Rd, qv = flash_backward(L, shift, mode, dT)
        R2 = Rd.view(L, d)
        # ---- the GEMM path: dq_r with and without the structural-zero hint, then dq = dq_k + dq_r and the two column sums
        dqv = [torch.full((B, L, H, D), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
        for o, tri in zip(dqv, ((1, 0), (0, 0))):
            ops.gemm_batched(dT, R2.view(L, H, D).permute(1, 0, 2).unsqueeze(1).expand(H, B, L, D), o.permute(2, 0, 1, 3), tri=tri)
        same_bits("dq_r from the tri = (1, 0) GEMM against the GEMM without the hint", dqv[0], dqv[1], case)
        gemm = dqkv.clone()
        du_g, dv_g = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
        dq2d = gemm.view(B * L, 3 * d)[:, :d]
        ops.add2d_colsums(dqv[0].view(B * L, d), dq2d, dq2d, dv_g, du_g)
        dR = [torch.full((L, d), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
        for o, tri in zip(dR, ((2, L), (0, 0))):
            ops.gemm_batched(dT.view(H, B * L, L).transpose(1, 2).unsqueeze(1), qv.view(B * L, H, D).permute(1, 0, 2).unsqueeze(1),
                             o.view(L, H, D).permute(1, 0, 2).unsqueeze(1), tri=tri)
        same_bits("dR from the tri = (2, L) GEMM against the GEMM without the hint", dR[0], dR[1], case)
        # ---- the stream path, in place over dq_k
        du_s, dv_s = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
        scrub(ws_bytes(L, H))
        ops.relattn_dqr_fused(dT, R2, dqkv[:, :, 0], du_s, dv_s)
        torch.cuda.synchronize()
        assert torch.equal(bits(dqkv[:, :, 1:]), bits(gemm[:, :, 1:]))
        for path, g, du, dv in (("stream", dqkv, du_s, dv_s), ("GEMM", gemm, du_g, dv_g)):
            check(f"dq ({path})", g[:, :, 0], ref["dq"], tol_chain["dq"], case)
            check(f"du ({path})", du.view(H, D), ref["du"], tol["du"], case)
            check(f"dv_bias ({path})", dv.view(H, D), ref["dv_bias"], tol["dv_bias"], case)
        check("dR", dR[0].view(L, H, D), ref["dR"], tol["dR"], case)
