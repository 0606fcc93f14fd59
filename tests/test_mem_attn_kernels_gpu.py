"""db1_relattn_mem_fwd (attention of any number of new queries over a memory, one launch) on the index-revealing probes of tests/attn_probe.py
at the cases of tests/mem_attn_cases.py: ``out`` and ``lse`` per element against the float64 closed form under the tolerance derived from
the rounded model (tests/test_mem_attn_probe_cpu.py proves that every one-off index or mask error exceeds it ten times), both buffers
pre-filled with NaN inside guarded allocations, and a second launch that must give the same bits.  Then random data with another batch
and head count through views into a packed [B, klen, 3, H, D] projection, and the refusals."""
import functools
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

import attn_probe as A  # noqa: E402
from gpu_common import DEV, Guarded, _need_gpu  # noqa: E402,F401
from mem_attn_cases import MEM_CASES  # noqa: E402

B, H, D = A.B, A.H, A.D


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def probe(q, mlen, shift, nd):
    """inputs, float64 reference and tolerances of one case: computed once, never written to"""
    p, _ = A.build(q, mlen, shift, nd)
    ref = A.reference(p)
    tol = A.tolerances(ref, A.reference(p, rounded=True))
    for x in list(p.values()) + list(ref.values()):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return p, ref, tol


def check(what, got, ref, tol, case):
    got = got.detach().to(torch.float64).cpu().numpy()
    err = np.abs(got - ref)
    worst = float(np.nanmax(err)) if np.isfinite(got).any() else float("inf")
    print(f"mem_attn {case} {what}: max|got - ref| = {worst:.3e}, tol = {tol:.3e}, ratio = {worst / tol:.3f}")
    assert np.isfinite(got).all(), (case, what)
    assert worst <= tol, (case, what, worst, tol, np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("q,mlen,shift,nd", MEM_CASES)
def test_mem_probe(q, mlen, shift, nd):
    from bdm_db1_amd import ops
    p, ref, tol = probe(q, mlen, shift, nd)
    klen, ndr = mlen + q, p["R"].shape[0]
    kv = dev16(np.stack([p["k"], p["v"]], axis=2))                            # [B, klen, 2, H, D]
    qu, qv, Rd = dev16(p["q"] + p["u"]), dev16(p["q"] + p["vb"]), dev16(p["R"]).view(ndr, H * D)
    assert ops.relattn_mem_supported(B, q, klen, mlen, H, D, shift, torch.bfloat16, kv.stride(1), kv.stride(0))
    runs = []
    for _ in range(2):
        out, lse = Guarded(B * q, H * D, "bf16"), Guarded(B * H, q, "f32")
        out.t.fill_(float("nan"))
        lse.t.fill_(float("nan"))
        ops.relattn_mem_fwd(qu, qv, kv[:, :, 0], kv[:, :, 1], Rd, out.t.view(B, q, H, D), lse.t.view(B, H, q), B, q, klen, mlen, H, D, shift, p["scale"])
        torch.cuda.synchronize()
        out.intact("out")
        lse.intact("lse")
        runs.append((out.t.view(B, q, H, D).clone(), lse.t.view(B, H, q).clone()))
    case = ("mem", q, mlen, shift, nd)
    check("out", runs[0][0], ref["out"], tol["out"], case)
    check("lse", runs[0][1], ref["lse"], tol["lse"], case)
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)), (case, "two launches, other bits in out")
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), (case, "two launches, other bits in lse")
    # without lse: the same output
    out = torch.full((B, q, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.relattn_mem_fwd(qu, qv, kv[:, :, 0], kv[:, :, 1], Rd, out, None, B, q, klen, mlen, H, D, shift, p["scale"])
    assert torch.equal(out.view(torch.int16), runs[0][0].view(torch.int16)), (case, "lse = NULL changes out")


def test_mem_attention_random_data_other_strides():
    """B = H = 3 (a batch or head stride error that B = H = 2 hides), K / V as views into a packed [B, klen, 3, H, D] projection as the model
    passes them; bound: that of test_decode_gpu.py::test_decode_attention_matches_closed_form (bf16 rounding of P and of the output)"""
    from bdm_db1_amd import ops
    Bn, Hn, q, mlen, shift = 3, 3, 150, 70, 100
    klen = mlen + q
    rng = np.random.default_rng(150070)
    bf = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    qu, qv = bf(rng.standard_normal((Bn, q, Hn, D))), bf(rng.standard_normal((Bn, q, Hn, D)))
    qkv = bf(rng.standard_normal((Bn, klen, 3, Hn, D)))
    R = bf(rng.standard_normal((klen, Hn, D)))
    scale = 1.0 / math.sqrt(D)
    i, j = np.arange(q)[:, None], np.arange(klen)[None, :]
    AC = np.einsum("bihd,bjhd->bhij", qu, qkv[:, :, 1])
    T = np.einsum("bihd,rhd->bhir", qv, R)
    BD = np.take_along_axis(T, np.broadcast_to(np.clip(mlen + i - j, 0, klen - 1)[None, None], AC.shape), axis=3)
    vis = (j <= i + mlen) & (j > i - shift)
    S = np.where(vis[None, None], (AC + BD) * scale, -np.inf)
    mx = S.max(-1, keepdims=True)
    Pm = np.exp(S - mx)
    ref_lse = mx[..., 0] + np.log(Pm.sum(-1))
    Pm /= Pm.sum(-1, keepdims=True)
    ref = np.einsum("bhij,bjhd->bihd", Pm, qkv[:, :, 2])
    QKV = dev16(qkv)
    out = torch.full((Bn, q, Hn, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((Bn, Hn, q), float("nan"), device=DEV, dtype=torch.float32)
    assert ops.relattn_mem_supported(Bn, q, klen, mlen, Hn, D, shift, torch.bfloat16, QKV.stride(1), QKV.stride(0))
    ops.relattn_mem_fwd(dev16(qu), dev16(qv), QKV[:, :, 1], QKV[:, :, 2], dev16(R).view(klen, Hn * D), out, lse, Bn, q, klen, mlen, Hn, D, shift, scale)
    torch.cuda.synchronize()
    err = np.abs(out.double().cpu().numpy() - ref).max() / np.abs(ref).max()
    lerr = np.abs(lse.double().cpu().numpy() - ref_lse).max()
    print(f"mem attention random data: out rel err {err:.3e}, lse abs err {lerr:.3e}")
    assert err < 2e-2, f"mem attention rel err {err:.3e}"
    assert lerr < 1e-3      # fp32 scores of |s| < 8 from exact bf16 products, fp32 sums of at most 170 terms: 1e-3 is generous by two orders


def test_refusals_launch_nothing():
    from bdm_db1_amd import lib, ops
    q, mlen, shift = 70, 10, 80
    klen = mlen + q
    bf16 = torch.bfloat16
    mk = lambda *s, dt=bf16: torch.zeros(*s, device=DEV, dtype=dt)

    def attempt(dt=bf16, Dn=D, klen_=klen, mlen_=mlen, shift_=shift, pad=0):
        qu, qv = mk(B, q, H, Dn, dt=dt), mk(B, q, H, Dn, dt=dt)
        kbuf, vbuf = mk(B, klen_, H * Dn + pad, dt=dt), mk(B, klen_, H * Dn + pad, dt=dt)
        k = kbuf.as_strided((B, klen_, H, Dn), (klen_ * (H * Dn + pad), H * Dn + pad, Dn, 1))
        v = vbuf.as_strided(k.shape, k.stride())
        R = mk(klen_, H * Dn, dt=dt)
        out = torch.full((B, q, H, Dn), float("nan"), device=DEV, dtype=dt)
        assert not ops.relattn_mem_supported(B, q, klen_, mlen_, H, Dn, shift_, dt, k.stride(1), k.stride(0))
        with pytest.raises(lib.Db1Error):
            ops.relattn_mem_fwd(qu, qv, k, v, R, out, None, B, q, klen_, mlen_, H, Dn, shift_, 1.0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())

    attempt(dt=torch.float32)
    attempt(Dn=64)
    attempt(klen_=klen + 1)
    attempt(mlen_=0, klen_=q, shift_=0)        # shift + mlen == 0: no row would see a key
    attempt(pad=4)                             # a row stride of H D + 4 elements: not a multiple of 8
    assert ops.relattn_mem_supported(B, q, klen, mlen, H, D, shift, bf16, 3 * H * D, klen * 3 * H * D)
    assert not ops.relattn_mem_supported(B, 8193, mlen + 8193, mlen, H, D, shift, bf16) and not ops.relattn_mem_supported(B, 8192, 16385, 8193, H, D, shift, bf16)
    assert int(lib.load().db1_relattn_mem_workspace_bytes(B, q, klen, H)) == 0
