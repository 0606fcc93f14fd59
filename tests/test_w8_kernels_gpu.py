"""The fp8 decode-weight kernels (include/db1_hip.h, "fp8 decode weights"): db1_w8_quantize byte for byte against tests/w8_rule.py;
db1_linear_decode_w8 / db1_linear_decode_attn_w8 BIT FOR BIT against db1_linear_decode / db1_linear_decode_attn over the dequantised weight, in
every form of the launch (plain, split over K, LayerNorm tail, GEGLU, LayerNorm prologue, attention merge), and per element against float64
x . deq(W)^T so that the two launches cannot be wrong together; the refusals.

Weights are index-revealing (tests/w8_rule.py: revealing_weights): no two neighbouring rows or blocks -- nor a GEGLU value row and its gate
row -- share a scale, so a scale or payload taken from a wrong row, block or GEGLU row changes bits.  Outputs start as NaN inside NaN margins."""
import ctypes
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
import w8_rule as W8  # noqa: E402
crafted_rows = W8.crafted_rows

DEV = "cuda"
MARGIN = 1024           # elements of NaN before and after every output
MS = (1, 2, 4, 5, 16, 17, 33, 64)
REL_TOL = 1e-2          # tests/test_decode_gpu.py, test_linear_decode_equals_the_unfused_launches: |got - ref| <= 1e-2 max|ref|
BAD_ALIGN = -2          # DB1_ERR_BAD_ALIGN (include/db1_hip.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)


class Out:
    """a NaN-filled bf16 [M, N] output inside NaN margins"""

    def __init__(self, M, N):
        self.buf = torch.full((2 * MARGIN + M * N,), float("nan"), device=DEV, dtype=torch.bfloat16)
        self.t = self.buf[MARGIN:MARGIN + M * N].view(M, N)

    def check(self, what):
        n = self.t.numel()
        assert bool(torch.isnan(self.buf[:MARGIN].float()).all()) and bool(torch.isnan(self.buf[MARGIN + n:].float()).all()), (what, "margins")
        assert bool(torch.isfinite(self.t.float()).all()), (what, "an element was not written, or is not finite")
        return self.t


def bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def weight(rows, K, geglu_rows=None):
    """(values float64 [rows, K] read-only, the packed buffer on the device from the HOST rule, the dequantised bf16 weight on the device,
    its float64 values) -- scales asserted on the CPU before anything is launched"""
    from bdm_db1_amd import ops
    w = W8.revealing_weights(rows, K)
    pay, s = W8.quantize(w)
    assert np.array_equal(s, W8.expected_scales(rows, K))
    W8.assert_neighbours_differ(s, geglu_rows)
    buf = ops.w8_pack(torch.from_numpy(w))
    assert np.array_equal(buf.numpy(), W8.pack(w))
    deq = ops.w8_unpack(buf, rows, K)[0]
    d64 = W8.dequantize(pay, s)
    assert np.array_equal(deq.to(torch.float64).numpy(), d64)
    assert (np.abs(d64[d64 != 0]) >= 2.0 ** -100).all()                        # (nothing subnormal in bf16: inside the identity)
    for a in (w, d64):
        a.setflags(write=False)
    return w, buf.to(DEV), deq.to(DEV), d64


def operands(M, N, K, seed, bias_rows=0):
    rng = np.random.default_rng([seed, M, N, K])
    x = A.bf16(rng.standard_normal((M, K)))
    bias = A.bf16(rng.standard_normal(bias_rows) * 4.0) if bias_rows else None
    return x, bias


def ln_params(rng, M, n):
    res = A.bf16(rng.standard_normal((M, n)))
    gam, bet = A.bf16(1.0 + 0.25 * rng.standard_normal(n)), A.bf16(0.1 * rng.standard_normal(n))
    return res, gam, bet


def ln64(s, gam, bet, eps):
    mu = s.mean(-1, keepdims=True)
    var = ((s - mu) ** 2).mean(-1, keepdims=True)
    return (s - mu) / np.sqrt(var + eps) * gam + bet


def close(got, ref, what):
    err = np.abs(got.to(torch.float64).cpu().numpy() - ref)
    tol = REL_TOL * np.abs(ref).max()
    print(f"w8 {what}: max|got - ref| = {err.max():.3e}, tol = {tol:.3e}")
    assert (err <= tol).all(), (what, float(err.max()), tol, np.unravel_index(err.argmax(), err.shape))


def tickets_are_zero(what):
    from bdm_db1_amd import ops
    torch.cuda.synchronize()
    assert int(ops.decode_tickets(torch.device(DEV, torch.cuda.current_device())).abs().sum().item()) == 0, what


def run_pair(M, N, x, wbuf, deq, bias, geglu=False, ln=None, pre=None):
    """the fp8 launch twice and the bf16 launch over the dequantised weight: bit-equal outputs, intact margins, tickets zero ->
    the fp8 outputs (y, the LayerNorm output or None)"""
    from bdm_db1_amd import ops
    xd, bd = dev16(x), (dev16(bias) if bias is not None else None)

    def go(fn, w):
        y = Out(M, N)
        extra = None
        kw = {}
        if ln is not None:
            extra = Out(M, N)
            kw["ln"] = ln[:5] + (extra.t,)
        if pre is not None:
            extra = Out(M, x.shape[1])
            kw["pre"] = pre[:5] + (extra.t,)
        fn(xd, w, bd, y.t, geglu=geglu, **kw)
        tickets_are_zero((fn.__name__, M, N))
        return y.check((fn.__name__, M, N, "y")), (extra.check((fn.__name__, M, N, "LayerNorm rows")) if extra is not None else None)

    got, again, ref = go(ops.linear_decode_w8, wbuf), go(ops.linear_decode_w8, wbuf), go(ops.linear_decode, deq)
    case = (M, N, x.shape[1], geglu, ln is not None, pre is not None)
    for k in range(2):
        if got[k] is not None:
            assert torch.equal(bits(got[k]), bits(ref[k])), (case, k, "fp8 launch != bf16 launch over the dequantised weight")
            assert torch.equal(bits(got[k]), bits(again[k])), (case, k, "second launch")
    return got


# ------------------------------------------------------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("N,K,ld", [(16, 128, 128), (48, 384, 384), (32, 4096, 4096), (48, 384, 520)])
def test_w8_quantize_is_the_rule(N, K, ld):
    from bdm_db1_amd import ops
    w = W8.revealing_weights(N, K)
    src = torch.full((N, ld), float("nan"), dtype=torch.bfloat16, device=DEV)      # (ld > K: the columns beyond K are never read -- NaN would show)
    src[:, :K] = dev16(w)
    nb = W8.nbytes(N, K)
    assert ops.w8_bytes(N, K) == nb
    buf = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.w8_quantize(src[:, :K], out=buf[:nb])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[nb:] == 0xA5).all(), "guard"
    gp, gs = W8.unpack(got[:nb], N, K)
    wp, ws = W8.quantize(w)
    assert np.array_equal(gs, ws), "scales"
    assert np.array_equal(gp, wp), np.argwhere(gp != wp)[:8]
    assert np.array_equal(got[:nb], ops.w8_pack(torch.from_numpy(w)).numpy())
    if ld == K:
        assert torch.equal(ops.w8_quantize(src), buf[:nb])                             # (the allocating form)


def test_w8_quantize_crafted_rows():
    """a zero block, amax exactly 448 s and the next bf16 above it, NaN / inf elements, a block at the exponent floor, a block of non-finite
    elements (tests/w8_rule.py: crafted_rows), and random rows over many binades"""
    from bdm_db1_amd import ops
    rng = np.random.default_rng(4)
    w = np.concatenate([crafted_rows(), A.bf16(rng.standard_normal((24, 256)) * np.exp2(rng.integers(-30, 30, (24, 2)).repeat(128, 1).astype(np.float64)))])
    src = torch.from_numpy(w).to(torch.bfloat16).to(DEV)
    got = ops.w8_quantize(src).cpu().numpy()
    gp, gs = W8.unpack(got, *w.shape)
    wp, ws = W8.quantize(w)
    assert np.array_equal(gs, ws), np.argwhere(gs != ws)[:8]
    assert np.array_equal(gp, wp), np.argwhere(gp != wp)[:8]


# ------------------------------------------------------------------------------------------------------------------ the linear maps
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (32, 4096)])
def test_linear_decode_w8_plain(N, K, M):
    """(16, 128): two k-steps, so two of the four waves have an empty share; (48, 384): six k-steps over three blocks -- a wave's share starts
    in the middle of a block; (32, 4096): split over K (S = 2, partial tiles through the workspace and a ticket); with a bias at (48, 384)"""
    from bdm_db1_amd import ops
    assert ops.linear_decode_w8_supported(M, N, K)
    assert (ops.lib.load().db1_linear_decode_workspace_bytes(M, N, K, 0) > 0) == (K == 4096)
    _, wbuf, deq, d64 = weight(N, K)
    x, bias = operands(M, N, K, 1, bias_rows=N if K == 384 else 0)
    y, _ = run_pair(M, N, x, wbuf, deq, bias)
    close(y, x @ d64.T + (bias if bias is not None else 0.0), ("plain", M, N, K))


@pytest.mark.parametrize("M", MS)
def test_linear_decode_w8_layernorm_tail(M):
    N, K, eps, alpha = 512, 256, 1e-5, 0.81
    _, wbuf, deq, d64 = weight(N, K)
    x, bias = operands(M, N, K, 2, bias_rows=N)
    res, gam, bet = ln_params(np.random.default_rng([2, M]), M, N)
    y, h = run_pair(M, N, x, wbuf, deq, bias, ln=(dev16(res), alpha, dev16(gam), dev16(bet), eps))
    y64 = x @ d64.T + bias
    close(y, y64, ("LayerNorm tail, y", M))
    close(h, ln64(alpha * res + y64, gam, bet, eps), ("LayerNorm tail, rows", M))


@pytest.mark.parametrize("M", MS)
def test_linear_decode_w8_geglu(M):
    """value rows n and gate rows N + n of one [2 N, K] buffer in one MFMA tile: their scales differ (asserted in weight())"""
    N, K = 16, 256
    _, wbuf, deq, d64 = weight(2 * N, K, N)
    x, bias = operands(M, N, K, 3, bias_rows=2 * N)
    y, _ = run_pair(M, N, x, wbuf, deq, bias, geglu=True)
    z = x @ d64.T + bias
    gate = z[:, N:]
    gelu = 0.5 * gate * (1.0 + np.vectorize(math.erf)(gate / math.sqrt(2.0)))
    close(y, z[:, :N] * gelu, ("GEGLU", M))


@pytest.mark.parametrize("M", [1, 3, 4, 9, 16])
@pytest.mark.parametrize("K", [256, 2048])
@pytest.mark.parametrize("geglu", [False, True])
def test_linear_decode_w8_layernorm_prologue(geglu, K, M):
    """the three instantiations of the prologue (1, <= 4, <= 16 rows), plain (N = 48) and through GEGLU (N = 16, as the model's first
    feed-forward map); K = 256: one k-step per wave, K = 2048: a wave's whole batch of eight"""
    from bdm_db1_amd import ops
    N, eps, alpha = (16 if geglu else 48), 1e-5, 0.9
    rows = 2 * N if geglu else N
    assert ops.linear_decode_w8_supported(M, N, K, geglu, False, True)
    _, wbuf, deq, d64 = weight(rows, K, N if geglu else None)
    x, bias = operands(M, N, K, 4, bias_rows=rows if geglu else 0)
    res, gam, bet = ln_params(np.random.default_rng([4, M, K]), M, K)
    y, xn = run_pair(M, N, x, wbuf, deq, bias, geglu=geglu, pre=(dev16(res), alpha, dev16(gam), dev16(bet), eps))
    xn64 = ln64(alpha * res + x, gam, bet, eps)
    close(xn, xn64, ("LayerNorm prologue, rows", geglu, K, M))
    z = xn64 @ d64.T + (bias if bias is not None else 0.0)
    if geglu:
        gate = z[:, N:]
        z = z[:, :N] * 0.5 * gate * (1.0 + np.vectorize(math.erf)(gate / math.sqrt(2.0)))
    close(y, z, ("LayerNorm prologue, y", geglu, K, M))


@pytest.mark.parametrize("B,q", [(1, 1), (1, 2), (2, 1)])
def test_linear_decode_attn_w8(B, q):
    """the attention-merge form at H = 2 (K = 256), B q in {1, 2}: partial results of 3 chunks per (row, head), rows the call does not own NaN"""
    from bdm_db1_amd import ops
    H, D, nunit, N = 2, 128, 3, 48
    klen, K, M = 128 * nunit - 20, H * D, B * q
    assert ops.linear_decode_attn_w8_supported(B, q, H, D, klen, N) and ops.linear_decode_attn_supported(B, q, H, D, klen, N)
    _, wbuf, deq, d64 = weight(N, K)
    rng = np.random.default_rng([5, B, q])
    part = np.full((B * H, nunit, 64, D + 2), np.nan, np.float32)
    part[:, :, :q, :D] = rng.standard_normal((B * H, nunit, q, D)).astype(np.float32)
    part[:, :, :q, D] = rng.standard_normal((B * H, nunit, q)).astype(np.float32) * 3.0        # the chunk's maximum
    part[:, :, :q, D + 1] = rng.uniform(0.5, 40.0, (B * H, nunit, q)).astype(np.float32)       # ... and its sum
    pd = torch.from_numpy(part).to(DEV)
    p64 = part.astype(np.float64).reshape(B, H, nunit, 64, D + 2)[:, :, :, :q]
    wt = np.exp(p64[..., D] - p64[..., D].max(2, keepdims=True))                               # [B, H, nunit, q]
    merged = (p64[..., :D] * wt[..., None]).sum(2) / (p64[..., D + 1] * wt).sum(2)[..., None]  # [B, H, q, D]
    x64 = merged.transpose(0, 2, 1, 3).reshape(M, K)

    def go(fn, w):
        y = Out(M, N)
        fn(pd, klen, B, q, H, D, w, y.t)
        tickets_are_zero(fn.__name__)
        return y.check((fn.__name__, B, q))
    got, again, ref = go(ops.linear_decode_attn_w8, wbuf), go(ops.linear_decode_attn_w8, wbuf), go(ops.linear_decode_attn, deq)
    assert torch.equal(bits(got), bits(ref)) and torch.equal(bits(got), bits(again))
    close(got, x64 @ d64.T, ("attention merge", B, q))


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_w8_refusals_launch_nothing():
    """DB1_ERR_UNSUPPORTED (K % 128 != 0, an fp32 bias, fp32 LayerNorm parameters), DB1_ERR_BAD_SHAPE (a NULL operand), DB1_ERR_BAD_ALIGN (a
    packed buffer that is not 16-byte aligned) -- the codes of db1_linear_decode, all before a launch; the wrappers' ValueErrors"""
    from bdm_db1_amd import lib, ops
    Lb = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    M, N, K = 4, 16, 256
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    tk = ops.decode_tickets(y.device)
    off = ctypes.c_void_p(buf.data_ptr() + 8)

    def lin(x=P(buf), w=P(buf), K=K, bias=null, dtb=lib.DB1_BF16, pre=False, dtp=lib.DB1_BF16, fn=Lb.db1_linear_decode_w8):
        pr = (P(buf), K, 1.0, P(buf), P(buf), 1e-5, P(buf), K) if pre else (null, 0, 1.0, null, null, 0.0, null, 0)
        return fn(x, K, w, bias, dtb, P(y), N, M, N, K, 0, *pr, null, 0, 1.0, null, null, 0.0, null, 0, dtp, P(tk), null, 0, null)

    assert lin(K=192) == ops.DB1_ERR_UNSUPPORTED and Lb.db1_linear_decode_supported(M, N, 192, 0, 0) == 1      # (the bf16 entry point takes K % 64 == 0)
    assert lin(bias=P(buf), dtb=lib.DB1_F32) == ops.DB1_ERR_UNSUPPORTED and lin(pre=True, dtp=lib.DB1_F32) == ops.DB1_ERR_UNSUPPORTED
    assert lin(x=null) == lin(w=null) == ops.DB1_ERR_BAD_SHAPE == lin(x=null, fn=Lb.db1_linear_decode)
    assert lin(w=off) == BAD_ALIGN == lin(w=off, fn=Lb.db1_linear_decode)
    attn = lambda w=P(buf), part=P(buf): Lb.db1_linear_decode_attn_w8(part, 3, 1, 1, 2, 128, w, P(y), N, N, null)
    assert attn(w=null) == attn(part=null) == ops.DB1_ERR_BAD_SHAPE and attn(w=off) == BAD_ALIGN
    qz = lambda w=P(buf), out=P(buf), ldw=K, K=K: Lb.db1_w8_quantize(w, ldw, N, K, out, null)
    assert qz(K=192) == ops.DB1_ERR_UNSUPPORTED and qz(w=null) == qz(out=null) == qz(ldw=K - 8) == ops.DB1_ERR_BAD_SHAPE
    assert qz(out=off) == qz(w=off) == qz(ldw=K + 4) == BAD_ALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()) and not bool(buf.any()) and not bool(tk.any())        # nothing was launched
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    good = torch.zeros(ops.w8_bytes(N, K), dtype=torch.uint8, device=DEV)
    for bad in (good[:-4], good.view(torch.int8), torch.zeros(N, K, dtype=torch.bfloat16, device=DEV), good.cpu()):
        with pytest.raises(ValueError):
            ops.linear_decode_w8(x, bad, None, y)
    with pytest.raises(ValueError):
        ops.linear_decode_attn_w8(torch.zeros(1 << 16, device=DEV), 300, 1, 1, 2, 128, good[:-4], torch.zeros(1, N, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        ops.w8_quantize(torch.zeros(N, 192, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        ops.w8_quantize(torch.zeros(N, K, dtype=torch.bfloat16, device=DEV), out=torch.zeros(8, dtype=torch.uint8, device=DEV))
