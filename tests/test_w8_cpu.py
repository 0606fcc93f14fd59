"""The fp8 decode-weight format (include/db1_hip.h, "fp8 decode weights") on the host: ops.w8_pack / ops.w8_unpack against tests/w8_rule.py byte
for byte, the rule on crafted rows, a block packed alone against kv8_rule.quantize, the half-ulp bound per element, the prototypes, and the
refusals that come before a launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import attn_probe as A  # noqa: E402
import kv8_rule as K8  # noqa: E402
import w8_rule as W8  # noqa: E402

NEW_PROTOTYPES = ("db1_w8_bytes", "db1_w8_quantize", "db1_linear_decode_w8_supported", "db1_linear_decode_w8", "db1_linear_decode_attn_w8_supported",
                  "db1_linear_decode_attn_w8")


crafted_rows = W8.crafted_rows


def same(a, b):
    return np.array_equal(np.nan_to_num(a, nan=3.0), np.nan_to_num(b, nan=3.0))


def test_crafted_rows_follow_the_rule():
    w = crafted_rows()
    assert same(torch.from_numpy(w).to(torch.bfloat16).to(torch.float64).numpy(), w)          # (all bf16 values)
    pay, s = W8.quantize(w)
    assert s[0, 0] == 1.0 and pay[0, 5] == 0x80 and not np.delete(pay[0, :128], 5).any()      # zero block: scale 1, zero bytes (-0 keeps its sign)
    assert s[1, 0] == 2.0 ** -3 and pay[1, 17] == 0x7E                                        # 448 s: the largest finite byte
    assert s[2, 0] == 2.0 ** -2 and pay[2, 17] == (0x80 | 0x76)                               # 450 s / 2 s = 225 -> rne to 224 = 1.75 * 2^7
    assert (pay[3, [3, 50, 127]] == 0x7F).all()
    clean = w[3].copy()
    clean[[3, 50, 127]] = 0.0
    p3, s3 = W8.quantize(clean[None])
    others = np.setdiff1d(np.arange(256), [3, 50, 127])
    assert s[3, 0] == s3[0, 0] and np.array_equal(pay[3, others], p3[0, others])              # the non-finite elements reach only themselves
    assert s[4, 0] == 2.0 ** -126 and pay[4, 9] == 0x48                                       # 2^-124 / 2^-126 = 4 -> (2 + 7) << 3
    assert s[5, 0] == 2.0 ** 5 and pay[5, 127] == 0x7E
    assert s[6, 0] == 1.0 and (pay[6, :128] == 0x7F).all()
    deq = W8.dequantize(pay, s)
    assert np.isnan(deq[3, [3, 50, 127]]).all() and np.isnan(deq[6, :128]).all()
    assert same(torch.from_numpy(deq).to(torch.bfloat16).to(torch.float64).numpy(), deq)      # payload * s is exact in bf16


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (5, 1024)])
def test_host_pack_and_unpack_are_the_rule(N, K):
    from bdm_db1_amd import ops
    rng = np.random.default_rng([N, K])
    w = A.bf16(rng.standard_normal((N, K)) * np.exp2(rng.integers(-30, 30, (N, K // 128)).repeat(128, 1).astype(np.float64)))
    w[N // 2, :128] = 0.0
    for x in (w, W8.revealing_weights(N, K)):
        buf = ops.w8_pack(torch.from_numpy(x))
        want = W8.pack(x)
        assert buf.dtype == torch.uint8 and tuple(buf.shape) == (W8.nbytes(N, K),) == (ops.w8_bytes(N, K),)
        assert np.array_equal(buf.numpy(), want)
        assert np.array_equal(ops.w8_pack(torch.from_numpy(x).to(torch.bfloat16)).numpy(), want)           # any float dtype holding the values
        deq, s = ops.w8_unpack(buf, N, K)
        pay_r, s_r = W8.unpack(want, N, K)
        assert deq.dtype == torch.bfloat16 and np.array_equal(s.numpy(), s_r)
        assert np.array_equal(deq.to(torch.float64).numpy(), W8.dequantize(pay_r, s_r))
        assert torch.equal(ops.w8_unpack(ops.w8_pack(deq), N, K)[0], deq)                                  # dequantised values are a fixed point
    s = W8.quantize(W8.revealing_weights(N, K))[1]
    assert np.array_equal(s, W8.expected_scales(N, K))
    W8.assert_neighbours_differ(s)


def test_host_pack_of_the_crafted_rows():
    from bdm_db1_amd import ops
    w = crafted_rows()
    buf = ops.w8_pack(torch.from_numpy(w))
    assert np.array_equal(buf.numpy(), W8.pack(w))
    deq, _ = ops.w8_unpack(buf, *w.shape)
    assert same(deq.to(torch.float64).numpy(), W8.dequantize(*W8.quantize(w)))


def test_a_block_packed_alone_is_the_ring_rule():
    rng = np.random.default_rng(2)
    w = np.concatenate([crafted_rows(), A.bf16(rng.standard_normal((8, 256)) * np.exp2(rng.integers(-20, 20, (8, 1)).astype(np.float64)))])
    pay, s = W8.unpack(W8.pack(w), *w.shape)
    for n in range(w.shape[0]):
        for b in range(2):
            p1, s1 = K8.quantize(w[n, 128 * b:128 * (b + 1)])
            assert np.array_equal(pay[n, 128 * b:128 * (b + 1)], p1) and s[n, b] == s1, (n, b)
            alone = W8.pack(w[n:n + 1, 128 * b:128 * (b + 1)])
            assert np.array_equal(alone[:128], p1) and alone[128:].view(np.float32)[0] == s1, (n, b)


def test_half_ulp_bound_per_element():
    """|deq - w| <= max(2^-4 |w|, 2^-10 s) (tests/w8_rule.py derives it), on random, index-revealing and crafted weights"""
    rng = np.random.default_rng(9)
    rand = A.bf16(rng.standard_normal((64, 512)) * np.exp2(rng.integers(-40, 40, (64, 4)).repeat(128, 1).astype(np.float64)))
    mixed = A.bf16(rng.standard_normal((64, 512)) * np.exp2(rng.integers(-12, 1, (64, 512)).astype(np.float64)))      # magnitudes mixed INSIDE a block
    for w in (rand, mixed, W8.revealing_weights(48, 384), crafted_rows()):
        pay, s = W8.quantize(w)
        fin = np.isfinite(w)
        err = np.abs(np.where(fin, W8.dequantize(pay, s) - np.where(fin, w, 0.0), 0.0))
        bound = W8.half_ulp_bound(np.where(fin, w, 0.0), s)
        assert (err <= bound).all(), np.argwhere(err > bound)[:8]
    # the bound is sharp: a tie rounds by exactly half a step
    w = np.zeros((1, 128))
    w[0, 0], w[0, 1] = 448.0, 17.0                       # scale 1; 17 lies between 16 and 18: half a step of the binade [16, 32)
    pay, s = W8.quantize(w)
    assert s[0, 0] == 1.0 and abs(W8.dequantize(pay, s)[0, 1] - 17.0) == 1.0 == 2.0 ** -4 * 16.0


def test_prototypes_are_declared():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for n in NEW_PROTOTYPES:
        assert n in names, n
    Lb = lib.load()
    for n in NEW_PROTOTYPES:
        assert hasattr(Lb, n), n


def test_host_refusals():
    from bdm_db1_amd import lib, ops
    with pytest.raises(ValueError):
        ops.w8_pack(torch.zeros(4, 192))                 # K % 128 != 0
    with pytest.raises(ValueError):
        ops.w8_pack(torch.zeros(128))                    # not a matrix
    with pytest.raises(ValueError):
        ops.w8_pack(torch.zeros(0, 128))
    buf = ops.w8_pack(torch.ones(4, 256))
    for bad in ((buf, 4, 128), (buf, 2, 256), (buf[:-4], 4, 256), (buf.to(torch.int8), 4, 256), (buf, 4, 192), (buf.view(2, -1), 4, 256)):
        with pytest.raises(ValueError):
            ops.w8_unpack(*bad)
    with pytest.raises(ValueError):
        ops.w8_quantize(torch.zeros(4, 256))             # a CPU tensor, fp32
    with pytest.raises(ValueError):
        ops.w8_quantize(torch.zeros(4, 256, dtype=torch.bfloat16))
    assert ops.w8_bytes(16, 128) == 16 * 128 + 64 and ops.w8_bytes(2048, 8192) == 2048 * 8192 + 4 * 2048 * 64
    assert ops.w8_bytes(16, 192) == 0 and ops.w8_bytes(16, 64) == 0 and ops.w8_bytes(0, 128) == 0
    # _supported: the bf16 entry point's answer, and K % 128 == 0
    Lb = lib.load()
    for M, N, K, geglu, ln in ((1, 16, 128, 0, 0), (64, 48, 384, 0, 0), (65, 16, 128, 0, 0), (4, 24, 128, 0, 0), (4, 512, 256, 0, 1), (4, 48, 256, 0, 1),
                               (16, 16, 256, 1, 2), (17, 16, 256, 0, 2), (4, 16, 192, 0, 0), (4, 16, 64, 0, 0), (4, 16, 320, 1, 0)):
        assert Lb.db1_linear_decode_w8_supported(M, N, K, geglu, ln) == int(bool(Lb.db1_linear_decode_supported(M, N, K, geglu, ln)) and K % 128 == 0)
        assert ops.linear_decode_w8_supported(M, N, K, bool(geglu), bool(ln & 1), bool(ln & 2)) == bool(Lb.db1_linear_decode_w8_supported(M, N, K, geglu, ln))
    assert Lb.db1_linear_decode_supported(4, 16, 192, 0, 0) == 1 and Lb.db1_linear_decode_w8_supported(4, 16, 192, 0, 0) == 0
    for a in ((1, 1, 4, 128, 3, 512), (1, 2, 2, 128, 12, 256), (3, 1, 4, 128, 3, 512), (1, 1, 4, 64, 3, 512), (1, 1, 4, 128, 13, 512)):
        assert Lb.db1_linear_decode_attn_w8_supported(*a) == Lb.db1_linear_decode_attn_supported(*a)
    # the entry points refuse before they touch the device: K % 128 (DB1_ERR_UNSUPPORTED), a NULL operand (DB1_ERR_BAD_SHAPE), a buffer that is
    # not 16-byte aligned (DB1_ERR_BAD_ALIGN) -- the pointers below are never dereferenced
    BAD_ALIGN = -2
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)

    def lin(x=p, w=p, y=p, tickets=p, K=256, dtb=lib.DB1_BF16, bias=null):
        return Lb.db1_linear_decode_w8(x, 256, w, bias, dtb, y, 16, 4, 16, K, 0, null, 0, 1.0, null, null, 0.0, null, 0, null, 0, 1.0, null, null, 0.0, null, 0, 0,
                                       tickets, null, 0, null)
    assert lin(K=192) == ops.DB1_ERR_UNSUPPORTED and lin(K=64) == ops.DB1_ERR_UNSUPPORTED
    assert lin(bias=p, dtb=lib.DB1_F32) == ops.DB1_ERR_UNSUPPORTED                            # (instantiated for a bf16 model's operands)
    assert lin(x=null) == lin(w=null) == lin(y=null) == lin(tickets=null) == ops.DB1_ERR_BAD_SHAPE
    assert lin(w=off) == lin(x=off) == lin(y=off) == BAD_ALIGN
    attn = lambda part=p, w=p, y=p, H=2: Lb.db1_linear_decode_attn_w8(part, 3, 1, 1, H, 128, w, y, 512, 512, null)
    assert attn(H=3) == ops.DB1_ERR_UNSUPPORTED
    assert attn(part=null) == attn(w=null) == attn(y=null) == ops.DB1_ERR_BAD_SHAPE
    assert attn(w=off) == attn(part=off) == attn(y=off) == BAD_ALIGN
    qz = lambda w=p, out=p, ldw=256, N=4, K=256: Lb.db1_w8_quantize(w, ldw, N, K, out, null)
    assert qz(K=192) == qz(N=0) == ops.DB1_ERR_UNSUPPORTED
    assert qz(w=null) == qz(out=null) == qz(ldw=128) == ops.DB1_ERR_BAD_SHAPE
    assert qz(w=off) == qz(out=off) == qz(ldw=260) == BAD_ALIGN
