"""The fp8 decode-weight format of include/db1_hip.h ("fp8 decode weights") restated in NumPy on top of tests/kv8_rule.py (no torch, no
library), and the index-revealing weights of the kernel tests.

A weight W [N, K] (bf16 values, K % 128 == 0) is ONE buffer: N K bytes of e4m3 payload, row-major, then N (K / 128) fp32 scales, row-major.
A block is the 128 consecutive k of one row; its scale, payload, NaN byte and exponent floor are kv8_rule.quantize's.

The half-ulp bound the tests check per element, |deq - w| <= max(2^-4 |w|, 2^-10 s) with s the block's scale: y = w / s is exact and
|y| <= 448.  Where |y| >= 2^-6 (e4m3's normal range) y lies in a binade 2^e <= |y| with spacing 2^(e - 3), so the rounding moves it by at most
2^(e - 4) <= 2^-4 |y|; below 2^-6 the spacing is the subnormal one, 2^-9, and the rounding moves y by at most 2^-10.  Times s (exact)."""
import numpy as np

import kv8_rule as K8

BLOCK = 128


def nbytes(N, K):
    assert K % BLOCK == 0
    return N * K + 4 * N * (K // BLOCK)


def quantize(w):
    """w [N, K] -> (payload uint8 [N, K], scales float32 [N, K / 128])"""
    w = np.asarray(w, np.float64)
    N, K = w.shape
    assert K % BLOCK == 0
    pay, s = K8.quantize(w.reshape(N, K // BLOCK, BLOCK))
    return pay.reshape(N, K), s


def pack(w):
    """w [N, K] -> the buffer, uint8 [N K + 4 N K / 128]"""
    pay, s = quantize(w)
    return np.concatenate([pay.reshape(-1), np.ascontiguousarray(s).view(np.uint8).reshape(-1)])


def unpack(buf, N, K):
    """the buffer -> (payload uint8 [N, K], scales float32 [N, K / 128])"""
    buf = np.ascontiguousarray(buf, np.uint8)
    assert buf.shape == (nbytes(N, K),)
    return buf[:N * K].reshape(N, K), np.ascontiguousarray(buf[N * K:]).view(np.float32).reshape(N, K // BLOCK)


def dequantize(pay, s):
    """(payload [N, K], scales [N, K / 128]) -> values float64 [N, K]"""
    N, K = pay.shape
    return K8.dequantize(pay.reshape(N, K // BLOCK, BLOCK), s).reshape(N, K)


def half_ulp_bound(w, s):
    """the per-element bound of the docstring: max(2^-4 |w|, 2^-10 s)"""
    w = np.asarray(w, np.float64)
    N, K = w.shape
    return np.maximum(np.abs(w) * 2.0 ** -4, np.repeat(np.asarray(s, np.float64), BLOCK, axis=1) * 2.0 ** -10)


# ------------------------------------------------------------------------------------------------------------------ the kernel tests' weights
def magnitude_class(N, K):
    """[N, K / 128]: the exponent c of the magnitude class 2^c of row n, block b: (5 n + 3 b) mod 9 - 4"""
    n, b = np.arange(N)[:, None], np.arange(K // BLOCK)[None, :]
    return (5 * n + 3 * b) % 9 - 4


def revealing_weights(N, K, seed=0):
    """index-revealing weights [N, K] (bf16 values as float64): block (n, b) holds 2^c(n, b) times values in [-1.75, 1.75] whose largest
    magnitude IS 1.75 (element (7 n + b) mod 128), so its scale is exactly 2^(c - 8) -- no two neighbouring rows or blocks share a scale
    (5 and 3 are no multiples of 9), and a wrong row, block or GEGLU-row index reads another scale"""
    import attn_probe as A
    rng = np.random.default_rng([seed, N, K])
    c = magnitude_class(N, K)
    w = A.bf16(rng.uniform(-1.75, 1.75, (N, K // BLOCK, BLOCK)))
    n, b = np.meshgrid(np.arange(N), np.arange(K // BLOCK), indexing="ij")
    w[n, b, (7 * n + b) % BLOCK] = np.where((n + b) % 2 == 0, 1.75, -1.75)
    return (w * np.exp2(c.astype(np.float64))[..., None]).reshape(N, K)


def expected_scales(N, K):
    return np.exp2((magnitude_class(N, K) - 8).astype(np.float64)).astype(np.float32)


def assert_neighbours_differ(s, geglu_rows=None):
    """no two neighbouring rows or blocks share a scale; ``geglu_rows`` = N of a [2 N, K] GEGLU weight: neither do value row n and gate row N + n"""
    s = np.asarray(s)
    assert (s[1:] != s[:-1]).all(), "neighbouring rows share a scale"
    if s.shape[1] > 1:
        assert (s[:, 1:] != s[:, :-1]).all(), "neighbouring blocks share a scale"
    if geglu_rows is not None:
        assert (s[:geglu_rows] != s[geglu_rows:]).all(), "a value row and its gate row share a scale"


def _bf16(x):
    import attn_probe as A
    return A.bf16(x)


def crafted_rows():
    """[8, 256] bf16 values (float64): per row two blocks; the rule's edges sit in block 0 of rows 0 .. 6, block 1 is ordinary.
    row 0: a zero block (with a -0)                      row 1: amax exactly 448 * 2^-3
    row 2: amax the next bf16 above 448 * 2^-3           row 3: a NaN, +inf and -inf among ordinary values
    row 4: a block at the exponent floor (amax 2^-124: the scale would be 2^-132, stays 2^-126)
    row 5: amax exactly 448 * 2^5                        row 6: every element non-finite (amax over nothing: scale 1)"""
    rng = np.random.default_rng(21)
    w = _bf16(rng.standard_normal((8, 256)))
    w[0, :128] = 0.0
    w[0, 5] = -0.0
    w[1, :128] = _bf16(rng.uniform(-40, 40, 128))
    w[1, 17] = 448.0 * 2.0 ** -3
    w[2, :128] = w[1, :128]
    w[2, 17] = -450.0 * 2.0 ** -3                       # 450 = 1.7578125 * 2^8: the bf16 after 448
    w[3, [3, 50, 127]] = [np.nan, np.inf, -np.inf]
    w[4, :128] = _bf16(rng.uniform(-1, 1, 128) * 2.0 ** -124)
    w[4, 9] = 2.0 ** -124
    w[5, :128] = _bf16(rng.uniform(-10000, 10000, 128))
    w[5, 127] = 448.0 * 2.0 ** 5
    w[6, :128] = np.nan
    w[6, 0:128:2] = np.inf
    return w
