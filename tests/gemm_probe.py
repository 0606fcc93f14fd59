"""Exact integer probes for the GEMM family (C = alpha A.B + beta C + bias): two operand designs whose results are exactly representable,
ONE reference rule, and mutants of that rule (never of a kernel) with which the CPU test proves that a one-off error changes at least
one element under exact comparison.  numpy only: neither torch nor the library is imported here.

Both designs are deterministic in (M, N, K, seed) and build A as [M, K] and B as [K, N]; the nt / nn / tn storage forms are views of the
same values.  Every operand value is a small integer (exact in bf16), so every product and every partial sum is an integer far below
2^24: fp32 accumulators, split-K partials and the fixed-order reduce are exact in ANY summation order, and a kernel has to return the
mathematically exact result, bit for bit, on every element.  The tolerance is zero.

  dense    A, B i.i.d. uniform integers in [-3, 3] (asymmetric: A is not its own transpose, nor is B, so a transposed operand shows),
           bias integers in [-64, 64], c0 EVEN integers in [-128, 128].  alpha in {1, 1/2}, beta in {0, 1, 1/2}, K <= 32768: every
           intermediate value is a multiple of 1/2 of magnitude <= 9 K + 192 < 2^24 (check()).  An fp32 output must equal the exact
           value; a bf16 output is that value rounded ONCE (the only rounding in the whole computation), which shows the rounding mode.
  bounded  row m of A has exactly 32 nonzeros, each +-1, at k = (m s + j K / 32) mod K, j = 0 .. 31, with s odd, coprime to K / 32 and
           fixed per probe: any K / 32 consecutive rows cover every k exactly once (K % 32 == 0 is required; the tile kernels need K % 64
           == 0 anyway).  B integers in [-2, 2], bias integers in [-32, 32], c0 even integers in [-64, 64].  With alpha = 1 every
           result is an integer of magnitude <= 64 + 32 + 64 = 160 <= 256; with alpha = 1/2 (the skinny cases) a multiple of 1/2 of
           magnitude <= 32 + 32 + 64 = 128 (check()).  bf16 holds all of these exactly: a bf16 output must equal the exact value with
           no rounding in play, so one lost product on a nonzero B entry shows even in bf16.

Which (design, output dtype) catches which mutant -- asserted by tests/test_gemm_probe_cpu.py at (256, 384, 192) and (64, 576, 2048):
  drop_product, drop_last_k, drop_ktile, drop_slice      dense / fp32 and bounded / bf16   (a product with a zero factor cannot show:
                                                         the mutants pick an (m, k) with A[m, k] != 0; bounded needs M >= K / 32 rows
                                                         to have a nonzero in every k, the skinny cases have fewer: dense / fp32 there)
  bias_shift, no_bias, swap_cols                         every (design, dtype) that runs with a bias / at all
  ignore_beta, c0_row_off                                every (design, dtype) that runs with beta != 0
  truncate, double_round                                 dense / bf16 -- where values leave bf16's exact range, |v| > 256: a dense product
                                                         has standard deviation 4 sqrt(K), so K = 2048 (181) shows both and K = 192 (55)
                                                         shows neither: at the small-K branch cases the dense / bf16 run checks the
                                                         indices once more and the rounding mode not at all
"""
import math

import numpy as np

DESIGNS = {   # amplitude of A, of B, of the bias, of c0 (c0 even)
    "dense": dict(a=3, b=3, bias=64, c0=128),
    "bounded": dict(a=1, b=2, bias=32, c0=64),
}
NNZ = 32           # nonzeros per row of a bounded A
ALPHAS = (1.0, 0.5)
BETAS = (0.0, 1.0, 0.5)


# ------------------------------------------------------------------------------------------------------------------ number formats
def bf16_rne(x):
    """round to nearest even bf16, returned as float64 (finite inputs that float32 holds exactly)"""
    x = np.asarray(x, np.float64)
    a = np.ascontiguousarray(x.astype(np.float32)).reshape(-1)
    assert (a.astype(np.float64) == x.reshape(-1)).all(), "not exact in float32: the rounding would not be ONE rounding"
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(x.shape)


def bf16_trunc(x):
    """bf16 by dropping the low 16 bits (round toward zero), as float64"""
    x = np.asarray(x, np.float64)
    a = np.ascontiguousarray(x.astype(np.float32)).reshape(-1)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64).reshape(x.shape)


# ------------------------------------------------------------------------------------------------------------------ bounds
def bound(design, K, alpha, beta, with_bias=True):
    """the largest magnitude any intermediate value can take: alpha * |A.B| + |beta| * |c0| + |bias|"""
    d = DESIGNS[design]
    dot = d["a"] * d["b"] * (K if design == "dense" else NNZ)
    return abs(alpha) * dot + abs(beta) * d["c0"] + (d["bias"] if with_bias else 0)


def check(design, M, N, K, alpha=1.0, beta=0.0, with_bias=True):
    """the conditions under which the design's result is exact (fp32) / exactly representable in bf16 (bounded); shapes only, no product"""
    assert alpha in ALPHAS and beta in BETAS, (alpha, beta)      # multiples of 1/2 times (even) integers: every term a multiple of 1/2
    assert M >= 1 and N >= 1 and 1 <= K <= 32768, (M, N, K)
    b = bound(design, K, alpha, beta, with_bias)
    if design == "dense":
        assert b <= 9 * 32768 + 192 < 2 ** 24, b                 # multiples of 1/2 below 2^23: exact in fp32
    else:
        assert K % NNZ == 0, K
        # bf16 has 8 significant bits: integers up to 256, multiples of 1/2 up to 128
        assert b <= (256 if alpha == 1.0 else 128), (alpha, beta, b)
    return b


def bounded_step(K, seed=0):
    """the odd row step s of a bounded A: coprime to K / 32, so that K / 32 consecutive rows reach every residue"""
    G = K // NNZ
    s = 7 + 2 * (seed % 16)
    while math.gcd(s, G) != 1:
        s += 2
    return s


def bounded_positions(rows, K, seed=0):
    """[len(rows), 32] int64: the k of the nonzeros of the given rows of a bounded A"""
    rows = np.asarray(rows, np.int64)
    return (rows[:, None] * bounded_step(K, seed) + np.arange(NNZ, dtype=np.int64)[None, :] * (K // NNZ)) % K


def check_coverage(M, K, seed=0):
    """the coverage property of `bounded` at one shape, without building A: (a) the first, a middle and the last window of K / 32 consecutive
    rows reach every k exactly once (where M has that many rows); (b) with M >= 256, every 64-wide k-tile has a nonzero in every 256-row
    block, so that no k-tile of no row block can be dropped unseen.  Returns the number of windows checked."""
    G = K // NNZ
    assert K % NNZ == 0 and math.gcd(bounded_step(K, seed), G) == 1
    n = 0
    if M >= G:
        for m0 in sorted({0, (M - G) // 2, M - G}):
            pos = bounded_positions(np.arange(m0, m0 + G), K, seed)
            assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(K)), (M, K, m0)
            n += 1
    if M >= 256 and K % 64 == 0:
        m = np.arange(M - M % 256)
        cell = (m[:, None] // 256) * (K // 64) + bounded_positions(m, K, seed) // 64
        assert np.unique(cell).size == (M // 256) * (K // 64), (M, K)
    return n


# ------------------------------------------------------------------------------------------------------------------ the probe
def build(design, M, N, K, seed=0):
    """dict(A [M, K] int8, B [K, N] int8, bias [N] int16, c0 [M, N] int16, design, step)"""
    d = DESIGNS[design]
    rng = np.random.default_rng([seed, M, N, K, 0 if design == "dense" else 1])
    step = 0
    if design == "dense":
        A = rng.integers(-d["a"], d["a"] + 1, (M, K), dtype=np.int8)
    else:
        assert K % NNZ == 0
        step = bounded_step(K, seed)
        A = np.zeros((M, K), np.int8)
        sign = (rng.integers(0, 2, (M, NNZ), dtype=np.int8) * 2 - 1).astype(np.int8)
        np.put_along_axis(A, bounded_positions(np.arange(M), K, seed), sign, axis=1)
        assert ((A != 0).sum(1) == NNZ).all()
    B = rng.integers(-d["b"], d["b"] + 1, (K, N), dtype=np.int8)
    bias = rng.integers(-d["bias"], d["bias"] + 1, N, dtype=np.int16)
    c0 = (2 * rng.integers(-d["c0"] // 2, d["c0"] // 2 + 1, (M, N), dtype=np.int16)).astype(np.int16)
    return dict(A=A, B=B, bias=bias, c0=c0, design=design, step=step)


def product(A, B):
    """A . B as int64.  Computed in float64, where sums of these integers (far below 2^53) are exact in any order; the CPU test checks
    it against numpy's int64 product."""
    return np.rint(A.astype(np.float64) @ B.astype(np.float64)).astype(np.int64)


def _product(p):
    if "_P" not in p:
        p["_P"] = product(p["A"], p["B"])
    return p["_P"].copy()


def finish(P, alpha, beta, bias, c0, out_dtype, rounding=bf16_rne):
    """the epilogue in float64 on an exact product P, then ONE rounding for a bf16 output (none for fp32: the value is exact there)"""
    v = alpha * P.astype(np.float64)
    if beta != 0.0:
        v = v + beta * c0.astype(np.float64)
    if bias is not None:
        v = v + bias.astype(np.float64)[None, :]
    assert np.abs(v).max() < 2 ** 23 and np.array_equal(v * 2, np.round(v * 2))
    return rounding(v) if out_dtype == "bf16" else v


def expected(p, alpha=1.0, beta=0.0, with_bias=True, out_dtype="f32"):
    """THE reference rule: out = round_once(alpha A.B + beta c0 + bias), float64 [M, N]"""
    M, K = p["A"].shape
    check(p["design"], M, p["B"].shape[1], K, alpha, beta, with_bias)
    return finish(_product(p), alpha, beta, p["bias"] if with_bias else None, p["c0"], out_dtype)


# ------------------------------------------------------------------------------------------------------------------ mutants of the rule
MUTANTS = ("drop_product", "drop_last_k", "drop_ktile", "drop_slice", "bias_shift", "no_bias", "ignore_beta", "c0_row_off", "truncate",
           "double_round", "swap_cols")
NEEDS_BIAS = ("bias_shift", "no_bias")
NEEDS_BETA = ("ignore_beta", "c0_row_off")
ROUNDING = ("truncate", "double_round")       # only a bf16 output of values beyond bf16's exact range can show these


def mutant(name, p, alpha=1.0, beta=0.0, with_bias=True, out_dtype="f32", slices=4):
    """the reference rule under one error:
    drop_product   the product at one (m, k) with A[m, k] != 0 is lost, in every column
    drop_last_k    k = K - 1 is lost for all rows
    drop_ktile     one k-tile of 64 (the last) is lost for one 256-row block (the last, or all rows if M < 256)
    drop_slice     one of `slices` split-K slices (the second) is lost
    bias_shift     the bias is read one column off (bias[n + 1])
    no_bias        the bias is never added
    ignore_beta    beta is taken as 0
    c0_row_off     c0 is read one row off (c0[m + 1])
    truncate       bf16 by truncation instead of round-to-nearest-even
    double_round   alpha A.B is rounded to bf16 BEFORE bias and beta c0 are added, and the sum is rounded again
    swap_cols      two neighbouring output columns inside one 16-column group change places"""
    A, B, bias, c0 = p["A"], p["B"], (p["bias"] if with_bias else None), p["c0"]
    M, K = A.shape
    P = _product(p)
    rounding = bf16_rne
    if name == "drop_product":
        m = M // 2
        k = int(np.flatnonzero(A[m])[-1])
        P[m] -= int(A[m, k]) * B[k].astype(np.int64)
    elif name == "drop_last_k":
        P -= np.outer(A[:, K - 1].astype(np.int64), B[K - 1].astype(np.int64))
    elif name == "drop_ktile":
        r0 = (M - 1) // 256 * 256
        P[r0:] -= product(A[r0:, K - 64:], B[K - 64:])
    elif name == "drop_slice":
        kc = K // slices
        P -= product(A[:, kc:2 * kc], B[kc:2 * kc])
    elif name == "bias_shift":
        bias = np.roll(bias, -1)
    elif name == "no_bias":
        bias = None
    elif name == "ignore_beta":
        beta = 0.0
    elif name == "c0_row_off":
        c0 = np.roll(c0, -1, axis=0)
    elif name == "truncate":
        rounding = bf16_trunc
    elif name == "double_round":
        assert out_dtype == "bf16"
        v = bf16_rne(alpha * P.astype(np.float64))
        if beta != 0.0:
            v = v + beta * c0.astype(np.float64)
        if bias is not None:
            v = v + bias.astype(np.float64)[None, :]
        return bf16_rne(v)
    elif name == "swap_cols":
        out = finish(P, alpha, beta, bias, c0, out_dtype)
        n = 16 * (out.shape[1] // 32) + 5
        out[:, [n, n + 1]] = out[:, [n + 1, n]]
        return out
    else:
        raise KeyError(name)
    return finish(P, alpha, beta, bias, c0, out_dtype, rounding)


# ------------------------------------------------------------------------------------------------------------------ the cases
# the epilogues of the branch test: (design, output dtype, alpha, beta, bias dtype or None)
EPILOGUES = (
    ("dense", "f32", 1.0, 0.0, None),
    ("dense", "f32", 0.5, 1.0, "bf16"),
    ("dense", "f32", 1.0, 0.5, "f32"),
    ("bounded", "bf16", 1.0, 0.0, "bf16"),
    ("bounded", "bf16", 1.0, 1.0, None),
    ("bounded", "bf16", 1.0, 0.5, "bf16"),
    ("dense", "bf16", 1.0, 0.0, "bf16"),
)
LARGE_TILE_SHAPES = ((256, 256, 64), (512, 768, 320), (768, 512, 1024), (512, 768, 256), (768, 512, 384))
TAIL_SHAPES = ((200, 72, 128), (328, 576, 64), (72, 200, 192), (1568, 2048, 256), (576, 64, 512))
SKINNY_M = (1, 5, 16, 33, 64)
SKINNY_NK = ((2048, 2048), (33280, 2048))
BATCHED = ((2, 3, 128, 128, 1024), (2, 1, 1024, 128, 8192))       # (z0, z1, M, N, K)
HINT_GEOMETRIES = ((2, 3, 512), (3, 8, 1024))                     # (H, B, L): dq_r / dR of test_gemm_structural_zero_hints, dR of the dispatch test
HEADBIAS = ((4096, 2048, 512), (4096, 1024, 512))                 # (M, d, K), N = 3 d
STRIDED_ODD = (70, 130, 37)                                       # no tile kernel takes it (dense only: K % 32 != 0)


def is_small(M, N, K):
    """operands built on the host by build(); beyond this (about 10^8 elements) the GPU test draws them on the device by the same rule"""
    return M * K + K * N + M * N <= 10 ** 8
