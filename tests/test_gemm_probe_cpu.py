"""The GEMM probes of tests/gemm_probe.py, checked without a GPU: the builder's bounds and the coverage of `bounded` at every shape the GPU
test runs (shapes only), the reference rule against a plain int64 product, every mutant of the rule detected under EXACT comparison in
the (design, output dtype) the GPU test relies on for it -- and the gap this closes: which of those mutants the Gaussian operands and the
6e-3-of-the-maximum rule of the older GEMM tests let through at K = 8192."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gemm_probe as G  # noqa: E402
import gemm_dispatch_table as gdt  # noqa: E402

SMALL = ((256, 384, 192), (64, 576, 2048))


def gpu_shapes():
    """{(M, N, K)} of every product the GPU test runs"""
    s = {c[0] for c in gdt.BRANCH_CASES} | set(G.LARGE_TILE_SHAPES) | set(G.TAIL_SHAPES)
    s |= {(M, N, K) for M in G.SKINNY_M for N, K in G.SKINNY_NK}
    s |= {(M, N, K) for _, _, M, N, K in G.BATCHED}
    s |= {(L, 128, L) for _, _, L in G.HINT_GEOMETRIES} | {(L, 128, B * L) for _, B, L in G.HINT_GEOMETRIES}
    s |= {(M, 3 * d, K) for M, d, K in G.HEADBIAS}
    return sorted(s)


@pytest.fixture(scope="module")
def probes():
    return {(d, s): G.build(d, *s) for d in G.DESIGNS for s in SMALL}


def test_bounds_and_coverage_at_every_gpu_shape():
    shapes = gpu_shapes()
    assert len(shapes) >= 30 and max(K for _, _, K in shapes) == 32768
    windows = 0
    for M, N, K in shapes:
        for alpha in G.ALPHAS:
            for beta in G.BETAS:
                assert G.check("dense", M, N, K, alpha, beta) <= 9 * K + 192
        for beta in G.BETAS:
            assert G.check("bounded", M, N, K, 1.0, beta) <= 160
        assert G.check("bounded", M, N, K, 0.5, 1.0) == 128            # the skinny epilogue
        windows += G.check_coverage(M, K)
        if M >= K // 32:
            assert G.check_coverage(M, K) >= 1
    assert windows > len(shapes)
    for alpha in G.ALPHAS:
        for beta in G.BETAS:
            G.check("dense", *G.STRIDED_ODD, alpha, beta)
    # what the bounds rest on: 2^24 for fp32, 8 significant bits for bf16
    assert np.float32(2 ** 24 - 1) + np.float32(1) == 2 ** 24 and np.float32(2 ** 24) + np.float32(1) == 2 ** 24
    for v in (255.0, 256.0, 127.5, 128.0, -160.0):
        assert G.bf16_rne(v) == v
    assert G.bf16_rne(257.0) == 256.0 and G.bf16_rne(259.0) == 260.0 and G.bf16_rne(128.5) == 128.0 and G.bf16_rne(129.5) == 130.0
    for bad in (("dense", 8, 8, 65536), ("dense", 8, 8, 64, 0.25), ("bounded", 64, 64, 48), ("bounded", 64, 64, 64, 2.0)):
        with pytest.raises(AssertionError):
            G.check(*bad)


def test_the_designs_are_what_the_docstring_says(probes):
    for (design, (M, N, K)), p in probes.items():
        d = G.DESIGNS[design]
        A, B = p["A"].astype(np.int64), p["B"].astype(np.int64)
        assert A.shape == (M, K) and B.shape == (K, N) and p["bias"].shape == (N,) and p["c0"].shape == (M, N)
        assert np.abs(A).max() == d["a"] and np.abs(B).max() == d["b"] and np.abs(p["bias"]).max() <= d["bias"]
        assert np.abs(p["c0"]).max() <= d["c0"] and not (p["c0"] % 2).any() and np.unique(p["c0"]).size > d["c0"] // 2
        assert np.unique(p["bias"]).size > 16
        q = G.build(design, M, N, K)
        assert all(np.array_equal(p[k], q[k]) for k in ("A", "B", "bias", "c0"))                   # deterministic
        assert not np.array_equal(G.build(design, M, N, K, seed=1)["B"], p["B"])
        if design == "dense":
            m = min(M, K)
            assert not np.array_equal(A[:m, :m], A[:m, :m].T) and not np.array_equal(B[:m, :m], B[:m, :m].T)
            assert set(np.unique(A)) == set(range(-3, 4))
        else:
            assert ((A != 0).sum(1) == 32).all() and set(np.unique(A)) == {-1, 0, 1}
            assert (A != 0).sum(0).min() >= 1                                                # M >= K / 32 at both small shapes
            for m0 in (0, M - K // 32):
                assert ((A[m0:m0 + K // 32] != 0).sum(0) == 1).all()


def test_expected_is_the_int64_product_and_one_rounding(probes):
    torch = pytest.importorskip("torch")
    for (design, shape), p in probes.items():
        P = np.einsum("mk,kn->mn", p["A"].astype(np.int64), p["B"].astype(np.int64))
        assert P.dtype == np.int64 and np.array_equal(G.product(p["A"], p["B"]), P)
        for alpha in ((1.0, 0.5) if design == "dense" else (1.0,)):
            for beta in G.BETAS:
                for with_bias in (False, True):
                    exact = alpha * P + beta * p["c0"].astype(np.int64) + (p["bias"].astype(np.int64)[None] if with_bias else 0)
                    assert np.array_equal(G.expected(p, alpha, beta, with_bias, "f32"), exact)
                    got = G.expected(p, alpha, beta, with_bias, "bf16")
                    # the torch route (bf() of tests/test_kernels_gpu.py): float32 holds `exact`, so this is one rounding too
                    want = torch.from_numpy(exact.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
                    assert np.array_equal(got, want)
                    if design == "bounded":
                        assert np.array_equal(got, exact), "a bounded result that bf16 does not hold"
    # the two rounding helpers against torch on values that do round, ties included
    v = np.concatenate([np.arange(-2100, 2100) * 0.5, np.arange(250, 3000) * 1.0, [257.0, 258.0, 259.0, 770.0, 774.0]])
    assert np.array_equal(G.bf16_rne(v), torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy())
    assert (G.bf16_trunc(v) != G.bf16_rne(v)).sum() > 1000 and (np.abs(G.bf16_trunc(v)) <= np.abs(v)).all()


# (design, out dtype, alpha, beta, bias) the GPU test relies on for each family of mutants
PRODUCT_MUTANTS = ("drop_product", "drop_last_k", "drop_ktile", "drop_slice")


def _detecting_runs(name):
    runs = [e for e in G.EPILOGUES]
    if name in PRODUCT_MUTANTS:
        runs = [e for e in runs if (e[0], e[1]) in (("dense", "f32"), ("bounded", "bf16"))]
    elif name in G.ROUNDING:
        runs = [e for e in runs if (e[0], e[1]) == ("dense", "bf16")]
    if name in G.NEEDS_BIAS:
        runs = [e for e in runs if e[4] is not None]
    if name in G.NEEDS_BETA:
        runs = [e for e in runs if e[3] != 0.0]
    return runs


@pytest.mark.parametrize("name", G.MUTANTS)
def test_every_mutant_changes_the_expected_output_under_exact_comparison(probes, name):
    runs = _detecting_runs(name)
    assert runs, name
    if name in PRODUCT_MUTANTS:
        assert {(e[0], e[1]) for e in runs} == {("dense", "f32"), ("bounded", "bf16")}
    counts = {}
    for shape in SMALL:
        for design, od, alpha, beta, bias_dt in runs:
            if name in G.ROUNDING and shape[2] < 2048:
                continue          # (K = 192: no value leaves bf16's exact range, see below)
            p = probes[(design, shape)]
            ref = G.expected(p, alpha, beta, bias_dt is not None, od)
            mut = G.mutant(name, p, alpha, beta, bias_dt is not None, od)
            n = int((ref != mut).sum())
            counts[(shape, design, od, alpha, beta)] = n
            assert n >= 1, (name, shape, design, od, alpha, beta)
            if name in ("drop_product", "drop_last_k") and design == "dense":
                assert np.abs(ref - mut).max() >= 0.5
    assert counts
    print(name, counts)


def test_rounding_mutants_need_values_beyond_256():
    """dense / bf16 shows the rounding mode only where |value| > 256: at K = 2048 thousands of elements, at K = 192 almost none (6 of
    98 304 values exceed 256 and 2 of them round differently under truncation: the branch cases with K <= 320 check indices in that
    run and the rounding mode next to not at all, as the module docstring says)"""
    p = G.build("dense", 256, 384, 192)
    ref = G.expected(p, 1.0, 0.0, True, "bf16")
    beyond = np.abs(G.expected(p, 1.0, 0.0, True, "f32")) > 256
    assert beyond.sum() < 20
    for name in G.ROUNDING:
        assert np.array_equal(G.mutant(name, p, 1.0, 0.0, True, "bf16")[~beyond], ref[~beyond])
    p = G.build("dense", 64, 576, 2048)
    ref = G.expected(p, 1.0, 0.0, True, "bf16")
    assert (G.mutant("truncate", p, 1.0, 0.0, True, "bf16") != ref).sum() > 1000
    assert (G.mutant("double_round", p, 1.0, 0.0, True, "bf16") != ref).sum() > 100


# ------------------------------------------------------------------------------------------------------------------ the gap
def _gaussian_case(torch, M, N, K):
    """operands as tests/test_gemm_dispatch_gpu.py draws them (0.5 N(0, 1) -> bf16; bias 0.3 N(0, 1) -> bf16; c0 0.2 N(0, 1)), on the CPU"""
    g = torch.Generator().manual_seed(11)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(torch.bfloat16).to(torch.float64).numpy()
    A, B = r(M, K), r(K, N)
    bias = (torch.randn(N, generator=g) * 0.3).to(torch.bfloat16).to(torch.float64).numpy()
    c0 = (torch.randn(M, N, generator=g) * 0.2).to(torch.bfloat16).to(torch.float64).numpy()
    return A, B, bias, c0


def _bf(torch, x):
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def test_what_the_old_rule_lets_through_at_k_8192():
    """The older tests compare bf16 outputs by  max|got - want| <= 6e-3 max|want|  on Gaussian operands.  At K = 8192 (max|want| = 111
    on this 256 x 2048 output, N as in the dispatch test's (1024, 2048, 8192) case) that allows an absolute error of 0.67 on every element.
    Measured here, as drawn (nothing about the inputs is bent):
                                  largest error   in allowances   elements inside the allowance
      drop the last k-element         2.50            3.8               97.0 %
      omit the bias                   1.25            1.9               97.8 %
      bias one column off             1.63            2.4               88.6 %
      ignore beta (= 1, bf16 C)       1.00            1.5               99.9 %
    So the estimate that these stay INSIDE the rule does not hold for its maximum norm: the largest of 524 288 elements carries each of
    them outside, by a factor of 1.5 to 3.8.  What the rule cannot see is the same error on most of the output: 89 to 99.9 % of the
    elements are individually inside, and the error confined to those elements -- a kernel that drops the bias, ignores beta or loses a
    k-element everywhere but on a few percent of the output -- passes.  Both halves are asserted.  (The fp32 paths of the older tests, at
    2e-5 of the maximum, do see all of these; they run beta = 1 without a bias.)"""
    torch = pytest.importorskip("torch")
    M, N, K = 256, 2048, 8192
    A, B, bias, c0 = _gaussian_case(torch, M, N, K)
    P = A @ B
    last = np.outer(A[:, -1], B[-1])
    want, want_beta = _bf(torch, P + bias), _bf(torch, P + c0)
    cases = {
        "drop_last_k": (want, _bf(torch, P - last + bias)),
        "no_bias": (want, _bf(torch, P)),
        "bias_shift": (want, _bf(torch, P + np.roll(bias, -1))),
        "ignore_beta": (want_beta, _bf(torch, P)),
    }
    for name, (ref, got) in cases.items():
        tol = 6e-3 * np.abs(ref).max()
        assert 0.6 < tol < 0.75, tol
        err = np.abs(got - ref)
        inside = err <= tol
        print(f"{name}: max error {err.max():.3f} = {err.max() / tol:.2f} allowances; {100 * inside.mean():.2f} % of the elements inside")
        assert tol < err.max() < 4 * tol, (name, err.max(), tol)        # seen as drawn, through the largest elements only
        assert inside.mean() > 0.88, (name, inside.mean())
        partial = np.where(inside, got, ref)                            # the same error on the elements where it is inside: passes
        assert (partial != ref).mean() > 0.5 and np.abs(partial - ref).max() <= tol, name
