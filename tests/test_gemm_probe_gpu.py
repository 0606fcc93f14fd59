"""The GEMM family against the exact integer probes of tests/gemm_probe.py: every row of tools/gemm_dispatch_table.BRANCH_CASES with a set
of epilogues, the pinned tile kernels and the ragged tails, the skinny kernel, batched products, the structural-zero hints and the head-bias
epilogue.  Every comparison is bit equality on the WHOLE output (tolerance zero: tests/test_gemm_probe_cpu.py shows why nothing rounds
except the one conversion to a bf16 output, and that every one-off error of the reference rule changes at least one element).

The reference is torch.matmul in float64 on the device, in row (and k) chunks whose temporaries stay under 1 GiB, with the epilogue applied
in float64 and ONE rounding to the output type.  Float64 sums of these integers are exact in any order, so the reference does not depend
on the BLAS algorithm; test_reference_equals_the_int64_product anchors it to numpy's int64 product.  The project's strided kernel is the
reference nowhere in this file.

Outputs are views into a canvas with a sentinel guard band on all four sides wherever the plan picks the same kernel for the strided view
as for a contiguous output (checked with gemm_kernel_choice); with beta = 0 the output is prefilled with NaN, so a finite and equal result
proves that C is not read.  The fp32 bias is accepted by every entry point that takes a bias (db1_gemm_strided and its nt / nn / tn forms);
gemm_batched (db1_gemm_strided_tri through ops) has no bias argument and db1_gemm_nt_headbias takes bf16 biases only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

torch = pytest.importorskip("torch")
import gemm_probe as G  # noqa: E402
import gemm_dispatch_table as gdt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
SENT = -32768.0                # the guard band's value (exact in bf16)
MAXEL = 1 << 26                # float64 elements per temporary of the reference: 512 MiB
LAYOUTS = ("nt", "nn", "tn")
TILE_KERNELS = ("tile128", "tile256", "pp-k64", "pp-k32", "w4", "w4n")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops as _ops, lib
    assert lib.load().db1_device_is_gfx950() == 1
    return _ops


# ------------------------------------------------------------------------------------------------------------------ operands
def _device_values(design, M, N, K, seed=0):
    """the rule of gemm_probe.build drawn on the device (shapes too large to build on the host): the same ranges, the same index formula"""
    d = G.DESIGNS[design]
    g = torch.Generator(device=DEV)
    g.manual_seed(1000003 * seed + 7 * M + 3 * N + K + (0 if design == "dense" else 1))
    if design == "dense":
        A = torch.randint(-d["a"], d["a"] + 1, (M, K), device=DEV, dtype=torch.int8, generator=g)
    else:
        s, grp = G.bounded_step(K, seed), K // G.NNZ
        pos = (torch.arange(M, device=DEV)[:, None] * s + torch.arange(G.NNZ, device=DEV)[None, :] * grp) % K
        sign = torch.randint(0, 2, (M, G.NNZ), device=DEV, dtype=torch.int8, generator=g) * 2 - 1
        A = torch.zeros(M, K, device=DEV, dtype=torch.int8).scatter_(1, pos, sign)
    B = torch.randint(-d["b"], d["b"] + 1, (K, N), device=DEV, dtype=torch.int8, generator=g)
    bias = torch.randint(-d["bias"], d["bias"] + 1, (N,), device=DEV, dtype=torch.int16, generator=g)
    c0 = lambda: torch.randint(-d["c0"] // 2, d["c0"] // 2 + 1, (M, N), device=DEV, dtype=torch.int16, generator=g).mul_(2)
    return A, B, bias, c0


_values = {}


def values(design, M, N, K, seed=0):
    """dict(A int8 [M, K], B int8 [K, N], bias float64 [N], c0() int16 [M, N]) on the device; the last two (design, shape) pairs are kept"""
    key = (design, M, N, K, seed)
    if key not in _values:
        while len(_values) >= 2:
            _values.pop(next(iter(_values)))
        if G.is_small(M, N, K):
            p = G.build(design, M, N, K, seed)
            A, B, bias = (torch.from_numpy(p[k]).to(DEV) for k in ("A", "B", "bias"))
            c0 = lambda p=p: torch.from_numpy(p["c0"]).to(DEV)
        else:
            A, B, bias, c0 = _device_values(design, M, N, K, seed)
        _values[key] = dict(A=A, B=B, bias=bias.double(), c0=c0, views={}, c0_cache=[])
    return _values[key]


def c0_of(v):
    if not v["c0_cache"]:
        v["c0_cache"].append(v["c0"]())
    return v["c0_cache"][0]


def stored(v, layout, dt=torch.bfloat16):
    """the operand views a [M, K], b [K, N] of one storage form: nt = x [M, K], W [N, K]; nn = dy [M, K], W [K, N]; tn = dy [K, M], x [K, N]"""
    if (layout, dt) not in v["views"]:
        A, B = v["A"].to(dt), v["B"].to(dt)
        a = A if layout != "tn" else A.t().contiguous().t()
        b = B.t().contiguous().t() if layout == "nt" else B
        v["views"] = {(layout, dt): (a, b)}
    return v["views"][(layout, dt)]


# ------------------------------------------------------------------------------------------------------------------ the reference
def ref_product(A8, B8, r0, r1, maxel=MAXEL):
    """rows r0 .. r1 of A . B in float64 (exact: integers far below 2^53), no temporary above `maxel` elements"""
    K, N = B8.shape
    kc = max(1, min(K, maxel // max(r1 - r0, N)))
    acc = None
    for k0 in range(0, K, kc):
        part = torch.matmul(A8[r0:r1, k0:k0 + kc].double(), B8[k0:k0 + kc].double())
        acc = part if acc is None else acc.add_(part)
    return acc


def finish(P, alpha, beta, bias, c0, od):
    """the epilogue in float64, then ONE rounding: every value is a multiple of 1/2 below 2^23, so float32 holds it exactly and the only
    rounding is float32 -> bf16 (round to nearest even); an fp32 output is not rounded at all"""
    v = P.mul(alpha)
    if beta != 0.0:
        v.add_(c0.double(), alpha=beta)
    if bias is not None:
        v.add_(bias)
    f = v.float()
    assert torch.equal(f.double(), v), "the exact value does not fit float32"
    return f.to(od)


def _where(m, n):
    return (f"tile256 ({m // 256}, {n // 256}) + ({m % 256}, {n % 256}); tile128 ({m // 128}, {n // 128}) + ({m % 128}, {n % 128}); "
            f"16 x 16 fragment ({m % 128 // 16}, {n % 128 // 16}) + ({m % 16}, {n % 16})")


def _k_report(A8, B8, m, n, diff, alpha):
    """which 64-wide k-tiles, lost or counted twice, explain the difference at (m, n)"""
    K = A8.shape[1]
    if K % 64:
        return ""
    part = (A8[m].double() * B8[:, n].double()).view(K // 64, 64).sum(1) * alpha
    lost = (part == -diff).nonzero().flatten().tolist() if diff != 0 else []
    twice = (part == diff).nonzero().flatten().tolist() if diff != 0 else []
    T = K // 64
    sl = lambda ts: [(t, {S: t * S // T for S in (2, 4, 8) if T % S == 0}) for t in ts[:8]]
    return f"; {T} k-tiles of 64 -- k-tiles whose loss explains it (tile, {{slices: slice}}): {sl(lost)}, counted twice: {sl(twice)}"


def assert_exact(got, A8, B8, alpha, beta, bias, c0, od, what, maxel=MAXEL):
    """torch.equal on every element of got [M, N] against the float64 reference, row chunk by row chunk"""
    M, N = got.shape
    rows = max(1, min(M, maxel // N))
    nbad, first = 0, None
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        want = finish(ref_product(A8, B8, r0, r1, maxel), alpha, beta, bias, None if c0 is None else c0[r0:r1], od)
        g = got[r0:r1]
        if torch.equal(g, want):
            continue
        ne = g != want                                   # (NaN differs from everything)
        nbad += int(ne.sum())
        if first is None:
            m, n = (int(x) for x in ne.nonzero()[0])
            gv, wv = float(g[m, n]), float(want[m, n])
            first = (f"first at (m, n) = ({r0 + m}, {n}): got {gv!r}, want {wv!r}; {_where(r0 + m, n)}"
                     + _k_report(A8, B8, r0 + m, n, gv - wv, alpha))
    assert nbad == 0, f"{what}: {nbad} of {M * N} elements differ; {first}"


class Output:
    """the output of one call: a view into a canvas with a sentinel band of one row above and below and eight columns left and right where
    `same_plan(view)` holds, else a contiguous tensor; filled with c0 (beta != 0) or NaN (beta = 0: C must not be read)"""

    def __init__(self, M, N, od, c0, same_plan):
        self.canvas = torch.full((M + 2, N + 16), SENT, device=DEV, dtype=od)
        self.t = self.canvas[1:M + 1, 8:8 + N]
        if not same_plan(self.t):
            self.canvas, self.t = None, torch.empty(M, N, device=DEV, dtype=od)   # (the plan takes another kernel for a strided C: contiguous)
        if c0 is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(c0)

    def intact(self, what):
        if self.canvas is None:
            return
        c = self.canvas
        for name, band in (("row above", c[0]), ("row below", c[-1]), ("columns left", c[:, :8]), ("columns right", c[:, -8:])):
            assert bool((band == SENT).all()), f"{what}: the guard {name} of the output was written"


def choice_of(ops, a, b, M, N, od, beta, ws_bytes, c_strides=None):
    out = torch.empty_strided((M, N), c_strides or (N, 1), dtype=od, device="meta")      # (strides and dtype only: nothing is allocated)
    return ops.gemm_kernel_choice(a, b, out, beta=beta, ws_bytes=ws_bytes)


def call_gemm(ops, a, b, out, bias, alpha, beta, offer="any"):
    """ops.gemm with the workspace the case offers ("none": the entry point is called without one)"""
    if offer != "none":
        return ops.gemm(a, b, out, bias=bias, alpha=alpha, beta=beta)
    from bdm_db1_amd import lib
    M, K = a.shape
    N = b.shape[1]
    lib.call("db1_gemm_strided", ops.P(a), ops.P(b), ops.P(out), ops.P(bias), M, N, K, ops.dt_code(a), ops.dt_code(b), ops.dt_code(out),
             ops.dt_code(bias) if bias is not None else 0, a.stride(0), a.stride(1), b.stride(0), b.stride(1), out.stride(0), out.stride(1),
             1, 1, 0, 0, 0, 0, 0, 0, alpha, beta, None, 0, ops.stream())


def run_epilogue(ops, shape, layout, epi, offer="any", expect=None, seed=0, operands=torch.bfloat16):
    """one exact product through ops.gemm; returns the plan's choice (asserted against `expect(od, beta)` if given)"""
    M, N, K = shape
    design, odn, alpha, beta, bias_dt = epi
    od = TD[odn]
    G.check(design, M, N, K, alpha, beta, bias_dt is not None)
    v = values(design, M, N, K, seed)
    a, b = stored(v, layout, operands)
    ws = {"any": -1, "none": 0}[offer]
    choice = choice_of(ops, a, b, M, N, od, beta, ws)
    if expect is not None:
        assert choice == expect(odn, beta), (shape, layout, epi, choice)
    c0 = c0_of(v) if beta != 0.0 else None
    out = Output(M, N, od, None if c0 is None else c0.to(od), lambda t: choice_of(ops, a, b, M, N, od, beta, ws, t.stride()) == choice)
    bias = None if bias_dt is None else v["bias"].to(TD[bias_dt])
    what = f"{M}x{N}x{K} {layout} {design}->{odn} alpha={alpha} beta={beta} bias={bias_dt} [{choice[0]}{' split-K' if choice[1] else ''}{' +tail' if choice[2] else ''}{'' if out.canvas is not None else ', contiguous C'}]"
    call_gemm(ops, a, b, out.t, bias, alpha, beta, offer)
    assert_exact(out.t, v["A"], v["B"], alpha, beta, None if bias is None else v["bias"], c0, od, what)
    out.intact(what)
    print(what, "exact")
    return choice


# ------------------------------------------------------------------------------------------------------------------ the anchor
@pytest.mark.parametrize("design", ["dense", "bounded"])
def test_reference_equals_the_int64_product(ops, design):
    """the float64 device reference (chunked, both chunk loops forced to several steps) and both operand generators against numpy's int64
    product and gemm_probe.expected at (256, 384, 192)"""
    M, N, K = 256, 384, 192
    p = G.build(design, M, N, K)
    A, B = torch.from_numpy(p["A"]).to(DEV), torch.from_numpy(p["B"]).to(DEV)
    P64 = np.einsum("mk,kn->mn", p["A"].astype(np.int64), p["B"].astype(np.int64))
    for maxel in (MAXEL, N * 100, N * 7):          # one chunk; 100 rows x 100 k; 7 rows
        rows = max(1, min(M, maxel // N))
        got = torch.cat([ref_product(A, B, r0, min(M, r0 + rows), maxel) for r0 in range(0, M, rows)])
        assert np.array_equal(got.cpu().numpy(), P64.astype(np.float64))
    bias, c0 = torch.from_numpy(p["bias"]).to(DEV).double(), torch.from_numpy(p["c0"]).to(DEV)
    for _, odn, alpha, beta, bias_dt in G.EPILOGUES:
        want = G.expected(p, alpha, beta, bias_dt is not None, odn)
        got = finish(ref_product(A, B, 0, M), alpha, beta, bias if bias_dt else None, c0, TD[odn])
        assert np.array_equal(got.double().cpu().numpy(), want)
        assert_exact(torch.from_numpy(want).to(DEV).to(TD[odn]), A, B, alpha, beta, bias if bias_dt else None, c0, TD[odn], "anchor", N * 50)
    wrong = torch.from_numpy(G.mutant("drop_last_k", p, out_dtype="f32")).to(DEV).float()
    with pytest.raises(AssertionError, match="elements differ; first at"):
        assert_exact(wrong, A, B, 1.0, 0.0, bias, None, torch.float32, "mutant")
    # the device generator draws the same designs: ranges, 32 nonzeros per row at the formula's positions, full coverage
    Ad, Bd, biasd, c0d = _device_values(design, M, N, K)
    d = G.DESIGNS[design]
    assert int(Ad.abs().max()) == d["a"] and int(Bd.abs().max()) == d["b"] and int(biasd.abs().max()) <= d["bias"]
    c = c0d()
    assert int(c.abs().max()) <= d["c0"] and not bool((c % 2).any()) and c.unique().numel() > d["c0"] // 2
    if design == "bounded":
        assert np.array_equal((Ad != 0).cpu().numpy(), p["A"] != 0)
    else:
        assert not torch.equal(Ad[:192, :192], Ad[:192, :192].t())
    assert np.array_equal(ref_product(Ad, Bd, 0, M).cpu().numpy(), (Ad.cpu().numpy().astype(np.int64) @ Bd.cpu().numpy().astype(np.int64)).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ a. every plan branch
def _case_id(c):
    return "%dx%dx%d-%s-%s-%s" % (c[0] + (c[1], "%s%d" % c[4] if c[4] else "default", c[5]))


def _epi_id(e):
    return "%s-%s-a%g-b%g-%s" % (e[0], e[1], e[2], e[3], e[4] or "nobias")


# (every case runs all seven epilogues: the largest, 65536 x 8192 x 2048 and K = 32768, take about 0.05 s per id on an MI355X, reference included)
BRANCH_RUNS = [pytest.param(c, e, id=_case_id(c) + "-" + _epi_id(e)) for c in gdt.BRANCH_CASES for e in G.EPILOGUES]


@pytest.mark.parametrize("case,epi", BRANCH_RUNS)
def test_every_plan_branch_is_exact(ops, case, epi):
    """each branch of gemm_plan with its knob and workspace offer.  No epilogue of the set changes the plan's choice at these cases, so the
    choice the case names is asserted for every one of them, twice: from the C ABI's plan query on contiguous strides and from
    gemm_kernel_choice on the operands that are passed (the fp32 outputs with beta = 1 of the 64 x 576 x 8192 case also take tile128's k-split
    through the workspace, which the choice code does not show)"""
    from bdm_db1_amd import lib
    shape, layout, dname, cbeta, knob, offer, want_choice = case
    try:
        if knob:
            lib.set_knob(*knob)
        ops._ws_query_cache.clear()          # (the workspace query depends on the knobs)

        def expect(odn, beta):
            code, _ = gdt.query(lib.load(), shape, layout, dict(gdt.DTC)[odn], (1, 1), beta, offer)
            planned = (gdt.KERNELS[code & 15], bool(code & 16), bool(code & 32))
            assert planned == want_choice, (case, odn, beta, planned)
            return planned

        run_epilogue(ops, shape, layout, epi, offer, expect)
    finally:
        lib.load().db1_test_clear_knobs()
        ops._ws_query_cache.clear()


# ------------------------------------------------------------------------------------------------------------------ b. pinned tiles, tails
SMALL_EPILOGUES = tuple(e for e in G.EPILOGUES if (e[0], e[1]) != ("dense", "bf16"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tile", [256, 512, 1024])
@pytest.mark.parametrize("shape", G.LARGE_TILE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_pinned_tile_kernels_are_exact(ops, layout, tile, shape):
    """the 256 x 128 and 256 x 256 kernels pinned through the ABI hook (the shapes of test_gemm_bf16_large_tile_kernels): 1, odd and even
    k-tile counts, the hand-scheduled 4-wave loops from K = 256 on"""
    ops.gemm_tile_override(tile)
    try:
        kernels = {run_epilogue(ops, shape, layout, e)[0] for e in SMALL_EPILOGUES}
        assert kernels <= set(TILE_KERNELS[1:]), kernels
    finally:
        ops.gemm_tile_override(0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", G.TAIL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tile_tails_are_exact(ops, layout, shape):
    """ragged M / N on the MFMA tile kernels (clamped loads, masked stores): the five shapes of test_gemm_bf16_tile_tails in every layout
    that fast_ok admits for them -- all three (M % 8 == 0 for the M-major A of tn, N % 8 == 0, leading dimensions % 8 == 0)"""
    from bdm_db1_amd import lib
    M, N, K = shape
    st = gdt.strides(layout, M, N, K)
    assert lib.load().db1_gemm_would_use_fast(M, N, K, 1, 1, 0, *st) == 1
    kernels = {run_epilogue(ops, shape, layout, e)[0] for e in SMALL_EPILOGUES}
    assert kernels <= {"tile128", "tile256"}, kernels


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_strided_kernel_is_exact(ops, layout, operands):
    """the strided fp32-MFMA kernel, which the other GEMM tests use as their reference: where the plan has no tile kernel -- the odd shape
    of test_gemm_strided_odd_shapes, 70 x 130 x 37, with bf16 and with fp32 operands (the integers are exact in both; K = 37 admits the
    dense design only) -- and forced through the test hook at 256 x 384 x 192, every epilogue of the set"""
    for e in (e for e in G.EPILOGUES if e[0] == "dense"):
        assert run_epilogue(ops, G.STRIDED_ODD, layout, e, operands=TD[operands]) == ("strided-fp32", False, False)
    if operands == "bf16":
        ops.gemm_force_generic(True)
        try:
            for e in G.EPILOGUES:
                assert run_epilogue(ops, (256, 384, 192), layout, e) == ("strided-fp32", False, False)
        finally:
            ops.gemm_force_generic(False)


# ------------------------------------------------------------------------------------------------------------------ c. skinny
@pytest.mark.parametrize("M", G.SKINNY_M)
@pytest.mark.parametrize("N,K", G.SKINNY_NK)
def test_skinny_is_exact(ops, M, N, K):
    """y = x W^T with 1 .. 64 rows, alpha = 1/2, beta = 1 and bias, both output types.  `bounded` covers only M of each K / 32 = 64 rows
    here -- every k only at M = 64 -- so the lost-product cases rest on dense / fp32; dense / bf16 adds the one rounding (half-integers)"""
    for design, odn in (("dense", "f32"), ("dense", "bf16"), ("bounded", "bf16")):
        choice = run_epilogue(ops, (M, N, K), "nt", (design, odn, 0.5, 1.0, "bf16"))
        assert choice == ("skinny", False, False), choice


# ------------------------------------------------------------------------------------------------------------------ d. batched, hints
def _batched_choice(ops, a, b, out, beta):
    from bdm_db1_amd import lib
    Z0, Z1, M, K = a.shape
    N = b.shape[3]
    code = lib.load().db1_gemm_kernel_choice(M, N, K, ops.dt_code(a), ops.dt_code(b), ops.dt_code(out), a.stride(2), a.stride(3), b.stride(2), b.stride(3),
                                             out.stride(2), out.stride(3), Z0, Z1, float(beta), -1)
    return ops.GEMM_KERNELS[code & 15], bool(code & 16), bool(code & 32)


def _assert_equal(got, want, what):
    if not torch.equal(got, want):
        ne = got != want
        idx = tuple(int(x) for x in ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {got.numel()} elements differ; first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}; "
                             + _where(idx[-2], idx[-1]))


@pytest.mark.parametrize("design,odn,alpha,beta", [("dense", "f32", 1.0, 0.0), ("dense", "f32", 0.5, 1.0), ("bounded", "bf16", 1.0, 0.0), ("bounded", "bf16", 1.0, 0.5)])
def test_batched_broadcast_is_exact(ops, design, odn, alpha, beta):
    """a (2, 3) batch of 128 x 128 x 1024 products with B broadcast over z0 (stride 0) and read as strided slices of one [K, 3 x 128] matrix"""
    Z0, Z1, M, N, K = G.BATCHED[0]
    p = G.build(design, Z0 * Z1 * M, Z1 * N, K)
    G.check(design, M, N, K, alpha, beta, False)
    od = TD[odn]
    A8, B8 = torch.from_numpy(p["A"]).to(DEV), torch.from_numpy(p["B"]).to(DEV)
    a = A8.to(torch.bfloat16).view(Z0, Z1, M, K)
    b = B8.to(torch.bfloat16).view(K, Z1, N).permute(1, 0, 2).unsqueeze(0).expand(Z0, Z1, K, N)
    assert b.stride(0) == 0 and b.stride(1) == N and b.stride(2) == Z1 * N
    c0 = torch.from_numpy(np.ascontiguousarray(p["c0"][:, :N])).to(DEV).view(Z0, Z1, M, N)
    out = c0.to(od) if beta != 0.0 else torch.full((Z0, Z1, M, N), float("nan"), device=DEV, dtype=od)
    ops.gemm_batched(a, b, out, alpha=alpha, beta=beta)
    P = torch.einsum("xymk,kyn->xymn", A8.view(Z0, Z1, M, K).double(), B8.view(K, Z1, N).double())
    _assert_equal(out, finish(P, alpha, beta, None, c0, od), f"batched {design}->{odn} beta={beta} {_batched_choice(ops, a, b, out, beta)}")


@pytest.mark.parametrize("design,odn,alpha,beta", [("dense", "f32", 0.5, 1.0), ("bounded", "bf16", 1.0, 0.0), ("bounded", "bf16", 1.0, 0.5), ("dense", "bf16", 1.0, 0.0)])
def test_batched_split_k_is_exact(ops, design, odn, alpha, beta):
    """nb = 2 products of 1024 x 128 x 8192 with M-major operands: the workspace split-K as a batch (partials + the fixed-order reduce), the
    reduce's bf16 output with and without beta"""
    nb, _, M, N, K = G.BATCHED[1]
    G.check(design, M, N, K, alpha, beta, False)
    od = TD[odn]
    ps = [G.build(design, M, N, K, seed=z) for z in range(nb)]
    A8 = torch.stack([torch.from_numpy(p["A"]) for p in ps]).to(DEV)
    B8 = torch.stack([torch.from_numpy(p["B"]) for p in ps]).to(DEV)
    a = A8.to(torch.bfloat16).transpose(1, 2).contiguous().transpose(1, 2).unsqueeze(1)      # stored [nb, K, M]
    b = B8.to(torch.bfloat16).unsqueeze(1)
    c0 = torch.stack([torch.from_numpy(p["c0"]) for p in ps]).to(DEV).unsqueeze(1)
    out = c0.to(od) if beta != 0.0 else torch.full((nb, 1, M, N), float("nan"), device=DEV, dtype=od)
    choice = _batched_choice(ops, a, b, out, beta)
    assert choice[1], f"the batched case no longer takes the split-K: {choice}"
    ops.gemm_batched(a, b, out, alpha=alpha, beta=beta)
    for z in range(nb):
        assert_exact(out[z, 0], A8[z], B8[z], alpha, beta, None, c0[z, 0] if beta != 0.0 else None, od, f"batched split-K z={z} {design}->{odn} beta={beta} {choice}")


def _ints(shape, amp, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-amp, amp + 1, shape, dtype=np.int8)).to(DEV)


@pytest.mark.parametrize("H,B,L", G.HINT_GEOMETRIES, ids=lambda x: str(x))
@pytest.mark.parametrize("odn", ["f32", "bf16"])
def test_structural_zero_hints_are_exact(ops, odn, H, B, L):
    """the two contractions over dT (zero above the causal diagonal: a dense probe masked to the structure) with and without the k-tile
    skipping hints: BOTH calls equal the exact reference (fp32: the exact integers; bf16: rounded once).  The hinted calls read an A whose
    skipped region holds NaNs."""
    D, od = 128, TD[odn]
    G.check("dense", L, D, B * L)
    i = torch.arange(L, device=DEV)[:, None]
    dd = torch.arange(L, device=DEV)[None, :]
    dT = _ints((H, B, L, L), 3, [17, H, B, L]).masked_fill_(dd > i, 0)
    R, qv = _ints((L, H, D), 3, [18, H, L]), _ints((B, L, H, D), 3, [19, H, B, L])
    ref_dq = torch.einsum("hbik,khd->bihd", dT.double(), R.double()).float().to(od)
    ref_dR = torch.einsum("hbik,bihd->khd", dT.double(), qv.double()).float().to(od)
    Rb, qvb = R.to(torch.bfloat16), qv.to(torch.bfloat16)
    plain = dT.to(torch.bfloat16)
    poison1 = plain.clone().masked_fill_((dd // 64) * 64 > (i // 256) * 256 + 255, float("nan"))     # mode 1 never touches k-tiles right of the 256-row tile
    poison2 = plain.clone().masked_fill_((i // 64) * 64 + 63 < (dd // 256) * 256, float("nan"))      # mode 2 never touches query k-tiles above the 256-distance tile
    for src, tri in ((plain, (0, 0)), (poison1, (1, 0))):
        dq = torch.full((B, L, H, D), float("nan"), device=DEV, dtype=od)
        ops.gemm_batched(src, Rb.permute(1, 0, 2).unsqueeze(1).expand(H, B, L, D), dq.permute(2, 0, 1, 3), tri=tri)
        _assert_equal(dq, ref_dq, f"dq_r hint {tri}")
    for src, tri in ((plain, (0, 0)), (poison2, (2, L))):
        dR = torch.full((L, H * D), float("nan"), device=DEV, dtype=od)
        ops.gemm_batched(src.view(H, B * L, L).transpose(1, 2).unsqueeze(1), qvb.view(B * L, H, D).permute(1, 0, 2).unsqueeze(1),
                         dR.view(L, H, D).permute(1, 0, 2).unsqueeze(1), tri=tri)
        _assert_equal(dR.view(L, H, D), ref_dR, f"dR hint {tri}")


# ------------------------------------------------------------------------------------------------------------------ e. head bias
@pytest.mark.parametrize("M,d,K", G.HEADBIAS)
def test_head_bias_epilogue_is_exact(ops, M, d, K):
    """db1_gemm_nt_headbias on the bounded design (every result an integer bf16 holds): qu, qv and out[:, d:] exact, out[:, :d] untouched;
    (4096, 2048, 512) is the 256 x 128 form, (4096, 1024, 512) -- 16 x 12 tiles, admitted by ..._supported -- the 256 x 256 one"""
    N = 3 * d
    assert ops.gemm_nt_headbias_supported(M, N, K, d)
    assert G.check("bounded", M, N, K, 1.0, 0.0, True) + 1 <= 256
    v = values("bounded", M, N, K)
    x, wt = stored(v, "nt")
    rng = np.random.default_rng([5, M, d, K])
    bu = rng.integers(-32, 33, d)
    bv = rng.integers(-32, 33, d)
    bv = np.where(bv == bu, bu + 1, bv)                     # the two biases differ in every column (|bv| <= 33)
    assert (bu != bv).all()
    bu_d, bv_d = torch.from_numpy(bu).to(DEV).double(), torch.from_numpy(bv).to(DEV).double()
    out = torch.full((M, N), SENT, device=DEV, dtype=torch.bfloat16)
    qu = torch.full((M, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    qv = torch.full((M, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt_headbias(x, wt.t(), out, qu, qv, bu_d.to(torch.bfloat16), bv_d.to(torch.bfloat16), d)
    A8, B8 = v["A"], v["B"]
    assert_exact(qu, A8, B8[:, :d], 1.0, 0.0, bu_d, None, torch.bfloat16, "head bias qu")
    assert_exact(qv, A8, B8[:, :d], 1.0, 0.0, bv_d, None, torch.bfloat16, "head bias qv")
    assert_exact(out[:, d:], A8, B8[:, d:], 1.0, 0.0, None, None, torch.bfloat16, "head bias k, v columns")
    assert bool((out[:, :d] == SENT).all()), "the query columns of the packed output were written"
