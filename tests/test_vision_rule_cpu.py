"""The rule of tests/vision_rule.py proved usable without a GPU: its float64 references agree with the project's oracle, every exact probe
meets its exactness condition and an fp32 transcription in two shuffled term orders reproduces the expected bits, the fp32 model of every
bounded kernel stays under half of every bound, and every one-mistake mutant is caught in every case it applies to (exact kernels: a
differing bit pattern; bounded kernels: an element moved by ten bounds)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stream_rule as S  # noqa: E402
import vision_rule as V  # noqa: E402
from oracle import db1_oracle as O  # noqa: E402

EXACT = V.cases(*V.EXACT_KINDS)
BOUNDED = V.cases(*V.BOUNDED_KINDS)
ids = lambda cs: [c["id"] for c in cs]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ------------------------------------------------------------------------------------------------ 1. the references against the oracle
def test_references_agree_with_the_oracle():
    rng = np.random.default_rng(5)
    N, C, p = 3, 6, 5
    x, w, b = rng.standard_normal((N, C, p, p)), rng.standard_normal((4, C, 3, 3)), rng.standard_normal(4)
    cl = lambda a: a.reshape(a.shape[0], a.shape[1], -1).transpose(0, 2, 1)                  # NCHW -> [N, p p, C]
    cols = O._im2col3x3(x).reshape(N * p * p, C * 9)
    assert rel(V.ref_im2col(x, "nchw", C * 9 + 3)[:, :C * 9], cols) < 1e-12
    assert rel(V.ref_im2col(cl(x), "nhwc", C * 9), cols.reshape(-1, C, 9).transpose(0, 2, 1).reshape(-1, 9 * C)) < 1e-12
    dcols = rng.standard_normal((N, p, p, C * 9))
    want = O._col2im3x3(dcols, C)
    assert rel(V.ref_col2im(dcols.reshape(-1, C * 9), "nchw", N, C, p), want) < 1e-12
    tapmajor = dcols.reshape(-1, C, 9).transpose(0, 2, 1).reshape(-1, 9 * C)
    assert rel(V.ref_col2im(tapmajor, "nhwc", N, C, p), cl(want)) < 1e-12
    # convolution, data gradient, weight and bias gradient (the oracle's go through the column matrix; these do not)
    y_ref, ocols = O.conv3x3_fwd(x, w, b)
    fwd = dict(mode="fwd")
    assert rel(V.conv_core(cl(x), V.conv_Wk(fwd, w), 1) + b, cl(y_ref)) < 1e-12
    dy = rng.standard_normal((N, 4, p, p))
    dx_ref, dw_ref, db_ref = O.conv3x3_bwd(dy, w, ocols)
    assert rel(V.conv_core(cl(dy), V.conv_Wk(dict(mode="dgrad"), w), -1), cl(dx_ref)) < 1e-12
    assert rel(V.ref_permute(w, 9 * C + 2)[:, :9 * C], w.reshape(4, C, 9).transpose(0, 2, 1).reshape(4, -1)) == 0
    assert rel(V.ref_unpermute(V.ref_permute(w, 9 * C + 2), np.zeros_like(w)), w) == 0
    assert rel(V.ref_permute_t(w).reshape(C, 9, 4), w.reshape(4, C, 9).transpose(1, 2, 0)) == 0
    # (the 64-channel weight-gradient reference on a random probe against the oracle's)
    x64, dy64 = rng.standard_normal((2, 64, 16, 16)), rng.standard_normal((2, 64, 16, 16))
    case = dict(kind="wgrad", N=2, form="patch", ks_knob=0, gbias=True)
    got = V.ref_wgrad(case, dict(x=cl(x64), dy=cl(dy64), g0=np.zeros((64, 576)), b0=np.zeros(64)))
    _, dw64, db64 = O.conv3x3_bwd(dy64, np.zeros((64, 64, 3, 3)), O._im2col3x3(x64), need_dx=False)
    assert rel(V.ref_unpermute(got["gp"], np.zeros((64, 64, 3, 3))), dw64) < 1e-12 and rel(got["gb"], db64) < 1e-12
    # conv1 through the same pieces
    x3, w3 = rng.standard_normal((2, 3, 16, 16)), rng.standard_normal((64, 3, 3, 3))
    wp = np.concatenate([V.ref_permute(w3, 27), np.ones((64, 5))], 1)
    c1 = V.ref_conv1(dict(kind="conv1", N=2), dict(x=cl(x3), wp=wp, bias=None))
    assert rel(c1["y"].reshape(2, 256, 64), cl(O.conv3x3_fwd(x3, w3, 0.0)[0])) < 1e-12 and (c1["cols"][:, 27:] == 0).all()
    # patch normalise
    img = rng.random((2, 3, 32, 48)) * 255
    pc = dict(kind="pnorm", layout="nchw", p=16, dto="f32")
    assert rel(V.expect_pnorm(pc, dict(x=img))["out"][0], O.patch_normalize(O.patchify(img, 16), 16).reshape(-1, 3, 256)) < 1e-12
    # GroupNorm + GELU forward and backward
    gc = dict(kind="gn", layout="nchw", dt="f32", pdt="f32", N=3, C=64, hw=256, groups=32, res=False)
    gi = {k: (np.asarray(v, np.float64) if v is not None else None) for k, v in V.inputs(dict(gc, id="oracle")).items()}
    h, cache = O.groupnorm_fwd(gi["x"].reshape(3, 64, 16, 16), gi["gamma"], gi["beta"])
    stats = dict(mean=gi["x"].reshape(96, -1).mean(1), rstd=cache[1].reshape(-1))
    e = V.expect_gn(gc, gi, stats)
    assert rel(e["y"][0], O.gelu(h).reshape(3, 64, 256)) < 1e-12 and rel(e["rstd"][0], cache[1].reshape(-1)) < 1e-12
    dxr, dgr, dbr = O.groupnorm_bwd(gi["dy"].reshape(3, 64, 16, 16) * O.gelu_grad(h), gi["gamma"], cache)
    assert rel(e["dx"][0], dxr.reshape(3, 64, 256)) < 1e-12
    assert rel(e["dgamma"][0] - gi["dg0"], dgr) < 1e-12 and rel(e["dbeta"][0] - gi["db0"], dbr) < 1e-12


def test_shuffle_reference_is_the_transpose():
    case = V.BY_ID["shuffle-nchw-f32-N2-C33-hw31"]
    inp = V.inputs(case)
    assert np.array_equal(V.reference(case, inp)["y"], inp["x"].transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_exact_probe_is_exact_in_any_order(case):
    inp = V.inputs(case)
    assert V.representable(case, inp), "an input is not a grid value of its storage type"
    units = V.sumabs_units(case, inp)
    assert units < 2 ** 24, f"sum of |terms| = {units} grid units: partial sums are not exact in fp32"
    if not V.cheap(case):
        return
    want = V.expected(case, inp)
    for name, v in want.items():
        assert not (v == V.SENT).any(), f"{name}: an expected value equals the sentinel"
    for seed in (1, 2):
        got = V.exact_model(case, inp, seed)
        for name, v in want.items():
            assert np.array_equal(bits(got[name]).reshape(-1), bits(v).reshape(-1)), f"{case['id']} {name}: the fp32 model in term order {seed} gives other bits"


# ------------------------------------------------------------------------------------------------ 3. bounds of the non-exact kernels
def run_bounded(case, mutant=None, share=1.0):
    inp = V.inputs(case)
    got = V.model(case, inp, mutant)
    S.SHARE = share
    try:
        with np.errstate(all="ignore"):
            return got, V.expect(case, inp, got)
    finally:
        S.SHARE = 1.0


@pytest.mark.parametrize("case", BOUNDED, ids=ids(BOUNDED))
def test_model_within_half_of_every_bound(case):
    got, exp = run_bounded(case, share=V.HEADROOM)
    for name, (ref, bnd) in exp.items():
        V.check(got[name], ref, bnd, f"{case['id']} {name} (fp32 allowance x {V.HEADROOM})")
        assert np.all(np.abs(np.asarray(ref, np.float64) - V.SENT) > bnd), f"{case['id']} {name}: a reference value within its bound of the sentinel"
    if case["kind"] == "pnorm" and case["const"]:
        ref, bnd = exp["out"]
        sel = (0, 0) if case["layout"] == "nchw" else (0, slice(None), 0)
        assert (ref[sel] == 0).all() and (bnd[sel] == 0).all(), "the constant patch's reference is exactly 0, with no allowance"
        assert (got["out"][sel] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. mutants
@pytest.mark.parametrize("case", V.CASES, ids=ids(V.CASES))
def test_every_applicable_mutant_is_caught(case):
    """exact kernels: at least one expected bit pattern differs; bounded kernels: an element moves by ten bounds.  (Per case, so that a
    case's own reference is computed once; a case no mutant applies to fails here.)"""
    ms = [m for m in V.MUTANTS if V.applicable(m, case)]
    assert ms, f"no mutant applies to {case['id']}"
    if case["kind"] in V.EXACT_KINDS:
        inp = V.inputs(case)
        want = V.expected(case, inp)
        for m in ms:
            bad = V.expected(case, inp, m)
            n = sum(int((bits(want[k]) != bits(bad[k])).sum()) for k in want)
            assert n > 0, f"{m} is not caught by {case['id']}: {n} bit patterns differ"
        return
    for m in ms:
        got, exp = run_bounded(case, m)
        worst = max(float(V.ratio(got[name], ref, bnd).max()) for name, (ref, bnd) in exp.items())
        assert worst >= V.MARGIN, f"{m} is not caught by {case['id']}: worst ratio {worst:.2f} (needs {V.MARGIN})"


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_every_mutant_applies_somewhere(mutant):
    hit = [c["id"] for c in V.CASES if V.applicable(mutant, c)]
    print(f"{mutant}: judged in {len(hit)} cases")
    assert hit, f"{mutant} applies to no case of the table"


def test_table_reaches_every_branch():
    """the dispatcher arithmetic restated in the rule selects what the table claims"""
    ks = {(c["N"], c["ks_knob"]): V.wgrad_ksplit(c["N"], c["ks_knob"]) for c in V.cases("wgrad") if c["form"] == "tile"}
    assert ks == {(1, 0): 1, (3, 0): 1, (128, 0): 51, (255, 0): 102, (256, 0): 102, (257, 0): 102, (513, 0): 102, (37, 7): 7}
    assert (4 * 255) % 102 == 0 and (4 * 256) % 102 != 0 and (4 * 128) % 51 != 0 and (4 * 37) % 7 != 0
    paths = {(c["kind"], c["dt"], V.vec_path(c), c["kpad"] > 9 * c["C"], bool(c.get("unaligned"))) for c in V.cases("im2col", "col2im") if c["layout"] == "nhwc"}
    for kind in ("im2col", "col2im"):
        for dt in ("f32", "bf16"):
            assert {(kind, dt, True, False, False), (kind, dt, True, True, False), (kind, dt, False, True, False), (kind, dt, False, True, True)} <= paths
    big = [c for c in V.cases("im2col", "col2im") if V.stream_items(c) > V.GRID_CAP]
    assert {(c["kind"], c["layout"]) for c in big} == {("im2col", "nchw"), ("col2im", "nchw"), ("im2col", "nhwc"), ("col2im", "nhwc")}
    assert all(V.stream_items(c) < 2 * V.GRID_CAP for c in big)
    assert {c["C"] // c["groups"] for c in V.cases("gn") if c["layout"] == "nhwc"} == {1, 2, 4, 8, 16, 64}
