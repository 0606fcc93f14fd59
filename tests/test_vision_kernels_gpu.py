"""The image-patch embedder kernels (csrc/vision.hip, csrc/conv_implicit.hip) at every dispatch branch and edge, through bdm_db1_amd.ops,
under the rule of tests/vision_rule.py (proved usable by test_vision_rule_cpu.py).  The exact kernels -- the three convolution forms, conv1,
both im2cols and col2ims, the permutes, the un-permute, the shuffles -- are compared BIT FOR BIT with the correctly rounded float64 result of
dyadic-grid probes; patch normalise and GroupNorm + GELU per element against counted bounds.  Every output and accumulator lies in a Guarded
allocation pre-filled with the sentinel; the inputs of the persistent kernels too, and every N > 256 case runs twice with different values
behind its inputs and must give the same bits.

branch -> case id (the ids of vision_rule.CASES; * = every value of the table)
  conv_patch_kernel<bf16_t> / <float> (bias f32 or none)      conv-fwd-N*-bf16-* / conv-fwd-N*-f32-*, conv-fwd-N*--*, conv-dgrad-*     [knob conv_patch = 1]
  conv_implicit_kernel<bf16_t> / <float>, res path and not    the same cases                                                             [knob conv_patch = 0]
  fewer patches than workgroups / one each / extra patch      N1, N3, N255 / N256 / N257, N513
  conv_wgrad_patch_kernel + reduce                            wgrad-patch-N*            (gbias None: wgrad-patch-N255-*)
  conv_wgrad_implicit_kernel + reduce                         wgrad-tile-N*             (gbias None: wgrad-tile-N3-*)
    ci_wgrad_ksplit: ks = 1 / halved to 51 / 102 even / 102 with a remainder and empty ranges / conv_wgrad_ks = 7
                                                              N1, N3 / N128 / N255 / N256, N257, N513 / wgrad-tile-N37-ks_knob7-*
  conv1_fused_kernel<bf16_t> / <float> (f32 bias, no bias)    conv1-N*-bf16 / conv1-N*-f32, conv1-N*-
  im2col_kernel<T>, col2im_kernel<T>                          im2col-nchw-*, col2im-nchw-*;  second grid-stride pass: -N200-C5-, -N130-C64-
  im2col_nhwc_kernel<T, 16 / sizeof T>, col2im_nhwc likewise  *-nhwc-*-C64-p16-kpad576, *-nhwc-*-C8-p16-kpad80 (+ zero_pad_cols_kernel)
  im2col_nhwc_kernel<T, 1>, col2im_nhwc_kernel<T, 1>          by shape: *-C3-p16-kpad32, *-C8-p16-kpad76;  by alignment: *-C8-p16-kpad80-unaligned1
  vis_grid cap                                                im2col-nhwc-bf16-N120-C64-*, col2im-nhwc-bf16-N2800-C3-* (scalar path)
  conv_weight_permute_kernel<TI, TO>, ..._t_kernel<TI, TO>    permute-*, permute_t-* (the four dtype pairs, Cin = 64 and 3)
  conv_wgrad_unpermute_kernel                                 unpermute-*
  nhwc_nchw_kernel<T, TO_NCHW>                                shuffle-*; partial 32 x 33 tiles: -N2-C33-hw31, -N1-C1-hw1; second gridDim.z chunk: -N65538-
  patch_normalize(_nhwc)_kernel<TI, TO>                       pnorm-nchw-*, pnorm-nhwc-* (four dtype pairs; p = 16, 3, 10, 8; the constant patch: -const1)
  gn_gelu_nhwc_kernel<bf16_t, bf16_t / float, fwd / bwd>      gn-nhwc-bf16-bf16-*, gn-nhwc-bf16-f32-* (cpg 1, 2, 4, 8, 16, 64; res given and not)
  gn_gelu_fwd / bwd / param_grad_kernel<T, TP>                gn-nchw-* (the four dtype pairs; (64, 256, 32), (6, 10, 3), (4, 1, 4));
                                                              gn_param_grad_kernel is launched unconditionally: no condition to stand on either side of
Left out: the vis_grid cap on col2im's VECTOR path needs about 300 MB of columns."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stream_rule as S  # noqa: E402
import vision_rule as V  # noqa: E402
from gpu_common import DEV, TD, Guarded, dev, host  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops as _ops, lib
    assert lib.load().db1_device_is_gfx950() == 1
    return _ops


def ids(cs):
    return [c["id"] for c in cs]


def knobs(**kw):
    """context: the library's thread-local A/B knobs set for the block, cleared after it"""
    from bdm_db1_amd import lib

    class K:
        def __enter__(self):
            for k, v in kw.items():
                lib.set_knob(k, v)

        def __exit__(self, *a):
            lib.load().db1_test_clear_knobs()
    return K()


def placed(a, dt, cols=None, off=0, behind=None):
    """a (as [rows, cols]) inside a Guarded allocation; ``behind``: what the margins hold instead of the sentinel (inputs only)"""
    a2 = np.reshape(a, (-1, cols or a.shape[-1]))
    g = Guarded(a2.shape[0], a2.shape[1], dt, fill=a2, off=off)
    if behind is not None:
        g.buf[:g.start] = behind
        g.buf[g.start + g.rows * g.ld:] = behind
    return g


def same_bits(name, got, want, dt, shape=None):
    """torch.equal on the bit view; on failure the first differing index (of ``shape``, e.g. (patch, pixel, channel)) and the count"""
    w = dev(np.reshape(want, tuple(got.shape)), dt)
    bits = torch.int16 if dt == "bf16" else torch.int32
    if torch.equal(got.contiguous().view(bits), w.view(bits)):
        return
    ne = (got.contiguous().view(bits) != w.view(bits)).reshape(-1)
    first = int(ne.nonzero()[0])
    at = tuple(int(i) for i in np.unravel_index(first, shape or tuple(got.shape)))
    raise AssertionError(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the expected bits; the first at {at}: "
                         f"got {float(got.reshape(-1)[first])!r} expected {float(w.reshape(-1)[first])!r}")


def intact(guards, cid):
    torch.cuda.synchronize()
    for name, g in guards.items():
        g.intact(f"{cid} {name}")


# ------------------------------------------------------------------------------------------------ convolutions
CONV = V.cases("conv")


@pytest.mark.parametrize("case", CONV, ids=ids(CONV))
def test_convolution_bit_exact_in_both_forms(ops, case):
    inp, N = V.inputs(case), case["N"]
    want = V.expected(case, inp)["y"]
    wop = dev(V.conv_operand(case, inp["w"]), "bf16")
    bias = dev(inp["bias"], case["bias"]) if case["bias"] else None
    for knob, form in ((1, "patch-resident"), (0, "tile")):
        outs = []
        for behind in (None, 3.0) if N > 256 else (None,):
            X = placed(inp["x"], "bf16", behind=behind)
            R = placed(inp["res"], "bf16", behind=behind) if case["res"] else None
            Y = Guarded(N * 256, 64, "bf16")
            with knobs(conv_patch=knob):
                ops.conv3x3_implicit_fwd(X.t, wop, bias, Y.t, N, sign=1 if case["mode"] == "fwd" else -1, res=R.t if R else None)
            intact(dict(y=Y), f"{case['id']} [{form}]")
            same_bits(f"{case['id']} [{form}] y", Y.t, want, "bf16", (N, 256, 64))
            outs.append(Y.t.clone())
        assert all(torch.equal(o, outs[0]) for o in outs), f"{case['id']} [{form}]: the output depends on what lies behind the inputs"


WGRAD = V.cases("wgrad")


@pytest.mark.parametrize("case", WGRAD, ids=ids(WGRAD))
def test_weight_gradient_bit_exact_and_repeatable(ops, case):
    """(the two forms of one N share their inputs: both equal the same expected bits, hence each other)"""
    inp, N = V.inputs(case), case["N"]
    want = V.expected(case, inp)
    kn = dict(conv_patch=1 if case["form"] == "patch" else 0)
    if case["ks_knob"]:
        kn["conv_wgrad_ks"] = case["ks_knob"]
    for behind in (None, 3.0) if N > 256 else (None, None):          # twice either way
        X, DY = placed(inp["x"], "bf16", behind=behind), placed(inp["dy"], "bf16", behind=behind)
        g = dict(gp=placed(inp["g0"], "f32"))
        if case["gbias"]:
            g["gb"] = placed(inp["b0"], "f32", cols=64)
        with knobs(**kn):
            ops.conv3x3_implicit_wgrad(DY.t, X.t, g["gp"].t, N, gbias_acc=g["gb"].t[0] if case["gbias"] else None)
        intact(g, case["id"])
        for name in g:
            same_bits(f"{case['id']} {name}", g[name].t, want[name], "f32")


CONV1 = V.cases("conv1")


@pytest.mark.parametrize("case", CONV1, ids=ids(CONV1))
def test_conv1_bit_exact(ops, case):
    inp, N = V.inputs(case), case["N"]
    want = V.expected(case, inp)
    g = dict(cols=Guarded(N * 256, 32, "bf16"), y=Guarded(N * 256, 64, "bf16"))
    X = placed(inp["x"], "bf16", cols=3)
    ops.conv1_fused_fwd(X.t, dev(inp["wp"], "bf16"), dev(inp["bias"], case["bias"]) if case["bias"] else None, g["cols"].t, g["y"].t, N)
    intact(g, case["id"])
    same_bits(f"{case['id']} cols", g["cols"].t, want["cols"], "bf16", (N, 256, 32))
    same_bits(f"{case['id']} y", g["y"].t, want["y"], "bf16", (N, 256, 64))


# ------------------------------------------------------------------------------------------------ im2col / col2im
COLS = V.cases("im2col", "col2im")


@pytest.mark.parametrize("case", COLS, ids=ids(COLS))
def test_im2col_col2im_bit_exact(ops, case):
    inp = V.inputs(case)
    N, C, p, kpad, dt, off = case["N"], case["C"], case["p"], case["kpad"], case["dt"], case.get("unaligned", 0)
    nchw = case["layout"] == "nchw"
    if case["kind"] == "im2col":
        X = placed(inp["x"], dt, cols=p * p if nchw else C, off=off)
        out = Guarded(N * p * p, kpad, dt, off=off)
        (ops.im2col3x3 if nchw else ops.im2col3x3_nhwc)(X.t.view(N, C, p, p) if nchw else X.t, out.t, N, C, p)
        want = V.expected(case, inp)["cols"]
    else:
        X = placed(inp["x"], dt, off=off)
        out = Guarded(N * C, p * p, dt, off=off) if nchw else Guarded(N * p * p, C, dt, off=off)
        (ops.col2im3x3 if nchw else ops.col2im3x3_nhwc)(X.t, out.t, N, C, p)
        want = V.expected(case, inp)["dx"]
    if not nchw:
        assert (X.t.data_ptr() % 16 == 0 and out.t.data_ptr() % 16 == 0) != bool(off)
    intact(dict(out=out), case["id"])
    same_bits(case["id"], out.t, want, dt)


# ------------------------------------------------------------------------------------------------ permutes, un-permute, shuffles
PERM = V.cases("permute", "permute_t", "unpermute")


@pytest.mark.parametrize("case", PERM, ids=ids(PERM))
def test_weight_permutes_bit_exact(ops, case):
    inp, Cout, Cin = V.inputs(case), case["Cout"], case["Cin"]
    want = V.expected(case, inp)
    if case["kind"] == "unpermute":
        out = placed(inp["g0"], "f32", cols=Cin * 9)
        ops.conv_wgrad_unpermute(dev(inp["gp"], "f32"), out.t, Cout, Cin)
        name, dto = "g", "f32"
    else:
        name, dto = "wp", case["dto"]
        w = dev(inp["w"], case["dti"])
        if case["kind"] == "permute":
            out = Guarded(Cout, case["kpad"], dto)
            ops.conv_weight_permute(w, out.t, Cout, Cin)
        else:
            out = Guarded(Cin, 9 * Cout, dto)
            ops.conv_weight_permute_t(w, out.t, Cout, Cin)
    intact(dict(out=out), case["id"])
    same_bits(case["id"], out.t, want[name], dto)


SHUF = V.cases("shuffle")


@pytest.mark.parametrize("case", SHUF, ids=ids(SHUF))
def test_layout_shuffles_bit_exact_and_round_trip(ops, case):
    inp, N, C, hw, dt = V.inputs(case), case["N"], case["C"], case["hw"], case["dt"]
    fwd, back = (ops.nhwc_to_nchw, ops.nchw_to_nhwc) if case["to"] == "nchw" else (ops.nchw_to_nhwc, ops.nhwc_to_nchw)
    inner = hw if case["to"] == "nchw" else C
    X = dev(inp["x"], dt)
    Y, Z = Guarded(N * (C * hw // inner), inner, dt), Guarded(N * inner, C * hw // inner, dt)
    fwd(X, Y.t, N, C, hw)
    back(Y.t, Z.t, N, C, hw)
    intact(dict(y=Y, z=Z), case["id"])
    same_bits(case["id"], Y.t, V.expected(case, inp)["y"], dt, (N, C * hw // inner, inner))
    same_bits(case["id"] + " round trip", Z.t, inp["x"], dt, (N, inner, C * hw // inner))


# ------------------------------------------------------------------------------------------------ bounded kernels
def verify(case, inp, got, guards):
    intact(guards, case["id"])
    worst = {name: S.check(got[name], ref, bnd, f"{case['id']} {name}") for name, (ref, bnd) in V.expect(case, inp, got).items()}
    print(case["id"], " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


PNORM = V.cases("pnorm")


@pytest.mark.parametrize("case", PNORM, ids=ids(PNORM))
def test_patch_normalize(ops, case):
    inp, p, C = V.inputs(case), case["p"], case["C"]
    npatch = case["n_img"] * (case["H"] // p) * (case["W"] // p)
    nchw = case["layout"] == "nchw"
    out = Guarded(npatch * C, p * p, case["dto"]) if nchw else Guarded(npatch * p * p, C, case["dto"])
    (ops.patch_normalize if nchw else ops.patch_normalize_nhwc)(dev(inp["x"], case["dti"]), out.t, p)
    got = dict(out=out.np().reshape((npatch, C, p * p) if nchw else (npatch, p * p, C)))
    verify(case, inp, got, dict(out=out))


GN = V.cases("gn")


@pytest.mark.parametrize("case", GN, ids=ids(GN))
def test_groupnorm_gelu_forward_and_backward(ops, case):
    inp = V.inputs(case)
    N, C, hw, G, dt, pdt = case["N"], case["C"], case["hw"], case["groups"], case["dt"], case["pdt"]
    nhwc = case["layout"] == "nhwc"
    rows, cols = (N * hw, C) if nhwc else (N * C, hw)
    up = lambda a: dev(V._gn_lay(case, a).reshape(rows, cols), dt)
    X, DY, gam, bet = up(inp["x"]), up(inp["dy"]), dev(inp["gamma"], pdt), dev(inp["beta"], pdt)
    g = dict(y=Guarded(rows, cols, dt), mean=Guarded(1, N * G, "f32"), rstd=Guarded(1, N * G, "f32"), dx=Guarded(rows, cols, dt),
             dgamma=placed(inp["dg0"], "f32", cols=C), dbeta=placed(inp["db0"], "f32", cols=C))
    mean, rstd = g["mean"].t[0], g["rstd"].t[0]
    if nhwc:
        ops.groupnorm_gelu_nhwc_fwd(X, gam, bet, g["y"].t, mean, rstd, N, C, hw, groups=G, eps=V.EPS)
        ops.groupnorm_gelu_nhwc_bwd(DY, X, gam, bet, mean, rstd, g["dx"].t, g["dgamma"].t[0], g["dbeta"].t[0], N, C, hw, groups=G,
                                    res=up(inp["res"]) if case["res"] else None)
    else:
        ops.groupnorm_gelu_fwd(X, gam, bet, g["y"].t, mean, rstd, N, C, hw, groups=G, eps=V.EPS)
        ops.groupnorm_gelu_bwd(DY, X, gam, bet, mean, rstd, g["dx"].t, g["dgamma"].t[0], g["dbeta"].t[0], N, C, hw, groups=G)
    shape = (N, hw, C) if nhwc else (N, C, hw)
    got = dict(y=g["y"].np().reshape(shape), dx=g["dx"].np().reshape(shape), mean=g["mean"].np(True), rstd=g["rstd"].np(True),
               dgamma=g["dgamma"].np(True), dbeta=g["dbeta"].np(True))
    verify(case, inp, got, g)
