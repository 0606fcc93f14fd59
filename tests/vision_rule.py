"""The rule the image-patch embedder kernels (csrc/vision.hip, csrc/conv_implicit.hip) are tested by: a case table with one case per dispatch
branch and edge, probe inputs on a dyadic grid, float64 references written from the definitions, the expected BITS of the exact kernels,
per-element bounds of the others, fp32 transcriptions and one-mistake mutants.  test_vision_rule_cpu.py proves the rule usable without a
GPU; test_vision_kernels_gpu.py applies it.  Pure NumPy.  check / ratio / bound / half_ulp / bf16 / SENT / GELU_C are stream_rule's.

NO CONSTANT BELOW CAME FROM RUNNING A KERNEL UNDER TEST.  The only free constants are the two of the earlier rule files: the fp32 model may
use HALF of an allowance, a mutant must move an element by TEN bounds (attn_probe's margin).

EXACT KERNELS.  Activations and gradients are drawn from {0, +-1/2, +-1, +-2}, weights from {0, +-1/4, +-1/2, +-1}, biases, residuals and
initial accumulators are multiples of 1/4 below 8.  Every product is then a multiple of 2^-4, and as long as the sum of |terms| of an output
element, in units of 2^-4, stays below 2^24 (sumabs_units(), computed per case, asserted by the CPU test), every partial sum in ANY order is
exact in fp32: the kernel must deliver the correctly rounded float64 result bit for bit.  Rounding points, one line per kernel:
  conv_implicit_kernel / conv_patch_kernel   fp32 accumulators + bias + residual in fp32 (all exact), ONE rounding to bf16 (store_frag / f2bf_pk)
  conv_wgrad_*_kernel + reduce               fp32 partial slabs, fp32 ordered reduce, += on the fp32 accumulator: no rounding at all
  conv1_fused_kernel                         cols: a copy (zeros at k >= 27, whatever the operand's pad columns hold); y as the convolution
  im2col*, zero_pad_cols, permutes, shuffles copies (f32 -> bf16 permutes: one rounding of a representable value = a copy)
  col2im*                                    fp32 sum of <= 9 values, ONE rounding to the output type
  conv_wgrad_unpermute                       one fp32 add of grid values
expected value = bf16_rne(exact) for bf16 outputs, float32(exact) for fp32 outputs; no tolerance anywhere.

BOUNDED KERNELS.  bound = half_ulp_T(ref) + k * 2^-24 * sum_i c_i A_i (stream_rule.bound with c = 1 and A = the sum; k = 2 for bf16 outputs).
bf16 kernels are compared with the reference on the bf16-rounded inputs; the backward starts from the STORED mean and rstd (themselves
checked).  Chains (S = serial adds of a statistic; units of 2^-24; sqrtf, 1/x, rsqrtf charged 2, 2, 4; __expf at h: 3 + 1.5 h^2):
  patch_normalize*   S = ceil(p^2 / 64) + 6.  mean: c = S + 1, A = mean|x|.  out = (x - mean) * inv: the mean's error, the subtraction (1), then
                     |out| * (ceil((S + 3) / 2) + 9): q's chain (sub, square, S, division) halved by the square root, sqrtf, + 1e-6, sqrtf(p), *, 1 / x,
                     the final product.  A constant patch of a value whose multiples are exact (64) gives exactly 0: bound 0.
  gn NCHW fwd        S = ceil(cpg hw / 64) + 6.  mean c = S + 1; rstd c = S + 9 (sub, square, S, / n, + eps, rsqrtf), relative;
                     h = (x - mu) rs gamma + beta: (S + 1) mean|x| rs |gamma| + (S + 9) |xh gamma| + 4 (|xh gamma| + |beta|) =: E_h;
                     y = gelu(h): 1.13 E_h (max |gelu'|) + GELU_C[f32] A_gelu(h).
  gn NHWC fwd        S = 8 + 32 cpg (8 values per thread, then 32 cpg partials serially); gelu by the bf16 storage path: GELU_C[bf16].
  gn bwd (both)      dh = dy gelu'(h): E_dh = |dy| ((GELU_C + 6 + 1.5 h^2) A_gelu'(h) + 4 (|xh gamma| + |beta|)) + |dh|; g = dh gamma: E_g = |gamma| E_dh + |g|;
                     dx = rs (g - c1 - xh c2): rs (E_g + mean E_g + |xh| mean(E_g |xh| + 2 |g xh|)) + (S' + 8) rs (|g| + mean|g| + |xh| mean|g xh|) [+ |res|]
                     with S' = ceil(hw / 64) + 6 + cpg + 1 (NCHW: wave sums per channel, * gamma, cpg adds) / 8 + 32 + 1 + cpg (NHWC).
  gn dgamma, dbeta   terms dh xh and dh: sum (|xh| E_dh + 3 |dh xh|) resp. sum E_dh, + chain * (sum |terms| + |acc0|);
                     chain NCHW = N ceil(hw / 256) + 10 (thread-serial, block_sum256, accumulator);
                     chain NHWC = 8 + 32 + colsum_chain(rows = N) of stream_rule (pgrad rows through db1_colsum_acc).
stale_weights (a workgroup keeping another call's weights) is not applicable here: the weights are staged once per launch from the one
operand the call is given; there is no second operand a launch could mix up."""
import functools
import math
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rule as S  # noqa: E402
from stream_rule import SENT, U, bf16, bound, check, half_ulp, ratio, rnd, GELU_C  # noqa: E402,F401
from oracle.db1_oracle import _erf  # noqa: E402

MARGIN = 10.0            # a mutant of a bounded kernel must move an element by this many bounds (attn_probe's margin)
HEADROOM = 0.5           # the fp32 model may use this share of an allowance (stream_rule's)
EPS = 1e-5
ACT = np.array([0, 0.5, -0.5, 1, -1, 2, -2], np.float32)
WGT = np.array([0, 0.25, -0.25, 0.5, -0.5, 1, -1], np.float32)
QUART = (np.arange(-31, 32) * 0.25).astype(np.float32)
GRID_CAP = 8192 * 256    # items one pass of the streaming loops covers (im2col / col2im: 8192 blocks; vis_grid: 256 * 32 blocks)
ZCHUNK = 65535

MUTANTS = ("tap_transpose", "sign_flip", "wrap_x", "leak_y", "corner_only", "chunk_swap", "k_order", "pad_cols_dirty",
           "bias_off4", "bias_dropped", "res_prev_pixel", "res_dropped", "stale_image", "last_round_dropped",
           "range_tail_dropped", "slab_twice", "acc_assign", "gbias_col_off", "k27_live",
           "group_stride", "stat_index", "swap_dgdb", "biased_var_off", "biased_std", "no_sqrt_p", "patch_rowmajor_swap",
           "tail_tile_unwritten", "zchunk_offset", "second_pass_missing")
EXACT_KINDS = ("conv", "wgrad", "conv1", "im2col", "col2im", "permute", "permute_t", "unpermute", "shuffle")
BOUNDED_KINDS = ("pnorm", "gn")


# ------------------------------------------------------------------------------------------------ dispatcher arithmetic (as in the .hip)
def wgrad_ksplit(N, knob=0):
    nk = N * 4
    ks = knob if knob > 0 else 102
    while ks > 1 and nk // ks < 8:
        ks >>= 1
    return ks


def vecw(dt):
    return 8 if dt == "bf16" else 4


def vec_path(case):
    V = vecw(case["dt"])
    return case["C"] % V == 0 and case["kpad"] % V == 0 and not case.get("unaligned")


def stream_items(case):
    """items of the kernel's grid-stride loop (one store, scalar or vector, each)"""
    k, N, C, p = case["kind"], case["N"], case["C"], case["p"]
    if case["layout"] == "nchw":
        return N * p * p * (case["kpad"] if k == "im2col" else C)
    cv = C // vecw(case["dt"]) if vec_path(case) else C
    return N * p * p * cv * (9 if k == "im2col" else 1)


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def _draw(rng, grid, shape):
    return grid[rng.integers(0, len(grid), shape)]


def acc0(shape, k=0):
    n = int(np.prod(shape))
    return (0.25 * ((np.arange(n) * 7 + k) % 23 - 11)).astype(np.float32).reshape(shape)


def inputs(case):
    rng, k = _rng(case), case["kind"]
    if k == "conv":
        N = case["N"]
        return dict(x=_draw(rng, ACT, (N, 256, 64)), w=_draw(rng, WGT, (64, 64, 3, 3)), bias=_draw(rng, QUART, 64) if case["bias"] else None,
                    res=_draw(rng, QUART, (N, 256, 64)) if case["res"] else None)
    if k == "wgrad":
        N = case["N"]
        rng = np.random.default_rng(zlib.crc32(f"wgrad-N{N}".encode()))      # the two forms of one N share their inputs, hence their expected bits
        return dict(x=_draw(rng, ACT, (N, 256, 64)), dy=_draw(rng, ACT, (N, 256, 64)), g0=acc0((64, 576)), b0=acc0(64, 3))
    if k == "conv1":
        N = case["N"]
        wp = _draw(rng, WGT, (64, 32))
        wp[:, 27:] = 1.0                # the operand's pad columns are NOT zero: the kernel's A entries k >= 27 must be
        return dict(x=_draw(rng, ACT, (N, 256, 3)), wp=wp, bias=_draw(rng, QUART, 64) if case["bias"] else None)
    if k in ("im2col", "col2im"):
        N, C, p, kpad = case["N"], case["C"], case["p"], case["kpad"]
        shape = ((N, C, p, p) if case["layout"] == "nchw" else (N, p * p, C)) if k == "im2col" else (N * p * p, kpad)
        return dict(x=_draw(rng, ACT, shape))
    if k in ("permute", "permute_t"):
        return dict(w=_draw(rng, WGT, (case["Cout"], case["Cin"], 3, 3)))
    if k == "unpermute":
        Cout, Cin = case["Cout"], case["Cin"]
        return dict(gp=_draw(rng, QUART, (Cout, case["kpad"])), g0=acc0((Cout, Cin, 3, 3)))
    if k == "shuffle":
        N, C, hw = case["N"], case["C"], case["hw"]
        return dict(x=_draw(rng, QUART, (N, hw, C) if case["to"] == "nchw" else (N, C, hw)))
    if k == "pnorm":
        n, C, H, W = case["n_img"], case["C"], case["H"], case["W"]
        x = (rng.random((n, C, H, W)) * 255).astype(np.float32)
        if case["const"]:
            x[0, 0, :case["p"], :case["p"]] = 64.0
        return dict(x=rnd(x, case["dti"]))
    if k == "gn":
        N, C, hw, dt, pdt = case["N"], case["C"], case["hw"], case["dt"], case["pdt"]
        f = lambda a: a.astype(np.float32)
        x = f(rng.standard_normal((N, C, hw)) * 2 + 0.3 + 0.5 * np.arange(C)[None, :, None] / C)      # stored [N, C, hw] whatever the layout
        return dict(x=rnd(x, dt), dy=rnd(f(rng.standard_normal((N, C, hw))), dt), gamma=rnd(f(1 + 0.2 * rng.standard_normal(C)), pdt),
                    beta=rnd(f(0.2 * rng.standard_normal(C)), pdt), res=rnd(f(rng.standard_normal((N, C, hw))), dt) if case["res"] else None,
                    dg0=(0.5 + 0.25 * (np.arange(C) % 5)).astype(np.float32), db0=(1.5 - 0.25 * (np.arange(C) % 7)).astype(np.float32))
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------ float64 references, from the definitions
def _d(a):
    return np.asarray(a, np.float64)


def shift(a, dy, dx, mutant=None):
    """a [N, p, p, C] -> out[n, y, x] = a[n, y + dy, x + dx], zero outside the patch (the mutants pad wrongly)"""
    N, p = a.shape[0], a.shape[1]
    if mutant not in ("wrap_x", "leak_y", "corner_only"):
        out = np.zeros(a.shape, np.result_type(a.dtype, np.float32))
        y0, y1, x0, x1 = max(0, -dy), min(p, p - dy), max(0, -dx), min(p, p - dx)
        out[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        return out
    ys, xs = np.arange(p)[:, None] + dy, np.arange(p)[None, :] + dx
    vy, vx = (ys >= 0) & (ys < p), (xs >= 0) & (xs < p)
    ok = np.broadcast_to(vy & vx, (N, p, p))
    flat_in = ys * p + xs
    wrap = np.broadcast_to(vy & (flat_in >= 0) & (flat_in < p * p), (N, p, p))
    if mutant == "wrap_x":
        ok = wrap
    elif mutant == "leak_y":
        r = np.arange(N)[:, None, None] * p + ys[None]
        ok = np.broadcast_to(vx, (N, p, p)) & (r >= 0) & (r < N * p)
    elif mutant == "corner_only":
        corner = np.zeros((p, p), bool)
        corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
        ok = ok | (wrap & corner)
    g = (np.arange(N)[:, None, None] * p + ys[None]) * p + xs[None]
    return np.where(ok[..., None], a.reshape(N * p * p, -1)[np.clip(g, 0, N * p * p - 1)], 0.0)


def _chunk_swap(a):
    C = a.shape[-1]
    return a[..., (np.arange(C) // 8 ^ 1) * 8 + np.arange(C) % 8]


def _k_order(Wk):
    """[9, Cin, Cout] whose flat operand [Cout, 9 Cin] (tap-major) is read channel-major"""
    _, Cin, Cout = Wk.shape
    return Wk.transpose(2, 0, 1).reshape(Cout, Cin, 9).transpose(2, 1, 0)


def conv_core(x, Wk, sign, mutant=None):
    """x [N, p*p, Cin], Wk [9, Cin, Cout] (tap = ky * 3 + kx) -> sum_tap shift(x, sign (ky - 1), sign (kx - 1)) @ Wk[tap]"""
    N, hw, Cin = x.shape
    p = int(round(math.sqrt(hw)))
    a = _d(x).reshape(N, p, p, Cin)
    if mutant == "chunk_swap":
        a = _chunk_swap(a)
    if mutant == "stale_image":
        a = a.copy()
        a[256:] = a[:-256]
    if mutant == "sign_flip":
        sign = -sign
    if mutant == "k_order":
        Wk = _k_order(Wk)
    out = np.zeros((N * hw, Wk.shape[2]))
    for ky in range(3):
        for kx in range(3):
            W = Wk[kx * 3 + ky] if mutant == "tap_transpose" else Wk[ky * 3 + kx]
            out += shift(a, sign * (ky - 1), sign * (kx - 1), mutant).reshape(N * hw, Cin) @ _d(W)
    return out.reshape(N, hw, -1)


def conv_Wk(case, w):
    """the [9, Cin', Cout'] operand of the case: forward w[o, c, tap] -> [tap, c, o]; data gradient (sign = -1) [tap, o, c]"""
    w9 = _d(w).reshape(w.shape[0], w.shape[1], 9)
    return w9.transpose(2, 1, 0) if case["mode"] == "fwd" else w9.transpose(2, 0, 1)


def conv_operand(case, w):
    """what the kernel is given: [64, 576] K-major, column tap * 64 + k"""
    Wk = conv_Wk(case, w)
    return Wk.transpose(2, 0, 1).reshape(Wk.shape[2], -1).astype(np.float32)


_CORE_MUTANTS = ("tap_transpose", "sign_flip", "wrap_x", "leak_y", "corner_only", "chunk_swap", "k_order", "stale_image")


@functools.lru_cache(maxsize=8)
def _conv_core_cached(cid, mutant):
    case = BY_ID[cid]
    inp = inputs(case)
    return conv_core(inp["x"], conv_Wk(case, inp["w"]), 1 if case["mode"] == "fwd" else -1, mutant)


def ref_conv(case, inp, mutant=None):
    y = _conv_core_cached(case["id"], mutant if mutant in _CORE_MUTANTS else None).copy()
    if inp["bias"] is not None and mutant != "bias_dropped":
        y += _d(np.roll(inp["bias"], -4) if mutant == "bias_off4" else inp["bias"])
    if inp["res"] is not None and mutant != "res_dropped":
        r = _d(inp["res"])
        y += np.roll(r.reshape(-1, 64), 1, 0).reshape(r.shape) if mutant == "res_prev_pixel" else r
    if mutant == "last_round_dropped":
        y[(case["N"] // 256) * 256:] = SENT
    return dict(y=y)


def wgrad_weights(case, mutant):
    """per-pixel multiplicity of the contraction (1; a mutant drops or doubles a range of pixels)"""
    N = case["N"]
    wt = np.ones(N * 256)
    if mutant == "last_round_dropped":
        wt[(N // 256) * 256 * 256:] = 0
    if mutant in ("range_tail_dropped", "slab_twice") and case["form"] == "tile":
        nk, ks = N * 4, wgrad_ksplit(N, case["ks_knob"])
        if mutant == "range_tail_dropped":
            wt[ks * (nk // ks) * 64:] = 0
        else:
            per = -(-nk // ks)
            z = (nk - 1) // per                          # the last pixel range that holds anything
            wt[z * per * 64:] = 2
    if mutant == "slab_twice" and case["form"] == "patch":
        wg = min(N, 256)
        wt.reshape(N, 256)[wg - 1::wg] = 2               # the patches of the last workgroup
    return wt


def ref_wgrad(case, inp, mutant=None, absolute=False):
    N = case["N"]
    f = np.abs if absolute else (lambda a: a)
    x, dy = f(_d(inp["x"])), f(_d(inp["dy"])).reshape(N * 256, 64) * wgrad_weights(case, mutant)[:, None]
    a = x.reshape(N, 16, 16, 64)
    if mutant == "chunk_swap":
        a = _chunk_swap(a)
    if mutant == "stale_image":
        a = a.copy()
        a[256:] = a[:-256]
    s = -1 if mutant == "sign_flip" else 1
    gp = np.zeros((64, 9, 64))
    for ky in range(3):
        for kx in range(3):
            t = kx * 3 + ky if mutant == "tap_transpose" else ky * 3 + kx
            gp[:, t] = dy.T @ shift(a, s * (ky - 1), s * (kx - 1), mutant).reshape(N * 256, 64)
    gp = gp.transpose(0, 2, 1).reshape(64, 576) if mutant == "k_order" else gp.reshape(64, 576)
    gb = dy.sum(0)
    if mutant == "gbias_col_off":
        gb = np.roll(gb, 1)
    if mutant != "acc_assign":
        gp, gb = gp + f(_d(inp["g0"])), gb + f(_d(inp["b0"]))
    out = dict(gp=gp)
    if case["gbias"]:
        out["gb"] = gb
    return out


def ref_im2col(x, layout, kpad, mutant=None):
    """x [N, C, p, p] (nchw: column c * 9 + tap) or [N, p*p, C] (nhwc: column tap * C + c) -> cols [N p p, kpad], pad columns zero"""
    if layout == "nchw":
        N, C, p, _ = x.shape
        a = _d(x).transpose(0, 2, 3, 1)
    else:
        N, hw, C = x.shape
        p = int(round(math.sqrt(hw)))
        a = _d(x).reshape(N, p, p, C)
    if mutant == "chunk_swap":
        a = _chunk_swap(a)
    t = np.zeros((N * p * p, 9, C))
    for ky in range(3):
        for kx in range(3):
            t[:, kx * 3 + ky if mutant == "tap_transpose" else ky * 3 + kx] = shift(a, ky - 1, kx - 1, mutant).reshape(-1, C)
    if (layout == "nchw") != (mutant == "k_order"):
        t = t.transpose(0, 2, 1)
    cols = np.full((N * p * p, kpad), SENT if mutant == "pad_cols_dirty" else 0.0)
    cols[:, :9 * C] = t.reshape(N * p * p, 9 * C)
    return cols


def ref_col2im(dcols, layout, N, C, p, mutant=None):
    """the adjoint of im2col: dx[pixel] = sum_tap dcols[pixel - s(tap)][tap]"""
    t = _d(dcols)[:, :9 * C]
    t = t.reshape(-1, C, 9).transpose(0, 2, 1) if (layout == "nchw") != (mutant == "k_order") else t.reshape(-1, 9, C)
    t = t.reshape(N, p, p, 9, C)
    dx = np.zeros((N, p, p, C))
    for ky in range(3):
        for kx in range(3):
            src = t[:, :, :, kx * 3 + ky if mutant == "tap_transpose" else ky * 3 + kx]
            s = 1 if mutant == "sign_flip" else -1
            dx += shift(src, s * (ky - 1), s * (kx - 1), mutant)
    if mutant == "chunk_swap":
        dx = _chunk_swap(dx)
    return dx.transpose(0, 3, 1, 2) if layout == "nchw" else dx.reshape(N, p * p, C)


def _unwritten_tail(case, out):
    """second_pass_missing: what the items past one pass of the grid would have stored keeps the sentinel"""
    k, C = case["kind"], case["C"]
    idx = np.arange(GRID_CAP, stream_items(case))
    flat = out.reshape(-1)
    if case["layout"] == "nchw":
        flat[idx] = SENT
        return out
    V = vecw(case["dt"]) if vec_path(case) else 1
    cv = C // V
    if k == "im2col":
        pix, rem = idx // (9 * cv), idx % (9 * cv)
        col = (rem // cv) * C + (rem % cv) * V
        for j in range(V):
            out[pix, col + j] = SENT
    else:
        o2 = out.reshape(-1, C)
        for j in range(V):
            o2[idx // cv, (idx % cv) * V + j] = SENT
    return out


def ref_permute(w, kpad, mutant=None):
    Cout, Cin = w.shape[:2]
    w9 = _d(w).reshape(Cout, Cin, 9)
    if mutant == "tap_transpose":
        w9 = w9.reshape(Cout, Cin, 3, 3).transpose(0, 1, 3, 2).reshape(Cout, Cin, 9)
    out = np.full((Cout, kpad), SENT if mutant == "pad_cols_dirty" else 0.0)
    out[:, :9 * Cin] = (w9 if mutant == "k_order" else w9.transpose(0, 2, 1)).reshape(Cout, 9 * Cin)
    return out


def ref_permute_t(w, mutant=None):
    Cout, Cin = w.shape[:2]
    w9 = _d(w).reshape(Cout, Cin, 9)
    if mutant == "tap_transpose":
        w9 = w9.reshape(Cout, Cin, 3, 3).transpose(0, 1, 3, 2).reshape(Cout, Cin, 9)
    return (w9.transpose(1, 0, 2) if mutant == "k_order" else w9.transpose(1, 2, 0)).reshape(Cin, 9 * Cout)


def ref_unpermute(gp, g0, mutant=None):
    Cout, Cin = g0.shape[:2]
    t = _d(gp)[:, :9 * Cin]
    t = t.reshape(Cout, Cin, 9) if mutant == "k_order" else t.reshape(Cout, 9, Cin).transpose(0, 2, 1)
    if mutant == "tap_transpose":
        t = t.reshape(Cout, Cin, 3, 3).transpose(0, 1, 3, 2).reshape(Cout, Cin, 9)
    t = t.reshape(g0.shape)
    return t if mutant == "acc_assign" else t + _d(g0)


def ref_shuffle(case, x, mutant=None):
    out = _d(x).transpose(0, 2, 1).copy()
    if mutant == "chunk_swap":
        out = _chunk_swap(out) if case["to"] == "nhwc" else np.ascontiguousarray(_chunk_swap(out.transpose(0, 2, 1)).transpose(0, 2, 1))
    rows, cols = (case["C"], case["hw"]) if case["to"] == "nchw" else (case["hw"], case["C"])
    if mutant == "tail_tile_unwritten":
        out[:, rows // 32 * 32:, :] = SENT
        out[:, :, cols // 32 * 32:] = SENT
    if mutant == "zchunk_offset":
        out[ZCHUNK:] = out[ZCHUNK - 1:-1].copy()
    return out


def ref_conv1(case, inp, mutant=None):
    N = case["N"]
    cols = ref_im2col(inp["x"], "nhwc", 32, mutant)
    wp = _d(inp["wp"])
    if mutant == "k27_live":
        cols[:, 27:] = _d(inp["x"]).reshape(N * 256, 3)[:, [0, 1, 2, 0, 1]]
    elif mutant != "pad_cols_dirty":
        cols[:, 27:] = 0.0
    y = cols[:, :27] @ wp[:, :27].T
    if mutant == "k27_live":
        y = y + cols[:, 27:] @ wp[:, 27:].T
    if inp["bias"] is not None and mutant != "bias_dropped":
        y = y + _d(np.roll(inp["bias"], -4) if mutant == "bias_off4" else inp["bias"])
    return dict(cols=cols, y=y)


def reference(case, inp, mutant=None):
    """{output: float64 array} of an exact case (a mutant: the same with one mistake); an element no kernel would write holds SENT"""
    k = case["kind"]
    if k == "conv":
        return ref_conv(case, inp, mutant)
    if k == "wgrad":
        return ref_wgrad(case, inp, mutant)
    if k == "conv1":
        return ref_conv1(case, inp, mutant)
    if k == "im2col":
        out = ref_im2col(inp["x"], case["layout"], case["kpad"], mutant)
        return dict(cols=_unwritten_tail(case, out) if mutant == "second_pass_missing" else out)
    if k == "col2im":
        out = np.ascontiguousarray(ref_col2im(inp["x"], case["layout"], case["N"], case["C"], case["p"], mutant))
        return dict(dx=_unwritten_tail(case, out) if mutant == "second_pass_missing" else out)
    if k == "permute":
        return dict(wp=ref_permute(inp["w"], case["kpad"], mutant))
    if k == "permute_t":
        return dict(wp=ref_permute_t(inp["w"], mutant))
    if k == "unpermute":
        return dict(g=ref_unpermute(inp["gp"], inp["g0"], mutant))
    if k == "shuffle":
        return dict(y=ref_shuffle(case, inp["x"], mutant))
    raise KeyError(k)


def out_dt(case, name):
    k = case["kind"]
    if k in ("wgrad", "unpermute"):
        return "f32"
    if k in ("conv", "conv1"):
        return "bf16"
    return case.get("dto") or case["dt"]


def expected(case, inp, mutant=None):
    """{output: float32 array holding the expected BITS}: the exact value rounded once to the output type (+ 0.0: an exact zero is +0)"""
    return {name: rnd((v + 0.0).astype(np.float32), out_dt(case, name)) for name, v in reference(case, inp, mutant).items()}


def sumabs_units(case, inp):
    """the largest sum of |terms| of an output element, in units of the product grid 2^-4: below 2^24 every fp32 partial sum is exact"""
    k = case["kind"]
    if k == "conv":
        a = conv_core(np.abs(inp["x"][:min(case["N"], 2)]), np.abs(conv_Wk(case, inp["w"])), 1 if case["mode"] == "fwd" else -1)
        m = a.max() + (np.abs(inp["bias"]).max() if inp["bias"] is not None else 0) + (np.abs(inp["res"]).max() if inp["res"] is not None else 0)
        m = max(m, 64 * 9 * 2.0 + 16)                                                  # (and the largest any patch could reach)
    elif k == "wgrad":
        m = 2.0 * np.abs(_d(inp["dy"])).reshape(-1, 64).sum(0).max() + 8          # |x| <= 2, |acc0| < 8: an upper bound of every element's sum
    elif k == "conv1":
        m = 27 * 2.0 + 8
    elif k == "col2im":
        m = 9 * 2.0
    elif k == "unpermute":
        m = 16.0
    else:
        m = max(np.abs(v).max() for v in inp.values() if v is not None)
    return float(m) * 16


def representable(case, inp):
    """every input is a value of its storage type and a multiple of 2^-4"""
    dts = {"conv": "bf16", "wgrad": "bf16", "conv1": "bf16", "unpermute": "f32"}
    dt = dts.get(case["kind"]) or case.get("dti") or case["dt"]
    return all(v is None or (np.array_equal(rnd(v, dt), v) and np.array_equal(np.round(v * 16), v * 16)) for v in inp.values())


def exact_model(case, inp, seed):
    """the fp32 transcription of an exact kernel with the terms of every sum taken in an order drawn from ``seed``: float32 throughout"""
    k, f32 = case["kind"], np.float32
    rng = np.random.default_rng(seed)
    if k in ("conv", "conv1"):
        if k == "conv":
            N, Wk, sign, C = case["N"], conv_Wk(case, inp["w"]).astype(f32), 1 if case["mode"] == "fwd" else -1, 64
        else:
            N, Wk, sign, C = case["N"], inp["wp"][:, :27].reshape(64, 9, 3).transpose(1, 2, 0).astype(f32), 1, 3
        a = inp["x"].reshape(N, 16, 16, C)
        G = np.concatenate([shift(a, sign * (t // 3 - 1), sign * (t % 3 - 1)).reshape(N * 256, C) for t in range(9)], 1).astype(f32)
        perm = rng.permutation(9 * C)
        y = np.zeros((N * 256, 64), f32)
        Wf = Wk.reshape(9 * C, 64)
        for blk in np.array_split(perm, 7):                       # fp32 partial sums of a shuffled term order, added in fp32
            y = y + G[:, blk] @ Wf[blk]
        if inp["bias"] is not None:
            y = y + inp["bias"]
        if inp.get("res") is not None:
            y = y + inp["res"].reshape(N * 256, 64)
        out = dict(y=rnd(y.reshape(N, 256, 64) if k == "conv" else y, "bf16"))
        if k == "conv1":
            out["cols"] = np.concatenate([G, np.zeros((N * 256, 5), f32)], 1)
        return out
    if k == "wgrad":
        N = case["N"]
        a, dy = inp["x"].reshape(N, 16, 16, 64), inp["dy"].reshape(N * 256, 64)
        perm = rng.permutation(N * 256)
        gp, gb = np.zeros((64, 9, 64), f32), np.zeros(64, f32)
        for blk in np.array_split(perm, 5):
            for t in range(9):
                gp[:, t] = gp[:, t] + dy[blk].T @ shift(a, t // 3 - 1, t % 3 - 1).reshape(N * 256, 64)[blk].astype(f32)
            gb = gb + dy[blk].sum(0, dtype=f32)
        out = dict(gp=inp["g0"] + gp.reshape(64, 576))
        if case["gbias"]:
            out["gb"] = inp["b0"] + gb
        return out
    if k == "col2im":
        N, C, p = case["N"], case["C"], case["p"]
        t = inp["x"][:, :9 * C]
        t = (t.reshape(-1, C, 9).transpose(0, 2, 1) if case["layout"] == "nchw" else t.reshape(-1, 9, C)).reshape(N, p, p, 9, C)
        dx = np.zeros((N, p, p, C), f32)
        for tap in rng.permutation(9):
            dx = dx + shift(t[:, :, :, tap], -(tap // 3 - 1), -(tap % 3 - 1)).astype(f32)
        dx = dx.transpose(0, 3, 1, 2) if case["layout"] == "nchw" else dx.reshape(N, p * p, C)
        return dict(dx=rnd(np.ascontiguousarray(dx), case["dt"]))
    return {n: rnd(v.astype(f32), out_dt(case, n)) for n, v in reference(case, inp).items()}       # copies: nothing to order


# ------------------------------------------------------------------------------------------------ bounded kernels: patch normalise
def _patches(x, p, swap=False):
    n, C, H, W = x.shape
    h, w = H // p, W // p
    t = x.reshape(n, C, h, p, w, p)
    t = t.transpose(0, 4, 2, 1, 3, 5) if swap else t.transpose(0, 2, 4, 1, 3, 5)
    return t.reshape(n * h * w, C, p * p)


def _pn_layout(y, layout):
    return y if layout == "nchw" else np.ascontiguousarray(y.transpose(0, 2, 1))      # [patch, C, p p] / [patch, p p, C]


def model_pnorm(case, inp, mutant=None):
    f, p = np.float32, case["p"]
    n = p * p
    x = _patches(inp["x"], p, mutant == "patch_rowmajor_swap")
    mean = x.sum(-1, dtype=f, keepdims=True) / f(n)
    d = x - mean
    std = np.sqrt((d * d).sum(-1, dtype=f, keepdims=True) / f(n if mutant == "biased_std" else n - 1))
    inv = f(1) / ((f(1e-6) + std) * (f(1) if mutant == "no_sqrt_p" else np.sqrt(f(p))))
    return dict(out=rnd(_pn_layout(d * inv, case["layout"]), case["dto"]))


def expect_pnorm(case, inp, got=None):
    p = case["p"]
    n = p * p
    x = _d(_patches(inp["x"], p))
    mean = x.mean(-1, keepdims=True)
    std = np.sqrt(((x - mean) ** 2).sum(-1, keepdims=True) / (n - 1))
    inv = 1.0 / ((1e-6 + std) * math.sqrt(p))
    ref = (x - mean) * inv
    Ssum = -(-n // 64) + 6
    mabs = np.abs(x).mean(-1, keepdims=True)
    A = inv * ((Ssum + 1) * mabs + np.abs(x) + np.abs(mean)) + np.abs(ref) * (-(-(Ssum + 3) // 2) + 9)
    b = bound(ref, A, 1, case["dto"])
    const = (x == x[..., :1]).all(-1, keepdims=True) & (x[..., :1] == 64.0)          # multiples of 64 up to 2^14 are exact: mean 64, out 0
    b = np.where(const, 0.0, b)
    return dict(out=(_pn_layout(ref, case["layout"]), _pn_layout(b, case["layout"])))


# ------------------------------------------------------------------------------------------------ bounded kernels: GroupNorm + GELU
def _gn_S(case):
    cpg = case["C"] // case["groups"]
    return 8 + 32 * cpg if case["layout"] == "nhwc" else -(-(cpg * case["hw"]) // 64) + 6


def _gn_lay(case, a):
    """[N, C, hw] (how the rule holds every activation) -> the layout the kernel stores"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if case["layout"] == "nhwc" else a


def _gelu_dt(case):
    return "bf16" if case["layout"] == "nhwc" else "f32"       # NHWC: gelu_*_t<bf16_t> (storage path); NCHW: erff whatever T


def model_gn(case, inp, mutant=None):
    """{y, mean, rstd, dx, dgamma, dbeta} in float32 arithmetic; the backward starts from the model's own stored mean / rstd"""
    f = np.float32
    N, C, hw, G, dt = case["N"], case["C"], case["hw"], case["groups"], case["dt"]
    cpg = C // G
    x, dy, gm, bt = inp["x"], inp["dy"], inp["gamma"][None, :, None], inp["beta"][None, :, None]
    grp = (lambda a: a.reshape(N, cpg, G, hw).transpose(0, 2, 1, 3).reshape(N, G, -1)) if mutant == "group_stride" else (lambda a: a.reshape(N, G, -1))
    ungrp = (lambda a: a.reshape(N, G, cpg, hw).transpose(0, 2, 1, 3).reshape(N, C, hw)) if mutant == "group_stride" else (lambda a: a.reshape(N, C, hw))
    n = cpg * hw
    xg = grp(x)
    mu = xg.sum(-1, dtype=f, keepdims=True) / f(n)
    d = xg - mu
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = f(1) / np.sqrt((d * d).sum(-1, dtype=f, keepdims=True) / f(n - 1 if mutant == "biased_var_off" else n) + f(EPS))
    xh = ungrp(d * rs)
    h = xh * gm + bt
    y, dg = S._gelu_both(h.astype(f), _gelu_dt(case))
    mean_o, rstd_o = mu.reshape(-1).copy(), rs.reshape(-1).astype(f)
    if mutant == "stat_index":
        mean_o, rstd_o = np.full(N * G, SENT, f), np.full(N * G, SENT, f)
        for c in range(0, C, cpg):
            if c < G:
                mean_o.reshape(N, G)[:, c], rstd_o.reshape(N, G)[:, c] = mu.reshape(N, G)[:, c // cpg], rs.reshape(N, G)[:, c // cpg]
    dh = dy * dg
    g = dh * gm
    c1 = grp(g).sum(-1, dtype=f, keepdims=True) / f(n)
    c2 = grp(g * xh).sum(-1, dtype=f, keepdims=True) / f(n)
    dx = ungrp(rs * (grp(g) - c1 - grp(xh) * c2))
    if inp["res"] is not None and mutant != "res_dropped":
        dx = dx + inp["res"]
    dga, dbe = inp["dg0"] + (dh * xh).sum((0, 2), dtype=f), inp["db0"] + dh.sum((0, 2), dtype=f)
    if mutant == "swap_dgdb":
        dga, dbe = dbe, dga
    return dict(y=rnd(_gn_lay(case, y), dt), mean=mean_o, rstd=rstd_o, dx=rnd(_gn_lay(case, dx.astype(f)), dt), dgamma=dga.astype(f), dbeta=dbe.astype(f))


def expect_gn(case, inp, got):
    """references and bounds; ``got`` supplies the stored mean and rstd the backward is defined on"""
    N, C, hw, G, dt = case["N"], case["C"], case["hw"], case["groups"], case["dt"]
    cpg, lay = C // G, functools.partial(_gn_lay, case)
    n, Ss = cpg * hw, _gn_S(case)
    x, dy, gam, bet = _d(inp["x"]), _d(inp["dy"]), _d(inp["gamma"])[None, :, None], _d(inp["beta"])[None, :, None]
    grp, ungrp = (lambda a: a.reshape(N, G, -1)), (lambda a: a.reshape(N, C, hw))
    bc = lambda a: ungrp(np.broadcast_to(a, (N, G, n)))
    cgel = GELU_C[_gelu_dt(case)]
    # forward
    xg = grp(x)
    mu = xg.mean(-1, keepdims=True)
    rs = 1.0 / np.sqrt(((xg - mu) ** 2).mean(-1, keepdims=True) + EPS)
    mabs = np.abs(xg).mean(-1, keepdims=True)
    xh = ungrp((xg - mu) * rs)
    h = xh * gam + bet
    with np.errstate(over="ignore", under="ignore"):
        erf = np.abs(_erf(h / math.sqrt(2.0)))
        yref = 0.5 * h * (1.0 + _erf(h / math.sqrt(2.0)))
    Eh = (Ss + 1) * bc(mabs * rs) * np.abs(gam) + (Ss + 13) * np.abs(xh * gam) + 4 * np.abs(bet)
    Ay = 1.13 * Eh + cgel * 0.5 * np.abs(h) * (1.0 + erf)
    out = dict(y=(lay(yref), lay(bound(yref, Ay, 1, dt))), mean=(mu.reshape(-1), bound(mu.reshape(-1), (Ss + 1) * mabs.reshape(-1), 1, "f32")),
               rstd=(rs.reshape(-1), bound(rs.reshape(-1), (Ss + 9) * rs.reshape(-1), 1, "f32")))
    # backward, from the stored statistics
    mu, rs = _d(got["mean"]).reshape(N, G, 1), _d(got["rstd"]).reshape(N, G, 1)
    xh = ungrp((xg - mu) * rs)
    h = xh * gam + bet
    with np.errstate(over="ignore", under="ignore"):
        e = _erf(h / math.sqrt(2.0))
        pdf = np.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    dgel = 0.5 * (1.0 + e) + h * pdf
    Agp = 0.5 * (1.0 + np.abs(e)) + np.abs(h) * pdf
    dh = dy * dgel
    Edh = np.abs(dy) * ((cgel + 6 + 1.5 * h * h) * Agp + 4 * (np.abs(xh * gam) + np.abs(bet))) + np.abs(dh)
    g = dh * gam
    Eg = np.abs(gam) * Edh + np.abs(g)
    m = lambda a: bc(grp(a).mean(-1, keepdims=True))
    dxref = bc(rs) * (g - m(g) - xh * m(g * xh))
    Sp = (-(-hw // 64) + 6 + cpg + 1) if case["layout"] == "nchw" else (8 + 32 + 1 + cpg)
    Adx = bc(rs) * (Eg + m(Eg) + np.abs(xh) * m(Eg * np.abs(xh) + 2 * np.abs(g * xh))
                    + (Sp + 8) * (np.abs(g) + m(np.abs(g)) + np.abs(xh) * m(np.abs(g * xh))))
    if inp["res"] is not None:
        dxref, Adx = dxref + _d(inp["res"]), Adx + np.abs(dxref) + np.abs(_d(inp["res"]))
    out["dx"] = (lay(dxref), lay(bound(dxref, Adx, 1, dt)))
    chain = (N * -(-hw // 256) + 10) if case["layout"] == "nchw" else \
        (8 + 32 + S.colsum_chain(dict(op="colsum", dt="f32", rows=N, cols=64, variant="strided")))
    dg0, db0 = _d(inp["dg0"]), _d(inp["db0"])
    dgr, dbr = (dh * xh).sum((0, 2)) + dg0, dh.sum((0, 2)) + db0
    out["dgamma"] = (dgr, bound(dgr, (np.abs(xh) * Edh + 3 * np.abs(dh * xh)).sum((0, 2)) + chain * (np.abs(dh * xh).sum((0, 2)) + np.abs(dg0)), 1, "f32"))
    out["dbeta"] = (dbr, bound(dbr, Edh.sum((0, 2)) + chain * (np.abs(dh).sum((0, 2)) + np.abs(db0)), 1, "f32"))
    return out


def model(case, inp, mutant=None):
    return model_pnorm(case, inp, mutant) if case["kind"] == "pnorm" else model_gn(case, inp, mutant)


def expect(case, inp, got):
    return expect_pnorm(case, inp, got) if case["kind"] == "pnorm" else expect_gn(case, inp, got)


# ------------------------------------------------------------------------------------------------ mutants: where each one is a mistake at all
def applicable(mutant, case):
    k = case["kind"]
    N = case.get("N", 0)
    spatial = k in ("conv", "wgrad", "conv1", "im2col", "col2im")
    small = N <= 37                                           # the index mistakes are the same at every N: judged where the reference is cheap
    if mutant == "tap_transpose":
        return (spatial and small) or k in ("permute", "permute_t", "unpermute")
    if mutant == "k_order":                                   # (one channel: both column orders are the same)
        return (spatial and small and case.get("C", 3) > 1) or k in ("permute", "permute_t", "unpermute")
    if mutant == "sign_flip":                                 # (also what judges the data gradient at N = 255, 256, where nothing else applies)
        return (k in ("conv", "wgrad", "col2im") and small) or (k == "conv" and case["mode"] == "dgrad" and N in (255, 256))
    if mutant in ("wrap_x", "corner_only"):
        return spatial and small
    if mutant == "leak_y":
        return spatial and small and N > 1
    if mutant == "chunk_swap":
        return (spatial and small and case.get("C", 3 if k == "conv1" else 64) % 16 == 0) or (k == "shuffle" and case["C"] % 16 == 0)
    if mutant == "pad_cols_dirty":
        return (k == "im2col" and case["kpad"] > 9 * case["C"]) or (k == "permute" and case["kpad"] > 9 * case["Cin"]) or k == "conv1"
    if mutant in ("bias_off4", "bias_dropped"):
        return k in ("conv", "conv1") and bool(case["bias"]) and N <= 256
    if mutant in ("res_prev_pixel", "res_dropped"):
        return (k == "conv" and case["res"] and N <= 256) or (mutant == "res_dropped" and k == "gn" and case["res"])
    if mutant == "last_round_dropped":
        return k in ("conv", "wgrad") and N > 256 and N % 256 != 0
    if mutant == "stale_image":                               # the same mistake at 257 and 513: judged at 257, once per kernel and epilogue family
        return k in ("conv", "wgrad") and N == 257 and (k == "wgrad" or case["mode"] == "dgrad" or (case["bias"] == "bf16" and case["res"]))
    if mutant == "range_tail_dropped":
        return k == "wgrad" and case["form"] == "tile" and (4 * N) % wgrad_ksplit(N, case["ks_knob"]) != 0
    if mutant == "slab_twice":
        return k == "wgrad" and N <= 257
    if mutant == "acc_assign":
        return (k == "wgrad" and N <= 256) or k == "unpermute"
    if mutant == "gbias_col_off":
        return k == "wgrad" and case["gbias"] and small
    if mutant == "k27_live":
        return k == "conv1"
    if mutant in ("group_stride", "stat_index"):
        return k == "gn" and 1 < case["C"] // case["groups"] < case["C"]
    if mutant == "swap_dgdb":
        return k == "gn"
    if mutant == "biased_var_off":                            # rstd moves by 1 / (2 n) of itself: ten of its bounds (S + 9 roundings) only where n is small
        if k != "gn":
            return False
        n = case["C"] // case["groups"] * case["hw"]
        return n == 1 or 0.5 / n > 1.5 * MARGIN * (_gn_S(case) + 10) * U
    if mutant == "biased_std":                                # a factor sqrt((n - 1) / n): under ten bf16 half-ulps unless the patch is tiny
        return k == "pnorm" and (case["dto"] == "f32" or case["p"] == 3)
    if mutant == "no_sqrt_p":
        return k == "pnorm"
    if mutant == "patch_rowmajor_swap":
        return k == "pnorm" and case["H"] // case["p"] > 1 and case["W"] // case["p"] > 1
    if mutant == "tail_tile_unwritten":
        return k == "shuffle" and (case["C"] % 32 != 0 or case["hw"] % 32 != 0)
    if mutant == "zchunk_offset":
        return k == "shuffle" and N > ZCHUNK
    if mutant == "second_pass_missing":
        return k in ("im2col", "col2im") and stream_items(case) > GRID_CAP
    raise KeyError(mutant)


# ------------------------------------------------------------------------------------------------ the case table
def _mk(kind, **kw):
    kw["kind"] = kind
    kw["id"] = kind + "-" + "-".join(f"{k}{v}" if not isinstance(v, str) else v for k, v in kw.items() if k != "kind")
    return kw


def _cases():
    T = []
    # convolution forward (bias x res crossed at N = 3, two combinations at every other N), data gradient; each runs under conv_patch = 0 and 1
    combos = [(b, r) for b in ("bf16", "f32", "") for r in (False, True)]
    for b, r in combos:
        T.append(_mk("conv", mode="fwd", N=3, bias=b, res=r))
    for i, N in enumerate((1, 255, 256, 257, 513)):
        b, r = combos[(2 * i + 1) % 6]
        T.append(_mk("conv", mode="fwd", N=N, bias=b, res=r))
        T.append(_mk("conv", mode="fwd", N=N, bias=combos[(2 * i + 4) % 6][0], res=combos[(2 * i + 4) % 6][1]))
    for N in (1, 3, 255, 256, 257, 513):
        T.append(_mk("conv", mode="dgrad", N=N, bias="", res=False))
    # weight gradient: patch form (slabs = min(N, 256) workgroups), tile form (ks from ci_wgrad_ksplit: 1, 1, 51 halved, 102 exact, 102 with
    # 4 N % 102 != 0 and empty last ranges), one conv_wgrad_ks override (7 ranges over 148 k-steps)
    for N in (1, 3, 255, 256, 257, 513):
        T.append(_mk("wgrad", form="patch", N=N, ks_knob=0, gbias=N != 255))
    for N in (1, 3, 128, 255, 256, 257, 513):
        T.append(_mk("wgrad", form="tile", N=N, ks_knob=0, gbias=N != 3))
    T.append(_mk("wgrad", form="tile", N=37, ks_knob=7, gbias=True))
    for N in (1, 37):
        for b in ("bf16", "f32", ""):
            T.append(_mk("conv1", N=N, bias=b))
    for dt in ("f32", "bf16"):
        for C, p, kpad in ((5, 16, 45), (3, 4, 32), (1, 3, 9)):
            T.append(_mk("im2col", layout="nchw", dt=dt, N=3, C=C, p=p, kpad=kpad))
            T.append(_mk("col2im", layout="nchw", dt=dt, N=3, C=C, p=p, kpad=kpad))
        for C, kpad in ((64, 576), (8, 80), (3, 32), (8, 76)):        # vector, vector with pad columns, scalar by C, scalar by kpad
            for kind in ("im2col", "col2im"):
                T.append(_mk(kind, layout="nhwc", dt=dt, N=3, C=C, p=16, kpad=kpad))
        for kind in ("im2col", "col2im"):                             # scalar by alignment: the base 4 bytes off
            T.append(_mk(kind, layout="nhwc", dt=dt, N=3, C=8, p=16, kpad=80, unaligned=1))
    T.append(_mk("im2col", layout="nchw", dt="f32", N=200, C=5, p=16, kpad=45))         # 2 304 000 items: the second pass
    T.append(_mk("col2im", layout="nchw", dt="bf16", N=130, C=64, p=16, kpad=576))      # 2 129 920 items
    T.append(_mk("im2col", layout="nhwc", dt="bf16", N=120, C=64, p=16, kpad=576))      # 2 211 840 items past vis_grid's cap
    T.append(_mk("col2im", layout="nhwc", dt="bf16", N=2800, C=3, p=16, kpad=32))       # 2 150 400 items, scalar path
    for Cout, Cin in ((64, 64), (64, 3)):
        for dti, dto in (("f32", "bf16"), ("bf16", "bf16"), ("f32", "f32"), ("bf16", "f32")):
            T.append(_mk("permute", Cout=Cout, Cin=Cin, kpad=576 if Cin == 64 else 32, dti=dti, dto=dto))
            T.append(_mk("permute_t", Cout=Cout, Cin=Cin, dti=dti, dto=dto))
        T.append(_mk("unpermute", Cout=Cout, Cin=Cin, kpad=576 if Cin == 64 else 32))
    for dt in ("f32", "bf16"):
        for to in ("nchw", "nhwc"):
            for N, C, hw in ((3, 64, 256), (2, 33, 31), (1, 1, 1), (65538, 3, 5)):
                T.append(_mk("shuffle", to=to, dt=dt, N=N, C=C, hw=hw))
    for layout in ("nchw", "nhwc"):
        for i, (n, C, H, W, p) in enumerate(((2, 3, 32, 48, 16), (1, 3, 6, 9, 3), (3, 1, 20, 10, 10), (1, 5, 16, 16, 8))):
            for dti in ("f32", "bf16"):
                for dto in ("f32", "bf16"):
                    T.append(_mk("pnorm", layout=layout, n_img=n, C=C, H=H, W=W, p=p, dti=dti, dto=dto, const=int(i == 0 and dti == "f32")))
    for G in (64, 32, 16, 8, 4, 1):
        for N, pdt, res in ((1, "bf16", False), (5, "f32", True), (5, "bf16", True)) if G in (32, 1) else ((5, "f32" if G in (64, 8) else "bf16", G in (64, 16)),):
            T.append(_mk("gn", layout="nhwc", dt="bf16", pdt=pdt, N=N, C=64, hw=256, groups=G, res=res))
    T.append(_mk("gn", layout="nhwc", dt="bf16", pdt="f32", N=1, C=64, hw=256, groups=32, res=False))
    for C, hw, G in ((64, 256, 32), (6, 10, 3), (4, 1, 4)):           # (one launcher: gn_param_grad_kernel always runs, no condition selects it)
        for dt, pdt in (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16")):
            T.append(_mk("gn", layout="nchw", dt=dt, pdt=pdt, N=3, C=C, hw=hw, groups=G, res=False))
    return T


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def cases(*kinds):
    return [c for c in CASES if c["kind"] in kinds]


def cheap(case):
    """small enough for the fp32 order check of the CPU proof (the exactness condition itself is computed for every case)"""
    return case.get("N", 1) <= 37
