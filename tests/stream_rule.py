"""The rule the streaming kernels of csrc/elementwise.hip are tested by: float64 references, per-element bounds, an fp32 model of every
kernel with one-mistake mutants, and the case table that the CPU proof (test_stream_rule_cpu.py) and the GPU tests
(test_stream_kernels_gpu.py) share.  Pure NumPy; nothing here touches a GPU.

NO CONSTANT BELOW CAME FROM RUNNING A KERNEL UNDER TEST.  Every c is a count of fp32 roundings read from the kernel's code; the CPU test
then asserts that the fp32 model (a different summation order than the device's in places) stays under HALF of every bound and that every
mutant breaks one.

Comparison.  check(got, ref, bound) compares EVERY element: |got - ref| <= bound, and a non-finite got where ref is finite fails.
    bound = half_ulp_T(ref) + k * c * 2^-24 * A            (floor: 2^-126, the smallest normal -- a flushed subnormal passes)
  half_ulp_T(ref) is half a unit in the last place of ref in the OUTPUT format T: 2^(e-8) for bf16 (8 significand bits), 2^(e-24) for f32,
    with 2^e <= |ref| < 2^(e+1).  As a fraction of |ref| that is between 2^-9 and 2^-8 (bf16) and at most 2^-24 (f32).  A flat 2^-9 |ref|
    for bf16 is NOT met by correct rounding (1 + 2^-8 + tiny rounds to 1 + 2^-7: error 2^-8 - tiny); the CPU test pins that example.
  A is the sum of the absolute values of the terms the kernel adds for the element, c the number of fp32 roundings on the longest chain
    a term passes (standard fp32 summation bound: error <= chain * 2^-24 * sum |terms|), k = 2 where the fp32 value is rounded once more to
    bf16 (nearest(v) is at most half_ulp(ref) + 2 |v - ref| from ref), else 1.
bf16 kernels are compared with the reference on the bf16-rounded inputs.  Where a kernel stores an intermediate that later results are
defined on (s of the LayerNorm forward, dz of the bias sums, the Adam state of the previous step), the reference starts from the stored
values: the stored tensor is itself checked, so nothing escapes, and no rounding flip of the intermediate is charged to its consumers.

c, one line per kernel (V = 4 f32 / 8 bf16 elements per lane and load; L(d) = V * ceil(d / 64V) lane-serial adds of a row):
  ln s_out          c = 2            alpha * x rounded, + r rounded (one rounding if contracted to an fma)
  ln mean           c = L(d) + 7     lane-serial L(d), 6 butterfly steps, the division;  A = mean |s|
  ln rstd           c = L(d) + 13    (s - mu), square, the same chain, + eps, rsqrtf (<= 2 ulp = 4), final; relative: A = rstd
  ln y              c = L(d) + 17    mean and rstd errors carried (L(d) + 13), (s - mu), * rs, * gamma, + beta;
                                     A = rs |gamma| (|s| + |mu| + mean |s|) + |beta|
  ln ds             c = L(d) + 14    g = dy * gamma, x^ (2), g * x^, chain L(d) + 7, then - c1, x^ * c2, - , * rs;
                                     A = rs (|g| + mean |g| + |x^| mean |g x^|): c1 = mean g and c2 = mean g x^ are sums themselves, and the
                                     terms they add are g_j / d and g_j x^_j / d.  (A = rs (|g| + |c1| + |x^ c2|) is no bound: where c1 cancels
                                     to nothing its rounding error does not, and the fp32 model misses that A in f32 at d = 132 and 2048.)
  ln dgamma, dbeta  c = 3 + chain    x^ (2) and the product, then: fused  rpb / 4 rows of a wave, 3 wave adds, ceil(nblocks / 16) partials of a
                                     reduce wave, 15 wave adds, the accumulator;  generic  rows + 1.   A = sum_r |dy x^| (|dy|) + |acc0|
  ln parts          c = 3 + rpb / 4 + 3 per block; parts.sum(0) in float64 adds none
  gelu (fp32)       c = 8            x / sqrt 2 (1), erff <= 2 ulp (4 in units of 2^-24), 1 + erf, 0.5 *, * x
  gelu (bf16 path)  c = 12           Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7 = 2.52 * 2^-24, one v_exp (2) and one v_rcp (2), 5 fma, scale
                                     A(gelu) = 0.5 |x| (1 + |erf|);  A(gelu') = 0.5 (1 + |erf|) + |x| pdf(x), c + 3 (x * pdf, exp, add)
  geglu / gated     + 2 for the two products with a and dout;  relu: exact, bound 0
  act bias sums     c = rpc + ceil(nchunks / 16) + 16     rows of a chunk in order, then the 16-wave ordered reduce and the accumulator
  colsum            scalar: rows + 1;  one workgroup: ceil(rows / 4) + 4;  chunked: rpc / 4 + 3 + ceil(nchunks / 16) + 16.   A = sum |x| + |acc0|
  sumsq_acc         c = V ceil(nv / 256) + 12             squares (1), lane-serial, tail (1), 6 + 3 block tree, accumulator.  A = sum x^2 + |acc0|
  sumsq_det         c = V ceil(nv / 256 g) + 11 + ceil(g / 256) + 10      g = min(4096, ceil((nv + 1) / 256)) blocks, then the final block
  adam              m: c = 12 (gs <= 7: sqrt, *, +, /, min, *, * g;  casts of beta1, 1 - beta1;  2 products, 1 add);  v: c = 24 (gr twice, casts, 3);
                    p: 4 |p| + (ss / denom) c_m A_m + |upd| (10 + c_v A_v / (2 sqrt(v) sqrt(bc2) denom)), in units of 2^-24
                    (float casts of lr, 1 - lr wd, bias corrections, eps; sqrt, *, +, *, /, -)
add / add2d / cast are exact or one rounding: compared bit for bit."""
import math
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import db1_oracle as O  # noqa: E402
from oracle.db1_oracle import _erf  # noqa: E402

U = 2.0 ** -24
TINY = 2.0 ** -126
SHARE = 1.0               # the share of the fp32 allowance k c 2^-24 A that check() grants; the CPU proof runs the model at 0.5
SENT = -7680.0            # what outputs and guard margins hold before a call (exact in bf16 and f32; no reference value comes near it)
EPS = 1e-5
BFMAX = 3.3895313892515355e38   # largest finite bf16
SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0, BFMAX], np.float32)
GELU_C = {"f32": 8, "bf16": 12}   # c of gelu (fp32 erff path) and gelu (bf16 storage path) in the table above
ADAM_HP = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
MUTANTS = ("drop_last_row", "tail_reads_past", "last_colvec_unwritten", "geglu_half_at_c", "swap_dgdb_group", "stale_waves", "acc_assign",
           "skip_tail", "swap_bf16_pair", "gscale_once", "no_s_round")


# ------------------------------------------------------------------------------------------------ formats
def bf16(a):
    """float32 values rounded to bf16 (nearest even), returned as float32"""
    shape = np.shape(a)
    u = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(shape)


def rnd(a, dt):
    return bf16(a) if dt == "bf16" else np.ascontiguousarray(a, np.float32)


def vec(dt):
    return 8 if dt == "bf16" else 4


def half_ulp(ref, dt):
    ref = np.abs(np.asarray(ref, np.float64))
    _, e = np.frexp(ref)                       # ref = m 2^e, 0.5 <= m < 1: one ulp is 2^(e - p)
    return np.where(ref > 0, np.ldexp(0.5, e - (8 if dt == "bf16" else 24)), 0.0)


def bound(ref, A, c, dt, exact=False):
    if exact:
        return np.zeros(np.shape(ref))
    k = 2.0 if dt == "bf16" else 1.0
    return np.maximum(half_ulp(ref, dt) + SHARE * k * c * U * np.asarray(A, np.float64), TINY)


def ratio(got, ref, bnd):
    """per element |got - ref| / bound (inf where got is not finite and ref is, or where a zero bound is missed)"""
    got, ref, bnd = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bnd, np.float64)
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got - ref)
        q = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isfinite(got) | ~np.isfinite(ref), q, np.inf)
    return np.where(np.isnan(q), np.inf, q)


def check(got, ref, bnd, name):
    q = ratio(got, ref, bnd)
    over = q > 1.0
    if over.any():
        i = np.unravel_index(np.argmax(q), q.shape) if q.ndim else ()
        g, r, b = np.asarray(got, np.float64)[i], np.asarray(ref, np.float64)[i], np.asarray(bnd, np.float64)[i]
        raise AssertionError(f"{name}: {int(over.sum())} of {q.size} elements over bound; worst at {tuple(int(x) for x in i)}: got {g!r} ref {r!r} "
                             f"bound {b:.3e} excess {abs(g - r) - b:.3e}")
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------------------------------------ dispatcher arithmetic (as in the .hip)
def ln_fused(dt, d):
    return dt == "bf16" and d in (512, 1024, 2048)


def ln_bwd_rpb(rows):
    rpb = 32
    while rpb > 4 and (rows + rpb - 1) // rpb < 512:
        rpb >>= 1
    return rpb


def act_fwd_rpc(rows):
    return 64 if rows >= 32768 else (32 if rows >= 4096 else 8)


def act_bias_rpc(rows):
    return 64 if rows >= 32768 else 32


def colsum_rpc(rows):
    rpc = 32
    while rows // rpc > 1024:
        rpc *= 2
    return rpc


def colsum_path(case):
    V = vec(case["dt"])
    ok = case["cols"] % V == 0 and colsum_ld(case) % V == 0 and case.get("variant") != "offset1"
    return ("chunk" if case["rows"] >= 1024 else "vec") if ok else "scalar"


def colsum_ld(case):
    v = case.get("variant", "plain")
    return case["cols"] + {"plain": 0, "offset1": 0, "strided": 2 * vec(case["dt"]), "odd_ld": 1}[v]


def sumsq_grid(n, V):
    return max(1, min(4096, (n // V + 1 + 255) // 256))


def L(d, V):
    return V * -(-d // (64 * V))


# ------------------------------------------------------------------------------------------------ fp32 building blocks
_IDX = np.arange(64)


def _wave_sum(x):
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., _IDX ^ o]
    return x[..., 0]


def _row_sum(a, V):
    """a row reduced as a wave does it: lane l adds the elements of its vectors l, l + 64, ... in order, then the xor butterfly"""
    rows, d = a.shape
    K = -(-d // (64 * V))
    t = np.zeros((rows, K * 64 * V), np.float32)
    t[:, :d] = a
    t = t.reshape(rows, K, 64, V)
    acc = np.zeros((rows, 64), np.float32)
    for k in range(K):
        for j in range(V):
            acc = acc + t[:, k, :, j]
    return _wave_sum(acc)


def _pad_rows(a, n):
    out = np.zeros((n,) + a.shape[1:], np.float32)
    out[:a.shape[0]] = a
    return out


def _block4(a, rows_per):
    """(rows, cols) -> per-block sums: wave w of a block adds rows w, w + 4, ... of the block in order, then ((w0 + w1) + w2) + w3"""
    nb = -(-a.shape[0] // rows_per)
    t = _pad_rows(a, nb * rows_per).reshape(nb, rows_per // 4, 4, a.shape[1])
    acc = np.zeros((nb, 4, a.shape[1]), np.float32)
    for i in range(rows_per // 4):
        acc = acc + t[:, i]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def _reduce16(part, acc0, mutant=None):
    """the 16-wave ordered reduce: wave w adds partial rows w, w + 16, ... in order; the 16 sums are added in wave order onto the accumulator"""
    nc, cols = part.shape
    K = -(-nc // 16)
    P = _pad_rows(part, K * 16)
    if mutant == "stale_waves" and nc < 16:
        P[nc:16] = part[0]
    P = P.reshape(K, 16, cols)
    acc = np.zeros((16, cols), np.float32)
    for k in range(K):
        acc = acc + P[k]
    t = acc[0]
    with np.errstate(over="ignore"):        # (a mutant may add the largest finite bf16 to itself)
        for w in range(1, 16):
            t = t + acc[w]
    return t if mutant == "acc_assign" else acc0 + t


def _erf32(x):
    return _erf(x.astype(np.float64)).astype(np.float32)


def _phi_fast(x):
    with np.errstate(over="ignore", under="ignore"):
        t = np.abs(x) * np.float32(0.70710678118654752440)
        e = np.exp2(x * x * np.float32(-0.72134752044448170368)).astype(np.float32)
        k = np.float32(1.0) / (np.float32(0.3275911) * t + np.float32(1.0))
        poly = np.float32(1.061405429) * k + np.float32(-1.453152027)
        for c in (1.421413741, -0.284496736, 0.254829592):
            poly = poly * k + np.float32(c)
        erf_abs = -poly * k * e + np.float32(1.0)
    return np.float32(0.5) + np.copysign(np.float32(0.5) * erf_abs, x), e


def _gelu_both(x, dt):
    """(gelu(x), gelu'(x)) in float32 as gelu_both_t<T> computes them"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if dt == "f32":
            e = _erf32(x * np.float32(0.70710678118654752440))
            y = np.float32(0.5) * x * (np.float32(1.0) + e)
            dy = np.float32(0.5) * (np.float32(1.0) + e) + x * np.exp(np.float32(-0.5) * x * x).astype(np.float32) * np.float32(0.39894228040143267794)
            return y, dy
        phi, e = _phi_fast(x)
        return x * phi, x * np.float32(0.39894228040143267794) * e + phi


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def _n32(rng, shape, scale=1.0, shift=0.0):
    return rng.standard_normal(shape, dtype=np.float32) * np.float32(scale) + np.float32(shift)


def acc0_vec(n):
    """what accumulators hold before a call: non-zero and not constant, so that '=' for '+=' and a shifted column both show"""
    return (0.5 + 0.25 * (np.arange(n) % 5)).astype(np.float32)


def act_ld(case):
    return 2 * case["n"] if case["act"] == "geglu" else case["n"]


def inputs(case):
    rng, op, dt = _rng(case), case["op"], case.get("dt")
    if op == "ln_fwd":
        rows, d, pdt = case["rows"], case["d"], case["pdt"]
        return dict(x=rnd(_n32(rng, (rows, d)), dt), r=rnd(_n32(rng, (rows, d), 1.0, 0.5), dt) if case["r"] else None,
                    gamma=rnd(_n32(rng, d, 0.1, 1.0), pdt), beta=rnd(_n32(rng, d, 0.1), pdt))
    if op == "ln_bwd":
        rows, d, pdt = case["rows"], case["d"], case["pdt"]
        s = rnd(_n32(rng, (rows, d), 1.3, 0.5), dt)
        s64 = s.astype(np.float64)
        mu = s64.mean(-1)
        rs = 1.0 / np.sqrt(((s64 - mu[:, None]) ** 2).mean(-1) + EPS)
        return dict(dy=rnd(_n32(rng, (rows, d)), dt), s=s, gamma=rnd(_n32(rng, d, 0.1, 1.0), pdt), mean=mu.astype(np.float32), rstd=rs.astype(np.float32),
                    dg0=acc0_vec(d), db0=acc0_vec(d)[::-1].copy())
    if op in ("act_fwd", "act_bwd", "act_bwd_bias"):
        rows, n, ld = case["rows"], case["n"], act_ld(case)
        z, dout = _n32(rng, (rows, ld), 1.5), _n32(rng, (rows, n))
        k = len(SPECIALS)
        flat = np.concatenate([np.arange(k), rows * n - k + np.arange(k)])   # the first and the last elements of the gelu argument
        r_, c_ = flat // n, flat % n
        z[r_, c_ + (ld - n)] = np.tile(SPECIALS, 2)
        if case["act"] == "geglu":
            z[r_, c_] = 0.5
        dout[r_, c_] = 0.5
        return dict(z=rnd(z, dt), dout=rnd(dout, dt), acc0=acc0_vec(ld))
    if op == "colsum":
        return dict(x=rnd(_n32(rng, (case["rows"], case["cols"]), 1.0, 0.25), dt), acc0=acc0_vec(case["cols"]))
    if op in ("sumsq_acc", "sumsq_det"):
        return dict(x=rnd(_n32(rng, case["n"]), dt), acc0=np.float32(0.75))
    if op == "adam":
        n, gdt, kind = case["n"], case["gdt"], case.get("grads", "normal")
        g = []
        for step in (1, 2, 3):
            a = _n32(rng, n, 0.1 if step == 2 else 2.0)
            if kind == "small":
                a = a * np.float32(0.5 / math.sqrt(n) / 2.0)       # ||g|| about 0.5 (0.025 at step 2): the clip is on and does nothing
            if kind == "zero2" and step == 2:
                a = np.zeros(n, np.float32)
            g.append(rnd(a * np.float32(1.0 / case["gscale"]), gdt))
        nsq = [np.float32((a.astype(np.float64) ** 2).sum()) for a in g]
        return dict(p0=_n32(rng, n), g=g, nsq=nsq)
    if op in ("add", "add2d", "cast"):
        rows, cols = case["rows"], case["cols"]
        return dict(a=rnd(_n32(rng, (rows, cols)), case["adt"]), b=rnd(_n32(rng, (rows, cols), 2.0), dt))
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ fp32 models (with mutants)
def model(case, inp, mutant=None):
    """what the kernel of this case stores, in float32 arithmetic and the kernel's own order; outputs start as SENT, accumulators as acc0"""
    return globals()["_model_" + case["op"]](case, inp, mutant)


def _model_ln_fwd(case, inp, mutant):
    dt, V, d = case["dt"], vec(case["dt"]), case["d"]
    s = np.float32(case["alpha"]) * inp["x"]
    if inp["r"] is not None:
        s = s + inp["r"]
    stored = rnd(s, dt)
    a = s if mutant == "no_s_round" else stored
    mu = _row_sum(a, V) / np.float32(d)
    c = a - mu[:, None]
    rs = np.float32(1.0) / np.sqrt(_row_sum(c * c, V) / np.float32(d) + np.float32(EPS))
    y = rnd(c * rs[:, None] * inp["gamma"] + inp["beta"], dt)
    got = dict(y=y, mean=mu, rstd=rs, _s=stored)
    if case["s_out"]:
        got["s_out"] = stored
    return got


def _model_ln_bwd(case, inp, mutant):
    dt, V, rows, d = case["dt"], vec(case["dt"]), case["rows"], case["d"]
    dy, s, mu, rs = inp["dy"], inp["s"], inp["mean"][:, None], inp["rstd"][:, None]
    xh = (s - mu) * rs
    g = dy * inp["gamma"]
    c1 = (_row_sum(g, V) / np.float32(d))[:, None]
    c2 = (_row_sum(g * xh, V) / np.float32(d))[:, None]
    ds = rnd(rs * (g - c1 - xh * c2), dt)
    A, B = dy * xh, dy.copy()
    fused = ln_fused(dt, d)
    rpb = ln_bwd_rpb(rows) if fused else rows
    partial = rows % rpb != 0
    extra = None
    if mutant == "drop_last_row" and partial:
        ds[rows - 1] = SENT
        A[rows - 1] = 0
        B[rows - 1] = 0
    if mutant == "tail_reads_past" and partial:      # the block tail takes the row after r1 (whatever memory follows: here a copy of row 0)
        extra = (A[0], B[0])
    got = dict(ds=ds)
    if not case["params"]:
        return got
    if fused:
        AB = np.concatenate([A, B], 1)
        if extra is not None:
            AB = np.concatenate([AB, np.concatenate(extra)[None]], 0)
        parts = _block4(AB, rpb)[:-(-rows // rpb)]
        if case.get("mode") == "parts":
            got["parts"] = parts
            return got
        t = _reduce16(parts, np.concatenate([inp["dg0"], inp["db0"]]), mutant)
        dg, db = t[:d].copy(), t[d:].copy()
    else:
        ag, ab = np.zeros(d, np.float32), np.zeros(d, np.float32)
        for r in range(rows):
            ag, ab = ag + A[r], ab + B[r]
        if extra is not None:
            ag, ab = ag + extra[0], ab + extra[1]
        dg, db = (ag, ab) if mutant == "acc_assign" else (inp["dg0"] + ag, inp["db0"] + ab)
    if mutant == "swap_dgdb_group" and d >= 128:
        dg[64:128], db[64:128] = db[64:128].copy(), dg[64:128].copy()
    got.update(dgamma=dg, dbeta=db)
    return got


def _act_apply(case, inp):
    dt, n, act = case["dt"], case["n"], case["act"]
    z, g = inp["z"], inp["dout"]
    with np.errstate(over="ignore", invalid="ignore"):
        if act == "geglu":
            a, b = z[:, :n], z[:, n:]
            y, dy = _gelu_both(b, dt)
            return a * y, (g * y, g * a * dy)
        if act == "gelu":
            y, dy = _gelu_both(z, dt)
            return y, (g * dy,)
        return np.maximum(z, np.float32(0)), (np.where(z > 0, g, np.float32(0)),)


def _model_act_fwd(case, inp, mutant):
    out = rnd(_act_apply(case, inp)[0], case["dt"])
    if mutant == "last_colvec_unwritten":
        out[:, -vec(case["dt"]):] = SENT
    return dict(out=out)


def _model_act_bwd(case, inp, mutant):
    dt, n = case["dt"], case["n"]
    halves = [rnd(h, dt) for h in _act_apply(case, inp)[1]]
    dz = np.concatenate(halves, 1)
    if mutant == "geglu_half_at_c" and case["act"] == "geglu":
        dz[:, :n], dz[:, n:] = halves[1], SENT
    if mutant == "last_colvec_unwritten":
        dz[:, -vec(dt):] = SENT
    return dict(dz=dz)


def _model_act_bwd_bias(case, inp, mutant):
    got = _model_act_bwd(case, inp, mutant if mutant in ("geglu_half_at_c", "last_colvec_unwritten") else None)
    rows, rpc = case["rows"], act_bias_rpc(case["rows"])
    dz = got["dz"].copy()
    if mutant == "drop_last_row" and rows % rpc:
        dz[rows - 1] = 0
    nch = -(-rows // rpc)
    t = _pad_rows(dz, nch * rpc).reshape(nch, rpc, dz.shape[1])
    part = np.zeros((nch, dz.shape[1]), np.float32)
    for i in range(rpc):
        part = part + t[:, i]
    got["dbias"] = _reduce16(part, inp["acc0"], mutant)
    return got


def _model_colsum(case, inp, mutant):
    x, rows, path = inp["x"].copy(), case["rows"], colsum_path(case)
    if path == "scalar":
        a = np.zeros(x.shape[1], np.float32)
        for r in range(rows - (mutant == "drop_last_row")):
            a = a + x[r]
        return dict(out=a if mutant == "acc_assign" else inp["acc0"] + a)
    rpc = colsum_rpc(rows) if path == "chunk" else 4 * -(-rows // 4)
    if mutant == "drop_last_row" and rows % rpc:
        x[rows - 1] = 0
    part = _block4(x, rpc)
    if path == "vec":
        return dict(out=part[0] if mutant == "acc_assign" else inp["acc0"] + part[0])
    return dict(out=_reduce16(part, inp["acc0"], mutant))


def _sumsq_blocks(x, V, nblocks, mutant):
    n, T = x.size, nblocks * 256
    nv = n // V
    trips = max(1, -(-nv // T))
    t = np.zeros(trips * T * V, np.float32)
    t[:nv * V] = x[:nv * V]
    t = t.reshape(trips, T, V)
    a = np.zeros(T, np.float32)
    for k in range(trips):
        for j in range(V):
            a = a + t[k, :, j] * t[k, :, j]
    tail = x[nv * V:]
    if tail.size and mutant != "skip_tail":
        a[:tail.size] = a[:tail.size] + tail * tail
    return _block_sum(a.reshape(nblocks, 256))


def _block_sum(a):
    w = _wave_sum(a.reshape(a.shape[0], 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _model_sumsq_acc(case, inp, mutant):
    a = _sumsq_blocks(inp["x"], vec(case["dt"]), 1, mutant)[0]
    return dict(acc=np.array([a if mutant == "acc_assign" else inp["acc0"] + a], np.float32))


def _model_sumsq_det(case, inp, mutant):
    V = vec(case["dt"])
    g = sumsq_grid(case["n"], V)
    part = _sumsq_blocks(inp["x"], V, g, mutant)
    K = -(-g // 256)
    t = _pad_rows(part[:, None], K * 256).reshape(K, 256)
    a = np.zeros(256, np.float32)
    for k in range(K):
        a = a + t[k]
    a = _block_sum(a[None])[0]
    return dict(acc=np.array([a if case["overwrite"] else inp["acc0"] + a], np.float32))


def _model_adam(case, inp, mutant):
    f, hp = np.float32, ADAM_HP
    p, m, v = inp["p0"].copy(), np.zeros_like(inp["p0"]), np.zeros_like(inp["p0"])
    got = {}
    for step in (1, 2, 3):
        g = inp["g"][step - 1]
        if mutant == "swap_bf16_pair" and case["gdt"] == "bf16":
            g = g.reshape(-1, 2)[:, ::-1].reshape(-1)
        gs = f(case["gscale"])
        if case["clip"] > 0 and case["nsq"]:
            nrm = np.sqrt(inp["nsq"][step - 1]) * (f(1) if mutant == "gscale_once" else f(case["gscale"]))
            gs = gs * min(f(1), f(case["clip"]) / (nrm + f(1e-6)))
        ss = f(hp["lr"]) / f(1.0 - hp["beta1"] ** step)
        rsq = f(1.0 / math.sqrt(1.0 - hp["beta2"] ** step))
        gr = g * gs
        if case["adamw"]:
            p = p * (f(1) - f(hp["lr"]) * f(hp["wd"]))
        else:
            gr = gr + f(hp["wd"]) * p
        m = m * f(hp["beta1"]) + f(1.0 - hp["beta1"]) * gr
        v = (v * f(hp["beta2"]) + f(1.0 - hp["beta2"]) * gr * gr) if mutant != "acc_assign" else f(1.0 - hp["beta2"]) * gr * gr
        p = p - ss * m / (np.sqrt(v) * rsq + f(hp["eps"]))
        got.update({f"p{step}": p.copy(), f"m{step}": m.copy(), f"v{step}": v.copy()})
        if case["pw"]:
            got[f"pw{step}"] = bf16(p)
    return got


# ------------------------------------------------------------------------------------------------ references and bounds
def expect(case, inp, got):
    """{output name: (float64 reference, per-element bound)} for every output of the case; ``got`` supplies the stored intermediates that
    later results are defined on (never the result under comparison itself)"""
    return globals()["_expect_" + case["op"]](case, inp, got)


def _d(a):
    return np.asarray(a, np.float64)


def _expect_ln_fwd(case, inp, got):
    dt, d, V = case["dt"], case["d"], vec(case["dt"])
    alpha = float(np.float32(case["alpha"]))
    ax = alpha * _d(inp["x"])
    r = _d(inp["r"]) if inp["r"] is not None else 0.0
    s = _d(got["_s"])
    y, (xhat, rstd) = O.layernorm_fwd(s, _d(inp["gamma"]), _d(inp["beta"]), EPS)
    mu, rstd = s.mean(-1), rstd[:, 0]
    mabs = np.abs(s).mean(-1)
    Ld = L(d, V)
    Ay = rstd[:, None] * np.abs(_d(inp["gamma"])) * (np.abs(s) + np.abs(mu)[:, None] + mabs[:, None]) + np.abs(_d(inp["beta"]))
    out = dict(y=(y, bound(y, Ay, Ld + 17, dt)), mean=(mu, bound(mu, mabs, Ld + 7, "f32")), rstd=(rstd, bound(rstd, rstd, Ld + 13, "f32")))
    sref = ax + r
    out["_s"] = (sref, bound(sref, np.abs(ax) + np.abs(r), 2, dt))
    if case["s_out"]:
        out["s_out"] = out["_s"]
    return out


def ln_param_chain(case):
    rows, d = case["rows"], case["d"]
    if not ln_fused(case["dt"], d):
        return 3 + rows + 1
    rpb = ln_bwd_rpb(rows)
    return 3 + rpb // 4 + 3 + -(-(-(-rows // rpb)) // 16) + 16


def _expect_ln_bwd(case, inp, got):
    dt, d, V = case["dt"], case["d"], vec(case["dt"])
    dy, s, gam, mu, rs = _d(inp["dy"]), _d(inp["s"]), _d(inp["gamma"]), _d(inp["mean"])[:, None], _d(inp["rstd"])[:, None]
    xh = (s - mu) * rs
    ds, dg, db = O.layernorm_bwd(dy, gam, (xh, rs))
    g = dy * gam
    m1, m2 = np.abs(g).mean(-1, keepdims=True), np.abs(g * xh).mean(-1, keepdims=True)
    out = dict(ds=(ds, bound(ds, rs * (np.abs(g) + m1 + np.abs(xh) * m2), L(d, V) + 14, dt)))
    if not case["params"]:
        return out
    Ag, Ab = np.abs(dy * xh).sum(0), np.abs(dy).sum(0)
    if case.get("mode") == "parts":
        ref = np.concatenate([dg, db])
        out["parts_sum"] = (ref, bound(ref, np.concatenate([Ag, Ab]), 3 + ln_bwd_rpb(case["rows"]) // 4 + 3, "f32"))
        return out
    c = ln_param_chain(case)
    out["dgamma"] = (dg + _d(inp["dg0"]), bound(dg + _d(inp["dg0"]), Ag + np.abs(_d(inp["dg0"])), c, "f32"))
    out["dbeta"] = (db + _d(inp["db0"]), bound(db + _d(inp["db0"]), Ab + np.abs(_d(inp["db0"])), c, "f32"))
    return out


def _act_terms(case, inp):
    """float64 references and A of (out, dz halves)"""
    n, act, dt = case["n"], case["act"], case["dt"]
    z, g = _d(inp["z"]), _d(inp["dout"])
    cg = GELU_C[dt]
    if act == "relu":
        return (np.maximum(z, 0.0), None, 0), [(g * (z > 0), None, 0)]
    x = z[:, n:] if act == "geglu" else z
    with np.errstate(over="ignore", under="ignore"):
        e = np.abs(_erf(x / math.sqrt(2.0)))
        y, dy = O.gelu(x), O.gelu_grad(x)
        Ay = 0.5 * np.abs(x) * (1.0 + e)
        Ady = 0.5 * (1.0 + e) + np.abs(x) * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == "gelu":
        return (y, Ay, cg), [(g * dy, np.abs(g) * Ady, cg + 4)]
    a = z[:, :n]
    return (a * y, np.abs(a) * Ay, cg + 1), [(g * y, np.abs(g) * Ay, cg + 1), (g * a * dy, np.abs(g * a) * Ady, cg + 5)]


def _expect_act_fwd(case, inp, got):
    ref, A, c = _act_terms(case, inp)[0]
    return dict(out=(ref, bound(ref, A, c, case["dt"], exact=A is None)))


def _expect_act_bwd(case, inp, got):
    hs = _act_terms(case, inp)[1]
    ref = np.concatenate([h[0] for h in hs], 1)
    bnd = np.concatenate([bound(h[0], h[1], h[2], case["dt"], exact=h[1] is None) for h in hs], 1)
    return dict(dz=(ref, bnd))


def _expect_act_bwd_bias(case, inp, got):
    out = _expect_act_bwd(case, inp, got)
    rows, rpc = case["rows"], act_bias_rpc(case["rows"])
    dz, a0 = _d(got["dz"]), _d(inp["acc0"])
    ref = dz.sum(0) + a0
    out["dbias"] = (ref, bound(ref, np.abs(dz).sum(0) + np.abs(a0), rpc + -(-(-(-rows // rpc)) // 16) + 16, "f32"))
    return out


def colsum_chain(case):
    rows, path = case["rows"], colsum_path(case)
    if path == "scalar":
        return rows + 1
    if path == "vec":
        return -(-rows // 4) + 4
    rpc = colsum_rpc(rows)
    return rpc // 4 + 3 + -(-(-(-rows // rpc)) // 16) + 16


def _expect_colsum(case, inp, got):
    x, a0 = _d(inp["x"]), _d(inp["acc0"])
    ref = x.sum(0) + a0
    return dict(out=(ref, bound(ref, np.abs(x).sum(0) + np.abs(a0), colsum_chain(case), "f32")))


def _expect_sumsq_acc(case, inp, got):
    V = vec(case["dt"])
    x = _d(inp["x"])
    ref = np.array([(x * x).sum() + float(inp["acc0"])])
    return dict(acc=(ref, bound(ref, ref, V * -(-(case["n"] // V) // 256) + 12, "f32")))


def _expect_sumsq_det(case, inp, got):
    V, n = vec(case["dt"]), case["n"]
    g = sumsq_grid(n, V)
    x = _d(inp["x"])
    a0 = 0.0 if case["overwrite"] else float(inp["acc0"])
    ref = np.array([(x * x).sum() + a0])
    return dict(acc=(ref, bound(ref, ref, V * -(-(n // V) // (256 * g)) + 11 + -(-g // 256) + 10, "f32")))


def _expect_adam(case, inp, got):
    hp, out = ADAM_HP, {}
    p, m, v = _d(inp["p0"]), np.zeros(case["n"]), np.zeros(case["n"])
    gscale = float(np.float32(case["gscale"]))
    for step in (1, 2, 3):
        g = _d(inp["g"][step - 1])
        coef = O.clip_coef(math.sqrt(float(inp["nsq"][step - 1])) * gscale, case["clip"]) if case["clip"] > 0 and case["nsq"] else 1.0
        S = gscale * coef
        pr, mr, vr = O.adam_step(p, g, m, v, step, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], case["adamw"], grad_scale=S)
        grA = np.abs(g * S) + (0.0 if case["adamw"] else hp["wd"] * np.abs(p))
        Am = hp["beta1"] * np.abs(m) + (1 - hp["beta1"]) * grA
        Av = hp["beta2"] * v + (1 - hp["beta2"]) * grA * grA
        bc1, bc2 = 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step
        denom = np.sqrt(vr) / math.sqrt(bc2) + hp["eps"]
        ss = hp["lr"] / bc1
        upd = np.abs(ss * mr / denom)
        with np.errstate(divide="ignore", invalid="ignore"):
            dden = np.where(vr > 0, 24 * Av / (2 * np.sqrt(vr) * math.sqrt(bc2) * denom), 0.0)
        Ap = 4 * np.abs(p) + ss / denom * 12 * Am + upd * (10 + dden)
        out[f"p{step}"] = (pr, bound(pr, Ap, 1, "f32"))
        out[f"m{step}"] = (mr, bound(mr, Am, 12, "f32"))
        out[f"v{step}"] = (vr, bound(vr, Av, 24, "f32"))
        if case["pw"]:
            pw = _d(bf16(got[f"p{step}"]))
            out[f"pw{step}"] = (pw, np.zeros_like(pw))
        p, m, v = _d(got[f"p{step}"]), _d(got[f"m{step}"]), _d(got[f"v{step}"])     # the next step starts from what was stored
    return out


# ------------------------------------------------------------------------------------------------ the case table
def _mk(op, **kw):
    kw["op"] = op
    kw["id"] = op + "-" + "-".join(f"{k}{v}" if not isinstance(v, str) else v for k, v in kw.items() if k != "op")
    return kw


def _cases():
    C = []
    ln_shapes = [("bf16", d) for d in (512, 1024, 2048, 8, 264, 1536, 4096)] + [("f32", d) for d in (4, 132, 2048)]
    for dt, d in ln_shapes:
        for rows in (1, 5, 37):
            C.append(_mk("ln_fwd", dt=dt, pdt=dt, rows=rows, d=d, r=True, s_out=True, alpha=1.3))
            C.append(_mk("ln_bwd", dt=dt, pdt=dt, rows=rows, d=d, params=True))
    for dt, pdt, d in (("bf16", "f32", 512), ("bf16", "f32", 264), ("f32", "bf16", 132), ("f32", "bf16", 2048)):   # mixed (T, TP); same-dtype pairs are above
        C.append(_mk("ln_fwd", dt=dt, pdt=pdt, rows=5, d=d, r=True, s_out=True, alpha=1.3))
        C.append(_mk("ln_bwd", dt=dt, pdt=pdt, rows=5, d=d, params=True))
    for dt, d in (("bf16", 1024), ("bf16", 264), ("f32", 132)):
        C.append(_mk("ln_fwd", dt=dt, pdt=dt, rows=5, d=d, r=False, s_out=True, alpha=1.3))
        C.append(_mk("ln_fwd", dt=dt, pdt=dt, rows=5, d=d, r=True, s_out=False, alpha=1.3))
        C.append(_mk("ln_fwd", dt=dt, pdt=dt, rows=5, d=d, r=False, s_out=False, alpha=1.0))
        C.append(_mk("ln_bwd", dt=dt, pdt=dt, rows=5, d=d, params=False))
    for rows in (4088, 4089, 8177, 16353):          # rows per block 4, 8, 16, 32; the last block of the last three holds one row
        C.append(_mk("ln_bwd", dt="bf16", pdt="bf16" if rows != 8177 else "f32", rows=rows, d=512, params=True))
    C.append(_mk("ln_bwd", dt="bf16", pdt="f32", rows=4091, d=2048, params=True))
    C.append(_mk("ln_bwd", dt="bf16", pdt="bf16", rows=4089, d=512, params=False))
    for rows, d in ((5, 512), (37, 1024), (4089, 512)):
        C.append(_mk("ln_bwd", dt="bf16", pdt="bf16", rows=rows, d=d, params=True, mode="parts"))
    for act in ("geglu", "gelu", "relu"):
        for dt in ("f32", "bf16"):
            n = 1028 if dt == "f32" else 2056
            for rows in (1, 9, 33, 65, 545):
                for op in ("act_fwd", "act_bwd", "act_bwd_bias"):
                    C.append(_mk(op, act=act, dt=dt, rows=rows, n=n))
            for rows in (4097, 32769):
                C.append(_mk("act_fwd", act=act, dt=dt, rows=rows, n=vec(dt)))
            C.append(_mk("act_bwd_bias", act=act, dt=dt, rows=32769, n=vec(dt)))
    C.append(_mk("act_bwd", act="relu", dt="f32", rows=4081, n=1028))       # 4081 * 257 vectors > 2^20: the grid-stride loop's second trip
    for dt in ("f32", "bf16"):
        for rows in (1023, 1024, 1025, 32801):
            for cols in (8, 72, 520):
                C.append(_mk("colsum", dt=dt, rows=rows, cols=cols, variant="plain"))
        for rows in (300, 1025):
            C.append(_mk("colsum", dt=dt, rows=rows, cols=72, variant="strided"))
            C.append(_mk("colsum", dt=dt, rows=rows, cols=72, variant="odd_ld"))
            C.append(_mk("colsum", dt=dt, rows=rows, cols=72, variant="offset1"))
    for dt, ns in (("f32", (3, 4099)), ("bf16", (5, 4101))):
        for n in ns:
            C.append(_mk("sumsq_acc", dt=dt, n=n))
        for ow in (0, 1):
            C.append(_mk("sumsq_det", dt=dt, n=ns[1], overwrite=ow))
            C.append(_mk("sumsq_det", dt=dt, n=4 * 2 ** 20 + 5, overwrite=ow))          # past the grid cap of 4096 blocks
    A = lambda **kw: C.append(_mk("adam", **{**dict(gdt="f32", n=4104, adamw=True, pw=True, g8=False, gscale=1.0, clip=1.0, nsq=True, grads="normal"), **kw}))
    for adamw in (True, False):
        for gdt in ("f32", "bf16"):
            A(gdt=gdt, adamw=adamw)
    A(gdt="bf16", g8=True)                              # g 8-byte but not 16-byte aligned
    A(gdt="bf16", pw=False)
    A(pw=False, adamw=False)
    for n in (4, 4 * (2 ** 20 + 3)):
        A(n=n)
        A(n=n, gdt="bf16", g8=True)
    A(gscale=1.0 / 1024)
    A(gscale=1.0 / 1024, gdt="bf16", adamw=False)
    A(grads="small")
    A(clip=0.0)
    A(nsq=False)
    A(grads="zero2")
    A(grads="zero2", gdt="bf16")
    for dt in ("f32", "bf16"):
        V = vec(dt)
        for cols, form in ((16 * V, "vec"), (16 * V + 1, "scalar")):
            C.append(_mk("add", dt=dt, adt=dt, rows=37, cols=cols, form=form, alias=False))
        C.append(_mk("add", dt=dt, adt=dt, rows=37, cols=16 * V, form="offset1", alias=True))
        C.append(_mk("add", dt=dt, adt=dt, rows=4100, cols=256 * V + V, form="vec", alias=True))       # > 4096 * 256 vectors: grid-stride
        for form in ("vec", "odd_cols", "odd_ld", "mixed"):
            adt = dt if form != "mixed" else ("bf16" if dt == "f32" else "f32")
            C.append(_mk("add2d", dt=dt, adt=adt, rows=37, cols=16 * V + (form == "odd_cols"), form=form, alias=form != "vec"))
        C.append(_mk("add2d", dt=dt, adt=dt, rows=37, cols=16 * V, form="vec", alias=True))
        for odt in ("f32", "bf16"):
            C.append(_mk("cast", dt=odt, adt=dt, rows=37, cols=67, form="any", alias=False))
    C.append(_mk("cast", dt="bf16", adt="f32", rows=4100, cols=257, form="any", alias=False))           # > 4096 * 256 elements: grid-stride
    return C


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def cases(*ops):
    return [c for c in CASES if c["op"] in ops]


def elements(case):
    if "n" in case and "rows" not in case:
        return case["n"]
    return case["rows"] * (case.get("d") or case.get("cols") or act_ld(case))


def value(got, name):
    """the stored result that the expectation ``name`` is compared with"""
    return got["parts"].astype(np.float64).sum(0) if name == "parts_sum" else got[name]


def cheap(case):
    """small enough for the CPU proof (the rest runs on the GPU only; every bound formula keeps cheap cases)"""
    return elements(case) <= (1 << 21) and not (case["op"] == "colsum" and colsum_path(case) == "scalar" and case["rows"] > 2000)
