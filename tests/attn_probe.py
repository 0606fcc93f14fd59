"""Index-revealing probes for the relative-position attention kernels: a probe builder, ONE float64 closed form for both geometries
(training: mlen = 0, q = klen = L; inference: q new rows against klen = mlen + q keys), the same closed form with bf16 rounding where the
kernels round (it only sizes the tolerance), and mutants of the closed form (never of a kernel) that the CPU test uses to prove that a
one-off index or mask error moves the result by at least ten tolerances.  numpy only: neither torch nor the library is imported here.

Geometry (relattn_decode.hip and relattn_decode_step.h, oracle.db1_oracle.attention_mask_dense):
    score[i, j] = ((q_i + u).k_j + (q_i + v).R[clip(mlen + i - j, 0, nd - 1)]) * scale,   visible iff  i - shift < j <= i + mlen
so the oldest visible key of row i is max(0, i - shift + 1) and the window holds up to shift + mlen keys (`shift` is the kernels' argument).

The probe.  Every value is exactly representable in bf16, q + u and q + v too, and every raw dot product is a multiple of 2^-6 below 2^11: the
scores are exact in fp32 whatever the summation order, so the only rounding left is exp, P -> bf16, the accumulations of P.V and the stores.
  K[b, j, h]  one-hot (value 16) at dim  (j + 7 b + 13 h) % pk           (dims 0 .. pk - 1)        + noise in {0, +-1/4} on its own dims
  R[d, h]     one-hot (value 16) at dim  pk + (d + 9 h) % pr            (dims pk .. pk + pr - 1)  + noise in {0, +-1/4} on its own dims
              (pk, pr): one of PERIODS, e.g. (67, 61), chosen per geometry -- see build()
  q[b, i, h]  selects (key t, distance mlen + i - t) PAIRS: weight w at K's dim of t and at R's dim of the distance.  A key scores
              16 (w_K + w_R) scale = 1.414 (w_K + w_R): both channels are needed, and a key that matches one channel only (the codes repeat
              every pk keys / pr distances, jointly every pk pr > 3700) is e^-8 below a target.
      targets (w = 6, score 17): the oldest visible key, the diagonal key i + mlen (distance 0), one mid-window key that differs per (b, h, i)
      decoys  (w = 8): key i - shift, one past the old edge (score 22.6), and key i + mlen + 1, one into the future (its distance -1 clamps to
              R[0], which the diagonal target selected: score 19.8).  Admitting either moves most of the row's mass.
  u, v        multiples of 1/4 in [-1/2, 1/2], u on K's dims and v on R's dims, different per head: swapping them moves scores by ~0.7
  V, dout     entries in {+-1/2, +-1}, different for every (b, key, h): a wrong batch / head stride or key index shows in the output

Two things that go beyond the plain rules, stated here so that nobody has to find them in the code:
  * applicability.  A mutant is applicable where it changes a pair (visibility, or the R row of a visible pair).  One EXTRA exclusion: a
    changed R row in a query row with ONE visible key does not count (changed_pairs), because out and every gradient are blind to the
    score of a lone key.  lse is not blind; the CPU test proves the margin on lse for every such case instead (shift = 1).
  * the rounded lse.  Besides the rounding points q + u, q + v, P before P.V, the stored output and dT / dS, the rounded model takes the row
    sum for lse over the bf16 p~.  Only relattn_flash_fwd3 (the default loop when probabilities are kept at shift >= L) sums that way;
    the other forwards sum the fp32 p~.  One lse tolerance, sized by this point (about 6.5e-3), is used for all of them.
"""
import functools

import numpy as np

D = 128
AMP, W_T, W_D = 16.0, 6.0, 8.0
SCALE = 1.0 / np.sqrt(128.0)
B, H = 2, 2


# ------------------------------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """round to nearest even bf16, returned as float64 (finite inputs)"""
    a = np.ascontiguousarray(np.asarray(x, np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def ulp(x, bits):
    """spacing of a format with `bits` significant bits (bf16: 8, float32: 24) at magnitude x"""
    x = float(x)
    return 0.0 if x == 0.0 else 2.0 ** (np.floor(np.log2(x)) - (bits - 1))


def tolerance(ref, rounded, bits=8):
    """4 x what the rounded model moves + one last place of the stored format at max|ref| (bits = 8: bf16, 24: float32).  Per tensor; the
    comparison is per element, |got - ref| <= tol.  The 4 covers what the model leaves out: fp32 accumulation order, exp2 vs exp, deferred maxima."""
    fin = np.isfinite(ref)
    return 4.0 * float(np.abs(np.where(fin, ref - rounded, 0.0)).max()) + ulp(np.abs(np.where(fin, ref, 0.0)).max(), bits)


F32_KEYS = ("lse", "delta")       # stored as float32; everything else is (assembled from) bf16 stores


def tolerances(ref, rnd):
    return {k: tolerance(ref[k], rnd[k], 24 if k in F32_KEYS else 8) for k in ref if k in rnd}


# ------------------------------------------------------------------------------------------------------------------ geometry + mutants
def geometry(q, klen, mlen, shift, nd):
    i = np.arange(q)[:, None]
    j = np.arange(klen)[None, :]
    vis = (j > i - shift) & (j <= i + mlen)
    dist = np.clip(mlen + i - j, 0, nd - 1)
    return vis, dist


MASK_MUTANTS = ("lo+1", "lo-1", "hi+1", "hi-1", "dist+1", "dist-1", "noclamp", "skip_last", "skip_first", "rring")


def mutate_geometry(name, q, klen, mlen, shift, nd):
    """(vis, dist) of the closed form under one index / mask error.
    lo+-1 / hi+-1   the window's old / new edge moved by one key
    dist+-1         the relative distance one off (then clamped as usual)
    noclamp         the distance wraps modulo nd instead of clamping
    skip_last       a block skip (`j0 + 31 <= i0 - shift`) one too eager: a row loses the 32-key block of which it sees the LAST key only
    skip_first      a block skip (`j0 > i0 + 15 + mlen`) one too eager: a row loses the block of which it sees the FIRST key only (its diagonal key)
    rring           the 256-row R ring one slot off after its first wrap: distances >= 256 read R[d - 1]
    Not a mutant: "keys at or past klen not zeroed".  The rows a 32-key step clamps to klen - 1 stand for keys j >= klen > i + mlen, in the
    future of every query: the causal test hides them whatever their scores, so the closed form (which has no such keys) cannot change."""
    i = np.arange(q)[:, None]
    j = np.arange(klen)[None, :]
    lo, hi, raw = i - shift, i + mlen, mlen + i - j
    vis, dist = geometry(q, klen, mlen, shift, nd)
    if name in ("lo+1", "lo-1"):
        vis = (j > lo + (1 if name == "lo+1" else -1)) & (j <= hi)
    elif name in ("hi+1", "hi-1"):
        vis = (j > lo) & (j <= hi + (1 if name == "hi+1" else -1))
    elif name in ("dist+1", "dist-1"):
        dist = np.clip(raw + (1 if name == "dist+1" else -1), 0, nd - 1)
    elif name == "noclamp":
        dist = np.mod(raw, nd)
    elif name == "skip_last":
        vis = vis & ~((j == lo + 1) & (j % 32 == 31))
    elif name == "skip_first":
        vis = vis & ~((j == hi) & (j % 32 == 0))
    elif name == "rring":
        dist = np.where(dist >= 256, dist - 1, dist)
    else:
        raise KeyError(name)
    return vis, dist


def changed_pairs(geo, mut):
    """(i, j) pairs whose visibility changes, or that stay visible and read another R row -- in a row with more than one visible key.
    That last condition is an exclusion of its own, beyond "changes no pair": where a row sees ONE key, out and every gradient are blind to
    that key's score (p = 1, dS = 0), so no margin on them exists.  lse is not blind, and test_one_key_windows_show_their_distance_in_lse
    asserts the margin on lse for every such case (the shift = 1 entries of FLASH_FWD_CASES), which the device test checks per element."""
    (v0, d0), (v1, d1) = geo, mut
    several = (v0.sum(1, keepdims=True) > 1)      # the softmax over ONE key does not depend on its score: no result can show that key's R row
    return (v0 != v1) | (v0 & v1 & (d0 != d1) & several)


# ------------------------------------------------------------------------------------------------------------------ the closed form
def _T(x):
    return x.transpose(0, 2, 1, 3)


def forward(p, geo=None, rounded=False):
    """p: dict q [B,q,H,D], k, v [B,klen,H,D], R [nd,H,D], u, vb [H,D], mlen, shift, scale.  Returns out [B,q,H,D], lse [B,H,q] and the cache
    for backward().  rounded: bf16 at q + u, q + v, P before P.V and the stored output; lse from the row sum of the bf16 p~ in fp32 arithmetic
    (m scale + log l, as the kernels store it).  A row without a visible key gives out = 0 (what the kernels store), lse = -inf."""
    r = bf16 if rounded else (lambda x: x)
    q, k, v, R = p["q"], p["k"], p["v"], p["R"]
    vis, dist = geo if geo is not None else geometry(q.shape[1], k.shape[1], p["mlen"], p["shift"], R.shape[0])
    qu, qv = _T(r(q + p["u"])), _T(r(q + p["vb"]))
    AC = qu @ k.transpose(0, 2, 3, 1)
    T = qv @ R.transpose(1, 2, 0)[None]
    BD = np.take_along_axis(T, np.broadcast_to(dist[None, None], AC.shape), axis=3)
    raw = np.where(vis[None, None], AC + BD, -np.inf)
    mraw = raw.max(-1, keepdims=True)
    mraw = np.where(np.isfinite(mraw), mraw, 0.0)
    E = np.exp((raw - mraw) * p["scale"])
    l = E.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(l > 0, E / l, 0.0)
        if rounded:
            Eb = bf16(E)
            out = r(_T(np.where(l > 0, (Eb @ _T(v)) / l, 0.0)))
            f = np.float32
            lse = (f(mraw[..., 0]) * f(p["scale"]) + np.log(Eb.sum(-1).astype(f))).astype(np.float64)
        else:
            out = _T(P @ _T(v))
            lse = mraw[..., 0] * p["scale"] + np.log(l[..., 0])
    return dict(out=out, lse=lse), (P, vis, dist, qu, qv)


def _to_dist(dS, vis, dist, mlen, nd):
    """dT[b,h,i,r] = sum of dS[b,h,i,j] over the visible j that read R row r"""
    Bn, Hn, q, klen = dS.shape
    i = np.arange(q)[:, None]
    if bool((dist == mlen + i - np.arange(klen)[None, :])[vis].all()):       # every visible pair reads the row of its own distance: a gather
        jj = mlen + i - np.arange(nd)[None, :]
        ok = (jj >= 0) & (jj < klen)
        return np.take_along_axis(dS, np.broadcast_to(np.clip(jj, 0, klen - 1)[None, None], (Bn, Hn, q, nd)), axis=3) * ok[None, None]
    dT = np.zeros((Bn, Hn, q, nd))
    np.add.at(dT, (slice(None), slice(None), np.broadcast_to(i, dist.shape), dist), dS)
    return dT


def backward(p, dout, fwd, cache, rounded=False, round_dq=False):
    """dq, dk, dv, dR, du, dv_bias, delta (and dT) of the closed form.  rounded: P and dS (= dT) rounded to bf16 before their products, delta
    from the bf16 output, dq_k / dk / dv stored as bf16, and dq, dR, du, dv_bias assembled from those stores as the GPU test assembles them.
    round_dq (with rounded): one more rounding point, dq = bf16(dq_k + dq_r), which is what the kernels that finish the query gradient store
    (relattn_dqr_fused, add2d_colsums); off by default, so every tolerance derived without it is unchanged."""
    r = bf16 if rounded else (lambda x: x)
    P, vis, dist, qu, qv = cache
    k, v, R = p["k"], p["v"], p["R"]
    do = _T(dout)
    delta = (_T(fwd["out"]) * do).sum(-1)                                     # [B,H,q]
    dP = do @ v.transpose(0, 2, 3, 1)
    dS = np.where(vis[None, None], P * (dP - delta[..., None]) * p["scale"], 0.0)
    Pr, dSr = r(P), r(dS)
    dv = r(_T(Pr.transpose(0, 1, 3, 2) @ do))
    dk = r(_T(dSr.transpose(0, 1, 3, 2) @ qu))
    dqk = r(_T(dSr @ _T(k)))
    dT = _to_dist(dSr, vis, dist, p["mlen"], R.shape[0])
    dqr = _T(dT @ R.transpose(1, 0, 2)[None])
    dR = (dT.transpose(0, 1, 3, 2) @ qv).sum(0).transpose(1, 0, 2)                # [nd,H,D]
    return dict(dq=r(dqk + dqr) if round_dq else dqk + dqr, dk=dk, dv=dv, dR=dR, du=dqk.sum((0, 1)), dv_bias=dqr.sum((0, 1)), delta=delta, dT=dT)


def reference(p, dout=None, geo=None, rounded=False, round_dq=False):
    fwd, cache = forward(p, geo, rounded)
    if dout is not None:
        fwd.update(backward(p, dout, fwd, cache, rounded, round_dq))
    return fwd


def materialised(AC, T, dP, mlen, shift, scale, rounded=False):
    """relattn_softmax_fwd + relattn_softmax_bwd (relattn_mat.hip, the fp32 parity path) in closed form: AC [H,B,Lq,Lk], T [H,B,Lq,nd], dP like AC.
    Returns P, lse [H,B,Lq], dS and dT [H,B,Lq,nd] with dT[.., mlen + i - j] = dS[.., j] on the visible pairs and 0 elsewhere; `written` is that
    set.  A row without a visible key is uniform, P = 1 / Lk and lse = -1e30 + log Lk, and passes no gradient.
    rounded: float32 at every value the kernels hold or store -- the scaled score, the difference to the row maximum, exp evaluated as the
    kernel's __expf evaluates it (exp2 of the float32 product with log2 e), the row sum, its reciprocal, P, lse, the row dot and dS."""
    f = (lambda x: np.asarray(x, np.float32)) if rounded else (lambda x: np.asarray(x, np.float64))
    Lq, Lk, nd = AC.shape[2], AC.shape[3], T.shape[3]
    i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    vis = (j > i - shift) & (j <= i + mlen)
    ridx = np.clip(mlen + i - j, 0, nd - 1)
    assert ((mlen + i - j)[vis] >= 0).all() and ((mlen + i - j)[vis] < nd).all()
    BD = np.take_along_axis(f(T), np.broadcast_to(ridx[None, None], AC.shape), axis=3)
    s = f(f(f(AC) + BD) * f(scale))
    s = np.where(vis, s, -np.inf)
    empty = ~vis.any(1)
    m = np.where(empty[None, None, :, None], 0.0, s.max(-1, keepdims=True)).astype(s.dtype)
    x = f(s - m)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp2(f(x * np.float32(1.4426950408889634))) if rounded else np.exp(x)
    e = np.where(vis, e, 0.0).astype(s.dtype)
    tot = e.sum(-1, keepdims=True, dtype=s.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = f(e * f(1.0 / tot))
        lse = f(m[..., 0] + f(np.log(tot[..., 0])))
    P = np.where(empty[None, None, :, None], f(1.0 / Lk), P).astype(s.dtype)
    lse = np.where(empty[None, None, :], f(-1e30) + f(np.log(f(Lk))), lse).astype(s.dtype)
    dot = np.where(vis, f(P * f(dP)), 0.0).sum(-1, keepdims=True, dtype=s.dtype)
    dS = np.where(vis, f(f(P * f(f(dP) - dot)) * f(scale)), 0.0).astype(s.dtype)
    dT = np.zeros(T.shape, s.dtype)
    written = np.zeros((Lq, nd), bool)
    ii, jj = np.nonzero(vis)
    dT[:, :, ii, mlen + ii - jj] = dS[:, :, ii, jj]
    written[ii, mlen + ii - jj] = True
    return dict(P=P.astype(np.float64), lse=lse.astype(np.float64), dS=dS.astype(np.float64), dT=dT.astype(np.float64)), written


def mutants(p, dout=None, names=MASK_MUTANTS):
    """{name: (reference under the mutant, changed (i, j) pairs [q, klen] bool)}; a mutant that changes no pair is left out (not applicable)"""
    q, klen, nd = p["q"].shape[1], p["k"].shape[1], p["R"].shape[0]
    geo = geometry(q, klen, p["mlen"], p["shift"], nd)
    res = {}
    for name in names:
        mut = mutate_geometry(name, q, klen, p["mlen"], p["shift"], nd)
        ch = changed_pairs(geo, mut)
        if ch.any():
            res[name] = (reference(p, dout, mut), ch)
    return res


def separation(ref, mut, changed, tol):
    """max|mutant - ref| / tol over the rows the mutant touches: `out` (and dq) over the affected query rows, dk / dv over the affected keys"""
    rows, cols = changed.any(1), changed.any(0)
    ratio = lambda d, t: float(d / t) if t > 0 else (float("inf") if d > 0 else 0.0)
    sep = {"out": ratio(np.abs(mut["out"] - ref["out"])[:, rows].max(), tol["out"])}
    if "dk" in ref:
        sep["dq"] = ratio(np.abs(mut["dq"] - ref["dq"])[:, rows].max(), tol["dq"])
        for n in ("dk", "dv"):
            sep[n] = ratio(np.abs(mut[n] - ref[n])[:, cols].max(), tol[n])
    return sep


# ------------------------------------------------------------------------------------------------------------------ the probe
PERIODS = ((67, 61), (65, 63), (69, 59), (71, 57), (66, 61), (64, 61), (63, 59), (67, 59))   # (keys, distances): coprime, sum <= D (a sum of
# exactly D makes distance D - 1 repeat the code of key + 1: the last four pairs are there for the windows whose oldest key sits at D - 1)


def _selections(q, mlen, shift, nd, pk, pr):
    """weights of q on K's and R's code dims [B,H,q,pk] / [B,H,q,pr], the code of every key / distance, and the target pairs [B,H,q,klen]"""
    klen = mlen + q
    i = np.arange(q)
    diag, edge = i + mlen, np.maximum(0, i - shift + 1)
    WK, WR = np.zeros((B, H, q, pk)), np.zeros((B, H, q, pr))
    target = np.zeros((B, H, q, klen), bool)
    kcode = np.array([[(np.arange(klen) + 7 * b + 13 * h) % pk for h in range(H)] for b in range(B)])
    rcode = np.array([(np.arange(nd) + 9 * h) % pr for h in range(H)])
    for b in range(B):
        for h in range(H):
            def select(rows, t, w, is_target):
                d = np.clip(diag[rows] - t, 0, nd - 1)
                np.maximum.at(WK[b, h], (rows, kcode[b, h, t]), w)
                np.maximum.at(WR[b, h], (rows, rcode[h, d]), w)
                if is_target:
                    target[b, h, rows, t] = True
            select(i, diag, W_T, True)
            select(i, edge, W_T, True)
            de = np.minimum(diag - edge, nd - 1)
            room = de >= 2
            dm = 1 + (7 + 11 * b + 5 * h + 3 * i) % np.maximum(de - 1, 1)           # strictly between the diagonal (0) and the oldest key (de)
            select(i[room], (diag - dm)[room], W_T, True)
            lo = i - shift >= 0
            select(i[lo], (i - shift)[lo], W_D, False)                           # one past the old edge
            hi = diag + 1 < klen
            np.maximum.at(WK[b, h], (i[hi], kcode[b, h, (diag + 1)[hi]]), W_D)   # one into the future (its clamped distance is the diagonal's R[0])
    return WK, WR, kcode, rcode, target


def _stray_pairs(q, mlen, shift, nd, pk, pr):
    """visible pairs that are no target and still collect a target's weight: a key that repeats one selected key's code (every pk keys)
    at a distance that repeats another selected distance's code (every pr)"""
    WK, WR, kcode, rcode, target = _selections(q, mlen, shift, nd, pk, pr)
    vis, dist = geometry(q, mlen + q, mlen, shift, nd)
    n = 0
    for b in range(B):
        for h in range(H):
            w = np.take_along_axis(WK[b, h], np.broadcast_to(kcode[b, h][None], vis.shape), 1) + np.take_along_axis(WR[b, h], rcode[h][dist], 1)
            n += int((vis & ~target[b, h] & (w >= 2 * W_T)).sum())
    return n


@functools.lru_cache(maxsize=None)
def _periods(q, mlen, shift, nd):
    best = None
    for c in PERIODS:
        n = _stray_pairs(q, mlen, shift, nd, *c)
        if n == 0:
            return c
        if best is None or n < best[0]:
            best = (n, c)
    return best[1]


def build(q, mlen, shift, nd=None, seed=0):
    """the probe inputs for one geometry (B = H = 2): the dict forward() takes, plus dout.  The code periods are the first pair of PERIODS
    with the fewest stray pairs for this geometry (the strays sit at fixed offsets that depend on shift, so a pair without any usually exists).
    dout is 8 x larger on the rows that a mutant can touch alone -- the last row (with shift = L the only one whose oldest key is not key 0)
    and the rows that see only the last or only the first key of a 32-key block: the tolerance of a gradient is sized by its largest entry,
    and the share of one row has to stand out of it."""
    klen = mlen + q
    nd = klen if nd is None else nd
    pk, pr = _periods(q, mlen, shift, nd)
    WK, WR, kcode, rcode, _ = _selections(q, mlen, shift, nd, pk, pr)
    rng = np.random.default_rng([seed, q, mlen, shift, nd])
    K, R, Q = np.zeros((B, klen, H, D)), np.zeros((nd, H, D)), np.zeros((B, q, H, D))
    K[..., :pk] = rng.integers(-1, 2, (B, klen, H, pk)) * 0.25
    R[..., pk:pk + pr] = rng.integers(-1, 2, (nd, H, pr)) * 0.25
    for b in range(B):
        for h in range(H):
            K[b, np.arange(klen), h, kcode[b, h]] = AMP
            Q[b, :, h, :pk], Q[b, :, h, pk:pk + pr] = WK[b, h], WR[b, h]
    for h in range(H):
        R[np.arange(nd), h, pk + rcode[h]] = AMP
    V = rng.choice([-1.0, -0.5, 0.5, 1.0], (B, klen, H, D))
    dout = rng.choice([-1.0, -0.5, 0.5, 1.0], (B, q, H, D))
    i = np.arange(q)
    edge = i - shift + 1
    dout[:, (i == q - 1) | ((edge >= 0) & (edge % 32 == 31)) | ((i + mlen) % 32 == 0)] *= 8.0
    u, vb = np.zeros((H, D)), np.zeros((H, D))
    u[:, :pk] = rng.integers(-2, 3, (H, pk)) * 0.25
    vb[:, pk:pk + pr] = rng.integers(-2, 3, (H, pr)) * 0.25
    p = dict(q=Q, k=K, v=V, R=R, u=u, vb=vb, mlen=mlen, shift=shift, scale=SCALE)
    for name in ("q", "k", "v", "R", "u", "vb"):
        assert np.array_equal(bf16(p[name]), p[name]), name
    assert np.array_equal(bf16(Q + u), Q + u) and np.array_equal(bf16(Q + vb), Q + vb) and np.array_equal(bf16(dout), dout)
    return p, dout


# ------------------------------------------------------------------------------------------------------------------ the K / V ring
# db1_relattn_decode_ring_fwd: logical key j < mlen is ring row (start + j) % cap; the q new rows are read from this call's projections
# and written to rows (start + mlen + i) % cap; every other byte of the ring stays.  The model ring has `guard` extra rows behind row
# cap - 1 (zeros) so that a mutant that runs past the end has somewhere to read and write.
# origin+-1 stands for two errors that a kernel can make independently of each other -- the memory rows READ one row off (ring_view: shows
# in the output, the ring image stays right) and the new rows APPENDED one row off (ring_expected: shows in the ring image) -- and the CPU
# test asserts each detection on its own.  wrap_gt and unwrapped_write are errors of the append.
RING_MUTANTS = ("origin+1", "origin-1", "wrap_gt", "unwrapped_write")


def ring_rows(start, n0, n, cap, mutant=None, append=False):
    """ring rows of logical keys n0 .. n0 + n - 1: the memory rows that are read (n0 = 0, n = mlen) or, with append, the new rows that are
    written (n0 = mlen, n = q)"""
    j = np.arange(n0, n0 + n)
    if mutant == "origin+1":
        start = (start + 1) % cap
    elif mutant == "origin-1":
        start = (start - 1) % cap
    r = start + j
    if mutant == "wrap_gt" and append:       # (the append's wrap test; what a READ past the last row finds is not defined, so no margin can be shown for it)
        return np.where(r > cap, r - cap, r)
    return np.where(r >= cap, r - cap, r)


def ring_initial(p, cap, start, seed=0):
    """[B, cap, 2, H, D]: the mlen memory rows of the probe at their ring rows, distinct bf16-exact filler everywhere else"""
    mlen = p["mlen"]
    rng = np.random.default_rng([seed, cap, start, 77])
    ring = rng.choice([-0.75, -0.25, 0.25, 0.75], (B, cap, 2, H, D))
    rows = ring_rows(start, 0, mlen, cap)
    ring[:, rows, 0] = p["k"][:, :mlen]
    ring[:, rows, 1] = p["v"][:, :mlen]
    return ring


def ring_expected(p, ring0, start, mutant=None, guard=0):
    """the ring after the call ([B, cap + guard, 2, H, D]): new rows written, every other byte unchanged"""
    mlen, q, cap = p["mlen"], p["q"].shape[1], ring0.shape[1]
    img = np.concatenate([ring0, np.zeros((B, guard) + ring0.shape[2:])], 1)
    rows = start + np.arange(mlen, mlen + q) if mutant == "unwrapped_write" else ring_rows(start, mlen, q, cap, mutant, append=True)
    img[:, rows, 0] = p["k"][:, mlen:]
    img[:, rows, 1] = p["v"][:, mlen:]
    return img


def ring_view(p, ring0, start, mutant=None, guard=0):
    """the probe as a kernel under `mutant` would see it: memory keys / values read back from the ring, plus the (j < mlen) keys whose source
    row changed"""
    mlen, cap = p["mlen"], ring0.shape[1]
    ext = np.concatenate([ring0, np.zeros((B, guard) + ring0.shape[2:])], 1)
    rows = ring_rows(start, 0, mlen, cap, None if mutant == "unwrapped_write" else mutant)
    seen = dict(p)
    seen["k"] = np.concatenate([ext[:, rows, 0], p["k"][:, mlen:]], 1)
    seen["v"] = np.concatenate([ext[:, rows, 1], p["v"][:, mlen:]], 1)
    return seen, rows != ring_rows(start, 0, mlen, cap)


def ring_origins(q, mlen, cap):
    """0, 1, the last row, the origin at which the NEW rows wrap, the origin at which the OLD rows wrap inside a 32-key step"""
    return sorted({0, 1 % cap, cap - 1, (cap - q + 1) % cap, (cap - mlen // 2) % cap})


# ------------------------------------------------------------------------------------------------------------------ the cases
def flash_shifts(L):
    return sorted({1, 16, 17, 31, 32, 33, 64, 65, 127, 128, 129, L - 1, L, L + 5})


FLASH_LENGTHS = (128, 256, 384)                                   # 384 wraps the 256-row R ring
FLASH_FWD_CASES = [(L, s) for L in FLASH_LENGTHS for s in flash_shifts(L)]
# backward: the old edge on a 32-key boundary for the tile's first row (32), one before (31), one after (33), the full window (L), one key (1)
FLASH_BWD_CASES = [(L, s) for L in FLASH_LENGTHS for s in (1, 31, 32, 33, L)]
FLASH_BWD_MODES = ("fwd_probs", "scratch_p_ds", "recompute")

# (q, mlen, shift, nd): every q against a chunk edge (mlen 127 / 128 / 129: 128-key chunks) and a step edge (mlen 31 / 32: 32-key steps);
# shift in {1, 32, mlen + 1, klen}; nd < klen twice, with shift small enough that only masked pairs reach the clamp
DECODE_CASES = [
    (1, 0, 1, None), (1, 1, 2, None), (1, 31, 32, None), (1, 32, 1, None), (1, 127, 128, None), (1, 128, 129, None), (1, 129, 32, None), (1, 300, 301, None),
    (15, 0, 15, None), (15, 32, 32, None), (15, 127, 128, None), (15, 129, 1, None), (15, 300, 32, None),
    (16, 0, 16, None), (16, 31, 32, None), (16, 32, 48, None), (16, 128, 129, None), (16, 127, 143, None),
    (17, 0, 17, None), (17, 1, 2, None), (17, 31, 32, None), (17, 127, 1, 130), (17, 128, 145, None), (17, 300, 1, None),
    (64, 0, 64, None), (64, 32, 33, None), (64, 127, 1, 128), (64, 128, 192, None), (64, 129, 32, None), (64, 300, 364, None), (64, 300, 301, None),
    (1, 2047, 2048, None), (17, 2031, 2048, None),   # klen = 2048: 16 units, every slot of the ring kernels' in-launch merge
]


def ring_caps(q, mlen):
    return (mlen + q, mlen + q + 7)
