"""The grouped K/V ring of include/db1_hip.h ("grouped K/V ring") restated in NumPy, and the probe data its tests share.  numpy and
attn_probe only: neither torch nor the library is imported here.

The rule.  M = G W rows, row r in group g = r // W.  Per layer a base ring [G, cap_b, 2, H, D] with origin sb, a tail ring
[M, cap_t, 2, H, D] with origin st and window Lt, and n_tail valid tail keys.  Logical key j of row r:
    j <  mlen - n_tail            base slot (sb + n_tail + j) % cap_b of base row g
    mlen - n_tail <= j < mlen     tail slot (st + Lt - mlen + j) % cap_t of tail row r
    j == mlen                     the call's own key; appended at tail slot (st + Lt) % cap_t of row r
A count outside [0, min(Lt, mlen)] or an origin outside its ring is clamped and sets status bit 0.

The probe follows attn_probe's: K and R carry one-hot codes (value 16), q selects (key, distance) PAIRS with weight 6 -- the call's own
key, the oldest and the newest memory key, the two keys at the seam between base and tail, one key in the middle, at most three of
them per head -- so that a key read from a wrong
slot, row, group or distance loses or gains most of a row's mass; with shift = 0 the hidden key 0 is a decoy of weight 8.  V is different
for every (row or group, position, head).  The closed form is attn_probe.forward over the linearised window of every row."""
import numpy as np

import attn_probe as AP

D = 128
MUTANTS = ("seam+1", "seam-1", "group_mod", "tail_origin+1", "tail_origin-1", "base_nowrap", "tail_nowrap")
DIST_MUTANTS = ("dist+1", "dist-1")


def clamp(n_tail, sb, st, mlen, Lt, cap_b, cap_t):
    """(n_tail, sb, st) as the kernel uses them, and the status word"""
    lim = min(Lt, mlen)
    c = (min(max(n_tail, 0), lim), min(max(sb, 0), cap_b - 1), min(max(st, 0), cap_t - 1))
    return c + (int(c != (n_tail, sb, st)),)


def sources(G, W, mlen, Lt, n_tail, sb, st, cap_b, cap_t, mutant=None):
    """for every row and logical key j < mlen: (from the tail? [M, mlen], the ring row, the slot) -- under ``mutant``, one index error"""
    M = G * W
    r, j = np.arange(M)[:, None], np.arange(mlen)[None, :]
    seam = mlen - n_tail + {"seam+1": 1, "seam-1": -1}.get(mutant, 0)
    g = (r % W) % G if mutant == "group_mod" else r // W
    st_ = st + {"tail_origin+1": 1, "tail_origin-1": -1}.get(mutant, 0)
    bslot, tslot = sb + n_tail + j, st_ + Lt - mlen + j
    bslot = bslot if mutant == "base_nowrap" else bslot % cap_b
    tslot = tslot if mutant == "tail_nowrap" else tslot % cap_t
    is_tail = np.broadcast_to(j >= seam, (M, mlen))
    return is_tail, np.where(is_tail, r, g), np.where(is_tail, tslot, bslot)


def append_slot(st, Lt, cap_t):
    return (st + Lt) % cap_t


def read(base, tail, src, guard):
    """the [M, mlen, 2, H, D] windows the map ``src`` reads; a slot past its row's end runs on into the next row, and behind the last
    row into ``guard`` ([n, 2, H, D]), as a flat address would"""
    is_tail, row, slot = src
    fb = np.concatenate([base.reshape((-1,) + base.shape[2:]), guard])
    ft = np.concatenate([tail.reshape((-1,) + tail.shape[2:]), guard])
    it, ib = np.where(is_tail, row * tail.shape[1] + slot, 0), np.where(is_tail, 0, row * base.shape[1] + slot)
    return np.where(is_tail[..., None, None, None], ft[it], fb[ib])


def probe(G, W, H, mlen, shift, n_tail, seed=0):
    """the dict attn_probe.forward takes, over the M = G W linearised windows (q [M, 1, H, D], k / v [M, mlen + 1, H, D]); rows of a
    group share their first mlen - n_tail keys / values.  The code periods are the first pair of attn_probe.PERIODS without a stray pair --
    a visible key that is no target and still collects a target's weight on both channels -- or the pair with the fewest."""
    best = None
    for pk, pr in AP.PERIODS:
        codes = _codes(G, W, H, mlen, shift, n_tail, pk, pr)
        if best is None or codes[-1] < best[-1]:
            best = (pk, pr) + codes
        if codes[-1] == 0:
            break
    PK, PR, kcode, rcode, Q, _ = best
    M, klen, seam = G * W, mlen + 1, mlen - n_tail
    rng = np.random.default_rng([seed, G, W, H, mlen, shift, n_tail])
    K, V = np.zeros((M, klen, H, D)), np.zeros((M, klen, H, D))
    Kb = rng.integers(-1, 2, (G, mlen, H, PK)) * 0.25
    Vb = rng.choice([-1.0, -0.5, 0.5, 1.0], (G, mlen, H, D))
    for r in range(M):
        g = r // W
        K[r, :, :, :PK] = rng.integers(-1, 2, (klen, H, PK)) * 0.25
        V[r] = rng.choice([-1.0, -0.5, 0.5, 1.0], (klen, H, D))
        K[r, :seam, :, :PK], V[r, :seam] = Kb[g, n_tail:], Vb[g, n_tail:]
        K[r][np.arange(klen)[:, None], np.arange(H)[None, :], kcode[r]] = AP.AMP
    R = np.zeros((klen, H, D))
    R[..., PK:PK + PR] = rng.integers(-1, 2, (klen, H, PR)) * 0.25
    R[np.arange(klen)[:, None], np.arange(H)[None, :], PK + rcode] = AP.AMP
    u, vb = np.zeros((H, D)), np.zeros((H, D))
    u[:, :PK] = rng.integers(-1, 2, (H, PK)) * 0.25
    vb[:, PK:PK + PR] = rng.integers(-1, 2, (H, PR)) * 0.25
    p = dict(q=Q, k=K, v=V, R=R, u=u, vb=vb, mlen=mlen, shift=shift, scale=AP.SCALE)
    for name in ("q", "k", "v", "R", "u", "vb"):
        assert np.array_equal(AP.bf16(p[name]), p[name]), name
    assert np.array_equal(AP.bf16(Q + u), Q + u) and np.array_equal(AP.bf16(Q + vb), Q + vb)
    return p


def _codes(G, W, H, mlen, shift, n_tail, PK, PR):
    """(the code of every key [M, klen, H] and of every distance [nd, H], the queries that select the targets, the number of stray pairs)
    for one pair of code periods"""
    M, klen, seam = G * W, mlen + 1, mlen - n_tail
    hh, jj = np.arange(H)[None, :], np.arange(klen)[:, None]
    kcode = np.zeros((M, klen, H), np.int64)
    for r in range(M):
        kcode[r] = np.where(jj < seam, jj + n_tail + 7 * (M + r // W) + 13 * hh, jj + 7 * r + 13 * hh + 31) % PK
    rcode = (np.arange(klen)[:, None] + 9 * hh) % PR
    Q = np.zeros((M, 1, H, D))
    oldest = 0 if shift >= 1 else 1
    strays = 0
    for r in range(M):
        for h in range(H):
            mid = oldest + 1 + (7 + 11 * r + 5 * h) % max(mlen - oldest - 1, 1)
            # three targets per head at most, so that each holds a large share of its row: head 0 (mod 3) the call's own key and the two
            # keys at the seam, head 1 the own key, the newest memory key (the one a wrap moves) and the oldest visible one, head 2 the
            # seam and a key in the middle
            at_seam = ([seam - 1] if seam >= 1 + oldest else []) + ([seam] if n_tail >= 1 else [])
            picks = ([mlen] + at_seam, [mlen, mlen - 1, oldest], at_seam + [min(mid, mlen)])[h % 3]
            picks = [(j, AP.W_T) for j in picks] + ([(0, AP.W_D)] if shift == 0 else [])
            for j, w in picks:
                Q[r, 0, h, kcode[r, j, h]] = max(Q[r, 0, h, kcode[r, j, h]], w)
                c = PK + rcode[mlen - j, h]
                Q[r, 0, h, c] = max(Q[r, 0, h, c], w)
            weight = Q[r, 0, h, kcode[r, :, h]] + Q[r, 0, h, PK + rcode[mlen - np.arange(klen), h]]
            target = np.isin(np.arange(klen), [j for j, w in picks if w == AP.W_T])
            strays += int(((weight >= 2 * AP.W_T) & ~target & (np.arange(klen) >= oldest)).sum())
    return kcode, rcode, Q, strays


def rings(p, G, W, Lt, n_tail, sb, st, cap_b, cap_t, filler="nan", seed=0):
    """(base [G, cap_b, 2, H, D], tail [M, cap_t, 2, H, D]) holding the probe's windows by the rule; every other slot holds NaN
    (``filler`` "nan") or distinct bf16-exact values ("values": what a mutant of the rule reads there)"""
    M, mlen, H = G * W, p["mlen"], p["k"].shape[2]
    if filler == "nan":
        base, tail = np.full((G, cap_b, 2, H, D), np.nan), np.full((M, cap_t, 2, H, D), np.nan)
    else:
        rng = np.random.default_rng([seed, cap_b, cap_t, sb, st, 77])
        base, tail = rng.choice([-0.75, -0.25, 0.25, 0.75], (G, cap_b, 2, H, D)), rng.choice([-0.75, -0.25, 0.25, 0.75], (M, cap_t, 2, H, D))
    is_tail, row, slot = sources(G, W, mlen, Lt, n_tail, sb, st, cap_b, cap_t)
    for dst, sel in ((tail, is_tail), (base, ~is_tail)):     # (the rows of a group write the same values to their base row)
        rr, jj = np.nonzero(sel)
        dst[row[rr, jj], slot[rr, jj], 0], dst[row[rr, jj], slot[rr, jj], 1] = p["k"][rr, jj], p["v"][rr, jj]
    return base, tail


def expected_tail(p, tail, W, Lt, st, cap_t):
    """the tail ring after the call: the call's own key / value at the append slot of every row, every other byte unchanged"""
    img, mlen = tail.copy(), p["mlen"]
    img[:, append_slot(st, Lt, cap_t), 0], img[:, append_slot(st, Lt, cap_t), 1] = p["k"][:, mlen], p["v"][:, mlen]
    return img


def seen(p, base, tail, src, guard):
    """the probe as a kernel that reads by the map ``src`` sees it"""
    win = read(base, tail, src, guard)
    q = dict(p)
    q["k"] = np.concatenate([win[:, :, 0], p["k"][:, p["mlen"]:]], 1)
    q["v"] = np.concatenate([win[:, :, 1], p["v"][:, p["mlen"]:]], 1)
    return q


def reference(p, geo=None):
    """(out [M, 1, H, D] float64, the per-element tolerance attn_probe sizes from the bf16-rounded model)"""
    ref = AP.forward(p, geo)[0]["out"]
    return ref, AP.tolerance(ref, AP.forward(p, geo, rounded=True)[0]["out"])


# ------------------------------------------------------------------------------------------------------------------ the cases
# mlen crosses every 32-key step and the 128-key chunk; n_tail puts the seam on, before and after a step boundary; Lt one and two
# tail chunks; W one row, part of a tile, a full tile and two tiles.  cap_b != cap_t.  The other axes (G, the origins, shift) cycle
# through their values inside a (mlen, Lt, W) case so that every value meets every mlen, Lt and W.
H = 3
MLENS, LTS, WS = (31, 33, 96, 129, 160), (40, 130), (1, 3, 4, 16, 17)


def caps(mlen, Lt):
    return mlen + 7, Lt + 4


def n_tails(mlen, Lt):
    lim = min(Lt, mlen)
    return sorted({n for n in (0, 1, 31, 32, 33, lim) if n <= lim})


def base_origins(mlen, Lt):
    cap_b, _ = caps(mlen, Lt)
    return (0, cap_b - mlen // 2, 37 % cap_b)          # none, the window wraps, not a multiple of 32


def tail_origins(mlen, Lt):
    _, cap_t = caps(mlen, Lt)
    return (0, cap_t - 1, cap_t - Lt // 2 - 1)         # the append lands on the last-but-.. slot, everything wraps, the tail wraps inside


def cases(mlen, Lt, W):
    """[(G, n_tail, sb, st, shift)] of one (mlen, Lt, W)"""
    k = MLENS.index(mlen) + 2 * LTS.index(Lt) + 3 * WS.index(W)
    out = []
    for i, n in enumerate(n_tails(mlen, Lt)):
        c = k + i
        out.append((1 + c % 2, n, base_origins(mlen, Lt)[c % 3], tail_origins(mlen, Lt)[(c // 2) % 3], (c // 3) % 2))
    return out


def applicable(mutant, G, W, mlen, Lt, n_tail, sb, st, shift):
    """does the index error change a VISIBLE key of some row?"""
    cap_b, cap_t = caps(mlen, Lt)
    seam, first = mlen - n_tail, 0 if shift >= 1 else 1
    if mutant == "seam+1":
        return n_tail >= 1 and seam >= first
    if mutant.startswith("tail_origin"):
        return n_tail >= 1
    if mutant == "seam-1":
        return seam - 1 >= first
    if mutant == "group_mod":
        return G >= 2 and W >= 2 and seam - 1 >= first
    if mutant == "base_nowrap":
        return seam - 1 >= first and sb + n_tail + seam - 1 >= cap_b
    if mutant == "tail_nowrap":
        return n_tail >= 1 and st + Lt - 1 >= cap_t
    return True
