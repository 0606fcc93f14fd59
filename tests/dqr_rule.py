"""The tail of the attention backward -- the dq_r stream kernel (relattn_dqr.hip) in its four entry points -- as a float64 closed form, a
restatement of the stream's geometry, two integer probe builders whose results are bit-exact whatever the summation order, and mutants of the
closed form (never of a kernel) that tests/test_dqr_rule_cpu.py uses to prove that a misplaced term shows in the stored bits.  numpy only:
neither torch nor the library is imported here.

The operation (g(b) = b // (B / ng), the block of sequences that shares one R):
    dq_r[b, i, h, :] = sum_{dist <= i} dT[h, b, i, dist] R[g(b)][dist, h, :]         dq = bf16_rne(dq_k + dq_r)
    du = acc0[0] + sum_{b, i} dq_k        dv = acc0[1] + sum_{b, i} dq_r               sums = the [2, rows, H 128] partial table added over rows

The stream (relattn_dqr_kernel): wph = max(1, 256 // H) workgroups per head; the items of a group of sequences are its (sequence, 64-row tile)
pairs, item t = sequence t // NT, row tile (t + b) % NT (b: the sequence's index in the whole batch); workgroup j of a head works for group
j % ng and takes the items jj, jj + wph / ng, ... with jj = j // ng, and is idle where jj >= n_items.  Of an item with first row i0 the
kernel reads the 128-distance k-tiles kt <= (i0 + 63) // 128 and nothing else: `poison` fills every other k-tile of dT with NaN.

The probes.
  index   at most four non-zeros per row (h, b, i): dist 0, the diagonal dist = i (the last entry the contract allows), one entry in the row's
          last k-tile and one whose position differs per (h, b, i); values by (h + b + i) % 4: +-3 / +-4 at dist 0, +-1 / +-2 elsewhere.  R in [-15, 15] and dq_k
          in [-63, 63] are integers that depend on (group, dist, h, d) / (b, i, h, d), so |dq_r| <= 150 and |dq_k + dq_r| <= 213 < 256: every
          result is an integer that bf16 holds exactly (index_is_exact asserts it), and a misplaced term changes the stored bits.
  dense   dT in {-2 .. 2} on dist <= i, R in {-3 .. 3}, dq_k an integer in [-64, 64]: all products and sums are integers far below 2^24 (the
          builder asserts its bounds), so the fp32 accumulators are exact and dq is the round-to-nearest-even bf16 of an exact integer.

Mutants and their applicability.  Distance and row shifts wrap modulo L (a kernel that is one off reads SOMETHING), so
  dist+-s    R row (dist + s) % L instead of dist                 applicable where s % L != 0   (dist+-128 changes nothing at L = 128)
  row+-s, row^16   output row i gets the dq_r of row (i + s) % L / i ^ 16                        always
  heads / batches  dT of head h + 1 / of sequence b + 1 (cyclic)                                 H > 1 / B > 1
  groups           R of group g + 1 (cyclic)                                                     ng > 1
  no_diag / no_last_tile / no_first_tile   the terms dist = i / of k-tile i // 128 / of k-tile 0 dropped     always (one and the same at L = 128)
  dqk_row+4        dq_k taken from row (i + 4) % L                                               always (fused path: dq only)
  du_dv            the two column sums exchanged                                                 always (sums only)
  item_missing     the last 64-row item of the last sequence missing from both column sums       always (sums only)
On the index probe every row has its four entries, so an applicable mutant of the first four groups touches EVERY output row (b, i, h), and
the CPU test demands a bit difference in each of them; the sums-only mutants must change du and dv of every head.
"""
import numpy as np

D = 128
ROWS, KT = 64, 128            # rows of an item, distances of a k-tile
ACC0 = (3.0, -5.0)            # initial du / dv accumulators of the fused entry points
LIM = float(2 ** 24)


# ------------------------------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """round to nearest even bf16, returned as float64 (finite inputs)"""
    u = np.array(x, np.float32, order="C", ndmin=1).view(np.uint32)      # (a copy; 32-bit arithmetic: no finite input comes near the wrap)
    u += ((u >> 16) & 1) + np.uint32(0x7FFF)
    u &= np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """the 16 stored bits of bf16_rne(x) as int16 (-0 normalised to +0: an exact zero sum is +0 on every path)"""
    a = np.ascontiguousarray(np.asarray(x, np.float64) + 0.0, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16).view(np.int16)


# ------------------------------------------------------------------------------------------------------------------ the stream's geometry
def wph(H):
    return max(1, 256 // H)


def n_items(B, L, ng=1):
    return (B // ng) * (L // ROWS)


def item(t, grp, B, L, ng=1):
    """(sequence b, first row i0) of item t of group grp"""
    NT, bper = L // ROWS, B // ng
    b = grp * bper + t // NT
    return b, ((t + b) % NT) * ROWS


def workgroup(j, H, B, L, ng=1):
    """(group, items [(b, i0), ...]) of workgroup j of a head; an empty list: idle"""
    grp, jj, wpg = j % ng, j // ng, wph(H) // ng
    return grp, [item(t, grp, B, L, ng) for t in range(jj, n_items(B, L, ng), wpg)]


def idle(j, H, B, L, ng=1):
    return j // ng >= n_items(B, L, ng)


def read_ktiles(i0):
    """the k-tiles of dT an item with first row i0 reads"""
    return range((i0 + ROWS - 1) // KT + 1)


def poison_mask(L):
    """[L, L] bool: entries (i, dist) in k-tiles the row's item does not read"""
    i = np.arange(L)[:, None]
    return (np.arange(L)[None, :] // KT) > ((i // ROWS * ROWS + ROWS - 1) // KT)


# ------------------------------------------------------------------------------------------------------------------ the probes
def _finish(dT, R, dq_k, ng, poison):
    L = dT.shape[-1]
    if poison:
        dT[:, :, poison_mask(L)] = np.nan
    return dict(dT=dT, R=R, dq_k=dq_k, ng=ng, acc0=ACC0)


def _grid(H, B, L):
    return np.arange(H)[:, None, None], np.arange(B)[None, :, None], np.arange(L)[None, None, :]


def _R_index(ng, L, H):
    """an integer hash of (group, dist, h, d) into [-15, 15]: no linear structure that a shifted index could reproduce"""
    g, dist, h, d = np.ogrid[:ng, :L, :H, :D]
    u = ((dist + 1) * 2654435761 + d * 40503 + h * 9973 + g * 7919).astype(np.uint64) & 0xFFFFFFFF
    u ^= u >> 13
    u = (u * 0x5BD1E995) & 0xFFFFFFFF
    u ^= u >> 15
    return (u % 31).astype(np.float64) - 15.0


def _dqk_index(B, L, H):
    b, i, h, d = np.ogrid[:B, :L, :H, :D]
    return ((5 * i + 3 * (i >> 4) + 17 * b + 23 * h + 7 * d) % 127 - 63).astype(np.float64)


def index_positions(H, B, L):
    """[H, B, L, 4]: the distances of a row's four entries"""
    h, b, i = _grid(H, B, L)
    last = KT * (i // KT) + (13 * i + 7 * b + 29 * h + 5) % (i % KT + 1)
    rnd = (31 * i * i + 17 * i + 101 * b + 59 * h + 7) % (i + 1)
    last, rnd = np.maximum(last, np.minimum(i, 1)), np.maximum(rnd, np.minimum(i, 1))      # dist 0 keeps its own entry (row 0 has no other place)
    return np.stack(np.broadcast_arrays(0 * i + 0 * b + 0 * h, i + 0 * b + 0 * h, last, rnd), axis=-1)


def build_index(H, B, L, ng=1, poison=False):
    assert L % KT == 0 and B % ng == 0
    h, b, i = _grid(H, B, L)
    pos = index_positions(H, B, L)
    vals, vals0 = np.array([1.0, -2.0, 2.0, -1.0]), np.array([3.0, -4.0, 4.0, -3.0])
    dT = np.zeros((H, B, L, L))
    for k in range(4):                               # (entries that share a distance: the later one stays.  The values go by the row, not by k, so
        # the rows of neighbouring heads / sequences differ at dist 0 whatever coincides; dist 0 has values of its own, so exchanging it with
        # another entry -- dist + 128 at L = 256 maps {0, 128} onto itself -- shows)
        np.put_along_axis(dT, pos[..., k:k + 1], (vals if k else vals0)[(h + b + i) % 4][..., None], axis=3)
    assert (pos <= i[..., None]).all()
    return _finish(dT, _R_index(ng, L, H), _dqk_index(B, L, H), ng, poison)


def index_is_exact(res):
    """dq_r and dq_k + dq_r of the index probe are integers that bf16 holds exactly"""
    whole = lambda x: bool((x == np.rint(x)).all() and np.abs(x).max() <= 256)      # bf16 holds every integer up to 256
    return whole(res["dq_r"]) and whole(res["dq_exact"]) and bool(np.array_equal(res["dq"], res["dq_exact"]))


def build_dense(H, B, L, ng=1, poison=False, seed=0):
    assert L % KT == 0 and B % ng == 0
    rng = np.random.default_rng([seed, H, B, L, ng])
    dT = rng.integers(-2, 3, (H, B, L, L)).astype(np.float64)
    i = np.arange(L)
    dT *= (i[None, :] <= i[:, None])
    dT += 0.0                                        # entries above the diagonal are +0
    R = rng.integers(-3, 4, (ng, L, H, D)).astype(np.float64)
    dq_k = rng.integers(-64, 65, (B, L, H, D)).astype(np.float64)
    # every accumulator stays an exact integer: per element sum |dT| |R| <= rowsum |dT| max |R|, per column the same added over the rows
    row = np.abs(dT).sum(-1) * np.abs(R).max()       # [H, B, L]
    assert row.max() < LIM, "sum |dT| |R| per element"
    assert row.sum((1, 2)).max() + max(abs(a) for a in ACC0) < LIM, "dq_r column sums"
    assert np.abs(dq_k).sum((0, 1)).max() + max(abs(a) for a in ACC0) < LIM, "dq_k column sums"
    assert (np.abs(dq_k) + row.transpose(1, 2, 0)[..., None]).max() < LIM
    return _finish(dT, R, dq_k, ng, poison)


# ------------------------------------------------------------------------------------------------------------------ the closed form
MUTANTS = ("dist+1", "dist-1", "dist+8", "dist-8", "dist+32", "dist-32", "dist+128", "dist-128",
           "row+1", "row-1", "row+4", "row-4", "row+8", "row-8", "row^16",
           "heads", "batches", "groups",
           "no_diag", "no_last_tile", "no_first_tile",
           "dqk_row+4", "du_dv", "item_missing")
SUMS_ONLY = ("du_dv", "item_missing")


def applicable(name, H, B, L, ng=1):
    if name.startswith("dist"):
        return int(name[4:]) % L != 0
    return {"heads": H > 1, "batches": B > 1, "groups": ng > 1}.get(name, True)


def _dq_r(dT, R, ng, drop=None):
    """sum_{dist <= i} dT R per 128-row block over the k-tiles up to the block's own (the entries past the diagonal inside them are zero; the
    tiles beyond are never touched, poisoned or not)"""
    H, B, L, _ = dT.shape
    bper = B // ng
    out = np.zeros((B, L, H, D))
    for r0 in range(0, L, KT):
        c0, c1 = (KT if drop == "no_first_tile" else 0), (r0 if drop == "no_last_tile" else r0 + KT)
        if c1 <= c0:
            continue
        for g in range(ng):
            blk = np.ascontiguousarray(dT[:, g * bper:(g + 1) * bper, r0:r0 + KT, c0:c1])
            if drop == "no_diag" and c1 == r0 + KT:
                blk, k = blk.copy(), np.arange(KT)        # (ascontiguousarray may have returned a view of the probe)
                blk[:, :, k, r0 - c0 + k] = 0.0
            res = np.matmul(blk.reshape(H, bper * KT, c1 - c0), R[g, c0:c1].transpose(1, 0, 2))
            out[g * bper:(g + 1) * bper, r0:r0 + KT] = res.reshape(H, bper, KT, D).transpose(1, 2, 0, 3)
    return out + 0.0


CONTRACTION_MUTANTS = tuple(m for m in MUTANTS if m.startswith("dist") or m in ("heads", "batches", "groups", "no_diag", "no_last_tile", "no_first_tile"))


def closed_form(pr, mutant=None, base=None):
    """dict dq_r, dq_exact (= dq_k + dq_r), dq (its bf16), du, dv [H 128] and sums [2, H 128] (du, dv without the initial accumulators).
    base: the unmutated result of the same probe, whose contraction a mutant that leaves the contraction alone may reuse"""
    dT, R, dq_k, ng = pr["dT"], pr["R"], pr["dq_k"], pr["ng"]
    H, B, L, _ = dT.shape
    m = mutant
    assert m is None or m in MUTANTS, m
    drop = m if m in ("no_diag", "no_last_tile", "no_first_tile") else None
    if m is not None and m.startswith("dist"):
        R = np.roll(R, -int(m[4:]), axis=1)          # R'[dist] = R[(dist + s) % L]
    elif m == "groups":
        R = np.roll(R, -1, axis=0)
    elif m == "heads":
        dT = np.roll(dT, -1, axis=0)
    elif m == "batches":
        dT = np.roll(dT, -1, axis=1)
    dq_r = base["dq_r"] if (base is not None and m not in CONTRACTION_MUTANTS) else _dq_r(dT, R, ng, drop)
    if m == "row^16":
        dq_r = dq_r[:, np.arange(L) ^ 16]
    elif m is not None and m.startswith("row"):
        dq_r = np.roll(dq_r, -int(m[3:]), axis=1)
    dq_exact = (np.roll(dq_k, -4, axis=1) if m == "dqk_row+4" else dq_k) + dq_r
    sums = np.stack([dq_k.sum((0, 1)).reshape(-1), dq_r.sum((0, 1)).reshape(-1)])
    if m == "item_missing":
        sums -= np.stack([dq_k[B - 1, L - ROWS:].sum(0).reshape(-1), dq_r[B - 1, L - ROWS:].sum(0).reshape(-1)])
    if m == "du_dv":
        sums = sums[::-1].copy()
    return dict(dq_r=dq_r, dq_exact=dq_exact, dq=bf16(dq_exact), sums=sums, du=pr["acc0"][0] + sums[0], dv=pr["acc0"][1] + sums[1])


# ------------------------------------------------------------------------------------------------------------------ the cases
# (H, B, L, ng), each for a branch of the stream kernel:
CASES = [
    (1, 1, 128, 1),      # one-tile streams: `issued` never reaches 3; 254 of 256 workgroups idle
    (2, 2, 256, 1),      # items of 1 and 2 k-tiles, with the rotation
    (3, 2, 384, 1),      # wph = 85: a head stride that B = H = 2 would hide
    (1, 1, 1024, 1),     # all eight k-tile cases of the switch, every R^T register live
    (64, 1, 384, 1),     # wph = 4 < 6 items: a workgroup streams across items of unequal tile counts, the ring wraps
    (256, 1, 128, 1),    # wph = 1
    (2, 4, 256, 2),      # groups
    (16, 16, 128, 16),   # groups: one workgroup per group
    (64, 4, 256, 2),     # groups: more items than workgroups per group
]
