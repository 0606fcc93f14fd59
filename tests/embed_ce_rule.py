"""The rule the two ends of the training step are tested by: token embedding (csrc/elementwise.hip db1_embed_gather_fwd, db1_rl_assemble_fwd /
_bwd; csrc/scatter.hip db1_embed_scatter_add_bwd), the masked cross-entropy (db1_masked_ce_fwd / _bwd / _fwd_bwd) and the chunked head + loss
sweep (csrc/lmhead_ce.hip).  Case tables with one case per dispatch branch and edge, probe inputs, float64 references written from the
definitions, the expected BITS of the exact kernels, per-element bounds of the others, fp32 transcriptions and one-mistake mutants of the
reference.  test_embed_ce_rule_cpu.py proves the rule usable without a GPU; test_embed_ce_kernels_gpu.py applies it.  Pure NumPy: neither
torch nor the library is imported.  check / ratio / bound / half_ulp / bf16 / SENT / U are stream_rule's.

NO CONSTANT BELOW CAME FROM RUNNING A KERNEL UNDER TEST.  The only free constants are the two of the earlier rule files: the fp32 model may
use HALF of an allowance, a mutant of a bounded kernel must move an element by TEN bounds (attn_probe's margin).

EXACT KERNELS.  Table, dout and vis entries are hq(row, column): multiples of 1/4 with |v| <= 2 drawn from a hash of (row, column), so that
two rows differ in most columns and adjacent columns differ; initial accumulators are multiples of 1/4 below 8.  Every partial sum of such
values, in ANY order, is exact in fp32 while the sum of |terms| in units of 1/4 stays below 2^24 (scatter_units() / assemble_units(), asserted
per case by the CPU test): the kernel must deliver the correctly rounded exact result, bit for bit.  The f32 tables of the f32 -> bf16 cases carry ten fraction
bits (hq + t / 1024, t in -4 .. 3: exact ties among them); word + position rows are then multiples of 2^-10 below 8, exact in fp32.
Rounding points, one line per kernel:
  gather_kernel             a copy; f32 -> bf16: ONE rounding (stf / f2bf); ids outside the table give +0
  scatter_* (sort + runs)   fp32 sums of grid values onto the fp32 accumulator: no rounding at all (the summation order is NOT pinned)
  rl_assemble_kernel fwd    word-or-vis row + position row in fp32 (exact), ONE rounding to the output type
  rl_assemble_kernel bwd    dvis: a copy (unused rows: the zeros of the memset); dword / dpos: the scatter above
expected value = bf16_rne(exact) for bf16 outputs, float32(exact) for fp32 outputs; no tolerance anywhere.
Besides the tables of 200 .. 65 536 rows the scatter has one of 65 736: only there do ids above 65 535 exist, which a 16-bit key would merge.
The one bounded scatter case (Gaussian dout): bound = half_ulp_f32(ref) + (len + ceil(len / 256) + 1) 2^-24 (sum |terms| + |acc0|), len the
run's length: len adds of the run in whatever grouping, one per partial row, the accumulator.

BOUNDED KERNELS (cross-entropy, sweep).  Reference: float64 on the inputs as stored.  Units of 2^-24 (U).  Charges:
  __expf(a)   = v_exp_f32(a * log2 e): relative 3 + 3 |a| -- what vision_rule charges the same call in gelu' ("3 + 1.5 h^2" at a = -h^2 / 2):
                v_exp_f32 1 ulp = 2, its product 1, and the rounding of a * log2 e, an absolute error |a| 2^-24 log2 e of the exponent =
                |a| relative, charged 3 |a| as there (the constant's own rounding and the argument's included).  The argument x - m is itself
                one fp32 subtraction: + |a|.  Together 3 + 4 |a| relative per __expf, and + 1 where its result is multiplied into the sum.
  logf        3 ulp = 6, the OpenCL full-profile limit OCML documents for log (erff's 2 ulp are charged 4 the same way in stream_rule)
  a / b       2, as vision_rule charges 1 / x
  lse         thread: nv = ceil(V / (256 VN)) vectors (scalar path: ceil(V / 256) elements), VN nv serial adds (scalar: as many adds as
              elements) and at most one rescale per vector (element); then the rescale by __expf(m - M), six butterfly steps, three adds,
              logf, + M.  A term exp(x_j - M) reaches the sum through its own __expf and at most nresc + 1 rescales whose arguments
              telescope to M - x_j (the running maximum only grows), so relative to S
                  c_S = nadds + 9 + 4 (nresc + 2) + 4 sum_j p_j (M - x_j),        p_j = exp(x_j - lse)
              and  |lse - ref| <= half_ulp_f32(ref) + 2^-24 (c_S + 6 |lse - M|)      (A = 1: d log S = dS / S; the last add is the half ulp)
  tok loss    mk (lse - x_y): mk E_lse + 2 |tok| (subtraction, product)
  sums[0]     sum_t E_tok + (ceil(T / 1024) + 11) (sum |tok| + |sums0|): ce_sum_kernel's serial adds, ten tree steps, the accumulator
              (sweep: + chunks + 1 for lmhead_add_loss_kernel per chunk and lmhead_finish_kernel).  sums[1]: masks are dyadic: EXACT.
  dlogits     w (exp(x - lse) - [c = y]), w = mk / norm[1] * gscale: ABSOLUTE
                  |w| (p (3 + 4 |x - lse|) + |p - 1hot|) + 4 |w| |p - 1hot|  in U  (exp; subtraction; division 2, two products)
                  + |w| p E_lse                                               (lse's own error moves exp(x - lse) by p E_lse)
              bf16: the k = 2 and bf16 half-ulp terms of stream_rule.bound.  Pad columns V .. ld: exactly +0.
  sweep       logits of the probes are multiples of 1/8 below 16: exact in fp32 and bf16, so lse / loss follow the rule above unchanged.
              dh = dlogits W, dW = beta dW0 + dlogits^T h against float64 products of the reference dlogits:
                  sum E_dl |W| (sum E_dl |h|) + (K + chunks + 1) 2^-24 sum |terms| + the half ulp of the output type (k = 2 for bf16),
              K the contraction length (rows of W for dh, T for dW); E_dl is the bound of dlogits AS STORED (bf16: with its rounding).
The builds use -ffp-contract=fast: a multiply-add may be one rounding or two; every count above charges two."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rule as S  # noqa: E402
from stream_rule import SENT, U, bf16, bound, check, half_ulp, ratio, rnd  # noqa: E402,F401

MARGIN = 10.0
HEADROOM = 0.5
SC_CHUNK, SC_PART_MAX_D, RS_TILE, SCAN_BLOCK = 256, 8192, 512, 1024
RLA_TPB, RLA_MAX_L = 32, 12288
CE_MAXV = 17
SWEEP_DEFAULT_CHUNK = 16384
BEHIND = 3.0                     # what the pad columns of an INPUT hold (dout's columns d .. ld)

MUTANTS = dict(
    gather=("oob_row0", "id_trunc32", "ld_ignored", "tail_tokens_dropped", "cols_ge_512_dropped", "trunc_conversion"),
    scatter=("last_of_run_dropped", "t17_dropped", "behind_boundary_lost", "behind_boundary_twice", "third_chunk_lost", "oob_to_row0",
             "oob_to_last_row", "key8", "key16", "ld_ignored", "acc_assign", "sweep2_cols_dropped"),
    assemble=("before_not_counted", "rank_inclusive", "rank_wraps", "pos_omitted_for_placeholders", "labels_first_chunk_only",
              "dvis_unused_left"),
    ce=("pad_included", "last_partial_vector_dropped", "max_not_subtracted", "onehot_not_subtracted", "mask_ignored_in_w",
        "own_mask_sum_for_norm", "gscale_dropped", "oob_label_col0", "sums_assigned"),
    sweep=("per_chunk_normaliser", "beta_every_chunk", "beta_never", "ragged_rows_dropped", "pad_rows_included"))


def vn(dt):
    return 8 if dt == "bf16" else 4


def _d(a):
    return np.asarray(a, np.float64)


def _rng(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def _mix(r, c, salt):
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    h = (r * 73856093 + c * 19349663 + (r ^ (c << 7)) * 2654435761 + salt * 83492791) & 0x7FFFFFFF
    return ((h ^ (h >> 13)) * 1274126177) & 0x7FFFFFFF


def hq(r, c, salt=0):
    """index-revealing grid value of (row r, column c): a multiple of 1/4 in [-2, 2] as float32, broadcasting r against c"""
    return (((_mix(r, c, salt) >> 7) % 17 - 8) * 0.25).astype(np.float32)


def table(rows, d, salt, fine=False):
    r, c = np.arange(rows)[:, None], np.arange(d)[None, :]
    t = hq(r, c, salt)
    if fine:                       # ten fraction bits: f32 values that bf16 cannot hold, exact ties among them
        t = t + (((_mix(r, c, salt + 1) >> 9) % 8 - 4) / 1024.0).astype(np.float32)
    return t


def acc0(shape, k=0):
    n = int(np.prod(shape))
    return (0.25 * ((np.arange(n) * 7 + k) % 23 - 11)).astype(np.float32).reshape(shape)


def trunc_bf16(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _mk(kind, **kw):
    kw["kind"] = kind
    kw["id"] = kind + "-" + "-".join(f"{k}{v}" if not isinstance(v, str) else v for k, v in kw.items() if k != "kind")
    return kw


# ================================================================================================ gather
def gather_vec(case):
    """the kernel's vector condition"""
    return (case["tdt"] == "bf16" and case["dt"] == "bf16" and case["d"] % 8 == 0 and case["ld"] % 8 == 0
            and case["tab_off"] % 8 == 0 and case["out_off"] % 8 == 0)


def gather_inputs(case):
    rows, n = case["rows"], case["n"]
    ids = [rows - 1, 1 << 32, 3, rows, 0, -1, 1 << 40, 5, -100, (1 << 32) + 3, 1, rows - 2, 2]
    return dict(table=table(rows, case["d"], 11, fine=case["tdt"] == "f32" and case["dt"] == "bf16"), ids=np.array(ids[:n], np.int64))


def gather_expected(case, inp, mutant=None):
    """[n, ld] float32 holding the expected bits of the whole output body, pad columns (the sentinel) included"""
    n, d, ld, rows = case["n"], case["d"], case["ld"], case["rows"]
    ids = inp["ids"].copy()
    if mutant == "id_trunc32":
        ids = ids.astype(np.int32).astype(np.int64)
    ok = (ids >= 0) & (ids < rows)
    vals = inp["table"][np.where(ok, ids, 0)].astype(np.float64)
    if mutant != "oob_row0":
        vals[~ok] = 0.0
    vals = trunc_bf16(vals) if mutant == "trunc_conversion" else rnd(vals.astype(np.float32), case["dt"])
    if mutant == "cols_ge_512_dropped":
        vals[:, 512:] = SENT
    if mutant == "tail_tokens_dropped":
        vals[n - n % 4:] = SENT
    out = np.full((n, ld), SENT, np.float32)
    if mutant == "ld_ignored":
        out.reshape(-1)[:n * d] = vals.reshape(-1)
    else:
        out[:, :d] = vals
    return out


def gather_applicable(m, case):
    ids = gather_inputs(case)["ids"]
    oob = ((ids < 0) | (ids >= case["rows"])).any()
    return {"oob_row0": oob, "id_trunc32": (ids >= (1 << 31)).any(), "ld_ignored": case["ld"] > case["d"] and case["n"] > 1,
            "tail_tokens_dropped": case["n"] % 4 != 0, "cols_ge_512_dropped": case["d"] > 512,
            "trunc_conversion": case["tdt"] == "f32" and case["dt"] == "bf16"}[m]


def _gather_cases():
    T = []
    G = lambda **kw: T.append(_mk("gather", **{**dict(tdt="bf16", dt="bf16", rows=37, out_off=0, tab_off=0), **kw}))
    for d in (8, 512, 520, 2048):                               # vector path: one sweep of 512 columns, its edge, four sweeps
        for n in (1, 4, 5, 13):
            G(n=n, d=d, ld=d)
        G(n=5, d=d, ld=d + 8)                                   # strided output, still the vector path
        G(n=5, d=d, ld=d + 4)                                   # ... and one that falls to the scalar path
    G(n=13, d=520, ld=520, out_off=4)                           # the output's base 8 bytes off
    G(n=13, d=520, ld=520, tab_off=4)                           # a table view 8 bytes off
    for tdt, dt in (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")):
        for d in (1, 36, 65, 520):
            if not (tdt == dt == "bf16" and d == 520):
                G(tdt=tdt, dt=dt, n=13, d=d, ld=d + 3)
        for n in (1, 4, 5):
            G(tdt=tdt, dt=dt, n=n, d=65, ld=65)
    return T


# ================================================================================================ scatter
def sort_passes(rows):
    return -(-int(rows).bit_length() // 8)       # cap = rows: bits(rows) in 8-bit passes


def scatter_runs(case):
    """(list of (row, count) in ascending row order, list of out-of-table ids) of the case's design"""
    n, rows, spec = case["n"], case["rows"], case["spec"]
    mid = min(rows - 1, 100)
    if spec == "edges":                            # run lengths around the batches of sixteen
        return [(0, 1), (3, 16), (7, 17), (mid, 32), (rows - 1, 33)], []
    if spec == "b256":                             # a run that ends at sorted position 255, one that starts exactly at 256
        return [(1, 200), (5, 56), (9, 40), (50, 300), (rows - 1, 4)], []        # (and one, 296 .. 595, that crosses exactly one boundary)
    if spec == "span":                             # a run over positions 200 .. 800: a head, partial rows, the last ending mid-chunk
        return [(2, 200), (mid, 601), (rows - 1, 29)], [-1, rows, -100, 1 << 33]
    if spec == "one_row":
        return [(min(2, rows - 1), n)], []
    if spec == "oob_cross":                        # the out-of-table region (sorted positions 200 .. 319) crosses a chunk boundary
        return [(0, 120), (rows - 1, 80)], [(-1, rows, -7, rows + 5, 1 << 32, (1 << 32) + 3)[i % 6] for i in range(120)]
    if spec == "all_oob":
        return [], [(-1, rows, -100, 1 << 40)[i % 4] for i in range(n)]
    assert spec == "mix"
    cand = sorted({c for c in (0, 3, 7, 100, 199, 254, 255, 259, 263, 511, 65534, 65535, 65543, rows - 2, rows - 1) if 0 <= c < rows})
    lens, left, runs = (1, 16, 17, 32, 33, 2, 5), n, []
    oob = [-1, rows, (1 << 32) + 3][:max(0, min(3, n - 60))]
    left -= len(oob)
    bulk = cand[len(cand) // 2]
    for i, r in enumerate(c for c in cand if c != bulk):
        k = min(lens[i % len(lens)], left)
        if k:
            runs.append((r, k))
            left -= k
    if left:
        runs.append((bulk, left))
    return sorted(runs), oob


def scatter_inputs(case):
    n, d, ld, rows = case["n"], case["d"], case["ld"], case["rows"]
    runs, oob = scatter_runs(case)
    ids0 = np.concatenate([np.full(k, r, np.int64) for r, k in runs] + [np.array(oob, np.int64)])
    assert ids0.size == n, (case["id"], ids0.size)
    ids = ids0[_rng(case).permutation(n)]
    if case.get("gauss"):
        dout = rnd(_rng(case).standard_normal((n, d), dtype=np.float32), case["dt"])
    else:
        dout = hq(np.arange(n)[:, None], np.arange(d)[None, :], 23)
    buf = np.full((n, ld), BEHIND, np.float32)
    buf[:, :d] = dout
    return dict(ids=ids, dout=buf, acc0=acc0((rows, d), 5))


def scatter_layout(case, ids):
    """per token: in table?, sorted position (stable by (row, token)), first position and end of its run"""
    ok = (ids >= 0) & (ids < case["rows"])
    key = np.where(ok, ids, np.int64(1) << 62)
    order = np.argsort(key, kind="stable")
    pos = np.empty(ids.size, np.int64)
    pos[order] = np.arange(ids.size)
    sk = key[order]
    return ok, pos, np.searchsorted(sk, key, "left"), np.searchsorted(sk, key, "right")


def scatter_partials(case):
    return case["d"] <= SC_PART_MAX_D


def scatter_crossings(case):
    """chunk boundaries inside each in-table run (0, 1, >= 2 are the branches of the owner's partial-row loop)"""
    ids = scatter_inputs(case)["ids"]
    ok, pos, start, end = scatter_layout(case, ids)
    return sorted({int((e - 1) // SC_CHUNK - s // SC_CHUNK) for s, e in zip(start[ok], end[ok])})


def scatter_reference(case, inp, mutant=None, absolute=False):
    """float64 [rows, d]: acc0 + the run sums (a mutant: with one mistake); ``absolute``: of absolute values"""
    n, d, ld, rows = case["n"], case["d"], case["ld"], case["rows"]
    ids = inp["ids"]
    ok, pos, start, end = scatter_layout(case, ids)
    f = np.abs if absolute else (lambda a: a)
    dout = inp["dout"].reshape(-1)[:n * d].reshape(n, d) if mutant == "ld_ignored" else inp["dout"][:, :d]
    w = np.ones(n)
    b1 = (start // SC_CHUNK + 1) * SC_CHUNK
    part = scatter_partials(case)
    if mutant == "last_of_run_dropped":
        w[pos == end - 1] = 0
    elif mutant == "t17_dropped":
        w[pos - start == 16] = 0
    elif mutant == "behind_boundary_lost" and part:
        w[pos >= b1] = 0
    elif mutant == "behind_boundary_twice" and part:
        w[pos >= b1] = 2
    elif mutant == "third_chunk_lost" and part:
        w[(pos >= b1 + SC_CHUNK) & (pos < b1 + 2 * SC_CHUNK)] = 0
    tgt, use = ids.copy(), ok.copy()
    if mutant in ("oob_to_row0", "oob_to_last_row"):
        tgt[~ok], use = (0 if mutant == "oob_to_row0" else rows - 1), np.ones(n, bool)
    elif mutant in ("key8", "key16"):
        tgt = np.where(ok, ids & (255 if mutant == "key8" else 65535), ids)
    out = f(_d(inp["acc0"])).copy()
    for r in np.unique(tgt[use]):
        sel = use & (tgt == r)
        s = (w[sel, None] * f(_d(dout[sel]))).sum(0)
        if mutant == "sweep2_cols_dropped":
            s[4 * 64 * vn(case["dt"]):] = 0
        out[r] = s if mutant == "acc_assign" else out[r] + s
    return out


def scatter_expected(case, inp, mutant=None):
    return scatter_reference(case, inp, mutant).astype(np.float32)


def scatter_bound(case, inp):
    """(float64 reference, bound) of the Gaussian case"""
    ok, pos, start, end = scatter_layout(case, inp["ids"])
    ln = np.zeros(case["rows"])
    ln[inp["ids"][ok]] = (end - start)[ok]
    ref = scatter_reference(case, inp)
    A = scatter_reference(case, inp, absolute=True)
    return ref, bound(ref, (ln + np.ceil(ln / SC_CHUNK) + 1)[:, None] * A, 1, "f32")


def scatter_model(case, inp, seed=1):
    """fp32, another order than the device's: the tokens of every row added one by one in a shuffled order onto the accumulator"""
    d = case["d"]
    ok = (inp["ids"] >= 0) & (inp["ids"] < case["rows"])
    out = inp["acc0"].copy()
    for t in np.random.default_rng(seed).permutation(case["n"]):
        if ok[t]:
            out[inp["ids"][t]] = out[inp["ids"][t]] + inp["dout"][t, :d]
    return out


def scatter_units(case, inp):
    """the largest sum of |terms| of a table element in units of 1/4"""
    return float(scatter_reference(case, inp, absolute=True).max()) * 4


def scatter_applicable(m, case):
    if case.get("gauss"):
        return False
    inp = scatter_inputs(case)
    ids = inp["ids"]
    ok, pos, start, end = scatter_layout(case, ids)
    ln = (end - start)[ok]
    cross = (((end - 1) // SC_CHUNK) - (start // SC_CHUNK))[ok]
    part = scatter_partials(case)
    return bool({"last_of_run_dropped": ok.any(), "t17_dropped": ok.any() and ln.max() >= 17,
                 "behind_boundary_lost": part and ok.any() and cross.max() >= 1, "behind_boundary_twice": part and ok.any() and cross.max() >= 1,
                 "third_chunk_lost": part and ok.any() and cross.max() >= 2, "oob_to_row0": (~ok).any(), "oob_to_last_row": (~ok).any(),
                 "key8": ok.any() and ids[ok].max() >= 256, "key16": ok.any() and ids[ok].max() >= 65536,
                 "ld_ignored": case["ld"] > case["d"] and case["n"] > 1, "acc_assign": ok.any(),
                 "sweep2_cols_dropped": ok.any() and case["d"] > 4 * 64 * vn(case["dt"])}[m])


def _scatter_cases():
    T = []
    Sc = lambda **kw: T.append(_mk("scatter", **{**dict(dt="f32", rows=200, d=8, ldx=0), **kw}))
    for rows in (200, 65536):                                   # one and three sort passes at every tile / scan edge
        for n in (1, 63, 64, 65, 511, 512, 513, 2049):
            Sc(rows=rows, n=n, spec="mix")
    for rows in (255, 256, 65535, 65736):                       # one, two, two, three passes (65 736 rows: ids above 65 535 exist)
        for n in (513, 2049):
            Sc(rows=rows, n=n, spec="mix")
    for dt in ("f32", "bf16"):
        Sc(dt=dt, n=99, spec="edges")
        Sc(dt=dt, n=600, spec="b256")
        Sc(dt=dt, n=1000, spec="one_row")
        Sc(dt=dt, n=320, spec="oob_cross")
        Sc(dt=dt, n=300, spec="all_oob")
        for d in ((4, 1024, 1028) if dt == "f32" else (8, 2048, 2056)):      # one lane group, one full sweep of the four waves, a second sweep
            Sc(dt=dt, d=d, n=834, spec="span")
        Sc(dt=dt, d=vn(dt), ldx=2 * vn(dt), n=834, spec="span")            # ld_dout > d
        for d in (8192, 8200):                                              # the last shape with partial rows, the first without
            Sc(dt=dt, rows=5, d=d, n=600, spec="one_row")
        Sc(dt=dt, d=64, n=834, spec="span", gauss=1)
    for c in T:
        c["ld"] = c["d"] + c.pop("ldx")
    return T


# ================================================================================================ RL assembly
N_WORD, N_POS = 50, 40


def assemble_placeholders(B, L):
    """per row the placeholder positions: row 0 at the chunk edges; row 1 one whole chunk; row 2 few, one beyond each 256-step of the count"""
    rows = [[p for p in (0, 31, 32, 63, L - 1) if 0 <= p < L],
            list(range(32, 64)) if L >= 64 else list(range(min(L, 32))),
            [p for p in (3, 260, 520, L - 2) if 0 <= p < L - 1]]
    return [sorted(set(r)) for r in rows[:B]]


def assemble_nvis(case):
    ph = assemble_placeholders(case["B"], case["L"])
    return max(1, len(ph[0]))          # row 0: equal to nvis; row 1 (a whole chunk): above for L > 5; row 2: below


def assemble_inputs(case):
    B, L, d = case["B"], case["L"], case["d"]
    fine = case["tdt"] == "f32" and case["dt"] == "bf16"
    t = np.arange(B * L).reshape(B, L)
    ids = (_mix(t, 1, 31) % N_WORD).astype(np.int64)
    pid = (_mix(t, 2, 37) % N_POS).astype(np.int64)
    for b, ph in enumerate(assemble_placeholders(B, L)):
        ids[b, ph] = -1
    free = [(b, p) for b in range(B) for p in range(L) if ids[b, p] != -1]
    for k, v in enumerate((N_WORD, -2)):                         # word ids outside the table (-1 is the placeholder)
        if len(free) > 2 * k + 1:
            ids[free[2 * k + 1]] = v
    for k, v in enumerate((N_POS, -2)):
        if B * L > k + 1:
            pid.reshape(-1)[(k * 17 + 1) % (B * L)] = v
    lab = (_mix(t, 3, 41) % 90).astype(np.int64)
    lab[_mix(t, 4, 43) % 11 == 0] = -100
    lab[_mix(t, 5, 47) % 7 == 0] = -1
    c0 = 32 if L > 32 else 0
    lab[0, c0:c0 + 32] = -1                                      # every position of one chunk
    nvis = assemble_nvis(case)
    return dict(word=table(N_WORD, d, 51, fine), pos=table(N_POS, d, 53, fine), vis=table(B * nvis, d, 57).reshape(B, nvis, d), ids=ids, pid=pid,
                labels=lab, dout=hq(np.arange(B * L)[:, None], np.arange(d)[None, :], 59).reshape(B, L, d),
                dword0=acc0((N_WORD, d), 1), dpos0=acc0((N_POS, d), 2), nvis=nvis)


def assemble_ranks(ids, mutant=None):
    ph = ids == -1
    rk = np.cumsum(ph, 1) - ph                                   # exclusive
    if mutant == "before_not_counted":
        L = ids.shape[1]
        first = (np.arange(L) // RLA_TPB) * RLA_TPB
        rk = rk - np.take_along_axis(np.concatenate([np.zeros((ids.shape[0], 1), np.int64), np.cumsum(ph, 1)], 1), np.broadcast_to(first, ids.shape), 1)
    if mutant == "rank_inclusive":
        rk = rk + 1
    return np.where(ph, rk, -1)


def assemble_expected(case, inp, mutant=None):
    """{out, labels, dword, dpos, dvis}: the expected bits (float32 / int64)"""
    B, L, d, nvis = case["B"], case["L"], case["d"], inp["nvis"]
    ids, pid = inp["ids"], inp["pid"]
    rk = assemble_ranks(ids, mutant)
    if mutant == "rank_wraps":
        rk = np.where(rk >= nvis, 0, rk)
    id_ok, pid_ok = (ids >= 0) & (ids < N_WORD), (pid >= 0) & (pid < N_POS)
    vis_ok = ~id_ok & (rk >= 0) & (rk < nvis)
    out = {}
    bidx = np.broadcast_to(np.arange(B)[:, None], (B, L))
    v = np.where(id_ok[..., None], _d(inp["word"])[np.where(id_ok, ids, 0)], 0.0)
    if case["vis"]:
        v = np.where(vis_ok[..., None], _d(inp["vis"])[bidx, np.clip(rk, 0, nvis - 1)], v)
    padd = pid_ok if mutant != "pos_omitted_for_placeholders" else pid_ok & (ids != -1)
    v = v + np.where(padd[..., None], _d(inp["pos"])[np.where(pid_ok, pid, 0)], 0.0)
    out["out"] = rnd(v.astype(np.float32), case["dt"])
    lab = inp["labels"].copy()
    fix = lab == -1
    if mutant == "labels_first_chunk_only":
        fix = fix & (np.arange(L)[None, :] < RLA_TPB)
    lab[fix] = 0
    out["labels"] = lab
    if case["bwd"]:
        g = _d(inp["dout"]).reshape(B * L, d)
        dw, dp = _d(inp["dword0"]).copy(), _d(inp["dpos0"]).copy()
        np.add.at(dw, ids.reshape(-1)[id_ok.reshape(-1)], g[id_ok.reshape(-1)])
        np.add.at(dp, pid.reshape(-1)[pid_ok.reshape(-1)], g[pid_ok.reshape(-1)])
        dv = np.full((B, nvis, d), SENT if mutant == "dvis_unused_left" else 0.0)
        dv[bidx[vis_ok], rk[vis_ok]] = g.reshape(B, L, d)[vis_ok]
        out.update(dword=dw.astype(np.float32), dpos=dp.astype(np.float32), dvis=dv.astype(np.float32))
    return out


def assemble_units(case, inp):
    B, L, d = case["B"], case["L"], case["d"]
    g = np.abs(_d(inp["dout"])).reshape(B * L, d)
    dw, dp = np.abs(_d(inp["dword0"])), np.abs(_d(inp["dpos0"]))
    ok_w, ok_p = ((inp["ids"] >= 0) & (inp["ids"] < N_WORD)).reshape(-1), ((inp["pid"] >= 0) & (inp["pid"] < N_POS)).reshape(-1)
    np.add.at(dw, inp["ids"].reshape(-1)[ok_w], g[ok_w])
    np.add.at(dp, inp["pid"].reshape(-1)[ok_p], g[ok_p])
    return max(dw.max(), dp.max()) * 4, (np.abs(inp["word"]).max() + np.abs(inp["pos"]).max()) * 1024     # backward in 1/4, forward in 2^-10


def assemble_applicable(m, case):
    inp = assemble_inputs(case)
    cnt = (inp["ids"] == -1).sum(1)
    return bool({"before_not_counted": case["vis"] and case["L"] > 32, "rank_inclusive": case["vis"], "rank_wraps": case["vis"] and cnt.max() > inp["nvis"],
                 "pos_omitted_for_placeholders": True, "labels_first_chunk_only": case["labels"] and case["L"] > 32,
                 "dvis_unused_left": case["bwd"] and cnt.min() < inp["nvis"]}[m])


def _assemble_cases():
    T = []
    A = lambda **kw: T.append(_mk("assemble", **{**dict(B=3, tdt="f32", dt="f32", d=64, vis=1, labels=1, bwd=1), **kw}))
    for L in (1, 31, 32, 33, 300, 600):
        A(L=L, d=64)
        A(L=L, tdt="bf16", dt="bf16", d=64)
    A(L=300, d=4)
    A(L=300, tdt="bf16", dt="bf16", d=8)
    for tdt, dt in (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")):
        for d in (1, 40, 65):
            A(L=70, tdt=tdt, dt=dt, d=d, bwd=0)
        if tdt != dt:
            A(L=70, tdt=tdt, dt=dt, d=64, bwd=0)
    A(L=70, vis=0)
    A(L=70, labels=0)
    A(B=1, L=RLA_MAX_L, d=8)
    return T


# ================================================================================================ masked cross-entropy
DESIGNS = ("equal", "peak_at", "peak_off", "asc", "desc", "off30k", "gauss3")
PADS = {"inf": np.inf, "nan": np.nan, "big": 3e38}


def ce_vec_ok(case):
    return case["ld"] % vn(case["dt"]) == 0 and case["off"] == 0


def ce_supported(dt, V, ld):
    """db1_masked_ce_fwd_bwd_supported"""
    return not (ld % vn(dt) != 0 or ld > 256 * vn(dt) * CE_MAXV) and 0 < V <= ld


def ce_rows(T, V, dt, seed, designs=DESIGNS):
    """(logits [T, V] as stored, labels, masks): row t has design designs[t % len]"""
    rng = np.random.default_rng(seed)
    x = np.zeros((T, V), np.float32)
    lab_cycle = (0, V - 1, V, -1, -100, 1 % V)
    labels = np.array([lab_cycle[(t + t // 7) % 6] for t in range(T)], np.int64)
    masks = np.array([(1, 0.5, 1, 0, 1, 0.5, 1, 1)[t % 8] for t in range(T)], np.float32)
    for t in range(T):
        dsg = designs[t % len(designs)]
        if dsg == "equal":
            x[t] = 1.25
        elif dsg in ("peak_at", "peak_off"):
            pk = (7 * t + 3) % V
            x[t] = -1.0
            x[t, pk] = 39.0
            labels[t] = pk if dsg == "peak_at" else (pk + 1) % V
        elif dsg in ("asc", "desc"):
            r = np.linspace(-90.0, 90.0, V) if V > 1 else np.array([-90.0])
            x[t] = r if dsg == "asc" else r[::-1]
        elif dsg == "off30k":
            x[t] = 30000.0 + rng.standard_normal(V)
        else:
            x[t] = 3.0 * rng.standard_normal(V)
    return rnd(x, dt), labels, masks


def ce_inputs(case):
    T, V, ld, dt = case["T"], case["V"], case["ld"], case["dt"]
    x, labels, masks = ce_rows(T, V, dt, zlib.crc32(case["id"].encode()), tuple(case["designs"].split("+")) if case.get("designs") else DESIGNS)
    buf = np.full((T, ld), PADS[case["pad"]], np.float32)
    buf[:, :V] = x
    return dict(logits=buf, labels=labels, masks=masks, sums0=np.array([3.0, -2.0], np.float32), norm1=np.float32(6.5), gscale=case["gscale"])


def ce_chain(dt, V, vec):
    """(nadds, nresc) of a thread's online (max, sum)"""
    if vec:
        nv = -(-V // (256 * vn(dt)))
        return vn(dt) * nv, nv
    n = -(-V // 256)
    return n, n


def ce_expect(x, labels, masks, norm1, gscale, sums0, dt, vec, ld=None, sum_extra=0, sum_rows=None):
    """references and bounds {lse, sums, dlogits, tok} from logits x [T, V] (float64, as stored).  ``sum_extra``: further roundings of the
    loss sum (the sweep's chunk adds); ``sum_rows``: rows one ce_sum_kernel call sees (default T)."""
    x = _d(x)
    T, V = x.shape
    ld = ld or V
    M = x.max(1)
    with np.errstate(under="ignore"):
        e = np.exp(x - M[:, None])
    Ssum = e.sum(1)
    lse = M + np.log(Ssum)
    with np.errstate(under="ignore"):
        p = np.exp(x - lse[:, None])
    nadds, nresc = ce_chain(dt, V, vec)
    cS = nadds + 9 + 4 * (nresc + 2) + 4 * (p * (M[:, None] - x)).sum(1)
    E_lse = bound(lse, cS + 6 * np.abs(lse - M), 1, "f32")
    ok = (labels >= 0) & (labels < V)
    mk = np.where(ok, _d(masks), 0.0)
    xy = x[np.arange(T), np.where(ok, labels, 0)]
    tok = mk * np.where(ok, lse - xy, 0.0)
    E_tok = mk * E_lse + S.SHARE * 2 * U * np.abs(tok)
    s0 = _d(sums0)
    sums = np.array([s0[0] + tok.sum(), s0[1] + _d(masks).sum()])
    chain = -(-(sum_rows or T) // 1024) + 11 + sum_extra
    b0 = half_ulp(sums[0], "f32") + E_tok.sum() + S.SHARE * chain * U * (np.abs(tok).sum() + abs(s0[0]))
    w = mk / float(norm1) * float(gscale)
    hot = np.zeros((T, V))
    hot[np.arange(T)[ok], labels[ok]] = 1.0
    dl = w[:, None] * (p - hot)
    aw = np.abs(w)[:, None]
    E = S.SHARE * U * (aw * (p * (3 + 4 * np.abs(x - lse[:, None])) + np.abs(p - hot)) + 4 * aw * np.abs(p - hot)) + aw * p * E_lse[:, None]
    k = 2.0 if dt == "bf16" else 1.0
    bdl = np.maximum(half_ulp(dl, dt) + k * E, S.TINY)
    ref, bnd = np.zeros((T, ld)), np.zeros((T, ld))
    ref[:, :V], bnd[:, :V] = dl, bdl
    return dict(lse=(lse, E_lse), sums=(sums, np.array([b0, 0.0])), dlogits=(ref, bnd), tok=(tok, E_tok))


def _exp32(a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(a.astype(np.float64)).astype(np.float32)


def ce_model(x, labels, masks, norm1, gscale, sums0, dt, ld=None, mutant=None, vnw=None, pad=None):
    """fp32 transcription in ANOTHER order than the device's: the maximum first, then one pairwise sum of the exponentials (the device:
    online, serial per thread, then a tree); the loss sum serial in row order (the device: strided, then a tree).  x [T, V] float32 as stored."""
    f = np.float32
    T, V = x.shape
    ld = ld or V
    xs = x
    if mutant == "pad_included" and ld > V:
        xs = np.concatenate([x, np.full((T, ld - V), pad, f)], 1)
    if mutant == "last_partial_vector_dropped" and V % vnw:
        xs = x[:, :V - V % vnw]
    with np.errstate(all="ignore"):
        M = xs.max(1) if xs.shape[1] else np.full(T, -3e38, f)
        sh = xs if mutant == "max_not_subtracted" else xs - M[:, None]
        Ssum = _exp32(sh).sum(1, dtype=f)
        lg = np.log(Ssum.astype(np.float64)).astype(f)
        lse = lg if mutant == "max_not_subtracted" else M + lg
        ok = (labels >= 0) & (labels < V)
        col = np.where(ok, labels, 0)
        if mutant == "oob_label_col0":
            ok = np.ones(T, bool)
        mk = np.where(ok, masks, f(0))
        tok = mk * np.where(ok, lse - x[np.arange(T), col], f(0))
        a, b = f(0), f(0)
        for t in range(T):
            a, b = a + tok[t], b + masks[t]
        sums = np.array([a, b], f) if mutant == "sums_assigned" else np.array([sums0[0] + a, sums0[1] + b], f)
        n1 = b if mutant == "own_mask_sum_for_norm" else f(norm1)
        w = (np.where(ok, f(1), f(0)) if mutant == "mask_ignored_in_w" else mk) / n1
        if mutant != "gscale_dropped":
            w = w * f(gscale)
        hot = np.zeros((T, V), f)
        if mutant != "onehot_not_subtracted":
            hot[np.arange(T)[ok], col[ok]] = 1
        dl = np.zeros((T, ld), f)
        dl[:, :V] = rnd(w[:, None] * (_exp32(x - lse[:, None]) - hot), dt)
    return dict(lse=lse, sums=sums, dlogits=dl)


def ce_run_model(case, inp, mutant=None):
    V = case["V"]
    return ce_model(inp["logits"][:, :V], inp["labels"], inp["masks"], inp["norm1"], inp["gscale"], inp["sums0"], case["dt"], case["ld"], mutant,
                    vn(case["dt"]), PADS[case["pad"]])


def ce_run_expect(case, inp):
    V = case["V"]
    return {k: v for k, v in ce_expect(inp["logits"][:, :V], inp["labels"], inp["masks"], inp["norm1"], inp["gscale"], inp["sums0"], case["dt"],
                                       ce_vec_ok(case), case["ld"]).items() if k != "tok"}


def ce_applicable(m, case):
    inp = ce_inputs(case)
    V, lab = case["V"], inp["labels"]
    valid = (lab >= 0) & (lab < V)
    live = valid & (inp["masks"] > 0)
    return bool({"pad_included": case["ld"] > V, "last_partial_vector_dropped": V % vn(case["dt"]) != 0 and V > vn(case["dt"]) and ce_vec_ok(case),
                 "max_not_subtracted": case["T"] >= 7, "onehot_not_subtracted": live.any(), "mask_ignored_in_w": (valid & (inp["masks"] != 1)).any(),
                 "own_mask_sum_for_norm": live.any(), "gscale_dropped": case["gscale"] != 1 and live.any(),
                 "oob_label_col0": (~valid & (inp["masks"] > 0)).any(), "sums_assigned": True}[m])


def _ce_cases():
    T, k = [], [0]

    def C(**kw):
        pad = ("inf", "nan", "big")[k[0] % 3]
        gs = (1.0, 0.5, 2.0 ** -10)[k[0] % 3]
        k[0] += 1
        T.append(_mk("ce", **{**dict(T=14, off=0, pad=pad, gscale=gs), **kw}))
    for dt in ("f32", "bf16"):
        v = vn(dt)
        C(dt=dt, V=1, ld=v)
        C(dt=dt, V=5, ld=8)
        C(dt=dt, V=256 * v, ld=256 * v)                         # V = ld: one vector per thread exactly
        C(dt=dt, V=256 * v + 1, ld=256 * v + v)                 # a second vector for thread 0 alone, V % VN != 0
        C(dt=dt, V=1000, ld=1024)
        C(dt=dt, V=1003, ld=1024)                               # V % VN != 0 in both dtypes
        C(dt=dt, V=1000, ld=1024, off=1)                        # scalar path by alignment
        C(dt=dt, V=256 * v * CE_MAXV - 3, ld=256 * v * CE_MAXV, T=3, designs="gauss3+asc+peak_at")        # the fwd_bwd limit
        C(dt=dt, V=256 * v * CE_MAXV + 1, ld=256 * v * CE_MAXV + v, T=3, designs="gauss3+desc+peak_off")  # past it: the pair only
    C(dt="f32", V=1325, ld=1325)                                # scalar path by ld
    C(dt="bf16", V=33025, ld=33280, T=2, designs="gauss3+asc")           # the model's own vocabulary
    for T_ in (1, 1024, 1025):                                  # ce_sum_kernel: one serial add per thread, then two for thread 0
        C(dt="f32", V=8, ld=8, T=T_)
    C(dt="bf16", V=8, ld=8, T=1025)
    return T


# ================================================================================================ the sweep
def sweep_plan(case):
    """(chunk, number of chunks, ragged?, fused fwd_bwd?) as lmhead_plan / lmhead_sweep decide"""
    T = case["T"]
    chunk = min(case["chunk"] if case["chunk"] > 0 else SWEEP_DEFAULT_CHUNK, T)
    return chunk, -(-T // chunk), T % chunk != 0, ce_supported(case["dt"], case["V"], case["rows"])


def sweep_inputs(case):
    T, V, rows, d = case["T"], case["V"], case["rows"], case["d"]
    rng = _rng(case)
    nz = min(15, d - 1)

    def sparse(n, vals):
        a = np.zeros((n, d), np.float32)
        for i in range(n):
            a[i, 1 + rng.choice(d - 1, nz, replace=False)] = rng.choice(vals, nz)
        return a
    h = sparse(T, np.array([0.5, -0.5, 1, -1], np.float32))
    h[:, 0] = 1.0
    W = np.zeros((rows, d), np.float32)
    W[:V] = sparse(V, np.array([0.25, -0.25, 0.5, -0.5], np.float32))
    W[V:, 0] = 30.0                                             # a pad row's logit would be exactly +30 on every token
    _, labels, masks = ce_rows(T, V, "f32", 7, ("equal",))
    chunk = sweep_plan(case)[0]
    if case["mask0"]:
        masks[:chunk] = 0                                       # nothing counts in the first chunk: the normaliser is the sum over ALL rows
    return dict(h=h, W=W, labels=labels, masks=masks, sums0=np.array([3.0, -2.0], np.float32), gscale=0.5, dW0=acc0((rows, d), 3))


def sweep_logits(inp, V):
    return _d(inp["h"]) @ _d(inp["W"][:V]).T


def sweep_expect(case, inp):
    T, V, rows, d, dt = case["T"], case["V"], case["rows"], case["d"], case["dt"]
    chunk, nch, _, fused = sweep_plan(case)
    x = sweep_logits(inp, V)
    norm1 = float(_d(inp["masks"]).sum())
    ce = ce_expect(x, inp["labels"], inp["masks"], norm1, inp["gscale"], inp["sums0"], dt, True, rows, sum_extra=nch + 1, sum_rows=chunk)
    dl, Edl = ce["dlogits"]
    h, W = _d(inp["h"]), _d(inp["W"])
    dh = dl @ W
    Adh = Edl @ np.abs(W) / U + S.SHARE * (rows + nch + 1) * (np.abs(dl) @ np.abs(W))
    dW = case["beta"] * _d(inp["dW0"]) + dl.T @ h
    AdW = Edl.T @ np.abs(h) / U + S.SHARE * (T + nch + 1) * (np.abs(dl).T @ np.abs(h) + case["beta"] * np.abs(_d(inp["dW0"])))
    k = 2.0 if dt == "bf16" else 1.0
    bW = np.maximum(half_ulp(dW, "f32") + U * AdW, S.TINY)
    if case["beta"] == 0:
        bW[V:] = 0.0                                            # pad rows: exactly 0 (beta 1: dW0, whose half ulp the line above grants -- the GPU test compares their bits)
    return dict(lse=ce["lse"], sums=ce["sums"], dh=(dh, np.maximum(half_ulp(dh, dt) + k * U * Adh, S.TINY)), dW=(dW, bW))


def sweep_model(case, inp, mutant=None):
    """fp32 transcription: dense logits (exact), the cross-entropy model per chunk, products in float32 row by row"""
    f = np.float32
    T, V, rows, d, dt = case["T"], case["V"], case["rows"], case["d"], case["dt"]
    chunk = sweep_plan(case)[0]
    Vm = rows if mutant == "pad_rows_included" else V
    x = (inp["h"] @ inp["W"][:Vm].T).astype(f)
    labels = inp["labels"]
    norm1 = inp["masks"].sum(dtype=f)
    lse, dh = np.full(T, SENT, f), np.full((T, d), SENT, f)
    dW = inp["dW0"].copy()
    loss, first = f(0), True
    for r0 in range(0, T, chunk):
        r1 = min(T, r0 + chunk)
        if mutant == "ragged_rows_dropped" and r1 - r0 < chunk:
            continue
        n1 = inp["masks"][r0:r1].sum(dtype=f) if mutant == "per_chunk_normaliser" else norm1
        m = ce_model(x[r0:r1], labels[r0:r1], inp["masks"][r0:r1], n1, inp["gscale"], np.zeros(2, f), dt, rows)
        lse[r0:r1] = m["lse"]
        loss = loss + m["sums"][0]
        dl = m["dlogits"]
        dh[r0:r1] = rnd((dl @ inp["W"]).astype(f), dt)
        beta = f(case["beta"]) if (first or mutant == "beta_every_chunk") and mutant != "beta_never" else f(1)
        dW = beta * dW + (dl.T @ inp["h"][r0:r1]).astype(f)
        first = False
    return dict(lse=lse, sums=np.array([inp["sums0"][0] + loss, inp["sums0"][1] + norm1], f), dh=dh, dW=dW)


def sweep_applicable(m, case):
    chunk, nch, ragged, _ = sweep_plan(case)
    return bool({"per_chunk_normaliser": nch > 1, "beta_every_chunk": nch > 1 and case["beta"] == 0, "beta_never": case["beta"] == 0,
                 "ragged_rows_dropped": ragged, "pad_rows_included": case["rows"] > case["V"]}[m])


def _sweep_cases():
    T = []
    W = lambda **kw: T.append(_mk("sweep", **{**dict(dt="f32", T=40, V=1000, rows=1024, d=64, chunk=0, beta=1, mask0=0), **kw}))
    for dt in ("f32", "bf16"):
        for beta in (0, 1):
            W(dt=dt, T=300, chunk=128, beta=beta, mask0=beta)   # three chunks, the last ragged
    W(dt="bf16", chunk=40, beta=0)                              # chunk = T
    W(dt="f32", chunk=64)                                       # chunk > T
    W(dt="bf16", chunk=0)                                       # the default
    W(dt="f32", T=1, beta=0)
    W(dt="bf16", T=5, chunk=1, beta=0)                          # the smallest chunk the GEMM accepts: one row
    W(dt="f32", T=40, V=17409, rows=17472, d=16, chunk=16, beta=0)            # fwd_bwd unsupported: the forward / backward pair
    return T


# ================================================================================================ tables
CASES = _gather_cases() + _scatter_cases() + _assemble_cases() + _ce_cases() + _sweep_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
APPLICABLE = dict(gather=gather_applicable, scatter=scatter_applicable, assemble=assemble_applicable, ce=ce_applicable, sweep=sweep_applicable)


def cases(*kinds):
    return [c for c in CASES if c["kind"] in kinds]
