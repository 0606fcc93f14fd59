"""The rule of tests/embed_ce_rule.py proved usable without a GPU: every exact probe meets its exactness condition and an fp32 transcription
in shuffled term orders reproduces the expected bits; the fp32 model of every bounded case (another summation order than the device's) stays
under half of every bound; every one-mistake mutant of the reference is caught by at least one case of its family (exact cases: a differing
bit; bounded cases: an element moved by ten bounds), with the table of which case catches which mutant printed; and the dispatch predicates
restated in Python take every value over the case tables."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stream_rule as S  # noqa: E402
import embed_ce_rule as R  # noqa: E402

ids = lambda cs: [c["id"] for c in cs]
GATHER, SCATTER, ASSEMBLE, CE, SWEEP = (R.cases(k) for k in ("gather", "scatter", "assemble", "ce", "sweep"))
SCATTER_EXACT = [c for c in SCATTER if not c.get("gauss")]
SCATTER_GAUSS = [c for c in SCATTER if c.get("gauss")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid(a, dt, frac):
    """every value is one of its storage type and a multiple of 2^-frac"""
    a = np.asarray(a, np.float32)
    return np.array_equal(S.rnd(a, dt), a) and np.array_equal(np.round(a * 2.0 ** frac), a * 2.0 ** frac)


def shared(fn, lo=1.0):
    """run fn() with the fp32 allowance of every bound scaled by ``lo``"""
    S.SHARE = lo
    try:
        with np.errstate(all="ignore"):
            return fn()
    finally:
        S.SHARE = 1.0


# ------------------------------------------------------------------------------------------------ 1. exactness
def test_the_grid_hash_reveals_rows_and_columns():
    t = R.table(300, 64, 11)
    assert grid(t, "bf16", 2) and np.abs(t).max() <= 2.0
    diff = (t[:, None, :] != t[None, :, :]).mean(-1)[np.triu_indices(300, 1)]
    assert diff.min() > 0.7, "two rows agree in too many columns"
    assert (t[:, 1:] != t[:, :-1]).mean() > 0.85 and (t[:, 4:] != t[:, :-4]).mean() > 0.85 and (t[:, 8:] != t[:, :-8]).mean() > 0.85
    f = R.table(37, 520, 11, fine=True)
    assert grid(f, "f32", 10) and not grid(f, "bf16", 10)
    up, dn = S.bf16(f) > f, S.bf16(f) < f
    tie = (np.abs(S.bf16(f).astype(np.float64) - f) == S.half_ulp(f, "bf16")) & (f != 0)
    assert up.any() and dn.any() and tie.any(), "the f32 -> bf16 probe needs values rounded up, down and exact ties"
    assert (R.trunc_bf16(f) != S.bf16(f)).any()


@pytest.mark.parametrize("case", GATHER, ids=ids(GATHER))
def test_gather_probe(case):
    inp = R.gather_inputs(case)
    fine = case["tdt"] == "f32" and case["dt"] == "bf16"
    assert grid(inp["table"], case["tdt"], 10 if fine else 2)
    want = R.gather_expected(case, inp)
    assert grid(want, case["dt"], 10) and (want[:, :case["d"]] != R.SENT).all() and (want[:, case["d"]:] == R.SENT).all()
    assert inp["ids"].size == case["n"]


@pytest.mark.parametrize("case", SCATTER_EXACT, ids=ids(SCATTER_EXACT))
def test_scatter_probe_is_exact_in_any_order(case):
    inp = R.scatter_inputs(case)
    assert grid(inp["dout"], case["dt"], 2) and grid(inp["acc0"], "f32", 2) and np.abs(inp["acc0"]).max() < 8
    units = R.scatter_units(case, inp)
    assert units < 2 ** 24, f"sum of |terms| = {units} quarter units"
    want = R.scatter_expected(case, inp)
    assert np.array_equal(want.astype(np.float64), R.scatter_reference(case, inp)), "an expected value is not representable"
    assert not (want == R.SENT).any()
    if case["n"] * case["d"] <= 1 << 16:
        for seed in (1, 2):
            assert np.array_equal(bits(R.scatter_model(case, inp, seed)), bits(want)), f"{case['id']}: the fp32 model in token order {seed} gives other bits"
    # the runs of the design lie where the table says
    runs, oob = R.scatter_runs(case)
    ok, pos, start, end = R.scatter_layout(case, inp["ids"])
    p = 0
    for r, k in runs:
        sel = inp["ids"] == r
        assert sel.sum() == k and (start[sel] == p).all() and (end[sel] == p + k).all()
        p += k
    assert (~ok).sum() == len(oob) and (pos[~ok] >= p).all()


@pytest.mark.parametrize("case", ASSEMBLE, ids=ids(ASSEMBLE))
def test_assembly_probe_is_exact(case):
    inp = R.assemble_inputs(case)
    fine = case["tdt"] == "f32" and case["dt"] == "bf16"
    assert grid(inp["word"], case["tdt"], 10 if fine else 2) and grid(inp["pos"], case["tdt"], 10 if fine else 2)
    assert grid(inp["vis"], case["dt"], 2) and grid(inp["dout"], case["dt"], 2)
    ub, uf = R.assemble_units(case, inp)
    assert ub < 2 ** 24 and uf < 2 ** 24
    want = R.assemble_expected(case, inp)
    for name in ("out", "dword", "dpos", "dvis"):
        if name in want:
            assert not (want[name] == R.SENT).any(), name
    cnt = (inp["ids"] == -1).sum(1)
    if case["L"] >= 300 and case["B"] == 3:
        assert cnt[0] == inp["nvis"] and cnt[1] > inp["nvis"] and cnt[2] < inp["nvis"]
    assert ((inp["ids"] == R.N_WORD).any() and (inp["ids"] == -2).any()) or case["L"] < 5
    assert ((inp["pid"] == R.N_POS).any() and (inp["pid"] == -2).any()) or case["L"] < 5
    assert (inp["labels"] == -100).any() or case["L"] < 5
    assert (inp["labels"][0, (32 if case["L"] > 32 else 0):][:32] == -1).all()


@pytest.mark.parametrize("case", SWEEP, ids=ids(SWEEP))
def test_sweep_logits_are_exact(case):
    inp = R.sweep_inputs(case)
    V = case["V"]
    x = R.sweep_logits(inp, V)
    assert np.array_equal(np.round(x * 8), x * 8) and np.abs(x).max() < 16 and grid(x, "bf16", 3)
    assert grid(inp["h"], "bf16", 1) and grid(inp["W"], "bf16", 2)
    assert np.abs(R._d(inp["h"])).sum(1).max() * 0.5 * 8 < 2 ** 24                  # |W| <= 1/2: every partial sum of a logit is exact
    if case["rows"] > V:
        assert (R._d(inp["h"]) @ R._d(inp["W"][V:]).T == 30.0).all()
    chunk = R.sweep_plan(case)[0]
    if case["mask0"]:
        assert (inp["masks"][:chunk] == 0).all() and inp["masks"][chunk:].sum() > 0


# ------------------------------------------------------------------------------------------------ 2. the fp32 model under half of every bound
def within(got, exp, cid, share):
    worst = {}
    for name, (ref, bnd) in exp.items():
        worst[name] = R.check(got[name], ref, bnd, f"{cid} {name} (fp32 allowance x {share})")
        assert np.all(np.abs(np.asarray(ref, np.float64) - R.SENT) > bnd), f"{cid} {name}: a reference value within its bound of the sentinel"
    return worst


@pytest.mark.parametrize("case", CE, ids=ids(CE))
def test_ce_model_within_half_of_every_bound(case):
    inp = R.ce_inputs(case)
    exp = shared(lambda: R.ce_run_expect(case, inp), R.HEADROOM)
    got = shared(lambda: R.ce_run_model(case, inp))
    print(case["id"], within(got, exp, case["id"], R.HEADROOM))
    ref, bnd = exp["dlogits"]
    assert (ref[:, case["V"]:] == 0).all() and (bnd[:, case["V"]:] == 0).all()


@pytest.mark.parametrize("case", SWEEP, ids=ids(SWEEP))
def test_sweep_model_within_half_of_every_bound(case):
    inp = R.sweep_inputs(case)
    exp = shared(lambda: R.sweep_expect(case, inp), R.HEADROOM)
    got = shared(lambda: R.sweep_model(case, inp))
    print(case["id"], within(got, exp, case["id"], R.HEADROOM))


@pytest.mark.parametrize("case", SCATTER_GAUSS, ids=ids(SCATTER_GAUSS))
def test_scatter_model_within_half_of_the_bound(case):
    inp = R.scatter_inputs(case)
    ref, bnd = shared(lambda: R.scatter_bound(case, inp), R.HEADROOM)
    for seed in (1, 2):
        R.check(R.scatter_model(case, inp, seed), ref, bnd, f"{case['id']} order {seed}")


def test_equal_logits_have_the_closed_form():
    x, _, _ = R.ce_rows(7, 1000, "f32", 1)
    e = R.ce_expect(x, np.zeros(7, np.int64), np.ones(7, np.float32), 7.0, 1.0, np.zeros(2), "f32", True)
    assert abs(e["lse"][0][0] - (1.25 + np.log(1000.0))) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. mutants
def caught_exact(family, case, m):
    if family == "gather":
        inp = R.gather_inputs(case)
        return (bits(R.gather_expected(case, inp)) != bits(R.gather_expected(case, inp, m))).any()
    if family == "scatter":
        inp = R.scatter_inputs(case)
        return (bits(R.scatter_expected(case, inp)) != bits(R.scatter_expected(case, inp, m))).any()
    inp = R.assemble_inputs(case)
    a, b = R.assemble_expected(case, inp), R.assemble_expected(case, inp, m)
    return any(not np.array_equal(a[k].view(np.uint8) if a[k].dtype == np.int64 else bits(a[k]),
                                  b[k].view(np.uint8) if b[k].dtype == np.int64 else bits(b[k])) for k in a)


def worst_ratio(family, case, m):
    if family == "ce":
        inp = R.ce_inputs(case)
        got, exp = shared(lambda: R.ce_run_model(case, inp, m)), shared(lambda: R.ce_run_expect(case, inp))
    else:
        inp = R.sweep_inputs(case)
        got, exp = shared(lambda: R.sweep_model(case, inp, m)), shared(lambda: R.sweep_expect(case, inp))
    return max(float(R.ratio(got[k], ref, bnd).max()) for k, (ref, bnd) in exp.items())


@pytest.mark.parametrize("family", list(R.MUTANTS))
def test_every_mutant_is_caught(family):
    """per mutant: the cases it applies to and, of those, the ones that catch it (printed); at least one case of the family must"""
    small = lambda c: c.get("n", 0) * c.get("d", 0) <= 1 << 21 and c.get("L", 0) <= 600 and c.get("V", 0) <= 4200
    for m in R.MUTANTS[family]:
        hit, app = [], 0
        for case in R.cases(family):
            if not small(case) or not R.APPLICABLE[family](m, case):
                continue
            app += 1
            if (worst_ratio(family, case, m) >= R.MARGIN) if family in ("ce", "sweep") else caught_exact(family, case, m):
                hit.append(case["id"])
        print(f"{family} / {m}: caught by {len(hit)} of the {app} cases it applies to: {' '.join(hit[:3])}{' ...' if len(hit) > 3 else ''}")
        assert hit, f"{m} is caught by no case of the {family} table ({app} applicable)"


# ------------------------------------------------------------------------------------------------ 4. branches
def test_tables_reach_every_branch():
    # gather: both sides of the vector condition, each of its clauses failing alone, the four dtype pairs on the scalar path
    g = R.cases("gather")
    assert {R.gather_vec(c) for c in g} == {True, False}
    bb = [c for c in g if c["tdt"] == c["dt"] == "bf16" and not R.gather_vec(c)]
    assert any(c["d"] % 8 for c in bb) and any(c["d"] % 8 == 0 and c["ld"] % 8 for c in bb) and any(c["out_off"] % 8 for c in bb) and any(c["tab_off"] % 8 for c in bb)
    assert {(c["tdt"], c["dt"]) for c in g if not R.gather_vec(c)} == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")}
    assert {c["d"] for c in g if R.gather_vec(c)} == {8, 512, 520, 2048} and {c["n"] for c in g if R.gather_vec(c)} >= {1, 4, 5}
    assert any(R.gather_vec(c) and c["ld"] > c["d"] for c in g)
    # scatter: sort passes, tiles and scan blocks, partial rows, boundaries crossed by a run
    s = R.cases("scatter")
    assert {rows: R.sort_passes(rows) for rows in sorted({c["rows"] for c in s})} == {5: 1, 200: 1, 255: 1, 256: 2, 65535: 2, 65536: 3, 65736: 3}
    for p in (1, 3):
        ns = {c["n"] for c in s if R.sort_passes(c["rows"]) == p}
        assert {-(-n // R.RS_TILE) for n in ns} >= {1, 2, 5} and {n % 64 for n in ns} >= {0, 1, 63}
        assert {-(-256 * -(-n // R.RS_TILE) // R.SCAN_BLOCK) for n in ns} >= {1, 2}, "the scan over 256 x tiles counters: one block of 1024 and more"
    assert {R.scatter_partials(c) for c in s} == {True, False}
    assert {c["d"] for c in s if R.scatter_partials(c)} >= {8192} and {c["d"] for c in s if not R.scatter_partials(c)} == {8200}
    for dt in ("f32", "bf16"):
        cr = set()
        for c in s:
            if c["dt"] == dt and R.scatter_partials(c):
                cr |= set(R.scatter_crossings(c))
        assert cr >= {0, 1, 2}, (dt, cr)
        assert any(R.scatter_crossings(c)[-1] >= 2 for c in s if c["dt"] == dt and not R.scatter_partials(c))
        assert {c["d"] > 256 * R.vn(dt) for c in s if c["dt"] == dt} == {True, False} and any(c["ld"] > c["d"] for c in s if c["dt"] == dt)
    b = R.BY_ID["scatter-f32-rows200-d8-ldx0-n600-b256"]
    ok, pos, start, end = R.scatter_layout(b, R.scatter_inputs(b)["ids"])
    assert 256 in set(end) and 256 in set(start), "a run ends at sorted position 255 and the next starts at 256"
    sp = R.BY_ID["scatter-f32-rows200-d4-ldx0-n834-span"]
    ok, pos, start, end = R.scatter_layout(sp, R.scatter_inputs(sp)["ids"])
    assert (200, 801) in set(zip(start, end))
    oc = R.BY_ID["scatter-f32-rows200-d8-ldx0-n320-oob_cross"]
    ok, pos, start, end = R.scatter_layout(oc, R.scatter_inputs(oc)["ids"])
    assert pos[~ok].min() < 256 <= pos[~ok].max()
    # assembly
    a = R.cases("assemble")
    assert {c["L"] for c in a} >= {1, 31, 32, 33, 300, 600, R.RLA_MAX_L}
    assert {(c["tdt"], c["dt"]) for c in a} == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")}
    assert {c["d"] for c in a if not c["bwd"]} >= {1, 40, 64, 65} and {(c["dt"], c["d"]) for c in a if c["bwd"]} >= {("f32", 4), ("f32", 64), ("bf16", 8), ("bf16", 64)}
    assert any(not c["vis"] for c in a) and any(not c["labels"] for c in a)
    # cross-entropy: vec_ok, _fwd_bwd_supported (the issue's predicate), vectors per thread 1 and 2 and 17
    ce = R.cases("ce")
    for dt in ("f32", "bf16"):
        v = R.vn(dt)
        mine = [c for c in ce if c["dt"] == dt]
        assert {R.ce_vec_ok(c) for c in mine} == {True, False} and any(c["off"] for c in mine)
        sup = {(c["ld"], R.ce_supported(dt, c["V"], c["ld"])) for c in mine}
        assert (256 * v * 17, True) in sup and (256 * v * 17 + v, False) in sup
        for c in mine:
            assert R.ce_supported(dt, c["V"], c["ld"]) == (not (c["ld"] % v != 0 or c["ld"] > 256 * v * 17))
        assert {-(-c["V"] // (256 * v)) for c in mine if R.ce_vec_ok(c)} >= {1, 2, 17}
        assert any(c["V"] % v and c["V"] > v for c in mine) and any(c["V"] == c["ld"] for c in mine) and any(c["V"] == 1 for c in mine)
    assert any(c["ld"] % 4 for c in ce if c["dt"] == "f32") and {c["T"] for c in ce} >= {1, 1024, 1025}
    assert {c["pad"] for c in ce if c["ld"] > c["V"]} == {"inf", "nan", "big"} and {c["gscale"] for c in ce} == {1.0, 0.5, 2.0 ** -10}
    # the sweep: chunks and raggedness, fused or the pair, beta
    plans = {c["id"]: R.sweep_plan(c) for c in R.cases("sweep")}
    assert {(p[1] > 1, p[2], p[3]) for p in plans.values()} >= {(True, True, True), (False, False, True), (True, True, False), (True, False, True)}
    sw = R.cases("sweep")
    assert any(c["chunk"] == c["T"] for c in sw) and any(c["chunk"] > c["T"] for c in sw) and any(c["chunk"] == 0 for c in sw) and any(c["chunk"] == 1 for c in sw)
    assert any(c["T"] == 1 for c in sw) and {c["beta"] for c in sw if R.sweep_plan(c)[1] > 1} == {0, 1} and any(c["mask0"] for c in sw)
