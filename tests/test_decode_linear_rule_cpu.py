"""The rule of tests/decode_linear_rule.py proved usable without a GPU, per case: the exactness headroom of the integer designs, the range
condition of the GEGLU gates, the fp32 transcription within HALF of every bound (bit-equal where the bound is zero), every applicable
mutant of the reference detected -- changed bits in the exact designs, ten bounds in the bounded ones -- and every mutant applicable
somewhere.  The dispatcher arithmetic the rule transcribes is compared with the library's own queries (no GPU needed for those)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decode_linear_rule as R  # noqa: E402
import gemm_probe as G  # noqa: E402
import stream_rule as S  # noqa: E402

CHEAP = [c for c in R.CASES if R.cheap(c)]
IDS = [c["id"] for c in CHEAP]


def run(case, share=1.0):
    inp = R.inputs(case)
    got = R.model(case, inp)
    S.SHARE = share
    try:
        return inp, got, R.expect(case, inp, got)
    finally:
        S.SHARE = 1.0


def test_the_table_reaches_every_branch():
    plain = R.cases("plain")
    assert {c["M"] for c in plain} == set(R.PLAIN_M) and {(c["N"], c["K"]) for c in plain} == set(R.PLAIN_NK)
    assert {c["bias"] for c in plain} == set(R.BIASES)
    # wave shares of the plain shapes: (1, 0, 0, 0), ..., (2, 2, 1, 0), a share of 3, a share of 9
    shares = {(N, K): tuple(max(0, R.wave_steps(dict(kind="plain", N=N, K=K), 0, w)[1] - R.wave_steps(dict(kind="plain", N=N, K=K), 0, w)[0]) for w in range(4))
              for N, K in R.PLAIN_NK}
    assert shares[(16, 64)] == (1, 0, 0, 0) and shares[(48, 320)] == (2, 2, 1, 0) and shares[(32, 576)] == (3, 3, 3, 0) and shares[(16, 2112)][0] == 9
    for N, K, s in R.SPLIT_NK:
        assert R.split(N, K) == s and R.split(N, K, never=True) == 1 and (R.workspace_bytes(1, N, K) > 0) == (s > 1)
    assert all(N * K * 2 <= 4 << 20 or (N, K) == (4096, 4096) for c in R.CASES for N, K in [(c["N"] * (2 if c.get("geglu") else 1), c["K"])])
    pre = [c for c in R.CASES if c.get("pre")]
    assert {R.pre_rows(c["M"]) for c in pre} == {1, 4, 16} and {c["K"] for c in pre} >= {256, 512, 1792, 2048}
    assert {c["pdt"] for c in pre} == {"bf16", "f32"} == {c["pdt"] for c in R.CASES if c.get("tail")}
    assert {c["N"] for c in R.CASES if c.get("tail")} == {512, 1024, 2048}
    assert any(c.get("tail") and R.geometry(c)[0] > 1 for c in R.CASES) and any(c.get("tail") and c.get("geglu") for c in R.CASES)
    assert any(c.get("tail") and c.get("pre") for c in R.CASES)
    merge = R.cases("merge")
    assert {(c["B"], c["q"]) for c in merge} == set(R.MERGE_BQ) and {c["nunit"] for c in merge} == {1, 2, 11, 12} and {c["H"] for c in merge} == {2, 16}
    for c in R.CASES:
        if c["kind"] == "merge":
            assert R.attn_supported(c["B"], c["q"], c["H"], 128, c["nunit"], c["N"]), c["id"]
        else:
            assert R.supported(c["M"], c["N"], c["K"], c.get("geglu", False), c.get("tail", False), c.get("pre", False)), c["id"]
    assert {R.instantiation(c) for c in R.CASES} == R.all_instantiations()          # no template instantiation of the dispatchers is left out
    for _, a in R.REFUSALS:
        assert not R.supported(**a)
    for _, a in R.ATTN_REFUSALS:
        assert not R.attn_supported(**a)


def test_dispatcher_arithmetic_is_the_librarys():
    lib = pytest.importorskip("bdm_db1_amd.lib")
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("the library is not built")
    L = lib.load()
    shapes = [(c["M"], c["N"], c["K"], int(c.get("geglu", False)), int(c.get("tail", False)) | 2 * int(c.get("pre", False))) for c in R.CASES if c["kind"] != "merge"]
    shapes += [(a["M"], a["N"], a["K"], int(a.get("geglu", False)), int(a.get("tail", False)) | 2 * int(a.get("pre", False))) for _, a in R.REFUSALS]
    for M, N, K, g, ln in sorted(set(shapes)):
        assert bool(L.db1_linear_decode_supported(M, N, K, g, ln)) == R.supported(M, N, K, bool(g), bool(ln & 1), bool(ln & 2)), (M, N, K, g, ln)
        if R.supported(M, N, K, bool(g)):
            assert int(L.db1_linear_decode_workspace_bytes(M, N, K, g)) == R.workspace_bytes(M, N, K, bool(g)), (M, N, K, g)
    for a in [dict(B=c["B"], q=c["q"], H=c["H"], D=128, nunit=c["nunit"], N=c["N"]) for c in R.cases("merge")] + [a for _, a in R.ATTN_REFUSALS]:
        assert bool(L.db1_linear_decode_attn_supported(a["B"], a["q"], a["H"], a["D"], a["nunit"], a["N"])) == R.attn_supported(**a), a
    assert int(L.db1_linear_decode_tickets_bytes()) == 4 * R.TICKETS


def test_exactness_headroom_up_to_k_16384():
    for design in ("dense", "bounded"):
        for K in (64, 2112, 4096, 8192, 16384):
            for with_bias in (False, True):
                b = G.check(design, 64, 4096, K, 1.0, 0.0, with_bias)
                assert b < 2 ** 23 and (design == "dense" or b <= 96)
    # the geglu design: 8 z is an integer of magnitude <= 32 * 2 + 16 = 80 < 256: z is exact in fp32 and a bf16 value
    assert 32 * 2 + 16 < 256
    # the merge design: integers in [-4, 4] through 32 nonzeros of +-1: |y| <= 128, a bf16 value
    assert 32 * 4 <= 256


@pytest.mark.parametrize("case", [c for c in CHEAP if c.get("geglu")], ids=[c["id"] for c in CHEAP if c.get("geglu")])
def test_geglu_gates_stay_in_range(case):
    inp, got, exp = run(case)
    x = got["pre_out"] if case.get("pre") else inp["x"]
    z = R._d(x) @ R._d(inp["W"]).T + (0.0 if inp["bias"] is None else R._d(inp["bias"]))
    inside, neg, pos = R.gate_condition(z, case["N"])
    assert inside >= 0.9 and neg >= 0.1 and pos >= 0.1, (inside, neg, pos)
    if not case.get("pre"):
        assert np.array_equal(R.geglu_z(case, inp).astype(np.float64), z)


@pytest.mark.parametrize("case", CHEAP, ids=IDS)
def test_transcription_within_half_of_every_bound(case):
    inp, got, exp = run(case, share=R.HALF)
    assert set(exp) == set(got)
    for name, (ref, bnd) in exp.items():
        S.check(got[name], ref, bnd, f"{case['id']} {name} (fp32 allowance x {R.HALF})")
        # an element the kernel never wrote keeps NaN, which check() refuses; a reference is always finite
        assert np.isfinite(ref).all() and np.isfinite(bnd).all()
    if case["kind"] in ("plain", "split") or (case["kind"] == "merge" and case["others"] != "gauss"):
        assert not exp["y"][1].any()                       # expected bits


def _separation(ref, bnd, mref):
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(mref - ref)
        q = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isnan(q), np.inf, q).max())


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_applicable_mutant_is_detected(mutant):
    n, weakest = 0, (np.inf, None)
    for case in CHEAP:
        if not R.applies(mutant, case):
            continue
        inp, got, exp = run(case)
        mexp = R.expect(case, inp, got, mutant)
        sep = max(_separation(exp[name][0], exp[name][1], mexp[name][0]) for name in exp)
        # ten bounds where there is a bound; where the bound is zero any change of the expected bits is infinitely many
        assert sep > R.TEN, f"{mutant} at {case['id']}: the mutant moves no element by more than {sep:.2f} bounds"
        n += 1
        if sep < weakest[0]:
            weakest = (sep, case["id"])
    assert n > 0, f"{mutant} applies to no case"
    print(f"{mutant}: detected at {n} cases, weakest separation {weakest[0]:.1f} bounds at {weakest[1]}")


def test_inapplicable_mutants_change_nothing_where_that_is_claimed():
    """the explicit exclusions of R.applies that are structural (not a matter of magnitude): the mutated reference IS the reference there"""
    for mutant, pick in (("x_row0", lambda c: c["kind"] == "plain" and c["M"] == 1), ("out_tile0", lambda c: c["kind"] == "plain" and c["M"] == 16),
                         ("drop_slice", lambda c: c["kind"] == "split" and R.geometry(c)[0] == 1 and R.cheap(c)),
                         ("wrong_q", lambda c: c["kind"] == "merge" and c["M"] == 1), ("unit_plus", lambda c: c["kind"] == "merge" and c["nunit"] == 1),
                         ("dead_counted", lambda c: c["kind"] == "merge" and c["others"] == "low")):
        case = next(c for c in R.CASES if pick(c))
        assert not R.applies(mutant, case)
        inp, got, exp = run(case)
        if mutant == "out_tile0":
            continue                                        # (no row 16 exists)
        mexp = R.expect(case, inp, got, mutant)
        assert all(np.array_equal(mexp[k][0], exp[k][0]) for k in exp), (mutant, case["id"])


# ------------------------------------------------------------------------------------------------ the persistent chain
@pytest.fixture(scope="module")
def chain_w():
    return R.chain_weights()


@pytest.mark.parametrize("nunit,others", [(1, "dead"), (9, "dead"), (10, "low"), (12, "low")])
def test_chain_transcription_and_mutants(chain_w, nunit, others):
    case, part = R.chain_part(nunit, others)
    got = R.chain_model(chain_w, case, part)
    S.SHARE = R.HALF
    try:
        exp = R.chain_expect(chain_w, case, part, got)
    finally:
        S.SHARE = 1.0
    assert set(exp) == set(got)
    for name, (ref, bnd) in exp.items():
        q = S.check(got[name], ref, bnd, f"chain {name} (fp32 allowance x {R.HALF})")
        print(f"chain nunit {nunit} {name}: transcription max ratio {q:.3f}")
    assert not exp["y_o"][1].any()
    z = R._d(got["h1"]) @ R._d(chain_w["w1"]).T + R._d(chain_w["b1"])
    inside, neg, pos = R.gate_condition(z, R.CHAIN_DFF)
    assert inside >= 0.9 and neg >= 0.1 and pos >= 0.1
    exp = R.chain_expect(chain_w, case, part, got)
    # the merge mutants move the exact y_o row; a row of W lost or doubled moves its stage by ten bounds
    for mutant in R.MERGE_MUTANTS:
        if R.applies(mutant, case):
            merged = R.merged_rows(case, dict(part=part), mutant)
            assert not np.array_equal(merged @ R._d(chain_w["w_o"]).T, exp["y_o"][0]), mutant
    for stage, src, wname in (("f", "act", "w2"), ("qkv_next", "x_next", "w_qkv")):
        ref, bnd = exp[stage]
        x, W = R._d(got[src]), R._d(chain_w[wname])
        last_piece = slice(W.shape[1] - 512, W.shape[1])                            # the lane-pieces j = NL - 1 of every row
        moved = np.abs(x[:, last_piece] @ W[:, last_piece].T)
        assert (moved > R.TEN * bnd).mean() > 0.5, stage
