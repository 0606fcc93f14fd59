"""The rule of tests/stream_rule.py proved usable without a GPU: the fp32 model of every kernel stays under half of every bound against the
float64 reference, every one-mistake mutant of the model breaks a bound in a named case, and no output can hide an unwritten element."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stream_rule as S  # noqa: E402

EXACT_OPS = ("add", "add2d", "cast")
MODELLED = [c for c in S.CASES if S.cheap(c) and c["op"] not in EXACT_OPS]
HEADROOM = 0.5          # the device adds in another order than the model in places: the model may use half of the fp32 allowance

MUTANT_OPS = {
    "drop_last_row": ("ln_bwd", "colsum", "act_bwd_bias"),
    "tail_reads_past": ("ln_bwd",),
    "last_colvec_unwritten": ("act_fwd", "act_bwd", "act_bwd_bias"),
    "geglu_half_at_c": ("act_bwd", "act_bwd_bias"),
    "swap_dgdb_group": ("ln_bwd",),
    "stale_waves": ("ln_bwd", "act_bwd_bias", "colsum"),
    "acc_assign": ("ln_bwd", "act_bwd_bias", "colsum", "sumsq_acc", "adam"),
    "skip_tail": ("sumsq_acc", "sumsq_det"),
    "swap_bf16_pair": ("adam",),
    "gscale_once": ("adam",),
    "no_s_round": ("ln_fwd",),
}


def run(case, mutant=None, share=1.0):
    inp = S.inputs(case)
    got = S.model(case, inp, mutant)
    S.SHARE = share
    try:
        return got, S.expect(case, inp, got)
    finally:
        S.SHARE = 1.0


def test_half_ulp_is_the_formats_not_a_flat_fraction():
    x = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -20)
    r = S.bf16(x)
    assert float(r) == 1.0 + 2.0 ** -7                                        # nearest bf16
    err = abs(float(r) - float(x))
    assert err > 2.0 ** -9 * float(x)                                         # a flat 2^-9 |ref| refuses correct rounding
    assert err <= float(S.half_ulp(float(x), "bf16")) == 2.0 ** -8
    assert float(S.half_ulp(1.0, "f32")) == 2.0 ** -24 and float(S.half_ulp(0.99, "f32")) == 2.0 ** -25 and float(S.half_ulp(0.0, "f32")) == 0.0
    v = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 3
    assert np.all(np.abs(S.bf16(v).astype(np.float64) - v) <= S.half_ulp(v, "bf16"))
    import torch
    assert np.array_equal(S.bf16(v), torch.from_numpy(v).to(torch.bfloat16).float().numpy())
    assert np.array_equal(S.bf16(S.SPECIALS), S.SPECIALS[:2].tolist() + S.bf16(S.SPECIALS[2:4]).tolist() + S.SPECIALS[4:].tolist())


def test_check_reports_and_refuses():
    ref, b = np.zeros((3, 4)), np.full((3, 4), 1e-3)
    got = ref.copy()
    assert S.check(got, ref, b, "ok") == 0.0
    got[2, 1], got[0, 0] = 5e-3, 2e-3
    with pytest.raises(AssertionError, match=r"2 of 12 elements over bound; worst at \(2, 1\).*excess 4.000e-03"):
        S.check(got, ref, b, "x")
    got = ref.copy()
    got[1, 1] = np.nan
    with pytest.raises(AssertionError, match="1 of 12"):
        S.check(got, ref, b, "nan")
    got[1, 1] = np.inf
    with pytest.raises(AssertionError):
        S.check(got, ref, b, "inf")
    with pytest.raises(AssertionError):
        S.check(np.full(2, 1e-9), np.zeros(2), np.zeros(2), "exact")
    with pytest.raises(AssertionError):
        S.check(np.zeros(5), np.zeros(4), np.zeros(4), "shape")


def test_every_bound_formula_has_a_cheap_case():
    ops = {c["op"] for c in S.CASES} - set(EXACT_OPS)
    assert ops == {c["op"] for c in MODELLED}
    have = {(c["op"], c.get("dt") or c.get("gdt")) for c in MODELLED}
    for op in ops:
        assert (op, "f32") in have and (op, "bf16") in have, op
    assert {S.colsum_path(c) for c in MODELLED if c["op"] == "colsum"} == {"scalar", "vec", "chunk"}
    assert {S.ln_fused(c["dt"], c["d"]) for c in MODELLED if c["op"] == "ln_bwd"} == {True, False}
    assert any(c.get("mode") == "parts" for c in MODELLED)


@pytest.mark.parametrize("case", MODELLED, ids=[c["id"] for c in MODELLED])
def test_model_within_half_of_every_bound(case):
    got, exp = run(case, share=HEADROOM)        # half of the fp32 allowance on top of the output rounding, which a correct result uses up in full
    for name, (ref, bnd) in exp.items():
        S.check(S.value(got, name), ref, bnd, f"{case['id']} {name} (fp32 allowance x {HEADROOM})")
        # an element the kernel never wrote keeps the sentinel: that must be a failure wherever it happens
        assert np.all(np.abs(np.asarray(ref, np.float64) - S.SENT) > bnd), f"{case['id']} {name}: a reference value within its bound of the sentinel"


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for case in MODELLED:
        if case["op"] not in MUTANT_OPS[mutant]:
            continue
        got, exp = run(case, mutant)
        for name, (ref, bnd) in exp.items():
            if S.ratio(S.value(got, name), ref, bnd).max() > 1.0:
                caught.append(f"{case['id']}:{name}")
                break
    print(f"{mutant}: caught by {len(caught)} cases, first {caught[:3]}")
    assert caught, f"no case of the table catches the mutant {mutant}"


def test_mutant_table_is_complete():
    assert set(MUTANT_OPS) == set(S.MUTANTS)


@pytest.mark.parametrize("case", S.cases(*EXACT_OPS), ids=[c["id"] for c in S.cases(*EXACT_OPS)])
def test_exact_ops_reference_is_torch(case):
    """add / add2d / cast are compared bit for bit with torch on the GPU; here: the table's inputs are representable and the NumPy statement of
    the same arithmetic (float32 sum, one rounding to the output type) gives torch's bits"""
    import torch
    inp = S.inputs(case)
    td = {"f32": torch.float32, "bf16": torch.bfloat16}
    a, b = torch.from_numpy(inp["a"]).to(td[case["adt"]]), torch.from_numpy(inp["b"]).to(td[case["dt"]])
    assert np.array_equal(a.float().numpy(), inp["a"]) and np.array_equal(b.float().numpy(), inp["b"])
    if case["op"] == "cast":
        assert np.array_equal(a.to(td[case["dt"]]).float().numpy(), S.rnd(inp["a"], case["dt"]))
    else:
        assert np.array_equal((a.float() + b.float()).to(td[case["dt"]]).float().numpy(), S.rnd(inp["a"] + inp["b"], case["dt"]))
