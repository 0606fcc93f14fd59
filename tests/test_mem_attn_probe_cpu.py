"""The attention probes (tests/attn_probe.py) at the geometries of db1_relattn_mem_fwd (tests/mem_attn_cases.py), on the CPU: what
tests/test_attn_probe_cpu.py::_check asserts for the other kernels' cases -- the tolerance derived from the rounded model is small, every
applicable mutant of the closed form moves ``out`` by at least ten tolerances, and the applicable mutants are the expected ones."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_probe as A  # noqa: E402
import test_attn_probe_cpu as TP  # noqa: E402
from mem_attn_cases import MEM_CASES, ONE_KEY_CASE  # noqa: E402


@pytest.mark.parametrize("q,mlen,shift,nd", MEM_CASES)
def test_mem_probe_separates_every_mutant(q, mlen, shift, nd):
    seen, p, ref, tol = TP._check(q, mlen, shift, nd, False)
    assert "hi-1" in seen and ("hi+1" in seen) == (q > 1) and ("lo+1" in seen) == (shift <= q)
    if shift + mlen > 1:
        assert {"dist+1", "dist-1"} <= set(seen)
    if nd is not None:       # nd < klen: only masked pairs reach the clamp
        assert nd < mlen + q and "noclamp" not in seen
    print(f"mem probe {(q, mlen, shift, nd)}: tol(out) {tol['out']:.3e}, smallest separation {min(s['out'] for s in seen.values()):.1f} tolerances")


def test_case_list_covers_what_it_claims():
    qs, shifts, mlens = {c[0] for c in MEM_CASES}, {c[2] for c in MEM_CASES}, {c[1] for c in MEM_CASES}
    assert len(MEM_CASES) == 19 and len(set(MEM_CASES)) == 19
    assert {65, 129, 130, 200, 1} <= qs and any(q > 128 for q in qs) and any(q % 16 for q in qs)
    assert {0, 1, 32, 33} <= shifts and {31, 32, 33, 127, 128, 129} <= mlens
    assert all(s + m >= 1 for _, m, s, _ in MEM_CASES)                                # every row sees a key
    assert any(nd is not None and nd < q + m for q, m, _, nd in MEM_CASES)
    assert any(min(s + m, q + m) - 1 >= 256 for q, m, s, _ in MEM_CASES)               # visible distances past 256


def test_one_key_windows_show_their_distance_in_lse():
    """(64, 1, 0): each row sees key i + 1 alone, the softmax over it is 1 whatever its score, so ``out`` cannot show the R row it reads;
    lse can, in every row, and the device test checks lse per element"""
    q, mlen, shift, nd = ONE_KEY_CASE
    p, _ = A.build(q, mlen, shift, nd)
    ref, rnd = A.reference(p), A.reference(p, rounded=True)
    tol = A.tolerances(ref, rnd)
    vis, _ = A.geometry(q, mlen + q, mlen, shift, mlen + q)
    assert (vis.sum(1) == 1).all()
    mut = A.reference(p, None, A.mutate_geometry("dist+1", q, mlen + q, mlen, shift, mlen + q))
    assert np.array_equal(mut["out"], ref["out"])
    moved = np.abs(mut["lse"] - ref["lse"]).min()
    print(f"dist+1 moves every lse by at least {moved / tol['lse']:.3g} tolerances (tol {tol['lse']:.3e})")
    assert moved >= TP.MARGIN * tol["lse"]
