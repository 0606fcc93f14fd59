"""The attention probes (tests/attn_probe.py) on the CPU: the closed form is the oracle's, the tolerance is derived from the rounded model, and
every applicable mutant of the closed form moves the result by at least 10 tolerances in every case the GPU test runs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_probe as A  # noqa: E402
from oracle import db1_oracle as O  # noqa: E402

MARGIN = 10.0


@pytest.mark.parametrize("q,mlen,shift,nd", [(48, 0, 48, 48), (40, 0, 13, 40), (9, 30, 17, 39), (33, 20, 53, 53), (5, 11, 1, 12)])   # (the last: nd < klen, the clamp on masked pairs only)
def test_closed_form_is_the_oracles(q, mlen, shift, nd):
    rng = np.random.default_rng(q + mlen)
    klen = mlen + q
    p = dict(q=rng.standard_normal((2, q, 3, 16)), k=rng.standard_normal((2, klen, 3, 16)), v=rng.standard_normal((2, klen, 3, 16)),
             R=rng.standard_normal((nd, 3, 16)), u=rng.standard_normal((3, 16)), vb=rng.standard_normal((3, 16)), mlen=mlen, shift=shift, scale=0.25)
    dout = rng.standard_normal((2, q, 3, 16))
    got = A.reference(p, dout)
    vis, _ = A.geometry(q, klen, mlen, shift, nd)
    out, cache = O.relattn_core_fwd(p["q"], p["k"], p["v"], p["R"], p["u"], p["vb"], (~vis).astype(np.uint8), p["scale"], mlen=mlen)
    want = dict(zip(("dq", "dk", "dv", "dR", "du", "dv_bias"), O.relattn_core_bwd(dout, p["q"], p["k"], p["v"], p["R"], p["u"], p["vb"], p["scale"], cache)))
    want["out"] = out
    for n, w in want.items():
        assert np.abs(got[n] - w).max() <= 1e-10 * max(1.0, np.abs(w).max()), n
    assert np.abs(got["delta"] - np.einsum("bihd,bihd->bhi", out, dout)).max() < 1e-10
    # lse against the definition
    qu, qv = p["q"] + p["u"], p["q"] + p["vb"]
    i, j = np.arange(q)[:, None], np.arange(klen)[None, :]
    S = (np.einsum("bihd,bjhd->bhij", qu, p["k"]) + np.einsum("bihd,bijhd->bhij", qv, p["R"][np.clip(mlen + i - j, 0, nd - 1)][None])) * p["scale"]
    assert np.abs(got["lse"] - np.log(np.where(vis, np.exp(S), 0.0).sum(-1))).max() < 1e-10


def test_bf16_rounding_and_last_places():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3, 255.5, 3.0e-5])
    assert np.array_equal(A.bf16(x)[:3], [1.0, 1.0, 1.0 + 2.0 ** -6])          # ties to even
    assert np.all(np.abs(A.bf16(x) - x) <= np.abs(x) * 2.0 ** -8)         # half a last place
    assert A.ulp(1.0, 8) == 2.0 ** -7 and A.ulp(0.99, 8) == 2.0 ** -8 and A.ulp(20.0, 24) == 2.0 ** -19


def expected_applicable(q, mlen, shift, nd):
    """the mask mutants that change some pair of this geometry, worked out row by row in plain arithmetic, independently of mutate_geometry /
    changed_pairs: a later edit there that silently makes a mutant inapplicable fails the tests below instead of passing them vacuously"""
    klen = mlen + q
    nd = klen if nd is None else nd
    want = set()
    for i in range(q):
        hi = i + mlen                                   # the diagonal key; the oldest visible key is max(0, i - shift + 1)
        old = max(0, i - shift + 1)
        want.add("hi-1")                                # the diagonal key goes
        if hi + 1 < klen:
            want.add("hi+1")                            # one future key comes in
        if i - shift + 1 >= 0:
            want.add("lo+1")                            # the oldest key of the window goes
            if (i - shift + 1) % 32 == 31:
                want.add("skip_last")                   # ... and it is the last key of its 32-key block
        if i - shift >= 0:
            want.add("lo-1")                            # the key one past the old edge comes in
        if hi % 32 == 0:
            want.add("skip_first")                      # the diagonal key is the first of its block
        if hi - old + 1 > 1:                            # several visible keys: the distances 0 .. hi - old show in the result
            want.update(("dist+1", "dist-1"))           # (distance 0 -> 1 needs nd > 1, true whenever klen > 1)
            if min(hi - old, nd - 1) >= 256:
                want.add("rring")
            if hi - old > nd - 1:
                want.add("noclamp")                     # a VISIBLE pair past R's last row: in no listed case
    return want


def _check(q, mlen, shift, nd, backward):
    p, dout = A.build(q, mlen, shift, nd)
    d = dout if backward else None
    ref, rnd = A.reference(p, d), A.reference(p, d, rounded=True)
    tol = A.tolerances(ref, rnd)
    assert 0 < tol["out"] < 0.04                     # a bf16 last place at 1 and a few of them for P: were it larger, the probe would hide errors
    seen = {}
    for name, (mut, ch) in A.mutants(p, d).items():
        sep = A.separation(ref, mut, ch, tol)
        seen[name] = sep
        assert sep["out"] >= MARGIN, (name, sep)
        if backward:
            assert max(sep["dq"], sep["dk"], sep["dv"]) >= MARGIN, (name, sep)
    assert set(seen) == expected_applicable(q, mlen, shift, nd)
    return seen, p, ref, tol


@pytest.mark.parametrize("L,shift", A.FLASH_FWD_CASES)
def test_flash_forward_probe_separates_every_mutant(L, shift):
    seen, _, _, _ = _check(L, 0, shift, None, False)
    assert {"hi+1", "hi-1"} <= set(seen)             # applicable at every length and shift
    if shift <= L:
        assert "lo+1" in seen
    if shift < L:
        assert "lo-1" in seen
    if shift + 31 <= L:
        assert "skip_last" in seen
    if shift > 1:
        assert {"dist+1", "dist-1"} <= set(seen)
    if L == 384 and shift > 257:
        assert "rring" in seen


@pytest.mark.parametrize("L", [L for L, s in A.FLASH_FWD_CASES if s == 1])
def test_one_key_windows_show_their_distance_in_lse(L):
    """shift = 1: the softmax over the diagonal key alone is 1 whatever its score, so out and every gradient are blind to the R row it reads
    (changed_pairs leaves such pairs out); lse is not, in every row, and the GPU test checks lse per element.  (distance - 1 clamps to the
    same row 0, so distance + 1 is the only such error there is.)"""
    p, _ = A.build(L, 0, 1)
    ref, rnd = A.reference(p), A.reference(p, rounded=True)
    tol = A.tolerances(ref, rnd)
    mut = A.reference(p, None, A.mutate_geometry("dist+1", L, L, 0, 1, L))
    assert np.array_equal(mut["out"], ref["out"])
    assert np.abs(mut["lse"] - ref["lse"]).min() >= MARGIN * tol["lse"]
    assert np.array_equal(A.reference(p, None, A.mutate_geometry("dist-1", L, L, 0, 1, L))["lse"], ref["lse"])


@pytest.mark.parametrize("L,shift", A.FLASH_BWD_CASES)
def test_flash_backward_probe_separates_every_mutant(L, shift):
    seen, _, _, _ = _check(L, 0, shift, None, True)
    assert {"lo+1", "hi+1", "hi-1", "skip_first"} <= set(seen)
    if shift > 1:
        assert {"dist+1", "dist-1"} <= set(seen)


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_decode_probe_separates_every_mutant(q, mlen, shift, nd):
    seen, p, ref, tol = _check(q, mlen, shift, nd, False)
    klen = mlen + q
    assert "hi-1" in seen and ("lo+1" in seen) == (shift <= q) and ("hi+1" in seen) == (q > 1)
    assert ("skip_first" in seen) == any((i + mlen) % 32 == 0 for i in range(q))
    if shift + mlen > 1 and klen > 1:
        assert {"dist+1", "dist-1"} <= set(seen)
    if nd is not None:       # nd < klen: only masked pairs reach the clamp, so the result does not depend on it
        assert nd < klen and "noclamp" not in seen
    # ---- the ring.  Two detections, asserted independently of each other:
    #   READ side   origin +-1 moves every memory row the kernel reads; wherever a memory key is visible the OUTPUT separates by the margin
    #               (a kernel that reads one row off and appends correctly leaves the ring image right: only the output can show it)
    #   APPEND side origin +-1, the wrap test and the unwrapped index put new rows elsewhere; the ring IMAGE differs, and the GPU test
    #               compares it bit for bit
    vis, _ = A.geometry(q, klen, mlen, shift, p["R"].shape[0])
    memory_visible = bool(vis[:, :mlen].any())
    assert memory_visible == (mlen > 0)                          # row 0 sees keys -shift < j <= mlen: all of the memory, whatever the shift
    read_checks = 0
    append_seen = set()
    guard = klen + 1
    for cap in A.ring_caps(q, mlen):
        origins = A.ring_origins(q, mlen, cap)
        for start in origins:
            ring0 = A.ring_initial(p, cap, start)
            want = A.ring_expected(p, ring0, start, guard=guard)
            seen_p, moved = A.ring_view(p, ring0, start, guard=guard)
            assert not moved.any() and np.array_equal(seen_p["k"], p["k"]) and np.array_equal(seen_p["v"], p["v"])     # the layout reads back
            new_rows = A.ring_rows(start, mlen, q, cap, append=True)
            untouched = np.ones(cap, bool)
            untouched[new_rows] = False
            assert np.array_equal(want[:, :cap][:, untouched], ring0[:, untouched]) and not want[:, cap:].any()
            assert np.array_equal(A.bf16(want), want)                                                                 # bit-equal is a fair demand
            for m in A.RING_MUTANTS:
                # read side
                mp, moved = A.ring_view(p, ring0, start, m, guard=guard)
                ch = vis & np.concatenate([moved, np.zeros(q, bool)])[None, :]
                if m in ("origin+1", "origin-1"):
                    assert moved.all() and ch.any() == memory_visible      # (cap >= klen > mlen: one row off is another row)
                    if ch.any():
                        sep = A.separation(ref, A.reference(mp), ch, tol)
                        assert sep["out"] >= MARGIN, (m, cap, start, sep)
                        read_checks += 1
                else:
                    assert not moved.any()                                  # errors of the append only
                # append side: applicable where the mutant writes other rows (row numbers, not contents, decide that)
                if m == "unwrapped_write":
                    rows_m = start + np.arange(mlen, klen)
                else:
                    rows_m = A.ring_rows(start, mlen, q, cap, m, append=True)
                if not np.array_equal(rows_m, new_rows):
                    append_seen.add((m, cap, start))
                    assert not np.array_equal(A.ring_expected(p, ring0, start, m, guard=guard), want), (m, cap, start)
        # which origins make each append error applicable, from the arithmetic of the wrap
        for start in origins:
            assert (("origin+1", cap, start) in append_seen) == (cap > 1) and (("origin-1", cap, start) in append_seen) == (cap > 1)
            assert (("unwrapped_write", cap, start) in append_seen) == (start + klen - 1 >= cap)                       # the last new row is past the end
            assert (("wrap_gt", cap, start) in append_seen) == (0 <= cap - start - mlen < q)                          # some new row lands ON row cap
        if klen > 1:
            assert any(("unwrapped_write", cap, s) in append_seen for s in origins)
        if cap == klen and cap > 1:
            assert any(("wrap_gt", cap, s) in append_seen for s in origins)
    assert read_checks == (2 * sum(len(A.ring_origins(q, mlen, c)) for c in A.ring_caps(q, mlen)) if memory_visible else 0)


# The chain test (tests/test_dqr_probe_gpu.py) checks the dq that the kernels finish, bf16(dq_k + dq_r): one more rounding point than the numpy
# assembly, so its tolerance comes from reference(rounded=True, round_dq=True).  Every applicable mutant must still move dq by MARGIN of THOSE
# tolerances -- except the pairs listed here, which are findings, not allowances: the chain's dq check does not show them with the margin, and
# what does is asserted instead.
#   shift = 1: a row sees one key, dS = 0 and dq is zero whatever the mask does (tolerance 0, separation 0): dk / dv carry these mutants.
#   (128, 128) lo+1: only the last row loses a key; 7.4 chain tolerances in dq (10.7 of the assembled dq's, which test_flash_backward_probe keeps
#   checking), so for this one mutant the chain is the weaker of the two dq checks.
DQ_BELOW_MARGIN = {(L, 1): {"lo+1", "hi-1", "skip_last", "skip_first"} for L in A.FLASH_LENGTHS}
DQ_BELOW_MARGIN[(128, 128)] = {"lo+1"}


@pytest.mark.parametrize("L,shift", [c for c in A.FLASH_BWD_CASES if c[0] % 128 == 0])
def test_chain_dq_tolerance_separates_every_mutant(L, shift):
    p, dout = A.build(L, 0, shift)
    ref = A.reference(p, dout)
    tol = A.tolerances(ref, A.reference(p, dout, rounded=True))
    chain = A.tolerances(ref, A.reference(p, dout, rounded=True, round_dq=True))
    assert chain["dq"] <= 1.5 * tol["dq"] and all(chain[k] == tol[k] for k in tol if k != "dq")      # one more half last place, nothing else
    below = set()
    for name, (mut, ch) in A.mutants(p, dout).items():
        sep, old = A.separation(ref, mut, ch, chain), A.separation(ref, mut, ch, tol)
        print(f"chain {(L, shift)} {name}: dq moves by {sep['dq']:.1f} chain tolerances ({old['dq']:.1f} of the assembled dq's)")
        if sep["dq"] < MARGIN:
            below.add(name)
            assert max(old["dq"], old["dk"], old["dv"]) >= MARGIN, (name, old)           # what test_flash_backward_probe checks still shows it
    assert below == DQ_BELOW_MARGIN.get((L, shift), set()), below


def test_round_dq_is_off_by_default():
    p, dout = A.build(128, 0, 33)
    a, b, c = A.reference(p, dout, rounded=True), A.reference(p, dout, rounded=True, round_dq=False), A.reference(p, dout, rounded=True, round_dq=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(c["dq"], A.bf16(a["dq"])) and not np.array_equal(c["dq"], a["dq"]) and all(np.array_equal(a[k], c[k]) for k in a if k != "dq")
    assert np.array_equal(A.reference(p, dout, round_dq=True)["dq"], A.reference(p, dout)["dq"])      # (a rounding point of the rounded model only)
