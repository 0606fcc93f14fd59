"""tests/dqr_rule.py on the CPU: the closed form against a plain einsum, the restated stream geometry, and the proof that the probes of
tests/test_dqr_probe_gpu.py bite -- for every case the GPU test runs and every applicable mutant of the closed form,
  * index probe: every output row (b, i, h) the mutant touches differs IN BITS from the closed form.  An applicable mutant of the distance,
    row, batch / head / group and dropped-term groups touches every row (each row has its entries at dist 0, at the diagonal, in its last
    k-tile and at its own pseudo-random distance); dqk_row+4 touches every row of dq and no row of dq_r; the sums-only mutants (du_dv,
    item_missing) must change du and dv of every head;
  * dense probe: rounding at |x| > 256 can swallow a +-1, so the demand is one changed element of dq or of the sums; the count is printed.
    Heads are independent of each other (the heads mutant pairs h with h + 1), so the mutants are evaluated on the first four heads of the
    probe: an element that changes there changes in the whole probe.
Applicability (dqr_rule.applicable): dist+-s where s % L != 0 (dist+-128 changes nothing at L = 128), heads where H > 1, batches where B > 1,
groups where ng > 1, everything else always.  Every mutant is applicable in at least one case (asserted)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dqr_rule as Q  # noqa: E402


def test_closed_form_is_the_plain_contraction():
    rng = np.random.default_rng(5)
    H, B, L, ng = 3, 4, 256, 2
    i = np.arange(L)
    dT = rng.standard_normal((H, B, L, L)) * (i[None, :] <= i[:, None])
    R, dq_k = rng.standard_normal((ng, L, H, Q.D)), rng.standard_normal((B, L, H, Q.D))
    got = Q.closed_form(dict(dT=dT, R=R, dq_k=dq_k, ng=ng, acc0=Q.ACC0))
    want = np.concatenate([np.einsum("hbik,khd->bihd", dT[:, 2 * g:2 * g + 2], R[g]) for g in range(ng)], 0)
    assert np.abs(got["dq_r"] - want).max() < 1e-10
    assert np.array_equal(got["dq"], Q.bf16(dq_k + got["dq_r"]))
    assert np.abs(got["du"] - (3.0 + dq_k.sum((0, 1)).reshape(-1))).max() < 1e-9 and np.abs(got["dv"] - (-5.0 + want.sum((0, 1)).reshape(-1))).max() < 1e-9
    # poison changes nothing: the closed form reads what the kernel is allowed to read
    dT[:, :, Q.poison_mask(L)] = np.nan
    again = Q.closed_form(dict(dT=dT, R=R, dq_k=dq_k, ng=ng, acc0=Q.ACC0))
    assert np.array_equal(again["dq_r"], got["dq_r"])


def test_bf16_bits():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 257.0, 259.0, -183.0])
    assert np.array_equal(Q.bf16(x), [1.0, 1.0, 1.0 + 2.0 ** -6, 0.0, 256.0, 260.0, -183.0])
    assert Q.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0, 0x4380, 0x4382, -0x10000 + 0xC337]


@pytest.mark.parametrize("H,B,L,ng", Q.CASES)
def test_stream_geometry(H, B, L, ng):
    wph, NT = Q.wph(H), L // Q.ROWS
    assert wph % ng == 0 and B % ng == 0
    # the k-tiles an item reads cover every dist <= i of its rows, and the poison sits exactly on the rest
    pm = Q.poison_mask(L)
    for i0 in range(0, L, Q.ROWS):
        tiles = set(Q.read_ktiles(i0))
        assert tiles == set(range(max(tiles) + 1)) and max(tiles) * Q.KT <= i0 + Q.ROWS - 1 < (max(tiles) + 1) * Q.KT
        for i in range(i0, i0 + Q.ROWS):
            assert {d // Q.KT for d in (0, i)} <= tiles
            assert np.array_equal(pm[i], ~np.isin(np.arange(L) // Q.KT, list(tiles)))
    assert not pm[np.arange(L)[None, :] <= np.arange(L)[:, None]].any()
    # the workgroups of a head partition the items of their group; idle exactly where jj >= n_items
    seen = []
    for j in range(wph):
        grp, items = Q.workgroup(j, H, B, L, ng)
        assert grp == j % ng and all(b // (B // ng) == grp for b, _ in items)
        assert (len(items) == 0) == Q.idle(j, H, B, L, ng) == (j // ng >= Q.n_items(B, L, ng))
        seen += items
    assert len(seen) == len(set(seen)) == B * NT and set(seen) == {(b, t * Q.ROWS) for b in range(B) for t in range(NT)}
    assert sum(Q.idle(j, H, B, L, ng) for j in range(wph)) == max(0, wph - ng * Q.n_items(B, L, ng))


def test_case_list_reaches_its_branches():
    idle = {c: sum(Q.idle(j, *c) for j in range(Q.wph(c[0]))) for c in Q.CASES}
    assert idle[(1, 1, 128, 1)] == 254 and Q.wph(3) == 85 and Q.wph(256) == 1
    assert max(Q.read_ktiles(1024 - 64)) == 7
    assert len(Q.workgroup(0, 64, 1, 384, 1)[1]) == 2 and Q.n_items(1, 384) == 6 > Q.wph(64) == 4
    assert Q.wph(16) // 16 == 1 and Q.n_items(4, 256, 2) == 8 > Q.wph(64) // 2


@functools.lru_cache(maxsize=4)
def _probe(kind, H, B, L, ng):
    pr = (Q.build_index if kind == "index" else Q.build_dense)(H, B, L, ng, poison=True)
    return pr, Q.closed_form(pr)


@pytest.mark.parametrize("H,B,L,ng", Q.CASES)
def test_index_probe_is_exact_and_covers_every_position(H, B, L, ng):
    pr, ref = _probe("index", H, B, L, ng)
    assert Q.index_is_exact(ref) and np.isfinite(ref["dq"]).all()
    dT = np.where(Q.poison_mask(L), 0.0, pr["dT"])
    nz = dT != 0
    assert 1 <= nz.sum(-1).min() and nz.sum(-1).max() <= 4
    i = np.arange(L)
    assert not nz[:, :, i[None, :] > i[:, None]].any()
    assert nz[:, :, i, 0].all() and nz[:, :, i, i].all()                           # dist 0 and the diagonal, in every row
    dist = np.nonzero(nz.any((0, 1)))
    assert set(dist[1] // Q.KT) == set(range(L // Q.KT)) and set(dist[1] % Q.KT // 8) == set(range(16)) and set(dist[0] % 16) == set(range(16))
    pos = Q.index_positions(H, B, L)
    assert (pos[..., 2] // Q.KT == (i // Q.KT)).all()                            # one entry in the row's last k-tile
    if H * B > 1:                                                                  # the fourth entry's place differs per (h, b)
        assert (pos[..., 3].reshape(H * B, L)[0] != pos[..., 3].reshape(H * B, L)[1]).any()
    # R and dq_k differ in every index
    R, dq_k = pr["R"], pr["dq_k"]
    assert (R[:, 1:] != R[:, :-1]).any(-1).all() and (R[..., 1:] != R[..., :-1]).any(-1).all() and (dq_k[:, 1:] != dq_k[:, :-1]).all()
    assert H == 1 or (R[:, :, 1:] != R[:, :, :-1]).any(-1).all()
    assert ng == 1 or (R[1:] != R[:-1]).any(-1).all()


@pytest.mark.parametrize("kind", ["index", "dense"])
@pytest.mark.parametrize("H,B,L,ng", Q.CASES)
def test_every_applicable_mutant_shows(H, B, L, ng, kind):
    pr, ref = _probe(kind, H, B, L, ng)
    if kind == "dense" and H > 4:
        H = 4
        pr = dict(pr, dT=pr["dT"][:H], R=pr["R"][:, :, :H], dq_k=pr["dq_k"][:, :, :H])
        ref = Q.closed_form(pr)
    for m in Q.MUTANTS:
        if not Q.applicable(m, H, B, L, ng):
            continue
        mut = Q.closed_form(pr, m, base=ref)
        if kind == "dense":
            n = int((mut["dq"] != ref["dq"]).sum()) + int((mut["du"] != ref["du"]).sum()) + int((mut["dv"] != ref["dv"]).sum())
            print(f"dqr dense {(H, B, L, ng)} {m}: {n} elements of dq / du / dv change")
            assert n > 0, m
            continue
        sums_differ = (mut["du"] != ref["du"]).reshape(H, Q.D).any(1) | (mut["dv"] != ref["dv"]).reshape(H, Q.D).any(1)
        dq_rows = (mut["dq"] != ref["dq"]).any(-1)                                 # [B, L, H]; dq is what bf16 stores: other value, other bits
        dqr_rows = (Q.bf16(mut["dq_r"]) != ref["dq_r"]).any(-1)
        if m in Q.SUMS_ONLY:
            assert not dq_rows.any() and (mut["du"] != ref["du"]).reshape(H, Q.D).any(1).all() and (mut["dv"] != ref["dv"]).reshape(H, Q.D).any(1).all(), m
        elif m == "dqk_row+4":
            assert dq_rows.all() and not dqr_rows.any(), m
        else:
            assert dq_rows.all() and dqr_rows.all(), (m, int((~dq_rows).sum()), int((~dqr_rows).sum()), np.argwhere(~(dq_rows & dqr_rows))[:4].tolist())
            assert sums_differ.all() or m.startswith("row") or m == "batches", m  # (row shifts and the batch swap permute the rows of dq_r: its column sums stay)


def test_every_mutant_is_applicable_somewhere():
    counts = {m: sum(Q.applicable(m, *c) for c in Q.CASES) for m in Q.MUTANTS}
    print("dqr mutants, cases where each applies:", counts)
    assert all(n >= 1 for n in counts.values()), counts
    assert counts["dist+128"] == sum(c[2] > 128 for c in Q.CASES) and counts["groups"] == sum(c[3] > 1 for c in Q.CASES)
