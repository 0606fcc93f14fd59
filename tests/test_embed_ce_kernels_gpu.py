"""The two ends of the training step -- token embedding (db1_embed_gather_fwd, db1_embed_scatter_add_bwd, db1_rl_assemble_fwd / _bwd), the
masked cross-entropy (db1_masked_ce_fwd / _bwd / _fwd_bwd) and the chunked head + loss sweep (db1_lmhead_ce_fwd / _fwd_bwd / _bwd) -- at every
dispatch branch and edge, through bdm_db1_amd.ops, under the rule of tests/embed_ce_rule.py (proved usable by test_embed_ce_rule_cpu.py).
Gather, scatter and assembly are compared BIT FOR BIT with the correctly rounded exact result of dyadic-grid probes; the cross-entropy and
the sweep per element against counted bounds.  Every output and accumulator lies in a Guarded allocation pre-filled with the sentinel: the
margins, and the columns between cols and ld, must come back untouched.

branch -> case id (the ids of embed_ce_rule.CASES; * = every value of the table)
  gather_kernel vector path (bf16 -> bf16, d, ld_out % 8 == 0, aligned)      gather-bf16-bf16-*-d8 / d512 / d520 / d2048 with ld = d and ld = d + 8
  gather_kernel scalar path: by d, by ld_out, by the output's / table's base  *-ld(d + 3), *-ld(d + 4), *-out_off4-*, *-tab_off4-*; four dtype pairs
  four tokens per workgroup                                                    n1, n4, n5, n13; ids 0, rows - 1, rows, -1, -100, 2^32, 2^40, 2^32 + 3
  radix sort: one / two / three 8-bit passes                                   scatter-*-rows200, rows255 / rows256, rows65535 / rows65536, rows65736
  64-lane steps, the 512-key tile, the 1024-entry scan block                   n1, n63, n64, n65, n511, n512, n513, n2049
  batches of sixteen; runs ending at 255 / starting at 256 / one boundary      *-edges, *-b256
  a head plus partial rows; one row only; out-of-table region over a boundary  *-span, *-one_row, *-oob_cross, *-all_oob
  column sweeps of the four waves; partial rows used or not                    d4, d1024, d1028 / d8, d2048, d2056; d8192 / d8200; ld_dout > d: *-ldx*
  rl_assemble_kernel: chunks of 32 tokens, the count in steps of 256           assemble-*-L1, L31, L32, L33, L300, L600, L12288 (12289: refused)
  ce_fwd_kernel / ce_bwd_kernel vector and scalar paths                        ce-*-off0-* with ld % VN == 0 / ce-*-ld1325, ce-*-off1-*
  ce_fwd_bwd_kernel: 1, 2, 17 pieces per thread; past the limit                ce-*-V1*, V(256 VN + 1), ld(256 VN 17) / ld(256 VN 17 + VN): unsupported
  ce_sum_kernel: one add per thread, a second for thread 0                     ce-*-T1, T1024, T1025
  lmhead_sweep: chunks, a ragged one, chunk >= T, the default, one row         sweep-*-chunk128 (T300), chunk40 / chunk64 / chunk0 (T40), T1, chunk1
  lmhead_sweep's fallback to the forward / backward pair                       sweep-f32-T40-V17409-rows17472-*"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stream_rule as S  # noqa: E402
import embed_ce_rule as R  # noqa: E402
from gpu_common import DEV, TD, Guarded, dev, host  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops as _ops, lib
    assert lib.load().db1_device_is_gfx950() == 1
    return _ops


def ids(cs):
    return [c["id"] for c in cs]


def idev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def body(g):
    """the whole [rows, ld] region of a Guarded allocation, the columns cols .. ld included"""
    return g.buf[g.start:g.start + g.rows * g.ld].view(g.rows, g.ld)


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(name, got, want, dt):
    w = dev(np.reshape(want, tuple(got.shape)), dt)
    if torch.equal(ibits(got), ibits(w)):
        return
    ne = (ibits(got) != ibits(w)).reshape(-1)
    first = int(ne.nonzero()[0])
    at = tuple(int(i) for i in np.unravel_index(first, tuple(got.shape)))
    raise AssertionError(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the expected bits; the first at {at}: "
                         f"got {float(got.reshape(-1)[first])!r} expected {float(w.reshape(-1)[first])!r}")


def intact(guards, cid):
    torch.cuda.synchronize()
    for name, g in guards.items():
        g.intact(f"{cid} {name}")


def checked(cid, got, exp):
    worst = {name: R.check(got[name], ref, bnd, f"{cid} {name}") for name, (ref, bnd) in exp.items()}
    print(cid, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    return worst


# ------------------------------------------------------------------------------------------------ gather
GATHER = R.cases("gather")


@pytest.mark.parametrize("case", GATHER, ids=ids(GATHER))
def test_gather_bit_exact(ops, case):
    inp = R.gather_inputs(case)
    want = R.gather_expected(case, inp)
    rows, d = inp["table"].shape
    flat = torch.zeros(rows * d + 8, device=DEV, dtype=TD[case["tdt"]])
    tab = flat[case["tab_off"]:case["tab_off"] + rows * d].view(rows, d)
    tab.copy_(dev(inp["table"], case["tdt"]))
    out = Guarded(case["n"], d, case["dt"], ld=case["ld"], off=case["out_off"])
    assert (tab.data_ptr() % 16 == 0) == (case["tab_off"] % 8 == 0 or case["tdt"] == "f32") and (out.t.data_ptr() % 16 == 0) == (case["out_off"] == 0)
    ops.embed_gather(tab, idev(inp["ids"]), out.t)
    intact(dict(out=out), case["id"])
    same_bits(f"{case['id']} out (pad columns included)", body(out), want, case["dt"])


# ------------------------------------------------------------------------------------------------ scatter
SCATTER = R.cases("scatter")


@pytest.mark.parametrize("case", SCATTER, ids=ids(SCATTER))
def test_scatter_add_bit_exact_or_within_its_bound(ops, case):
    inp = R.scatter_inputs(case)
    n, d, rows, dt = case["n"], case["d"], case["rows"], case["dt"]
    dout = dev(inp["dout"], dt)[:, :d]
    idd = idev(inp["ids"])
    outs = []
    for _ in range(2):                       # same inputs -> same bits
        acc = Guarded(rows, d, "f32", fill=inp["acc0"])
        ops.embed_scatter_add(dout, idd, acc.t)
        intact(dict(dtable=acc), case["id"])
        outs.append(acc.t.clone())
    assert torch.equal(ibits(outs[0]), ibits(outs[1])), f"{case['id']}: two runs on the same inputs differ"
    if case.get("gauss"):
        ref, bnd = R.scatter_bound(case, inp)
        checked(case["id"], dict(dtable=host(outs[0])), dict(dtable=(ref, bnd)))
    else:
        same_bits(f"{case['id']} dtable", outs[0], R.scatter_expected(case, inp), "f32")


# ------------------------------------------------------------------------------------------------ RL assembly
ASSEMBLE = R.cases("assemble")
LAB_SENT = -7777


@pytest.mark.parametrize("case", ASSEMBLE, ids=ids(ASSEMBLE))
def test_rl_assembly_bit_exact(ops, case):
    inp = R.assemble_inputs(case)
    want = R.assemble_expected(case, inp)
    B, L, d, dt, nvis = case["B"], case["L"], case["d"], case["dt"], inp["nvis"]
    word, pos = dev(inp["word"], case["tdt"]), dev(inp["pos"], case["tdt"])
    vis = dev(inp["vis"], dt) if case["vis"] else None
    idd, pid = idev(inp["ids"]), idev(inp["pid"])
    lbuf = torch.full((B * L + 128,), LAB_SENT, device=DEV, dtype=torch.int64)
    lab = lbuf[64:64 + B * L].view(B, L)
    lab.copy_(idev(inp["labels"]))
    out = Guarded(B * L, d, dt)
    ops.rl_assemble_fwd(word, pos, vis, idd, pid, lab if case["labels"] else None, out.t.view(B, L, d))
    intact(dict(out=out), case["id"])
    same_bits(f"{case['id']} out", out.t, want["out"], dt)
    assert torch.equal(lab, idev(want["labels"] if case["labels"] else inp["labels"])), f"{case['id']}: labels"
    assert bool((lbuf[:64] == LAB_SENT).all()) and bool((lbuf[64 + B * L:] == LAB_SENT).all()), f"{case['id']}: labels written outside [B, L]"
    if not case["bwd"]:
        return
    dout = dev(inp["dout"], dt)
    g = dict(dword=Guarded(R.N_WORD, d, "f32", fill=inp["dword0"]), dpos=Guarded(R.N_POS, d, "f32", fill=inp["dpos0"]))
    if case["vis"]:
        g["dvis"] = Guarded(B * nvis, d, dt)          # pre-filled with the sentinel: the unused rows must come back exactly 0
    ops.rl_assemble_bwd(dout, idd, pid, g["dword"].t, g["dpos"].t, g["dvis"].t.view(B, nvis, d) if case["vis"] else None)
    intact(g, case["id"])
    for name, gd in g.items():
        same_bits(f"{case['id']} {name}", gd.t, want[name], "f32" if name != "dvis" else dt)


def test_rl_assembly_refuses_a_sequence_past_its_limit(ops):
    from bdm_db1_amd import lib
    B, L, d = 1, R.RLA_MAX_L + 1, 8
    z = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    word, out = torch.zeros(R.N_WORD, d, device=DEV), Guarded(B * L, d, "f32")
    with pytest.raises(lib.Db1Error, match="rl_assemble_fwd: shape"):
        ops.rl_assemble_fwd(word, word, None, z, z, None, out.t.view(B, L, d))
    acc = Guarded(R.N_WORD, d, "f32")
    with pytest.raises(lib.Db1Error, match="rl_assemble_bwd: shape"):
        ops.rl_assemble_bwd(out.t.view(B, L, d), z, z, acc.t, acc.t, None)
    torch.cuda.synchronize()
    assert bool((out.buf == S.SENT).all()) and bool((acc.buf == S.SENT).all())


# ------------------------------------------------------------------------------------------------ masked cross-entropy
CE = R.cases("ce")


@pytest.mark.parametrize("case", CE, ids=ids(CE))
def test_masked_ce_within_its_bounds_and_fused_equals_the_pair(ops, case):
    from bdm_db1_amd import lib
    inp = R.ce_inputs(case)
    exp = R.ce_run_expect(case, inp)
    T, V, ld, dt, off, cid = case["T"], case["V"], case["ld"], case["dt"], case["off"], case["id"]
    labels, masks = idev(inp["labels"]), dev(inp["masks"], "f32")
    norm = dev(np.array([0.0, inp["norm1"]]), "f32")
    LG = Guarded(T, ld, dt, fill=inp["logits"], off=off)
    before = ibits(body(LG)).clone()
    g = dict(lse=Guarded(1, T, "f32"), sums=Guarded(1, 2, "f32", fill=inp["sums0"]), dlogits=Guarded(T, ld, dt, off=off))
    ops.masked_ce_fwd(LG.t, labels, masks, g["lse"].t[0], g["sums"].t[0], V)
    ops.masked_ce_bwd(LG.t, labels, masks, g["lse"].t[0], norm, g["dlogits"].t, V, gscale=inp["gscale"])
    intact(dict(g, logits=LG), cid)
    assert torch.equal(ibits(body(LG)), before), f"{cid}: the forward / backward pair changed the logits"
    got = dict(lse=host(g["lse"].t[0]), sums=host(g["sums"].t[0]), dlogits=host(g["dlogits"].t))
    checked(cid, got, exp)
    assert not bool(ibits(g["dlogits"].t[:, V:]).any()), f"{cid}: a pad column of dlogits is not +0"
    # the one-pass form: bit-equal where it is supported, refused without touching anything where it is not
    sup = lib.load().db1_masked_ce_fwd_bwd_supported(V, ld, ops.dt_code(TD[dt]))
    assert sup == int(R.ce_supported(dt, V, ld)) == int(not (ld % R.vn(dt) != 0 or ld > 256 * R.vn(dt) * 17))
    LG2 = Guarded(T, ld, dt, fill=inp["logits"], off=off)
    g2 = dict(lse=Guarded(1, T, "f32"), sums=Guarded(1, 2, "f32", fill=inp["sums0"]), logits=LG2)
    if sup and off == 0:
        ops.masked_ce_fwd_bwd(LG2.t, labels, masks, g2["lse"].t[0], g2["sums"].t[0], norm, V, gscale=inp["gscale"])
        intact(g2, cid + " fwd_bwd")
        assert torch.equal(ibits(g2["lse"].t), ibits(g["lse"].t)) and torch.equal(ibits(g2["sums"].t), ibits(g["sums"].t)), f"{cid}: fwd_bwd lse / sums differ from the pair's"
        assert torch.equal(ibits(body(LG2)), ibits(body(g["dlogits"]))), f"{cid}: fwd_bwd dlogits differ from the pair's"
    else:
        with pytest.raises(lib.Db1Error, match="masked_ce_fwd_bwd"):
            ops.masked_ce_fwd_bwd(LG2.t, labels, masks, g2["lse"].t[0], g2["sums"].t[0], norm, V, gscale=inp["gscale"])
        intact(g2, cid + " fwd_bwd refused")
        assert torch.equal(ibits(body(LG2)), before) and bool((g2["lse"].t == S.SENT).all()) and torch.equal(g2["sums"].t[0], dev(inp["sums0"], "f32"))


# ------------------------------------------------------------------------------------------------ the sweep
SWEEP = R.cases("sweep")


@pytest.mark.parametrize("case", SWEEP, ids=ids(SWEEP))
def test_lmhead_sweep_within_its_bounds(ops, case):
    from bdm_db1_amd import lib
    inp = R.sweep_inputs(case)
    exp = R.sweep_expect(case, inp)
    T, V, rows, d, dt, cid = case["T"], case["V"], case["rows"], case["d"], case["dt"], case["id"]
    chunk, nch, ragged, fused = R.sweep_plan(case)
    assert bool(lib.load().db1_masked_ce_fwd_bwd_supported(V, rows, ops.dt_code(TD[dt]))) == fused
    h, W, labels, masks = dev(inp["h"], dt), dev(inp["W"], dt), idev(inp["labels"]), dev(inp["masks"], "f32")
    # loss only
    f = dict(lse=Guarded(1, T, "f32"), sums=Guarded(1, 2, "f32", fill=inp["sums0"]))
    ops.lmhead_ce(h, W, labels, masks, f["lse"].t[0], f["sums"].t[0], V, chunk_rows=case["chunk"])
    intact(f, cid + " fwd")
    checked(cid + " fwd", {k: host(v.t[0]) for k, v in f.items()}, {k: exp[k] for k in f})
    # training sweep
    g = dict(lse=Guarded(1, T, "f32"), sums=Guarded(1, 2, "f32", fill=inp["sums0"]), dh=Guarded(T, d, dt), dW=Guarded(rows, d, "f32", fill=inp["dW0"]))
    ops.lmhead_ce(h, W, labels, masks, g["lse"].t[0], g["sums"].t[0], V, dh=g["dh"].t, dW_acc=g["dW"].t, beta_dw=float(case["beta"]),
                  gscale=inp["gscale"], chunk_rows=case["chunk"])
    intact(g, cid)
    checked(cid, dict(lse=host(g["lse"].t[0]), sums=host(g["sums"].t[0]), dh=host(g["dh"].t), dW=host(g["dW"].t)), exp)
    assert torch.equal(ibits(g["lse"].t), ibits(f["lse"].t)) and torch.equal(ibits(g["sums"].t), ibits(f["sums"].t)), f"{cid}: the two sweeps' lse / sums differ"
    if rows > V:                             # W's pad rows (logits of +30 if they counted) get no gradient at all
        pad = g["dW"].t[V:]
        want = np.zeros((rows - V, d), np.float32) if case["beta"] == 0 else inp["dW0"][V:]
        same_bits(f"{cid} dW pad rows", pad, want, "f32")
    if not ragged:
        return
    # forward-only sweep from zero sums + db1_lmhead_ce_bwd == the fused sweep, bit for bit
    lse0, sums0 = torch.empty(T, device=DEV), torch.zeros(2, device=DEV)
    ops.lmhead_ce(h, W, labels, masks, lse0, sums0, V, chunk_rows=case["chunk"])
    b = dict(dh=Guarded(T, d, dt), dW=Guarded(rows, d, "f32", fill=inp["dW0"]))
    n = int(lib.load().db1_lmhead_ce_bwd_workspace_bytes(T, rows, d, case["chunk"], ops.dt_code(h)))
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    lib.call("db1_lmhead_ce_bwd", ops.P(h), ops.P(W), ops.P(labels), ops.P(masks), ops.P(lse0), ops.P(sums0), ops.P(b["dh"].t), ops.P(b["dW"].t),
             float(case["beta"]), float(inp["gscale"]), T, V, rows, d, case["chunk"], ops.dt_code(h), ops.P(ws), n, ops.stream())
    intact(b, cid + " bwd")
    assert torch.equal(ibits(lse0), ibits(g["lse"].t[0])), f"{cid}: lse of the forward sweep"
    assert torch.equal(ibits(b["dh"].t), ibits(g["dh"].t)) and torch.equal(ibits(b["dW"].t), ibits(g["dW"].t)), f"{cid}: db1_lmhead_ce_bwd differs from the fused sweep"
