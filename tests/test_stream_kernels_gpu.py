"""The streaming kernels of csrc/elementwise.hip at every dispatch branch and edge, through bdm_db1_amd.ops, under the rule of
tests/stream_rule.py: the case table, float64 references and derived per-element bounds are the ones test_stream_rule_cpu.py proves usable;
every output and accumulator lies inside a larger allocation whose margins (and the columns between cols and ld of strided outputs) must come
back bit-identical to the sentinel they were filled with."""
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
from gpu_common import Guarded  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops as _ops, lib
    assert lib.load().db1_device_is_gfx950() == 1
    return _ops


DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(TD[dt])


def host(t):
    return t.detach().float().cpu().numpy().copy()      # bf16 -> float32 is exact


def verify(case, inp, got, guards):
    torch.cuda.synchronize()
    for name, g in guards.items():
        g.intact(f"{case['id']} {name}")
    worst = {}
    for name, (ref, bnd) in S.expect(case, inp, got).items():
        worst[name] = S.check(S.value(got, name), ref, bnd, f"{case['id']} {name}")
    print(case["id"], " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def ids(cs):
    return [c["id"] for c in cs]


# ------------------------------------------------------------------------------------------------ LayerNorm
def run_ln_fwd(ops, case, inp):
    rows, d, dt = case["rows"], case["d"], case["dt"]
    X, R = dev(inp["x"], dt), dev(inp["r"], dt) if inp["r"] is not None else None
    G, B = dev(inp["gamma"], case["pdt"]), dev(inp["beta"], case["pdt"])
    g = dict(y=Guarded(rows, d, dt), mean=Guarded(1, rows, "f32"), rstd=Guarded(1, rows, "f32"))
    if case["s_out"]:
        g["s_out"] = Guarded(rows, d, dt)
    else:   # the row the statistics are defined on, from a call that stores it (the call under test then runs without)
        s_tmp, y_tmp, m_tmp, r_tmp = torch.empty_like(X), torch.empty_like(X), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        ops.layernorm_residual_fwd(X, R, case["alpha"], G, B, y_tmp, s_tmp, m_tmp, r_tmp, S.EPS)
    ops.layernorm_residual_fwd(X, R, case["alpha"], G, B, g["y"].t, g["s_out"].t if case["s_out"] else None, g["mean"].t[0], g["rstd"].t[0], S.EPS)
    got = dict(y=g["y"].np(), mean=g["mean"].np(True), rstd=g["rstd"].np(True))
    got["_s"] = g["s_out"].np() if case["s_out"] else host(s_tmp)
    if case["s_out"]:
        got["s_out"] = got["_s"]
    return got, g


@pytest.mark.parametrize("case", S.cases("ln_fwd"), ids=ids(S.cases("ln_fwd")))
def test_layernorm_fwd(ops, case):
    inp = S.inputs(case)
    verify(case, inp, *run_ln_fwd(ops, case, inp))


def run_ln_bwd(ops, case, inp):
    rows, d, dt = case["rows"], case["d"], case["dt"]
    DY, S_, G = dev(inp["dy"], dt), dev(inp["s"], dt), dev(inp["gamma"], case["pdt"])
    MU, RS = dev(inp["mean"], "f32"), dev(inp["rstd"], "f32")
    g = dict(ds=Guarded(rows, d, dt))
    if case.get("mode") == "parts":
        nb = ops.layernorm_bwd_parts_numel(rows, d, TD[dt]) // (2 * d)
        assert nb == -(-rows // S.ln_bwd_rpb(rows))
        g["parts"] = Guarded(nb, 2 * d, "f32")
        ops.layernorm_residual_bwd_parts(DY, S_, G, MU, RS, g["ds"].t, g["parts"].t)
    elif case["params"]:
        g["dgamma"], g["dbeta"] = Guarded(1, d, "f32", fill=inp["dg0"]), Guarded(1, d, "f32", fill=inp["db0"])
        ops.layernorm_residual_bwd(DY, S_, G, MU, RS, g["ds"].t, g["dgamma"].t[0], g["dbeta"].t[0])
    else:
        ops.layernorm_residual_bwd(DY, S_, G, MU, RS, g["ds"].t, None, None)
    return {k: (v.np(True) if k in ("dgamma", "dbeta") else v.np()) for k, v in g.items()}, g


@pytest.mark.parametrize("case", S.cases("ln_bwd"), ids=ids(S.cases("ln_bwd")))
def test_layernorm_bwd(ops, case):
    inp = S.inputs(case)
    verify(case, inp, *run_ln_bwd(ops, case, inp))


LN_TWICE = [c for c in S.cases("ln_bwd") if c["params"] and c.get("mode") != "parts" and (c["rows"], c["d"]) in ((37, 512), (8177, 512), (4091, 2048), (37, 264))]


@pytest.mark.parametrize("case", LN_TWICE, ids=ids(LN_TWICE))
def test_layernorm_bwd_twice_bit_identical(ops, case):
    inp = S.inputs(case)
    a, _ = run_ln_bwd(ops, case, inp)
    b, _ = run_ln_bwd(ops, case, inp)
    for k in ("ds", "dgamma", "dbeta"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


LN_PARTS = [c for c in S.cases("ln_bwd") if c.get("mode") == "parts"]


@pytest.mark.parametrize("case", LN_PARTS, ids=ids(LN_PARTS))
def test_layernorm_bwd_parts_reduce_to_the_direct_result(ops, case):
    """colsum_acc over the partials against the direct call's own reduce: both add the same float32 partials, each within its chain's
    allowance of their exact sum"""
    inp = S.inputs(case)
    rows, d = case["rows"], case["d"]
    got, g = run_ln_bwd(ops, case, inp)
    direct, _ = run_ln_bwd(ops, dict(case, mode=None), inp)
    acc = Guarded(1, 2 * d, "f32", fill=np.concatenate([inp["dg0"], inp["db0"]]))
    ops.colsum_acc(g["parts"].t, acc.t[0])
    torch.cuda.synchronize()
    acc.intact("colsum over parts")
    nb = got["parts"].shape[0]
    ref = np.concatenate([direct["dgamma"], direct["dbeta"]]).astype(np.float64)
    A = np.abs(got["parts"].astype(np.float64)).sum(0) + np.abs(np.concatenate([inp["dg0"], inp["db0"]]))
    c = (-(-nb // 16) + 16) + S.colsum_chain(dict(op="colsum", dt="f32", rows=nb, cols=2 * d, variant="plain"))
    S.check(acc.np(True), ref, S.bound(ref, A, c, "f32"), f"{case['id']} colsum(parts) vs direct")


def test_layernorm_bwd_parts_refuses_the_generic_path(ops):
    from bdm_db1_amd import lib
    case = dict(S.cases("ln_bwd")[0], d=264, rows=5, id="parts-generic")
    inp = S.inputs(case)
    args = [dev(inp["dy"], "bf16"), dev(inp["s"], "bf16"), dev(inp["gamma"], "bf16"), dev(inp["mean"], "f32"), dev(inp["rstd"], "f32")]
    assert ops.layernorm_bwd_parts_numel(5, 264, torch.bfloat16) == 0
    with pytest.raises(lib.Db1Error, match="register-resident"):
        ops.layernorm_residual_bwd_parts(*args, torch.empty(5, 264, device=DEV, dtype=torch.bfloat16), torch.empty(2, 528, device=DEV))


# ------------------------------------------------------------------------------------------------ activations
def run_act(ops, case, inp):
    rows, n, dt, act, ld = case["rows"], case["n"], case["dt"], case["act"], S.act_ld(case)
    Z = dev(inp["z"], dt)
    if case["op"] == "act_fwd":
        g = dict(out=Guarded(rows, n, dt))
        ops.ffn_act_fwd(Z, g["out"].t, act)
    elif case["op"] == "act_bwd":
        g = dict(dz=Guarded(rows, ld, dt))
        ops.ffn_act_bwd(Z, dev(inp["dout"], dt), g["dz"].t, act)
    else:
        g = dict(dz=Guarded(rows, ld, dt), dbias=Guarded(1, ld, "f32", fill=inp["acc0"]))
        ops.ffn_act_bwd_bias(Z, dev(inp["dout"], dt), g["dz"].t, g["dbias"].t[0], act)
    return {k: (v.np(True) if k == "dbias" else v.np()) for k, v in g.items()}, g


ACT = S.cases("act_fwd", "act_bwd", "act_bwd_bias")


@pytest.mark.parametrize("case", ACT, ids=ids(ACT))
def test_ffn_activation(ops, case):
    inp = S.inputs(case)
    verify(case, inp, *run_act(ops, case, inp))


# ------------------------------------------------------------------------------------------------ column sums, sums of squares
def colsum_view(case, inp):
    rows, cols, dt, ld, v = case["rows"], case["cols"], case["dt"], S.colsum_ld(case), case.get("variant", "plain")
    if v == "offset1":
        store = torch.zeros(rows * cols + 16, device=DEV, dtype=TD[dt])
        x = store[1:1 + rows * cols].view(rows, cols)
    else:
        store = torch.ones(rows, ld, device=DEV, dtype=TD[dt])       # (the columns past cols would show in every sum)
        x = store[:, :cols]
    x.copy_(dev(inp["x"], dt))
    assert x.stride(0) == ld and (x.data_ptr() % 16 != 0) == (v == "offset1")
    return x


def run_colsum(ops, case, inp):
    g = dict(out=Guarded(1, case["cols"], "f32", fill=inp["acc0"]))
    ops.colsum_acc(colsum_view(case, inp), g["out"].t[0])
    return dict(out=g["out"].np(True)), g


@pytest.mark.parametrize("case", S.cases("colsum"), ids=ids(S.cases("colsum")))
def test_colsum_acc(ops, case):
    inp = S.inputs(case)
    verify(case, inp, *run_colsum(ops, case, inp))


COLSUM_TWICE = [c for c in S.cases("colsum") if S.colsum_path(c) == "chunk" and c["cols"] == 72]


@pytest.mark.parametrize("case", COLSUM_TWICE, ids=ids(COLSUM_TWICE))
def test_colsum_chunked_twice_bit_identical(ops, case):
    inp = S.inputs(case)
    a, b = run_colsum(ops, case, inp)[0]["out"], run_colsum(ops, case, inp)[0]["out"]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_sumsq(ops, case, inp):
    from bdm_db1_amd import lib
    X = dev(inp["x"], case["dt"])
    g = dict(acc=Guarded(1, 1, "f32", fill=[inp["acc0"]]))
    if case["op"] == "sumsq_acc":
        ops.sumsq_acc(X, g["acc"].t[0])
    else:
        ws, wsn = ops._ws("db1_sumsq_det_workspace_bytes", (case["n"],), X.device)
        lib.call("db1_sumsq_det", ops.P(X), ops.P(g["acc"].t[0]), case["n"], ops.dt_code(X), case["overwrite"], ws, wsn, ops.stream())
    return dict(acc=g["acc"].np(True)), g


SUMSQ = S.cases("sumsq_acc", "sumsq_det")


@pytest.mark.parametrize("case", SUMSQ, ids=ids(SUMSQ))
def test_sumsq(ops, case):
    inp = S.inputs(case)
    got, g = run_sumsq(ops, case, inp)
    verify(case, inp, got, g)
    if case["op"] == "sumsq_det":
        again = run_sumsq(ops, case, inp)[0]["acc"]
        assert np.array_equal(got["acc"].view(np.uint32), again.view(np.uint32))


# ------------------------------------------------------------------------------------------------ Adam
def run_adam(ops, case, inp):
    n, hp = case["n"], S.ADAM_HP
    g = dict(p=Guarded(1, n, "f32", fill=inp["p0"]), m=Guarded(1, n, "f32", fill=np.zeros(n)), v=Guarded(1, n, "f32", fill=np.zeros(n)))
    if case["pw"]:
        g["pw"] = Guarded(1, n, "bf16")
    got = {}
    for step in (1, 2, 3):
        if case["g8"]:     # a gradient view 8 bytes into its allocation: aligned for the 8-byte loads of the bf16 form, not for 16
            store = torch.zeros(n + 8, device=DEV, dtype=torch.bfloat16)
            G = store[4:4 + n]
            G.copy_(dev(inp["g"][step - 1], "bf16"))
            assert G.data_ptr() % 16 == 8
        else:
            G = dev(inp["g"][step - 1], case["gdt"])
        nsq = torch.full((1,), float(inp["nsq"][step - 1]), device=DEV) if case["nsq"] else None
        ops.adam_step(g["p"].t[0], G, g["m"].t[0], g["v"].t[0], g["pw"].t[0] if case["pw"] else None, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"],
                      case["adamw"], step, gscale=case["gscale"], clip=case["clip"], norm_sq=nsq)
        for k in g:
            got[f"{k}{step}"] = g[k].np(True)
        if case["pw"]:
            assert torch.equal(g["pw"].t[0], g["p"].t[0].to(torch.bfloat16)), f"p_work != bf16(p) at step {step}"
    return got, g


@pytest.mark.parametrize("case", S.cases("adam"), ids=ids(S.cases("adam")))
def test_adam(ops, case):
    inp = S.inputs(case)
    if case.get("grads") == "small":
        assert all(np.sqrt(float(x)) < case["clip"] for x in inp["nsq"])
    elif case["clip"] > 0 and case["nsq"] and case.get("grads") == "normal" and case["n"] > 4:
        assert np.sqrt(float(inp["nsq"][0])) * case["gscale"] > case["clip"]          # clipping active
    verify(case, inp, *run_adam(ops, case, inp))


# ------------------------------------------------------------------------------------------------ add / add2d / cast: bit for bit
def _place(a, dt, ld=None, off=0):
    rows, cols = a.shape
    return Guarded(rows, cols, dt, ld=ld, fill=a, off=off)


EXACT = S.cases("add", "add2d", "cast")


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_add_add2d_cast_bit_exact(ops, case):
    inp = S.inputs(case)
    op, dt, adt, form, rows, cols, V = case["op"], case["dt"], case["adt"], case["form"], case["rows"], case["cols"], S.vec(case["dt"])
    if op == "cast":
        X, y = dev(inp["a"], adt).reshape(-1), Guarded(1, rows * cols, dt)
        ops.cast(X, y.t[0])
        want = X.to(TD[dt])
    elif op == "add":
        off = 1 if form == "offset1" else 0
        A, B = _place(inp["a"].reshape(1, -1), adt, off=off), _place(inp["b"].reshape(1, -1), dt, off=off)
        want = (A.t.float() + B.t.float()).to(TD[dt])[0]
        y = B if case["alias"] else Guarded(1, rows * cols, dt, off=off)
        n = rows * cols
        assert ((n % V == 0) and off == 0) == (form == "vec")
        ops.add(A.t[0], B.t[0], y.t[0])
    else:
        pad = {"vec": (V, 2 * V, V), "mixed": (4, 8, 8), "odd_cols": (3, 3, 3), "odd_ld": (1, V, V)}[form]
        A, B = _place(inp["a"], adt, ld=cols + pad[0]), _place(inp["b"], dt, ld=cols + pad[1])
        want = (A.t.float() + B.t.float()).to(TD[dt])
        y = B if case["alias"] else Guarded(rows, cols, dt, ld=cols + pad[2])
        ops.add2d(A.t, B.t, y.t)
    torch.cuda.synchronize()
    y.intact(case["id"])
    got = y.t[0] if op != "add2d" else y.t
    assert torch.equal(got, want), f"{case['id']}: {(got != want).sum().item()} elements differ from torch"
