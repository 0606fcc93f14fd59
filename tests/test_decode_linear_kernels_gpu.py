"""db1_linear_decode and db1_linear_decode_attn (csrc/gemm_skinny.hip) against the rule of tests/decode_linear_rule.py: every case of its table
through the C entry points themselves, with tickets, workspace and outputs owned by the test.  The exact designs are compared bit for bit
with the float64 reference rounded once; the bounded ones per element under the rule's bounds (tests/test_decode_linear_rule_cpu.py proves
that every one-mistake mutant of the reference breaks them tenfold).  After every launch: status 0, every ticket word zero, the guard
bands of every output and of the workspace intact, every output element finite (outputs start as NaN), and a second launch gives the same bits.

Template instantiations dispatched and the case that reaches each (gemm_skinny_fused_kernel<TBIAS, TP, MT, GEGLU, PRO>; decode_linear_rule
.instantiation names the one a case takes, and the CPU test asserts that the table reaches all 58 of all_instantiations()):
  linear_decode_launch
    PRO = 0, GEGLU false    (TBIAS, float): plain, M in {1, 15, 16} MT 1, {17, 32} MT 2, {33, 48} MT 3, {49, 64} MT 4, bias bf16 / f32 / none
                            (TBIAS, bf16): tail with bf16 parameters, M in {1, 4, 5} MT 1, 17 MT 2, 33 MT 3, 64 MT 4, bias bf16 / f32 / none
    PRO = 0, GEGLU true     (TBIAS, float): geglu, M in {1, 16} MT 1, 17 MT 2, 33 MT 3, 64 MT 4, bias bf16 / f32 / none
                            (TBIAS, bf16) and again (TBIAS, float): geglu + tail at N = 512, M in {1, 17, 33, 64}, bias bf16 / f32, bf16 / fp32 parameters
    PRO 1 / 4 / 16          pre, M = 1 / M in {2, 3, 4} / M in {5, 15, 16}; GEGLU false (N = 48) and true (N = 16); all four (TBIAS, TP) pairs
    skinny_ln_rows<TP, 1 / 2 / 4>   (a run-time choice inside every kernel) tail N = 512 / 1024 / 2048, TP bf16 and float
    S = 1, 2, 4, 8          plain; split (16, 4096), (48, 8192), (16, 16384); S = 1 by size at (16, 4032) and (4096, 4096); S = 1 by the knob
  linear_decode_attn_launch
    PRO -1        merge cases (B, q) = (1, 1);  PRO -2: (1, 2) and (2, 1)
  W8 = true (TBIAS = TP = bf16; attn: float)   test_fp8_form: every case with K % 128 == 0, a bf16 bias or none and bf16 parameters -- MT 1 / 2 / 4
                  at plain K = 128 and split-K, skinny_ln_rows<., 1> at tail (512, 4096), PRO 1 / 4 / 16 with GEGLU false and true, PRO -1 / -2;
                  GEGLU with PRO = 0 and MT 3 have no K % 128 == 0 case here: tests/test_w8_kernels_gpu.py compares them with the bf16 launch
  dc_launch: tests/test_decode_chain_probe_gpu.py"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_linear_rule as R  # noqa: E402
import stream_rule as S  # noqa: E402
from gpu_common import DEV, TD, Guarded, _need_gpu, dev, host  # noqa: E402,F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
_ratios = {}


@pytest.fixture(scope="module")
def env():
    from bdm_db1_amd import lib, ops
    L = lib.load()
    tickets = torch.zeros(int(L.db1_linear_decode_tickets_bytes()) // 4, dtype=torch.int32, device=DEV)
    yield dict(lib=lib, ops=ops, L=L, tickets=tickets)
    if _ratios:
        print("\nlargest observed ratio per bounded output: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_ratios.items())))


def ids(cs):
    return [c["id"] for c in cs]


def padded(a, pad, fill, dt="bf16"):
    """a [rows, cols] as a view with row stride cols + pad; the padding holds ``fill``"""
    rows, cols = a.shape
    buf = torch.full((rows, cols + pad), fill, device=DEV, dtype=TD[dt])
    buf[:, :cols] = dev(a, dt)
    return buf[:, :cols]


def nan_out(rows, cols, ld):
    g = Guarded(rows, cols, "bf16", ld=ld)
    g.t.fill_(NAN)
    return g


class Launch:
    """the operands of one case on the device, and the call"""

    def __init__(self, env, case, inp, form="bf16"):
        self.env, self.case = env, case
        M, N, K = case["M"], case["N"], case["K"]
        P, L = env["ops"].P, env["L"]
        strided = case["kind"] == "plain"
        self.out = dict(y=nan_out(M, N, N + 24 if strided else N))
        self.W = dev(inp["W"], "bf16")
        if form == "w8":                                    # the designs' weights (0, +-1/4, +-1, +-2, +-3) are lossless in e4m3 with power-of-two block scales
            w16, self.W = self.W, env["ops"].w8_quantize(self.W)
            assert torch.equal(env["ops"].w8_unpack(self.W, *w16.shape)[0], w16.cpu()), "the fp8 form of the probe's weight is not lossless"
        f_lin, f_attn = (L.db1_linear_decode_w8, L.db1_linear_decode_attn_w8) if form == "w8" else (L.db1_linear_decode, L.db1_linear_decode_attn)
        self.bias = None if inp["bias"] is None else dev(inp["bias"], case["bias"])
        dtb = 0 if self.bias is None else env["ops"].dt_code(self.bias.dtype)
        null = P(None)
        if case["kind"] == "merge":
            self.part = torch.from_numpy(inp["part"]).to(DEV)
            y = self.out["y"].t
            self.call = lambda: f_attn(P(self.part), case["nunit"], case["B"], case["q"], case["H"], 128, P(self.W), P(y), y.stride(0), N,
                                                         env["ops"].stream())
            return
        self.x = padded(inp["x"], 8 if strided else 0, 64.0)       # a read past K shows: the padding holds 64
        pre, tail, dtp = (null, 0, 1.0, null, null, 0.0, null, 0), (null, 0, 1.0, null, null, 0.0, null, 0), 0
        if case.get("pre"):
            self.pre_res = padded(inp["pre_res"], 8, 64.0)
            self.pre_g, self.pre_b = dev(inp["pre_gamma"], case["pdt"]), dev(inp["pre_beta"], case["pdt"])
            self.out["pre_out"] = nan_out(M, K, K + 8)
            po = self.out["pre_out"].t
            pre, dtp = (P(self.pre_res), self.pre_res.stride(0), R.ALPHA, P(self.pre_g), P(self.pre_b), R.EPS, P(po), po.stride(0)), env["ops"].dt_code(self.pre_g.dtype)
        if case.get("tail"):
            self.res = padded(inp["res"], 8, 64.0)
            self.g, self.b = dev(inp["gamma"], case["pdt"]), dev(inp["beta"], case["pdt"])
            self.out["ln_out"] = nan_out(M, N, N + 8)
            lo = self.out["ln_out"].t
            tail, dtp = (P(self.res), self.res.stride(0), R.ALPHA, P(self.g), P(self.b), R.EPS, P(lo), lo.stride(0)), env["ops"].dt_code(self.g.dtype)
        geglu = int(case.get("geglu", False))
        nws = int(L.db1_linear_decode_workspace_bytes(M, N, K, geglu))
        assert nws == R.workspace_bytes(M, N, K, bool(geglu)), "S differs from the rule's"
        self.ws = Guarded(1, max(nws // 4, 64), "f32")
        y = self.out["y"].t
        self.call = lambda: f_lin(P(self.x), self.x.stride(0), P(self.W), P(self.bias), dtb, P(y), y.stride(0), M, N, K, geglu, *pre, *tail, dtp,
                                                P(env["tickets"]), P(self.ws.t), nws, env["ops"].stream())

    def run(self):
        """one launch from NaN outputs -> {name: float32 array}, after the checks every launch gets"""
        for g in self.out.values():
            g.t.fill_(NAN)
        st = self.call()
        torch.cuda.synchronize()
        assert st == R.OK, (st, self.env["L"].db1_last_error())
        assert int(self.env["tickets"].abs().sum().item()) == 0, "a ticket word is not zero after the launch"
        got = {}
        for name, g in self.out.items():
            g.intact(f"{self.case['id']} {name}")
            got[name] = g.np()
            assert np.isfinite(got[name]).all(), f"{name}: {int((~np.isfinite(got[name])).sum())} elements not written (or not finite)"
        if hasattr(self, "ws"):
            self.ws.intact("workspace")
        return got


def verify(env, case, form="bf16"):
    inp = R.inputs(case)
    ln = Launch(env, case, inp, form)
    got = ln.run()
    again = ln.run()
    for name in got:
        assert np.array_equal(got[name].view(np.uint32), again[name].view(np.uint32)), f"{name}: a second launch gives other bits"
    worst = {}
    for name, (ref, bnd) in R.expect(case, inp, got).items():
        q = S.check(got[name], ref, bnd, f"{case['id']} {name}")
        if bnd.any():
            worst[name] = q
            # next to it, the share of the fp32 allowance in use: what is left of the error beyond half an output ulp, over the rest of the bound
            hu = S.half_ulp(ref, "bf16")
            with np.errstate(invalid="ignore", divide="ignore"):
                sh = np.where(bnd > hu, (np.abs(got[name] - ref) - hu) / (bnd - hu), 0.0)
            worst[name + " fp32"] = max(0.0, float(sh.max()))
            key = f"{case['kind']}{'+geglu' if case.get('geglu') and case['kind'] != 'geglu' else ''}{'/w8' if form == 'w8' else ''}.{name}"
            _ratios[key] = max(_ratios.get(key, 0.0), q)
            _ratios[key + " fp32"] = max(_ratios.get(key + " fp32", 0.0), worst[name + " fp32"])
    if worst:
        print(f"{case['id']}: max ratio = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return inp, ln, got


@pytest.mark.parametrize("case", R.cases("plain"), ids=ids(R.cases("plain")))
def test_plain(env, case):
    verify(env, case)


@pytest.mark.parametrize("case", R.cases("split"), ids=ids(R.cases("split")))
def test_split_k(env, case):
    inp, ln, got = verify(env, case)
    s = R.geometry(case)[0]
    assert (int(env["L"].db1_linear_decode_workspace_bytes(case["M"], case["N"], case["K"], 0)) > 0) == (s > 1)
    assert s == dict((nk[:2], nk[2]) for nk in R.SPLIT_NK)[(case["N"], case["K"])]
    try:                                                    # never split: the same bits, which exactness guarantees
        env["lib"].set_knob("linear_decode_splitk", 0)
        assert int(env["L"].db1_linear_decode_workspace_bytes(case["M"], case["N"], case["K"], 0)) == 0
        one = ln.run()
    finally:
        env["lib"].set_knob("linear_decode_splitk", -1)
    assert np.array_equal(one["y"].view(np.uint32), got["y"].view(np.uint32))


def _tail_equals_the_layernorm_launch(env, case, ln, got):
    ops, M, N = env["ops"], case["M"], case["N"]
    y = dev(got["y"], "bf16")
    h, mean, rstd = torch.empty(M, N, device=DEV, dtype=torch.bfloat16), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_residual_fwd(ln.res.contiguous(), y, R.ALPHA, ln.g, ln.b, h, None, mean, rstd, R.EPS)
    assert np.array_equal(host(h).view(np.uint32), got["ln_out"].view(np.uint32)), "the tail differs from db1_layernorm_residual_fwd on the same y"


@pytest.mark.parametrize("case", R.cases("tail"), ids=ids(R.cases("tail")))
def test_layernorm_tail(env, case):
    inp, ln, got = verify(env, case)
    _tail_equals_the_layernorm_launch(env, case, ln, got)


@pytest.mark.parametrize("case", R.cases("geglu"), ids=ids(R.cases("geglu")))
def test_geglu(env, case):
    inp, ln, got = verify(env, case)
    z = dev(R.geglu_z(case, inp), "bf16")
    a = torch.empty(case["M"], case["N"], device=DEV, dtype=torch.bfloat16)
    env["ops"].ffn_act_fwd(z, a, "geglu")
    assert np.array_equal(host(a).view(np.uint32), got["y"].view(np.uint32)), "differs from db1_ffn_act_fwd on the exact z"
    if case.get("tail"):
        _tail_equals_the_layernorm_launch(env, case, ln, got)


@pytest.mark.parametrize("case", R.cases("pre"), ids=ids(R.cases("pre")))
def test_layernorm_prologue(env, case):
    inp, ln, got = verify(env, case)
    if case.get("tail"):
        _tail_equals_the_layernorm_launch(env, case, ln, got)


@pytest.mark.parametrize("case", R.cases("merge"), ids=ids(R.cases("merge")))
def test_attention_merge(env, case):
    verify(env, case)


W8_CASES = [c for c in R.CASES if c["K"] % 128 == 0 and c.get("bias", "none") != "f32" and c.get("pdt", "bf16") != "f32"]


@pytest.mark.parametrize("case", W8_CASES, ids=ids(W8_CASES))
def test_fp8_form(env, case):
    """db1_linear_decode_w8 / db1_linear_decode_attn_w8 on every case they accept (K % 128 == 0, bf16 bias and parameters): the same expectations,
    not only equality with the bf16 launch"""
    assert {c["kind"] for c in W8_CASES} == {"plain", "split", "tail", "pre", "merge"}
    verify(env, case, "w8")


def test_refusals_launch_nothing(env):
    L, P, tickets = env["L"], env["ops"].P, env["tickets"]
    null = P(None)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device=DEV, dtype=dt)
    for name, a in R.REFUSALS:
        M, N, K, geglu, tail, pre = a["M"], a["N"], a["K"], a.get("geglu", False), a.get("tail", False), a.get("pre", False)
        x, W, y = z(M, K), z((2 * N if geglu else N), K), nan_out(M, N, N)
        outs = [y]
        t_pre = t_tail = (null, 0, 1.0, null, null, 0.0, null, 0)
        keep = []
        if pre:
            outs.append(nan_out(M, K, K))
            keep += [z(M, K), z(K), z(K)]
            t_pre = (P(keep[-3]), K, R.ALPHA, P(keep[-2]), P(keep[-1]), R.EPS, P(outs[-1].t), K)
        if tail:
            outs.append(nan_out(M, N, N))
            keep += [z(M, N), z(N), z(N)]
            t_tail = (P(keep[-3]), N, R.ALPHA, P(keep[-2]), P(keep[-1]), R.EPS, P(outs[-1].t), N)
        assert not L.db1_linear_decode_supported(M, N, K, int(geglu), int(tail) | 2 * int(pre)), name
        ws = z(1 << 20, dt=torch.float32)
        st = L.db1_linear_decode(P(x), K, P(W), null, 0, P(y.t), N, M, N, K, int(geglu), *t_pre, *t_tail, 1, P(tickets), P(ws), ws.numel() * 4, env["ops"].stream())
        torch.cuda.synchronize()
        assert st == R.UNSUPPORTED, (name, st)
        assert all(bool(torch.isnan(o.t).all()) for o in outs) and int(tickets.abs().sum().item()) == 0, name
    for name, a in R.ATTN_REFUSALS:
        K, N = a["H"] * a["D"], a["N"]
        part = z(a["B"] * a["H"] * a["nunit"] * R.PART_ROWS * R.PART_LD, dt=torch.float32)
        W, y = z(N, K), nan_out(a["B"] * a["q"], N, N)
        assert not L.db1_linear_decode_attn_supported(a["B"], a["q"], a["H"], a["D"], a["nunit"], N), name
        st = L.db1_linear_decode_attn(P(part), a["nunit"], a["B"], a["q"], a["H"], a["D"], P(W), P(y.t), N, N, env["ops"].stream())
        torch.cuda.synchronize()
        assert st == R.UNSUPPORTED, (name, st)
        assert bool(torch.isnan(y.t).all()) and int(tickets.abs().sum().item()) == 0, name
