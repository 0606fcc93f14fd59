"""db1_decode_chain_w8 alone (include/db1_hip.h, "fp8 weights in the persistent chain"): bit for bit db1_decode_chain over the dequantised weights
on index-revealing weights (both forms of the launch, both unrollings of the merge and their edges, alternating slots on one scratch), stage by
stage against fp32 arithmetic, a bf16 and an fp8 launch sharing one scratch, and the refusals that come before a launch.

The chain exists at one geometry (d 2048, dff 4096, 16 heads of 128), so that is the shape; the weights, their packed and dequantised forms
and the fp32 reference are made once per module."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_common import DEV, _need_gpu  # noqa: E402,F401
import w8_chain_rule as C8  # noqa: E402

D_, DFF, H, D = 2048, 4096, 16, 128
BAD_SHAPE, BAD_ALIGN, UNSUPPORTED = -1, -2, -6      # DB1_ERR_* (include/db1_hip.h)
ALPHA, EPS = 1.3, 1e-5
BF = torch.bfloat16
_slot = [100]


def _next_slot():
    _slot[0] += 1
    return _slot[0]


class _Case:
    pass


@pytest.fixture(scope="module")
def case():
    """index-revealing weights 0.02 randn 2^e(row, block), e = (3 row + 5 block) % 7 - 3 (tests/w8_chain_rule.py): a scale or payload taken from
    another row, block or piece changes bits.  W8: ops.w8_quantize of them; DQ: the bf16 weights ops.w8_unpack returns, back on the device"""
    from bdm_db1_amd import ops
    if not ops.decode_chain_w8_supported(D_, DFF, H, D, 9 * 128):
        pytest.skip("db1_decode_chain_w8 needs 256 CUs")
    c = _Case()
    c.dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cpu").manual_seed(5)
    c.W8, c.DQ = {}, {}
    for name, (N, K) in dict(o=(D_, D_), w1=(2 * DFF, D_), w2=(D_, DFF), qkv=(3 * D_, D_), o_next=(D_, D_)).items():
        w = (0.02 * torch.randn(N, K, generator=g, dtype=torch.float64) * torch.from_numpy(C8.revealing_factor(N, K))).to(BF).to(c.dev)
        c.W8[name] = ops.w8_quantize(w)
        deq, s = ops.w8_unpack(c.W8[name], N, K)
        # (a block's scale follows its exponent up to the block's own amax: 2^e times one of two neighbouring powers of two)
        assert (s[1:] != s[:-1]).float().mean() > 0.5 and (s[:, 1:] != s[:, :-1]).float().mean() > 0.5
        assert not torch.equal(deq, w.cpu())                                                                  # (quantising is no no-op here)
        c.DQ[name] = deq.to(c.dev)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(BF).to(c.dev)
    c.x = r(1, D_)
    c.b1, c.b2 = r(2 * DFF, sc=0.1), r(D_, sc=0.1)
    c.g1, c.be1 = (1 + 0.1 * torch.randn(D_, generator=g)).to(BF).to(c.dev), r(D_, sc=0.1)
    c.g2, c.be2 = (1 + 0.1 * torch.randn(D_, generator=g)).to(BF).to(c.dev), r(D_, sc=0.1)
    c.parts = {}
    for nunit in (1, 9, 10, 12):
        part = torch.full((H, nunit, 64, D + 2), float("nan"))                 # only query row 0 of every unit is read
        part[:, :, 0, :D] = torch.randn(H, nunit, D, generator=g)
        part[:, :, 0, D] = torch.randn(H, nunit, generator=g)
        part[:, :, 0, D + 1] = torch.rand(H, nunit, generator=g) + 0.5
        if nunit > 1:
            part[3, 2, 0, D + 1] = 0.0                                             # a chunk without visible keys contributes nothing
        c.parts[nunit] = part.to(c.dev)
    return c


def _launch(c, w8, nunit, slot, last):
    """one launch -> dict of its scratch rows (values as bf16 bits, tags), its outputs and the error flag, all on the host"""
    from bdm_db1_amd import ops
    W = c.W8 if w8 else c.DQ
    nan = lambda n: torch.full((1, n), float("nan"), device=c.dev, dtype=BF)
    h1o, fo, xn, qn = nan(D_), nan(D_), nan(D_), nan(3 * D_)
    fn = ops.decode_chain_w8 if w8 else ops.decode_chain
    fn(c.parts[nunit], nunit * 128, H, c.x, W["o"], W["w1"], c.b1, W["w2"], c.b2, None if last else W["qkv"], c.g1, c.be1, c.g2, c.be2, ALPHA, EPS,
       h1o if last else None, fo if last else None, None if last else xn, None if last else qn, slot, w_o_next=W["o_next"])
    torch.cuda.synchronize()
    w = ops.decode_chain_scratch(c.dev)[: (2 * D_ + DFF) * 4].view(torch.int32).cpu()
    out = dict(words=w, tags=(w & 0xffff), err=ops.decode_chain_error(c.dev))
    out.update(dict(h1_out=h1o, f_out=fo) if last else dict(x_next=xn, qkv_next=qn))
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


@pytest.mark.parametrize("nunit", [1, 9, 10, 12])
def test_bit_for_bit_the_bf16_chain_over_the_dequantised_weights(case, nunit):
    """the three scratch rows (values and tags, every word's tag slot + 1), h1_out and f_out or x_next and qkv_next equal as bits; the error
    flag is 0; two fp8 launches give equal bits.  nunit 1, 9: the 9-chunk unrolling and its edges; 10, 12: the 12-chunk one"""
    for last in (False, True):
        s16, s8, s8b = _next_slot(), _next_slot(), _next_slot()
        a = _launch(case, False, nunit, s16, last)
        b = _launch(case, True, nunit, s8, last)
        b2 = _launch(case, True, nunit, s8b, last)
        for r, s in ((a, s16), (b, s8), (b2, s8b)):
            assert r["err"] is False and r["tags"].unique().tolist() == [s + 1], (nunit, last, s)
        for other in (b, b2):
            assert torch.equal(a["words"] >> 16, other["words"] >> 16), (nunit, last, "scratch rows")
            for k in (("h1_out", "f_out") if last else ("x_next", "qkv_next")):
                assert not bool(torch.isnan(a[k].float()).any()), k
                assert torch.equal(_bits(a[k]), _bits(other[k])), (nunit, last, k)


def _fp32_reference(c, nunit):
    """the chain in fp32 torch arithmetic over the DEQUANTISED weights, bf16 rounding where the launches it replaces store bf16
    (tests/test_decode_gpu.py::test_decode_chain_stages_against_fp32_arithmetic)"""
    part, W = c.parts[nunit], c.DQ
    rb = lambda t: t.to(BF).float()
    m, l, o = part[:, :, 0, D], part[:, :, 0, D + 1], part[:, :, 0, :D]
    wt = torch.where(l > 0, torch.exp(m - torch.where(l > 0, m, torch.full_like(m, -1e30)).max(1, keepdim=True).values), torch.zeros_like(m))
    merged = rb(((o * wt[..., None]).sum(1) / (l * wt).sum(1, keepdim=True)).reshape(1, D_))

    def ln(s, g, b):
        s = rb(s)
        mu = s.mean(-1, keepdim=True)
        return rb((s - mu) * torch.rsqrt(((s - mu) ** 2).mean(-1, keepdim=True) + EPS) * g.float() + b.float())
    y = rb(merged @ W["o"].float().t())
    h1 = ln(ALPHA * c.x.float() + y, c.g1, c.be1)
    z = rb(h1 @ W["w1"].float().t() + c.b1.float())
    act = rb(z[:, :DFF] * torch.nn.functional.gelu(z[:, DFF:]))
    f = rb(act @ W["w2"].float().t() + c.b2.float())
    xn = ln(ALPHA * h1 + f, c.g2, c.be2)
    q = rb(xn @ W["qkv"].float().t())
    return {k: v.reshape(-1).cpu() for k, v in dict(y_o=y, h1=h1, act=act, f=f, x_next=xn, qkv_next=q).items()}


def test_stages_against_fp32_arithmetic(case):
    """the fp8 launch stage by stage against fp32 over the dequantised weights, with the bounds of the bf16 chain's stage test: y_o 4e-3, act / f /
    x_next / qkv_next 1e-2, h1_out 5e-3 of max"""
    nunit = 9
    ref = _fp32_reference(case, nunit)
    err = lambda a, b: ((a.reshape(-1).float() - b.reshape(-1)).abs().max() / b.abs().max()).item()
    for last in (False, True):
        slot = _next_slot()
        r = _launch(case, True, nunit, slot, last)
        val = (r["words"] >> 16).to(torch.int16).view(BF).float()
        y_o, act, f = val[:D_], val[D_:D_ + DFF], val[D_ + DFF:]
        e = dict(y_o=err(y_o, ref["y_o"]), act=err(act, ref["act"]), f=err(f, ref["f"]))
        if last:
            e.update(h1_out=err(r["h1_out"], ref["h1"]), f_out=err(r["f_out"], ref["f"]))
        else:
            e.update(x_next=err(r["x_next"], ref["x_next"]), qkv_next=err(r["qkv_next"], ref["qkv_next"]))
        print("w8 chain stages", "last" if last else "with qkv", {k: f"{v:.2e}" for k, v in e.items()})
        assert r["err"] is False and r["tags"].unique().tolist() == [slot + 1]
        assert e["y_o"] < 4e-3 and e["act"] < 1e-2 and e["f"] < 1e-2
        if last:
            assert e["h1_out"] < 5e-3 and e["f_out"] < 1e-2
        else:
            assert e["x_next"] < 1e-2 and e["qkv_next"] < 1e-2


def test_bf16_and_fp8_launches_share_one_scratch(case):
    """bf16, fp8, bf16, fp8 on one scratch with consecutive slots and no synchronisation in between: each is right (the outputs of the four are
    equal bits, and those of a launch run alone), and the flag stays clean"""
    from bdm_db1_amd import ops
    c, nunit = case, 12
    alone = _launch(c, False, nunit, _next_slot(), False)
    outs = []
    for i in range(4):
        w8 = bool(i & 1)
        W = c.W8 if w8 else c.DQ
        xn, qn = torch.zeros(1, D_, device=c.dev, dtype=BF), torch.zeros(1, 3 * D_, device=c.dev, dtype=BF)
        (ops.decode_chain_w8 if w8 else ops.decode_chain)(c.parts[nunit], nunit * 128, H, c.x, W["o"], W["w1"], c.b1, W["w2"], c.b2, W["qkv"], c.g1, c.be1,
                                                          c.g2, c.be2, ALPHA, EPS, None, None, xn, qn, _next_slot(), w_o_next=W["o_next"])
        outs.append((xn, qn))
    torch.cuda.synchronize()
    assert not ops.decode_chain_error(c.dev)
    for xn, qn in outs:
        assert torch.equal(_bits(xn.cpu()), _bits(alone["x_next"])) and torch.equal(_bits(qn.cpu()), _bits(alone["qkv_next"]))
    tags = ops.decode_chain_scratch(c.dev)[: (2 * D_ + DFF) * 4].view(torch.int32) & 0xffff
    assert tags.unique().tolist() == [_slot[0] + 1]


def test_refusals_launch_nothing(case):
    """db1_decode_chain's codes, before a launch: a NULL operand and a slot out of range (DB1_ERR_BAD_SHAPE), a packed buffer 8 bytes off a
    16-byte boundary (DB1_ERR_BAD_ALIGN), a geometry the query refuses (DB1_ERR_UNSUPPORTED); the scratch and the outputs stay as they were"""
    from bdm_db1_amd import lib, ops
    c, Lb = case, lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    off8 = lambda t: ctypes.c_void_p(t.data_ptr() + 8)
    before = _launch(c, True, 9, _next_slot(), False)["words"]          # (the scratch now carries this launch's tag)
    sc = ops.decode_chain_scratch(c.dev)
    xn, qn = torch.full((1, D_), float("nan"), device=c.dev, dtype=BF), torch.full((1, 3 * D_), float("nan"), device=c.dev, dtype=BF)
    W = c.W8

    def call(slot=3, d=D_, **over):
        a = dict(part=P(c.parts[9]), x=P(c.x), o=P(W["o"]), w1=P(W["w1"]), b1=P(c.b1), w2=P(W["w2"]), b2=P(c.b2), qkv=P(W["qkv"]), o_next=P(W["o_next"]),
                 g1=P(c.g1), be1=P(c.be1), g2=P(c.g2), be2=P(c.be2), xn=P(xn), qn=P(qn), sc=P(sc))
        a.update(over)
        return Lb.db1_decode_chain_w8(a["part"], 9, d // 128, a["x"], a["o"], a["w1"], a["b1"], a["w2"], a["b2"], a["qkv"], a["o_next"], a["g1"], a["be1"], a["g2"],
                                      a["be2"], ALPHA, EPS, null, null, a["xn"], a["qn"], a["sc"], slot, d, DFF, null)
    for k in ("part", "x", "o", "w1", "b1", "w2", "b2", "g1", "be1", "g2", "be2", "sc", "xn", "qn"):
        assert call(**{k: null}) == BAD_SHAPE, k
    for k in ("o", "w1", "w2", "qkv", "o_next"):
        assert call(**{k: off8(W[k])}) == BAD_ALIGN, k
    assert call(slot=-1) == BAD_SHAPE and call(slot=65535) == BAD_SHAPE
    assert call(d=1024) == UNSUPPORTED and Lb.db1_decode_chain_w8_supported(1024, DFF, 8, 128, 9) == 0
    assert Lb.db1_decode_chain_w8_supported(D_, DFF, H, D, 13) == 0 and Lb.db1_decode_chain_w8_supported(D_, DFF, H, D, 12) == 1
    for args in ((D_, DFF, H, D, 1), (D_, DFF, H, D, 13), (1024, DFF, 8, 128, 9), (D_, 2048, H, D, 9), (D_, DFF, 32, 64, 9)):
        assert Lb.db1_decode_chain_w8_supported(*args) == Lb.db1_decode_chain_supported(*args), args
    torch.cuda.synchronize()
    assert torch.equal(sc[: (2 * D_ + DFF) * 4].view(torch.int32).cpu(), before) and not ops.decode_chain_error(c.dev)
    assert bool(torch.isnan(xn.float()).all()) and bool(torch.isnan(qn.float()).all())
