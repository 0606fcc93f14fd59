"""db1_relattn_decode_group_fwd on the device against the float64 closed form over every row's linearised window (tests/group_ring_rule.py;
the detection margins of the probe are proven on the CPU in test_group_ring_cpu.py).  H = 3, G in {1, 2}; every slot of both rings outside
the windows holds NaN; the output and the workspace are NaN-filled and guarded; the rings are guarded.  Per case: out within
attn_probe.tolerance per element, the appended slot bit-equal to the new K / V and every other byte of both rings unchanged, two launches
bit-equal, status 0."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_common import DEV, Guarded, _need_gpu, dev, host  # noqa: F401
import group_ring_rule as GR

pytestmark = pytest.mark.gpu
H, D = GR.H, GR.D


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


class _Call:
    """the operands of one launch on the device: rings by the rule (NaN elsewhere), guarded; NaN-filled guarded output and workspace"""

    def __init__(self, p, G, W, Lt, n_tail, sb, st, cap_b, cap_t, held=None):
        from bdm_db1_amd import lib
        self.p, self.G, self.W, self.M, self.Lt, self.cap_b, self.cap_t = p, G, W, G * W, Lt, cap_b, cap_t
        M, mlen = self.M, p["mlen"]
        # (``held``: the counters the rings are laid out by, where the launch is given others)
        base, tail = GR.rings(p, G, W, Lt, *(held or (n_tail, sb, st)), cap_b, cap_t)
        self.tail0 = tail
        self.base = Guarded(G * cap_b, 2 * H * D, "bf16", fill=base)
        self.tail = Guarded(M * cap_t, 2 * H * D, "bf16", fill=tail)
        self.base_before, self.tail_before = self.base.buf.clone(), self.tail.buf.clone()
        qkv = np.stack([p["q"][:, 0], p["k"][:, mlen], p["v"][:, mlen]], 1)[:, None]            # [M, 1, 3, H, D]
        self.qkv, self.u, self.vb, self.R = dev(qkv, "bf16"), dev(p["u"], "bf16"), dev(p["vb"], "bf16"), dev(p["R"], "bf16")
        self.out = Guarded(M, H * D, "bf16", fill=np.full((M, H * D), np.nan))
        self.ws_bytes = int(lib.load().db1_relattn_decode_group_workspace_bytes(G, W, mlen, Lt, H))
        self.ws = Guarded(1, self.ws_bytes // 4, "f32", fill=np.full((1, self.ws_bytes // 4), np.nan))
        self.state_b, self.state_t, self.n_tail, self.status = _i32([sb]), _i32([st]), _i32([n_tail]), _i32([0])

    def args(self, **kw):
        from bdm_db1_amd.ops import P, stream
        p = self.p
        a = dict(qkv=P(self.qkv), u=P(self.u), vb=P(self.vb), base=P(self.base.t), state_b=P(self.state_b), cap_b=self.cap_b, tail=P(self.tail.t),
                 state_t=P(self.state_t), cap_t=self.cap_t, n_tail=P(self.n_tail), Lt=self.Lt, R=P(self.R), nd=p["R"].shape[0], out=P(self.out.t),
                 G=self.G, W=self.W, mlen=p["mlen"], H=H, D=D, shift=p["shift"], scale=float(p["scale"]), status=P(self.status), ws=P(self.ws.t),
                 ws_bytes=self.ws_bytes, stream=stream())
        a.update(kw)
        return tuple(a.values())

    def launch(self, **kw):
        from bdm_db1_amd import lib
        lib.call("db1_relattn_decode_group_fwd", *self.args(**kw))
        torch.cuda.synchronize()
        return host(self.out.t).reshape(self.M, 1, H, D)

    def refill(self):
        self.out.t.fill_(float("nan"))
        self.ws.t.fill_(float("nan"))

    def guards(self, what):
        for g, name in ((self.out, "out"), (self.ws, "workspace"), (self.base, "base ring"), (self.tail, "tail ring")):
            g.intact(f"{what}: {name}")


def _check(G, W, mlen, Lt, n_tail, sb, st, shift):
    what = f"G={G} W={W} mlen={mlen} Lt={Lt} n_tail={n_tail} sb={sb} st={st} shift={shift}"
    cap_b, cap_t = GR.caps(mlen, Lt)
    p = GR.probe(G, W, H, mlen, shift, n_tail)
    ref, tol = GR.reference(p)
    c = _Call(p, G, W, Lt, n_tail, sb, st, cap_b, cap_t)
    got = c.launch()
    err = np.abs(got - ref)
    print(f"{what}: max err {np.nanmax(err):.3e}, tolerance {tol:.3e}")
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} outputs are not finite"
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} > {tol:.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    assert int(c.status.cpu()) == 0, what
    # the rings: the appended slot holds the new K / V bit for bit, nothing else changed
    want = dev(GR.expected_tail(p, c.tail0, W, Lt, st, cap_t).reshape(-1, 2 * H * D), "bf16")
    assert torch.equal(_bits(c.tail.t), _bits(want)), f"{what}: the tail ring is not (its image + the appended slot)"
    assert torch.equal(_bits(c.base.buf), _bits(c.base_before)), f"{what}: the base ring changed"
    c.guards(what)
    first = _bits(c.out.t).clone()
    c.refill()
    c.launch()
    assert torch.equal(_bits(c.out.t), first), f"{what}: two launches differ"
    return c, got


@pytest.mark.parametrize("W", GR.WS)
@pytest.mark.parametrize("Lt", GR.LTS)
@pytest.mark.parametrize("mlen", GR.MLENS)
def test_against_the_closed_form(mlen, Lt, W):
    for case in GR.cases(mlen, Lt, W):
        G, n_tail, sb, st, shift = case
        _check(G, W, mlen, Lt, n_tail, sb, st, shift)


@pytest.mark.parametrize("W", (3, 17))
def test_rows_with_the_same_query_and_tail_give_the_same_bits(W):
    G, mlen, Lt, n_tail, shift = 2, 129, 40, 33, 1
    cap_b, cap_t = GR.caps(mlen, Lt)
    p = GR.probe(G, W, H, mlen, shift, n_tail)
    first = np.arange(G * W) // W * W
    for name in ("q", "k", "v"):
        p[name] = p[name][first]                  # every row is its group's first row
    c = _Call(p, G, W, Lt, n_tail, 100, 40, cap_b, cap_t)
    c.launch()
    out = _bits(c.out.t).view(G, W, H * D)
    assert bool(torch.isfinite(c.out.t.float()).all())
    assert torch.equal(out, out[:, :1].expand(G, W, H * D)), "rows of a group differ"
    assert not torch.equal(out[0], out[1]), "the two groups should not agree"


@pytest.mark.parametrize("mlen,Lt,W,n_tail", [(160, 40, 4, 33), (129, 130, 17, 129), (33, 40, 3, 0)])
def test_against_the_per_row_ring_kernel(mlen, Lt, W, n_tail):
    """same maths, different partial-sum grouping: relative error below 1e-2 (the bound test_decode_gpu.py uses for that)"""
    from bdm_db1_amd import ops
    G, shift = 2, 1
    M = G * W
    cap_b, cap_t = GR.caps(mlen, Lt)
    p = GR.probe(G, W, H, mlen, shift, n_tail)
    c = _Call(p, G, W, Lt, n_tail, 37, cap_t - 1, cap_b, cap_t)
    got = c.launch()
    cap = mlen + 5
    ring = np.full((M, cap, 2, H, D), np.nan)
    rows = (3 + np.arange(mlen)) % cap
    ring[:, rows, 0], ring[:, rows, 1] = p["k"][:, :mlen], p["v"][:, :mlen]
    out = torch.full((M, 1, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.relattn_decode_ring_fwd(c.qkv, c.u, c.vb, dev(ring, "bf16"), _i32([3]), c.R, out, M, 1, mlen, H, D, shift, float(p["scale"]))
    want = host(out)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"mlen={mlen} Lt={Lt} W={W} n_tail={n_tail}: relative error against the ring kernel {err:.3e}")
    assert err < 1e-2


@pytest.mark.parametrize("bad", [dict(n_tail=-1), dict(n_tail=41), dict(n_tail=1000000), dict(sb=-3), dict(sb=1 << 30), dict(st=-1), dict(st=44),
                                 dict(n_tail=-5, sb=200, st=-(1 << 30))])
def test_out_of_range_counters_are_clamped_and_reported(bad):
    """the launch behaves as with the clamped values (so every access stays in bounds: the guards and the NaN slots would show one that
    does not) and sets the status bit"""
    G, W, mlen, Lt, shift = 2, 3, 96, 40, 1
    cap_b, cap_t = GR.caps(mlen, Lt)
    given = dict(n_tail=32, sb=20, st=7)
    given.update(bad)
    n_tail, sb, st, status = GR.clamp(given["n_tail"], given["sb"], given["st"], mlen, Lt, cap_b, cap_t)
    assert status == 1
    p = GR.probe(G, W, H, mlen, shift, n_tail)
    ref, tol = GR.reference(p)
    c = _Call(p, G, W, Lt, given["n_tail"], given["sb"], given["st"], cap_b, cap_t, held=(n_tail, sb, st))
    got = c.launch()
    assert int(c.status.cpu()) == 1
    assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all()
    want = dev(GR.expected_tail(p, c.tail0, W, Lt, st, cap_t).reshape(-1, 2 * H * D), "bf16")
    assert torch.equal(_bits(c.tail.t), _bits(want)) and torch.equal(_bits(c.base.buf), _bits(c.base_before))
    c.guards(str(bad))


def test_the_wrapper_gives_the_entry_points_bits_and_advance_counts():
    from bdm_db1_amd import ops
    G, W, mlen, Lt, n_tail, shift = 2, 4, 96, 40, 31, 0
    cap_b, cap_t = GR.caps(mlen, Lt)
    p = GR.probe(G, W, H, mlen, shift, n_tail)
    c = _Call(p, G, W, Lt, n_tail, 5, 9, cap_b, cap_t)
    c.launch()
    out = torch.full((G * W, 1, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.relattn_decode_group_fwd(c.qkv, c.u.view(-1), c.vb.view(-1), c.base.t.view(G, cap_b, 2, H, D), c.state_b, c.tail.t.view(G * W, cap_t, 2, H, D),
                                 c.state_t, c.n_tail, Lt, c.R, out, G, W, mlen, H, D, shift, float(p["scale"]), c.status)
    assert torch.equal(_bits(out).view(-1), _bits(c.out.t).view(-1)) and int(c.status.cpu()) == 0
    assert ops.relattn_decode_group_supported(G, W, mlen, Lt, cap_b, cap_t, H, D, torch.bfloat16)
    state, n = _i32([cap_t - 2]), _i32([38])
    seen = []
    for _ in range(4):
        ops.group_ring_advance(state, n, cap_t, Lt, mlen)
        seen.append((int(state.cpu()), int(n.cpu())))
    assert seen == [(cap_t - 1, 39), (0, 40), (1, 40), (2, 40)]


def test_refusals_launch_nothing():
    from bdm_db1_amd import lib
    G, W, mlen, Lt, n_tail, shift = 2, 3, 33, 40, 1, 1
    cap_b, cap_t = GR.caps(mlen, Lt)
    c = _Call(GR.probe(G, W, H, mlen, shift, n_tail), G, W, Lt, n_tail, 0, 0, cap_b, cap_t)
    null = ctypes.c_void_p(0)
    E = dict(shape=-1, align=-2, ws=-4, unsupported=-6)
    bad = [(dict(D=64), E["unsupported"]), (dict(W=0), E["unsupported"]), (dict(W=65), E["unsupported"]), (dict(mlen=2048), E["unsupported"]),
           (dict(mlen=0), E["unsupported"]), (dict(Lt=0), E["unsupported"]), (dict(Lt=4097), E["unsupported"]), (dict(cap_b=mlen - 1), E["unsupported"]),
           (dict(cap_t=Lt), E["unsupported"]), (dict(G=0), E["unsupported"]), (dict(H=0), E["unsupported"]),
           (dict(nd=0), E["shape"]), (dict(shift=-1), E["shape"]), (dict(out=null), E["shape"]), (dict(status=null), E["shape"]),
           (dict(n_tail=null), E["shape"]), (dict(base=null), E["shape"]), (dict(state_t=null), E["shape"]),
           (dict(qkv=type(null)(c.qkv.data_ptr() + 2)), E["align"]), (dict(tail=type(null)(c.tail.t.data_ptr() + 8)), E["align"]),
           (dict(ws_bytes=c.ws_bytes - 1), E["ws"]), (dict(ws=null), E["ws"])]
    fn = lib.load().db1_relattn_decode_group_fwd
    for kw, code in bad:
        assert fn(*c.args(**kw)) == code, (kw, code)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.tail.buf), _bits(c.tail_before)) and torch.equal(_bits(c.base.buf), _bits(c.base_before))
    assert bool(torch.isnan(c.out.t.float()).all()) and bool(torch.isnan(c.ws.t).all()) and int(c.status.cpu()) == 0
    assert not lib.load().db1_relattn_decode_group_supported(G, W, mlen, Lt, cap_b, cap_t, H, D, 0)       # fp32
