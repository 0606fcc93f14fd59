"""The grouped K/V ring without a GPU: the rule of tests/group_ring_rule.py against a second formulation (np.roll and concatenation), the
proof that the probe data of test_group_ring_kernels_gpu.py shows every one-off index error by at least ten tolerances, the prototypes,
and the host refusals of ops and of share_prompt."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probe as AP  # noqa: E402
import group_ring_rule as GR  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ the rule, twice
def _materialised(base, tail, W, mlen, Lt, n_tail, sb, st):
    """every row's window the long way: roll both rings to their origins, take the base window and the last n_tail keys of the tail
    window, concatenate, keep the last mlen"""
    M = tail.shape[0]
    rows = []
    for r in range(M):
        bwin = np.roll(base[r // W], -sb, axis=0)[:mlen]
        twin = np.roll(tail[r], -st, axis=0)[:Lt]
        rows.append(np.concatenate([bwin, twin[Lt - n_tail:]])[-mlen:])
    return np.stack(rows)


@pytest.mark.parametrize("W", (1, 3, 16, 17))
@pytest.mark.parametrize("mlen,Lt,cap_b,cap_t", [(33, 40, 40, 41), (96, 40, 160, 47), (31, 130, 31, 135)])
def test_rule_against_roll_and_concatenate(W, mlen, Lt, cap_b, cap_t):
    assert cap_b != cap_t
    G = 2
    M = G * W
    base = np.arange(G * cap_b).reshape(G, cap_b) + 1
    tail = -(np.arange(M * cap_t).reshape(M, cap_t) + 1)
    for n_tail in sorted({0, 1, min(Lt, mlen)}):
        for sb in (0, cap_b - 1, cap_b - mlen // 2, 5):
            for st in (0, cap_t - 1, cap_t - Lt // 2, 3):
                is_tail, row, slot = GR.sources(G, W, mlen, Lt, n_tail, sb, st, cap_b, cap_t)
                got = np.where(is_tail, tail[np.where(is_tail, row, 0), np.where(is_tail, slot, 0)], base[np.where(is_tail, 0, row), np.where(is_tail, 0, slot)])
                assert np.array_equal(got, _materialised(base, tail, W, mlen, Lt, n_tail, sb, st)), (n_tail, sb, st)
                # the append: the slot behind the tail window, i.e. position Lt of the rolled ring
                img = tail.copy()
                img[:, GR.append_slot(st, Lt, cap_t)] = 0
                assert (np.roll(img, -st, axis=1)[:, Lt] == 0).all() and (img != tail).sum() == M
                assert (sb + n_tail + mlen - n_tail - 1 >= cap_b) == bool((slot[~is_tail] < sb).any()) or n_tail == mlen


def test_clamp():
    assert GR.clamp(3, 5, 7, 96, 40, 103, 44) == (3, 5, 7, 0)
    assert GR.clamp(41, 5, 7, 96, 40, 103, 44) == (40, 5, 7, 1)
    assert GR.clamp(35, 5, 7, 31, 40, 38, 44) == (31, 5, 7, 1)
    assert GR.clamp(-1, 103, -2, 96, 40, 103, 44) == (0, 102, 0, 1)
    assert GR.clamp(0, 0, 44, 96, 40, 103, 44) == (0, 0, 43, 1)


# ------------------------------------------------------------------------------------------------------------------ detection margins
def _separations(mlen, Lt):
    """{mutant: the smallest max|out(mutant) - out| / tolerance over the cases of (mlen, Lt) where it applies}"""
    worst = {}
    cap_b, cap_t = GR.caps(mlen, Lt)
    guard = np.full((2 * max(cap_b, cap_t), 2, GR.H, GR.D), 0.375)
    for W in GR.WS:
        for G, n_tail, sb, st, shift in GR.cases(mlen, Lt, W):
            p = GR.probe(G, W, GR.H, mlen, shift, n_tail)
            ref, tol = GR.reference(p)
            base, tail = GR.rings(p, G, W, Lt, n_tail, sb, st, cap_b, cap_t, filler="values")
            same = GR.seen(p, base, tail, GR.sources(G, W, mlen, Lt, n_tail, sb, st, cap_b, cap_t), guard)
            assert np.array_equal(same["k"], p["k"]) and np.array_equal(same["v"], p["v"])       # the rule reads back what it laid out
            for m in GR.MUTANTS + GR.DIST_MUTANTS:
                if not GR.applicable(m, G, W, mlen, Lt, n_tail, sb, st, shift):
                    continue
                if m in GR.DIST_MUTANTS:
                    out = AP.forward(p, AP.mutate_geometry(m, 1, mlen + 1, mlen, shift, mlen + 1))[0]["out"]
                else:
                    out = AP.forward(GR.seen(p, base, tail, GR.sources(G, W, mlen, Lt, n_tail, sb, st, cap_b, cap_t, m), guard))[0]["out"]
                worst[m] = min(worst.get(m, np.inf), float(np.abs(out - ref).max() / tol))
    return worst


@pytest.mark.parametrize("Lt", GR.LTS)
@pytest.mark.parametrize("mlen", GR.MLENS)
def test_every_index_error_moves_the_output_by_ten_tolerances(mlen, Lt):
    """a seam off by one in either direction, r % W in place of r / W, a tail origin off by one, a dropped wrap on either ring, a distance
    off by one -- on the probe data of the GPU test"""
    worst = _separations(mlen, Lt)
    print(mlen, Lt, {k: round(v, 1) for k, v in worst.items()})
    assert all(v >= 10.0 for v in worst.values()), worst


def test_every_mutant_and_every_axis_value_is_met():
    hit = {m: 0 for m in GR.MUTANTS}
    seen = dict(G=set(), shift=set(), sb=set(), st=set(), n=set())
    for mlen in GR.MLENS:
        for Lt in GR.LTS:
            per = dict(G=set(), shift=set(), sb=set(), st=set())
            for W in GR.WS:
                for G, n_tail, sb, st, shift in GR.cases(mlen, Lt, W):
                    assert 0 <= n_tail <= min(Lt, mlen) and 0 <= sb < GR.caps(mlen, Lt)[0] and 0 <= st < GR.caps(mlen, Lt)[1]
                    for m in GR.MUTANTS:
                        hit[m] += GR.applicable(m, G, W, mlen, Lt, n_tail, sb, st, shift)
                    per["G"].add(G); per["shift"].add(shift)
                    per["sb"].add(GR.base_origins(mlen, Lt).index(sb)); per["st"].add(GR.tail_origins(mlen, Lt).index(st))
                    seen["n"].add(n_tail)
            assert per == dict(G={1, 2}, shift={0, 1}, sb={0, 1, 2}, st={0, 1, 2}), (mlen, Lt, per)
            assert set(GR.n_tails(mlen, Lt)) >= {0, 1, min(Lt, mlen)}
    assert all(n > 0 for n in hit.values()), hit
    assert seen["n"] >= {0, 1, 31, 32, 33, 40, 96, 129, 130}


# ------------------------------------------------------------------------------------------------------------------ prototypes, refusals
def test_prototypes_are_declared():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for s in ("db1_relattn_decode_group_supported", "db1_relattn_decode_group_workspace_bytes", "db1_relattn_decode_group_fwd", "db1_group_ring_advance"):
        assert s in names, s
    restype, argtypes = lib.parse_header()["db1_relattn_decode_group_fwd"]
    assert len(argtypes) == 25


def _operands(G=2, W=3, mlen=33, Lt=40, H=2, D=128, cap_b=40, cap_t=44, nd=34):
    bf, i32 = torch.bfloat16, torch.int32
    M = G * W
    z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt)
    one = lambda: z(1, dt=i32)
    return dict(qkv_new=z(M, 1, 3, H, D), u=z(H, D), vb=z(H, D), base=z(G, cap_b, 2, H, D), state_b=one(), tail=z(M, cap_t, 2, H, D), state_t=one(),
                n_tail=one(), Lt=Lt, R=z(nd, H, D), out=z(M, 1, H, D), G=G, W=W, mlen=mlen, H=H, D=D, shift=1, scale=0.1, status=one())


def test_ops_refuses_on_the_host_before_the_library_is_called(monkeypatch):
    from bdm_db1_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    good = _operands()
    f32 = lambda t: t.float()
    bad = [dict(D=64), dict(W=0), dict(W=65), dict(G=0), dict(mlen=0), dict(mlen=2048), dict(Lt=0), dict(Lt=4097), dict(shift=-1),
           dict(base=good["base"][:, :32]), dict(tail=good["tail"][:, :40]), dict(base=f32(good["base"])), dict(tail=good["tail"][:5]),
           dict(base=good["base"][:1]), dict(base=good["base"].transpose(0, 1)), dict(qkv_new=good["qkv_new"][:5]), dict(qkv_new=f32(good["qkv_new"])),
           dict(out=good["out"][:5]), dict(out=f32(good["out"])), dict(u=good["u"][:1]), dict(vb=f32(good["vb"])), dict(R=good["R"][:0]),
           dict(R=good["R"][:, :1]), dict(R=f32(good["R"])), dict(state_b=good["state_b"].long()), dict(state_t=torch.zeros(2, dtype=torch.int32)),
           dict(n_tail=torch.zeros(1)), dict(status=torch.zeros(0, dtype=torch.int32)),
           dict(qkv_new=torch.zeros(6 * 3 * 2 * 128 + 1, dtype=torch.bfloat16)[1:])]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match="relattn_decode_group_fwd"):
            ops.relattn_decode_group_fwd(**args)


def _fake_model(**kw):
    m = dict(compute_dtype=torch.bfloat16, use_decode=True, mem_len=40, d_head=128, n_head=2)
    m.update(kw)
    return SimpleNamespace(**m)


def test_share_prompt_refusals_and_keys(monkeypatch):
    from bdm_db1_amd import generation as gen, ops
    cfg = gen.BeamSearchConfig(num_beams=4, max_new_tokens=6)
    key = gen.DecodeKey(rows=2, cfg=cfg, V=100, hi=100)
    asked = []
    monkeypatch.setattr(ops, "relattn_decode_group_supported", lambda *a: asked.append(a) or True)
    ok = lambda **kw: gen._with_share_prompt("beam_search", kw.pop("model", _fake_model()), kw.pop("key", key), kw.pop("share", True), kw.pop("W", 4),
                                             kw.pop("prompt", None), kw.pop("kv_cache", "bf16"), kw.pop("graphed", None))
    # off: the key itself, whatever else is asked for; equal to a key built without the keyword in mind
    assert ok(share=False, graphed=False, kv_cache="fp8", model=_fake_model(compute_dtype=torch.float32)) is key and not asked
    assert key == gen.DecodeKey(rows=2, cfg=cfg, V=100, hi=100) and key.share_prompt is False
    assert [f.name for f in dataclasses.fields(key)] == ["rows", "cfg", "V", "hi", "constraints", "n", "per_request", "caps"]
    # on: a key of another class with the same fields and the flag last
    shared = ok()
    assert isinstance(shared, gen.DecodeKeyShared) and shared.share_prompt is True and shared != key and shared == ok()
    assert all(getattr(shared, f.name) == getattr(key, f.name) for f in dataclasses.fields(key))
    assert asked[0][:4] == (2, 4, 40, 6)
    cache = object.__new__(gen.PrefixCache)
    prefixed = object.__new__(gen.Prefixed)
    for kw, what in ((dict(model=_fake_model(compute_dtype=torch.float32)), "bf16 model"), (dict(model=_fake_model(use_decode=False)), "bf16 model"),
                     (dict(graphed=False), "graphed=False"), (dict(kv_cache="fp8"), "kv_cache"), (dict(prompt=prefixed), "Prefixed"),
                     (dict(key=dataclasses.replace(key, cfg=dataclasses.replace(cfg, max_new_tokens=41))), "mem_len"),
                     (dict(key=dataclasses.replace(key, rows=1), W=1), "G = W = 1")):
        n = len(asked)
        with pytest.raises(ValueError, match=what):
            ok(**kw)
        assert len(asked) == n          # (refused before the library's query)
    monkeypatch.setattr(ops, "relattn_decode_group_supported", lambda *a: False)
    with pytest.raises(ValueError, match="not supported for this model"):
        ok(W=4)
    del cache
