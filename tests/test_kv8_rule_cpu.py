"""The fp8 K/V ring format (include/db1_hip.h, "fp8 K/V ring") without a GPU: tests/kv8_rule.py against torch.float8_e4m3fn on every finite
bf16 value, the host-side ops.kv8_pack / kv8_unpack against it, the attention probes under it (exact at 1x .. 8x the canonical scale), the
proof that a wrong scale moves the closed form by at least ten tolerances, and the refusals of RingMemory and of ``kv_cache=``."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import attn_probe as A  # noqa: E402
import kv8_rule as K8  # noqa: E402

MARGIN = 10.0


class Reached(Exception):
    """the patched driver was reached: every check before the first launch has passed"""


def finite_bf16():
    """every finite bf16 value as float64, in the order of the bit patterns: 510 rows of 128 -- a row is one binade of one sign"""
    bits = np.arange(1 << 16, dtype=np.uint32)
    bits = bits[(bits & 0x7FFF) < 0x7F80]
    return (bits << 16).view(np.float32).astype(np.float64).reshape(-1, 128)


def torch_e4m3(y):
    return torch.from_numpy(np.asarray(y, np.float64)).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def smallest_scale(amax):
    """the definition, by search: the smallest power of two s >= 2^-126 with amax <= 448 s (1 for amax == 0)"""
    if amax == 0:
        return 1.0
    e = -126
    while amax > 448.0 * 2.0 ** e:
        e += 1
    return 2.0 ** e


@pytest.mark.parametrize("arrangement", ["binades", "strided"])
def test_rule_against_torch_float8_on_every_finite_bf16(arrangement):
    x = finite_bf16()
    if arrangement == "strided":                       # rows that mix all magnitudes: most elements underflow to +-0 under the row's scale
        x = np.ascontiguousarray(x.T.reshape(-1, 128))
    pay, s = K8.quantize(x)
    assert s.dtype == np.float32 and pay.dtype == np.uint8
    want_s = np.array([smallest_scale(a) for a in np.abs(x).max(-1)])
    assert np.array_equal(s.astype(np.float64), want_s)
    y = x / want_s[:, None]
    assert float(np.abs(y).max()) <= 448.0
    assert np.array_equal(pay, torch_e4m3(y))
    # dequantisation: payload * s, and the decode table is torch's
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.nan_to_num(K8.e4m3_value(np.arange(256)), nan=7.0), np.nan_to_num(table, nan=7.0))
    xh = K8.dequantize(pay, s)
    # exact in bf16 wherever it is a normal bf16; the rest: subnormal inputs, and the top eight values of the last binade (248 .. 255 steps
    # of 2^120 under the scale 2^120), which round up to 256 steps -- past the format
    normal = ((np.abs(xh) >= 2.0 ** -126) & (np.abs(xh) < 2.0 ** 128)) | (xh == 0)
    assert np.array_equal(A.bf16(xh[normal]), xh[normal])
    assert ((np.abs(x[~normal]) < 2.0 ** -126) | (np.abs(x[~normal]) >= 248 * 2.0 ** 120)).all()
    # the rounding is the only error: half a spacing of e4m3 at the block's scale (spacing 2^-9 s at the bottom, 2^5 s at the top)
    step = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -6))) - 3), 2.0 ** -9)
    assert (np.abs(xh - x) <= 0.5 * step * want_s[:, None]).all()


def test_amax_over_scale_on_random_rows():
    rng = np.random.default_rng(5)
    x = A.bf16(rng.standard_normal((4096, 128)) * np.exp2(rng.integers(-40, 40, (4096, 1))))
    _, s = K8.quantize(x)
    r = np.abs(x).max(-1) / s
    print(f"kv8 amax / s over 4096 random rows: min {r.min():.2f}, max {r.max():.2f}")
    assert (r > 224.0).all() and (r <= 448.0).all()


def test_zero_row_and_non_finite_elements():
    pay, s = K8.quantize(np.zeros((2, 128)))
    assert np.array_equal(s, np.ones(2, np.float32)) and not pay.any()
    z = np.zeros(128)
    z[3] = -0.0
    pay, s = K8.quantize(z)
    assert s == 1.0 and pay[3] == 0x80 and not np.delete(pay, 3).any()
    # the header's rule: a non-finite element is stored as 0x7f and takes no part in amax, so it reaches only its own block
    rng = np.random.default_rng(6)
    x = A.bf16(rng.standard_normal((3, 2, 2, 128)))
    clean_pay, clean_s = K8.quantize(x)
    bad = x.copy()
    bad[1, 0, 1, 5], bad[1, 0, 1, 77], bad[1, 0, 1, 100] = np.inf, -np.inf, np.nan
    pay, s = K8.quantize(bad)
    assert np.array_equal(s, clean_s)
    hit = np.zeros(x.shape, bool)
    hit[1, 0, 1, [5, 77, 100]] = True
    assert (pay[hit] == K8.NAN_BYTE).all() and np.array_equal(pay[~hit], clean_pay[~hit])
    back = K8.dequantize(pay, s)
    assert np.isnan(back[hit]).all() and np.isfinite(back[~hit]).all()
    allbad = np.full((1, 128), np.nan)
    pay, s = K8.quantize(allbad)
    assert s[0] == 1.0 and (pay == K8.NAN_BYTE).all()


def test_host_pack_and_unpack_are_the_rule_and_round_trip():
    from bdm_db1_amd import ops
    rng = np.random.default_rng(7)
    Hn = 4
    kv = A.bf16(rng.standard_normal((3, 5, 2, Hn, 128)) * np.exp2(rng.integers(-12, 12, (3, 5, 2, Hn, 1))))
    kv[0, 0, 1, 2] = 0.0
    kv[2, 4, 0, 1, 9] = np.inf
    slots = ops.kv8_pack(torch.from_numpy(kv).to(torch.bfloat16))
    assert slots.dtype == torch.uint8 and tuple(slots.shape) == (3, 5, K8.slot_bytes(Hn))
    assert np.array_equal(slots.numpy(), K8.pack(kv))
    pay, s = K8.unpack(slots.numpy(), Hn)
    rp, rs = K8.quantize(kv)
    assert np.array_equal(pay, rp) and np.array_equal(s, rs)
    deq, s_t = ops.kv8_unpack(slots, Hn)
    assert deq.dtype == torch.bfloat16 and np.array_equal(s_t.numpy(), rs)
    want = K8.dequantize(rp, rs)
    got = deq.to(torch.float64).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    # packing what was unpacked keeps every value (the NaN stays NaN); a scale may halve where the block's largest element rounded down to 224
    deq2, s2 = ops.kv8_unpack(ops.kv8_pack(deq), Hn)
    assert torch.equal(deq2.view(torch.int16), deq.view(torch.int16)) and bool(((s2 == s_t) | (2 * s2 == s_t)).all())
    # given scales: the same values under 4 x the canonical scale
    s4 = torch.from_numpy(rs * 4.0)
    again, s_back = ops.kv8_unpack(ops.kv8_pack(torch.from_numpy(kv), scales=s4), Hn)
    assert torch.equal(s_back, s4) and np.array_equal(ops.kv8_pack(torch.from_numpy(kv), scales=s4).numpy(), K8.pack(kv, rs * 4.0))
    with pytest.raises(ValueError):
        ops.kv8_pack(torch.from_numpy(kv), scales=torch.from_numpy(rs / 4.0))         # |x / s| > 448
    for bad in (rs * 3.0, rs * 0.0, -rs, rs * 2.0 ** -140):                           # no power of two; zero; negative; below the normal fp32
        with pytest.raises(ValueError):
            ops.kv8_pack(torch.from_numpy(kv), scales=torch.from_numpy(bad.astype(np.float64)))
    with pytest.raises(ValueError):
        ops.kv8_pack(torch.zeros(2, 3, 128))                                          # an odd number of heads
    with pytest.raises(ValueError):
        ops.kv8_unpack(slots, Hn + 2)
    assert ops.kv8_slot_bytes(16, 128) == 4224 and ops.kv8_slot_bytes(3, 128) == 0 and ops.kv8_slot_bytes(2, 64) == 0


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_probes_are_exact_under_the_rule(q, mlen, shift, nd):
    p, _ = A.build(q, mlen, shift, nd)
    kv = np.stack([p["k"], p["v"]], axis=2)                                 # [B, klen, 2, H, D]
    pay, s = K8.quantize(kv)
    assert np.array_equal(s[:, :, 0], np.full(s[:, :, 0].shape, K8.K_CANON, np.float32))
    assert np.array_equal(s[:, :, 1], np.full(s[:, :, 1].shape, K8.V_CANON, np.float32))
    for mult in (1.0, 2.0, 4.0, 8.0):
        pm, sm = K8.quantize(kv, s * mult)
        assert np.array_equal(K8.dequantize(pm, sm), kv), mult


def scale_mutant_separations(q, mlen, shift, nd):
    """{(cap, start, mutant): max|mutant - reference| / tolerance over ``out``}; the reference seen through the crafted ring must be the
    probe itself"""
    p, _ = A.build(q, mlen, shift, nd)
    ref, _ = A.forward(p)
    tol = A.tolerances(ref, A.forward(p, rounded=True)[0])["out"]
    seps = {}
    for cap in A.ring_caps(q, mlen):
        scales = K8.crafted_scales(cap)
        for start in A.ring_origins(q, mlen, cap):
            ring0 = A.ring_initial(p, cap, start)
            seen = K8.ring_seen(p, ring0, scales, start)
            assert np.array_equal(seen["k"], p["k"]) and np.array_equal(seen["v"], p["v"])
            for m in K8.SCALE_MUTANTS:
                out = A.forward(K8.ring_seen(p, ring0, scales, start, m))[0]["out"]
                seps[(cap, start, m)] = float(np.abs(out - ref["out"]).max() / tol)
    return seps


def test_crafted_scales_differ_between_neighbours():
    for cap in (1, 2, 7, 33, 364):
        m = K8.crafted_multipliers(cap)
        assert set(np.unique(m)) <= {1.0, 2.0, 4.0, 8.0}
        assert (m != np.roll(m, -1, axis=3)).all()
        if cap > 1:
            assert (m != np.roll(m, -1, axis=1)).all()
        s = K8.crafted_scales(cap)
        assert (s[:, :, 0] != s[:, :, 1]).all()
    assert len(np.unique(K8.crafted_multipliers(364))) == 4


@pytest.mark.parametrize("q,mlen,shift,nd", A.DECODE_CASES)
def test_a_wrong_scale_moves_the_output_by_ten_tolerances(q, mlen, shift, nd):
    if mlen == 0:
        # no memory rows: nothing is read from the ring, so no scale mutant is applicable (the append's scales are checked byte for byte
        # on the ring image by the device test)
        p, _ = A.build(q, mlen, shift, nd)
        for cap in A.ring_caps(q, mlen):
            for m in K8.SCALE_MUTANTS:
                seen = K8.ring_seen(p, A.ring_initial(p, cap, 0), K8.crafted_scales(cap), 0, m)
                assert np.array_equal(seen["k"], p["k"]) and np.array_equal(seen["v"], p["v"])
        print(f"kv8 scale mutants {(q, mlen, shift, nd)}: not applicable (no memory rows)")
        return
    seps = scale_mutant_separations(q, mlen, shift, nd)
    worst = min(seps, key=seps.get)
    print(f"kv8 scale mutants {(q, mlen, shift, nd)}: smallest separation {seps[worst]:.1f} tolerances at {worst}")
    assert seps[worst] >= MARGIN, (worst, seps[worst])


# ------------------------------------------------------------------------------------------------------------------------- the host layer
def _text(n, rows=1):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.zeros(rows, n, dtype=torch.long),
                        text_len=None)


@pytest.fixture
def no_launch(monkeypatch):
    """a library in which any launch, prefill or generator fails the test"""
    from bdm_db1_amd import generation, lib, serving
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    seen = {}

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")

    def decode(model, prompt, State, key, *a, **k):
        seen["key"] = key
        raise Reached

    def stream(model, reqs, key, *a, **k):
        seen["key"] = key
        return iter(())

    monkeypatch.setattr(lib, "call", boom)
    for mod in (generation, serving):
        monkeypatch.setattr(mod, "_prefill", boom)
        monkeypatch.setattr(mod, "_ring_generator", boom)
    monkeypatch.setattr(generation, "_decode", decode)
    monkeypatch.setattr(serving, "_stream", stream)
    return seen


def fake_model(**kw):
    base = dict(mem_len=40, compute_dtype=torch.bfloat16, use_decode=True, d_head=128, n_head=2, total_vocab_size=33025, text_vocab_size=32000)
    return SimpleNamespace(**{**base, **kw})


def test_decode_key_default_is_what_it_was(no_launch):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search, generate, generate_stream, sample_best_of
    from bdm_db1_amd.generation import DecodeKey, DecodeKeyFp8, _with_kv_cache
    model, seen = fake_model(), no_launch
    cfg = GenerationConfig(max_new_tokens=8)
    plain = DecodeKey(rows=1, cfg=cfg, V=33025, hi=33025)
    assert plain.kv_cache == "bf16" and _with_kv_cache("t", model, plain, "bf16") is plain
    fp8 = _with_kv_cache("t", model, plain, "fp8")
    assert type(fp8) is DecodeKeyFp8 and fp8.kv_cache == "fp8" and [f.name for f in dataclasses.fields(fp8)][-1] == "kv_cache"
    assert all(getattr(fp8, f.name) == getattr(plain, f.name) for f in dataclasses.fields(plain))
    assert fp8 != plain and plain != fp8 and fp8 == _with_kv_cache("t", model, plain, "fp8") and len({fp8, plain}) == 2
    assert dataclasses.replace(fp8, caps=(1, 2)).kv_cache == "fp8"
    # the public entry points: without the keyword and with the default the key is the plain one; "fp8" gives the other class
    calls = ((generate, (cfg,), {}), (beam_search, (BeamSearchConfig(max_new_tokens=8, num_beams=2),), {}),
             (sample_best_of, (GenerationConfig(max_new_tokens=8, greedy=False), 2), {}), (generate_stream, (cfg,), {}))
    for fn, args, kw in calls:
        prompt = [_text(4)] if fn is generate_stream else _text(4)

        def run(**more):
            if fn is generate_stream:
                fn(model, prompt, *args, **kw, **more)
            else:
                with pytest.raises(Reached):
                    fn(model, prompt, *args, **kw, **more)
            return seen.pop("key")

        k0 = run()
        seen["key"] = run(kv_cache="bf16")
        assert seen["key"] == k0 and type(seen["key"]) is DecodeKey, fn.__name__
        seen["key"] = run(kv_cache="fp8")
        assert type(seen["key"]) is DecodeKeyFp8 and seen["key"] != k0, fn.__name__
        assert all(getattr(seen["key"], f.name) == getattr(k0, f.name) for f in dataclasses.fields(k0)), fn.__name__


def test_kv_cache_refusals_come_before_a_launch(no_launch):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search, generate, generate_many, generate_stream, sample_best_of
    cfg = GenerationConfig(max_new_tokens=8)
    calls = ((generate, (cfg,)), (beam_search, (BeamSearchConfig(max_new_tokens=8, num_beams=2),)),
             (sample_best_of, (GenerationConfig(max_new_tokens=8, greedy=False), 2)))
    for fn, args in calls:
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(), _text(4), *args, kv_cache="int8")
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(compute_dtype=torch.float32), _text(4), *args, kv_cache="fp8")        # an fp32 model: no ring path
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(), _text(4), *args, kv_cache="fp8", graphed=False)                    # the eager list-form loop
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(n_head=3), _text(4), *args, kv_cache="fp8")                           # a slot that is no multiple of 16 bytes
    for fn in (generate_stream, generate_many):
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(), [_text(4)], cfg, kv_cache="e5m2")
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(n_head=3), [_text(4)], cfg, kv_cache="fp8")
        with pytest.raises(ValueError, match="kv_cache"):
            fn(fake_model(mem_len=2048), [_text(4)], cfg, kv_cache="fp8")                       # klen beyond the attention's 2048 keys


def test_ring_memory_refusals_come_before_an_allocation():
    from bdm_db1_amd import lib
    from bdm_db1_amd.decode import RingMemory
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    # (the fake model has no device: anything past the checks would raise AttributeError, not ValueError)
    for kw, dtype in ((dict(), "int8"), (dict(), "fp16"), (dict(n_head=3), "fp8"), (dict(d_head=64), "fp8"), (dict(mem_len=2048), "fp8"),
                      (dict(compute_dtype=torch.float32), "fp8"), (dict(compute_dtype=torch.float32), "bf16")):
        with pytest.raises(ValueError):
            RingMemory(fake_model(n_layer=2, **kw), 2, kv_dtype=dtype)
