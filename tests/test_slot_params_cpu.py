"""Per-request sampling parameters without a GPU: the slot record's layout (ops.pack_slot_params against tests/slot_params_rule.py), what
``SamplingParams.resolve`` inherits and refuses, the request formats of a ``per_request`` stream, and the new entry point's prototype and
export."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import slot_params_rule as S  # noqa: E402

V, HI = 33025, 32000


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_pack_round_trips_through_the_rule():
    from bdm_db1_amd import ops
    for kw in (dict(greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=0, vocab_lo=0, vocab_hi=V),
               dict(greedy=False, temperature=0.8, top_k=50, top_p=0.9, seed=(1 << 40) + 12345, vocab_lo=1000, vocab_hi=3000),
               dict(greedy=False, temperature=3.0, top_k=1, top_p=0.25, seed=2 ** 64 - 1, vocab_lo=32000, vocab_hi=V)):
        rec = ops.pack_slot_params(**kw)
        assert rec.dtype == np.int32 and rec.shape == (ops.SLOT_PARAM_WORDS,) == (S.WORDS,)
        p = S.unpack(rec)
        for k in ("greedy", "top_k", "vocab_lo", "vocab_hi", "seed"):
            assert p[k] == kw[k], k
        assert p["top_p"] == np.float32(kw["top_p"])
        assert p["inv_temperature"] == (np.float32(1) if kw["greedy"] else np.float32(1) / np.float32(kw["temperature"]))
        assert not S.invalid(rec, V)
    # the words, one by one
    rec = ops.pack_slot_params(False, 0.5, 7, 0.75, (5 << 32) | 9, 11, 13)
    assert rec.tolist() == [0, 7, 11, 13, 9, 5, _bits(2.0), _bits(0.75)]
    assert ops.pack_slot_params(True, 0.0, 0, 1.0, 0, 0, 4)[0] == 1            # (greedy: the temperature is not divided by)


@pytest.mark.parametrize("T", [0.7, 3.0, 0.8, 1.0, 1e-3, 123.456])
def test_word_6_is_one_fp32_division(T):
    from bdm_db1_amd import ops
    rec = ops.pack_slot_params(False, T, 0, 1.0, 0, 0, V)
    want = np.float32(1) / np.float32(T)
    assert int(rec.view(np.uint32)[6]) == int(want.view(np.uint32))
    if T in (0.7, 3.0):      # (the cases where a float64 reciprocal rounded once, or a product, could differ: pin the bits themselves)
        assert int(rec.view(np.uint32)[6]) == {0.7: 0x3FB6DB6E, 3.0: 0x3EAAAAAB}[T]


def test_seeds_above_2_32_split_into_two_words():
    from bdm_db1_amd import ops
    for seed in (0, 1, 2 ** 32 - 1, 2 ** 32, (1 << 40) + 12345, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1):
        u = ops.pack_slot_params(False, 1.0, 0, 1.0, seed, 0, V).view(np.uint32)
        assert int(u[4]) == seed & 0xFFFFFFFF and int(u[5]) == seed >> 32
        assert S.unpack(u.view(np.int32))["seed"] == seed


def test_the_guard_of_the_rule():
    from bdm_db1_amd import ops
    ok = dict(greedy=False, temperature=0.8, top_k=5, top_p=0.9, seed=3, vocab_lo=0, vocab_hi=HI)
    pack = lambda **kw: ops.pack_slot_params(**{**ok, **kw})
    assert not S.invalid(pack(), V)
    for kw in (dict(vocab_lo=5, vocab_hi=5), dict(vocab_lo=9, vocab_hi=5), dict(vocab_hi=V + 1), dict(vocab_lo=-1), dict(top_p=0.0),
               dict(top_p=1.5), dict(top_p=float("nan")), dict(top_k=-1), dict(temperature=float("inf")), dict(temperature=float("nan")),
               dict(temperature=-2.0)):
        assert S.invalid(pack(**kw), V), kw
    rec = pack()
    rec[6] = 0                                                          # inv_temperature = 0.0
    assert S.invalid(rec, V)
    # a greedy slot: words 1 and 4 .. 7 are not looked at, the window still is
    g = pack(greedy=True)
    g[1], g[4:] = -5, np.array([-1, -1, 0x7FC00000, 0], np.int32)
    assert not S.invalid(g, V)
    g[3] = V + 1
    assert S.invalid(g, V)
    # and the rule's selection: an invalid record -> bit 2 and no token; an all-NaN window -> bit 0
    l = np.arange(V, dtype=np.float64) % 17
    assert S.select_slot(l, pack(top_p=0.0), V, 0, 0) == (S.BAD_PARAMS, None)
    assert S.select_slot(l, pack(greedy=True, vocab_lo=20, vocab_hi=30), V, 0, 0) == (0, 29)
    assert S.select_slot(np.full(V, np.nan), pack(greedy=True), V, 0, 0) == (1, -1)
    st, tok = S.select_slot(l, pack(vocab_lo=1000, vocab_hi=3000), V, 7, 2)
    assert st == 0 and 1000 <= tok < 3000
    got = S.step_slots(np.stack([l, l, l]), [2, 0, 5], np.stack([pack(greedy=True, vocab_lo=0, vocab_hi=5), pack(), pack(top_k=-1)]),
                       [0, 1, 0], [4, 1, 4], [0, 0, 0], [0, 1, 2], V)
    assert got == {2: (S.BAD_PARAMS, None), 0: (0, 4)}                  # slot 1 is not served, slot 5 does not exist; slot s reads params[s]


def test_resolve_inherits_and_refuses():
    from bdm_db1_amd import GenerationConfig, SamplingParams
    import dataclasses
    cfg = GenerationConfig(greedy=False, temperature=0.7, top_k=40, top_p=0.9, seed=3, vocab_lo=10)
    assert SamplingParams().resolve(cfg, V, HI) == dict(greedy=False, temperature=0.7, top_k=40, top_p=0.9, seed=3, vocab_lo=10, vocab_hi=HI)
    got = SamplingParams(greedy=True, vocab_lo=1000, vocab_hi=3000).resolve(cfg, V, HI)
    assert got["greedy"] is True and (got["vocab_lo"], got["vocab_hi"]) == (1000, 3000) and got["top_k"] == 40
    got = SamplingParams(temperature=2.0, top_k=0, top_p=1.0, seed=2 ** 64 - 1, vocab_hi=V).resolve(cfg, V, HI)
    assert got == dict(greedy=False, temperature=2.0, top_k=0, top_p=1.0, seed=2 ** 64 - 1, vocab_lo=10, vocab_hi=V)
    with pytest.raises(dataclasses.FrozenInstanceError):
        SamplingParams().greedy = True
    assert SamplingParams(top_k=3) == SamplingParams(top_k=3) and hash(SamplingParams()) == hash(SamplingParams())
    g = GenerationConfig()
    for p in (SamplingParams(vocab_lo=5, vocab_hi=5), SamplingParams(vocab_lo=HI), SamplingParams(vocab_hi=V + 1), SamplingParams(vocab_lo=-1),
              SamplingParams(top_p=0.0), SamplingParams(top_p=1.5), SamplingParams(greedy=False, temperature=0.0),
              SamplingParams(greedy=False, temperature=float("inf")), SamplingParams(top_k=-1), SamplingParams(seed=2 ** 64),
              SamplingParams(seed=-1)):
        with pytest.raises(ValueError):
            p.resolve(g, V, HI)
    assert SamplingParams(temperature=0.0).resolve(g, V, HI)["greedy"] is True          # (greedy: the temperature is unused, as in the config)


def _text(n, rows=1):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.zeros(rows, n, dtype=torch.long),
                        text_len=None)


def test_requests_take_params_only_with_the_flag():
    from bdm_db1_amd import GenerationConfig, SamplingParams
    from bdm_db1_amd.serving import _Item, _requests
    cfg = GenerationConfig(max_new_tokens=8)
    sp = SamplingParams(greedy=False, top_p=0.9)
    items = [_text(4), (_text(5), 3), (_text(6, rows=2), None, sp), (_text(4), 2, None), _Item(_text(3), [9], 5, sp)]
    reqs = list(_requests(items, cfg, per_request=True, window=(V, HI)))
    assert [r.index for r in reqs] == [0, 1, 2, 3, 4, 9]
    assert [r.limit for r in reqs] == [8, 3, 8, 8, 2, 5]
    assert [r.params for r in reqs] == [None, None, sp, sp, None, sp]
    # the flag off: the formats of before, and params are refused wherever they sit
    assert [r.params for r in _requests(items[:2], cfg)] == [None, None]
    for bad in ((_text(4), 2, sp), _Item(_text(3), [0], 5, sp), (_text(4), None, sp)):
        with pytest.raises(ValueError, match="per_request"):
            list(_requests([bad], cfg))
    with pytest.raises(ValueError):
        list(_requests([(_text(4), 2, None)], cfg))                     # (a 3-tuple is not a request of a stream without the flag)
    for flag in (False, True):
        with pytest.raises(ValueError):
            list(_requests([(_text(4), 2, sp, None)], cfg, per_request=flag))
        with pytest.raises(ValueError):
            list(_requests([(_text(4),)], cfg, per_request=flag))
    with pytest.raises(ValueError):
        list(_requests([(_text(4), 2, dict(greedy=True))], cfg, per_request=True))
    with pytest.raises(ValueError):                                     # params that do not resolve are refused where the list is checked
        list(_requests([(_text(4), 2, SamplingParams(vocab_hi=V + 1))], cfg, per_request=True, window=(V, HI)))
    with pytest.raises(ValueError):                                     # a limit below the constraints' minimum, flag or not
        list(_requests([(_text(4), 2, sp)], cfg, 3, per_request=True, window=(V, HI)))
    with pytest.raises(ValueError):
        list(_requests([(_text(4), 9, sp)], cfg, per_request=True))


def test_stream_wrappers_split_their_items():
    from bdm_db1_amd import SamplingParams
    from bdm_db1_amd.serving import _split
    sp = SamplingParams(top_k=3)
    assert _split("b") == ("b", None, ()) and _split(("b", 4)) == ("b", 4, ()) and _split(("b", None, sp)) == ("b", None, (sp,))
    with pytest.raises(ValueError):
        _split(("b",))


def test_the_new_symbol_is_declared_and_exported():
    from bdm_db1_amd import lib
    protos = lib.parse_header()
    ret, args = protos["db1_select_tokens_slots_per"]
    top = protos["db1_select_tokens_slots_top"][1]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    # (logits, M, V, ld, dt), params, then the slot form's arguments from eos_id on: the six sampling scalars and the window are gone
    assert ret is ci and args[:5] == top[:5] and args[5] is vp and args[6:] == top[13:] and len(args) == len(top) - 7
    assert not [n for n in protos if "_per_supported" in n or "_per_workspace_bytes" in n]
    assert "db1_select_tokens_slots_per" in lib.declared_symbols()
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    assert getattr(ctypes.CDLL(lib.LIB_PATH), "db1_select_tokens_slots_per") is not None
