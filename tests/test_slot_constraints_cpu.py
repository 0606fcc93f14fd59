"""Per-request decoding constraints without a GPU: the layout ``ops.pack_slot_constraints`` writes (against tests/slot_constraints_rule.py),
every refusal of a ``per_request_constraints`` stream before any launch, the request forms, the flag-off request path and cache key being
what they were, the prototypes, and the per-slot rule against the scalar rules slot by slot on seeded cases."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import constraint_rule as C  # noqa: E402
import penalty_rule as P  # noqa: E402
import slot_constraints_rule as Q  # noqa: E402
import stop_rule as R  # noqa: E402

V = 33025


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------- packing
def test_pack_layout_bits_and_fill():
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import ops
    c = D(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5, bad_token_ids=(7, 9, V + 2), frequency_penalty=0.25,
          presence_penalty=-0.5, logit_bias={11: 1.5, 4: -2.0}, stop_sequences=((1, 2, 3), (8,)))
    rec, bad, bi, bv, tok, n = ops.pack_slot_constraints(c, 2, 5, 4)
    assert rec.dtype == np.int32 and rec.shape == (ops.SLOT_CONS_WORDS,) == (Q.WORDS,) and ops.MAX_SLOT_LIST == Q.MAX_CAP == 1024
    inv = np.float32(1) / np.float32(1.3)
    assert rec.tolist() == [_bits(1.3), _bits(inv), 3, 5, _bits(0.25), _bits(-0.5) - (1 << 32), 3, 2]
    assert bad.dtype == np.int32 and bad.tolist() == [7, 9, V + 2, -1, -1]
    assert bi.dtype == np.int32 and bi.tolist() == [4, 11, -1, -1] and bv.dtype == np.float32 and bv.tolist() == [-2.0, 1.5, 0.0, 0.0]
    assert tok.shape == (16, 16) and n.shape == (16,) and tok.dtype == n.dtype == np.int32
    assert n.tolist() == [3, 1] + [0] * 14 and tok[0].tolist() == [1, 2, 3] + [-1] * 13 and tok[1, 0] == 8 and (tok[2:] == -1).all()
    want_tok, want_n = ops.pack_stop_sequences(c.stop_sequences)                 # (the stop table is pack_stop_sequences' own)
    assert (tok[:2] == want_tok).all() and (n[:2] == want_n).all()
    p = Q.unpack(rec)
    assert p == dict(theta=np.float32(1.3), inv_theta=inv, ngram=3, min_new=5, freq=np.float32(0.25), pres=np.float32(-0.5), n_bad=3, n_bias=2)
    assert not Q.invalid(rec, 5, 4) and not Q.noop(rec, 2) and Q.invalid(rec, 2, 4) and Q.invalid(rec, 5, 1)
    # no EOS: the minimum length is already 0 in the record
    assert ops.pack_slot_constraints(c, None, 5, 4)[0][3] == 0 and ops.pack_slot_constraints(c, -1, 5, 4)[0][3] == 0
    # None, and an object that edits nothing: the no-op record, empty lists, an empty stop table
    for nothing in (None, D()):
        rec, bad, bi, bv, tok, n = ops.pack_slot_constraints(nothing, 2, 3, 0)
        assert rec.tolist() == [_bits(1.0), _bits(1.0), 0, 0, 0, 0, 0, 0] and Q.noop(rec, 2) and not Q.invalid(rec, 0, 0)
        assert bad.tolist() == [-1] * 3 and bi.shape == bv.shape == (0,) and (n == 0).all() and (tok == -1).all()
    assert not Q.noop(ops.pack_slot_constraints(D(min_new_tokens=1), 2, 0, 0)[0], 2) and Q.noop(ops.pack_slot_constraints(D(min_new_tokens=1), 2, 0, 0)[0], -1)


@pytest.mark.parametrize("theta", [0.7, 3.0, 1.2, 1.3, 1e-3, 123.456])
def test_word_1_is_one_fp32_division(theta):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import ops
    rec = ops.pack_slot_constraints(D(repetition_penalty=theta), 2, 0, 0)[0].view(np.uint32)
    want = np.float32(1) / np.float32(theta)
    assert int(rec[1]) == int(want.view(np.uint32)) and int(rec[0]) == _bits(theta)
    assert want == np.float32(1.0 / float(np.float32(theta)))                    # (the value the scalar forms pass at the launch)
    if theta in (0.7, 3.0):
        assert int(rec[1]) == {0.7: 0x3FB6DB6E, 3.0: 0x3EAAAAAB}[theta]


def test_pack_refuses_what_the_guard_would():
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import ops
    for c, caps in ((D(bad_token_ids=(1, 2, 3)), (2, 0)), (D(logit_bias={1: 1.0}), (4, 0)), (None, (1025, 0)), (None, (0, 1025)), (None, (-1, 0)),
                    (D(repetition_penalty=1e-39), (0, 0)), (D(repetition_penalty=1e39), (0, 0))):
        with pytest.raises(ValueError):
            ops.pack_slot_constraints(c, 2, *caps)
    fake = SimpleNamespace(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, frequency_penalty=0.0, presence_penalty=0.0,
                           bad_token_ids=(), logit_bias=(), stop_sequences=())
    for k, v in (("repetition_penalty", float("nan")), ("repetition_penalty", -1.0), ("frequency_penalty", float("inf")),
                 ("presence_penalty", float("nan")), ("no_repeat_ngram_size", -1), ("min_new_tokens", -2)):
        with pytest.raises(ValueError):
            ops.pack_slot_constraints(SimpleNamespace(**{**vars(fake), k: v}), 2, 0, 0)
    ops.pack_slot_constraints(fake, 2, 1024, 1024)


# ----------------------------------------------------------------------------------------------------------------------- the request forms
def _text(n, rows=1):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.zeros(rows, n, dtype=torch.long),
                        text_len=None)


def test_requests_take_constraints_only_with_the_flag():
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import GenerationConfig, SamplingParams
    from bdm_db1_amd.serving import Request, _Item, _requests
    cfg = GenerationConfig(max_new_tokens=8)
    sp, c = SamplingParams(greedy=False, top_p=0.9), D(no_repeat_ngram_size=3, min_new_tokens=4, bad_token_ids=(1, 2))
    assert Request(0, 1, ()).constraints is None and _Item(None, [0]).constraints is None
    items = [_text(4), (_text(5), 3), (_text(6, rows=2), None, None, c), (_text(4), 5, sp, None), _Item(_text(3), [9], 5, None, c), (_text(4), 4, sp, c)]
    reqs = list(_requests(items, cfg, per_request=True, window=(V, 32000), caps=(2, 0)))
    assert [r.index for r in reqs] == [0, 1, 2, 3, 4, 9, 10] and [r.limit for r in reqs] == [8, 3, 8, 8, 5, 5, 4]
    assert [r.constraints for r in reqs] == [None, None, c, c, None, c, c] and [r.params for r in reqs] == [None] * 4 + [sp, None, sp]
    # the third element must be None unless per_request is set too
    assert [r.constraints for r in _requests([(_text(4), None, None, c)], cfg, caps=(2, 0))] == [c]
    with pytest.raises(ValueError, match="per_request=True"):
        list(_requests([(_text(4), None, sp, c)], cfg, caps=(2, 0)))
    # the flag off: a fourth element is refused wherever it sits
    for bad in ((_text(4), 2, None, c), _Item(_text(3), [0], 5, None, c)):
        for per in (False, True):
            with pytest.raises(ValueError, match="per_request_constraints"):
                list(_requests([bad], cfg, per_request=per))
    # not a DecodingConstraints; min_new_tokens above the request's OWN limit; more ids / biases than the capacities
    for item, caps in (((_text(4), 5, None, dict(no_repeat_ngram_size=3)), (2, 0)), ((_text(4), 3, None, c), (2, 0)), ((_text(4), 5, None, c), (1, 0)),
                       ((_text(4), 5, None, D(logit_bias={1: 1.0, 2: 1.0})), (2, 1)), ((_text(4), 5, None, c, None), (2, 0))):
        with pytest.raises(ValueError):
            list(_requests([item], cfg, caps=caps))
    # a request's object replaces the stream's as a whole: the stream's minimum length binds only the requests without their own
    assert [r.limit for r in _requests([(_text(4), 2, None, D(bad_token_ids=(1,)))], cfg, 6, caps=(2, 0))] == [2]
    with pytest.raises(ValueError):
        list(_requests([(_text(4), 2, None, None)], cfg, 6, caps=(2, 0)))


def test_the_flag_off_request_path_is_what_it_was():
    from bdm_db1_amd import GenerationConfig, SamplingParams
    from bdm_db1_amd.serving import _Item, _requests, _split
    cfg = GenerationConfig(max_new_tokens=8)
    sp = SamplingParams(top_k=3)
    items = [_text(4), (_text(5), 3), _Item(_text(3), [9], 5)]
    got = list(_requests(items, cfg))
    assert [(r.index, r.limit, r.params, r.constraints) for r in got] == [(0, 8, None, None), (1, 3, None, None), (9, 5, None, None)]
    for bad in ((_text(4), 2, None), (_text(4), 2, None, None), (_text(4),), (_text(4), 2, sp)):
        with pytest.raises(ValueError):
            list(_requests([bad], cfg))
    with pytest.raises(ValueError):
        list(_requests([(_text(4), 2, sp, None)], cfg, per_request=True))         # (a four-tuple is a request only under the new flag)
    assert _split("b") == ("b", None, ()) and _split(("b", 4)) == ("b", 4, ()) and _split(("b", None, sp)) == ("b", None, (sp,))
    assert _split(("b", 4, None, "c")) == ("b", 4, (None, "c"))


# ------------------------------------------------------------------------------------------------- refusals, before anything is launched
@pytest.fixture
def no_launch(monkeypatch):
    """a model that passes the stream's checks, and a library in which any launch, prefill or generator fails the test"""
    from bdm_db1_amd import lib, serving
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    seen = {}

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")

    def stream(model, reqs, key, *a):
        seen["key"] = key
        seen["reqs"] = list(reqs)
        return iter(())

    monkeypatch.setattr(lib, "call", boom)
    monkeypatch.setattr(serving, "_prefill", boom)
    monkeypatch.setattr(serving, "_ring_generator", boom)
    monkeypatch.setattr(serving, "_stream", stream)
    model = SimpleNamespace(mem_len=40, compute_dtype=torch.bfloat16, use_decode=True, d_head=128, total_vocab_size=V, text_vocab_size=32000)
    return model, seen


def test_every_refusal_comes_before_a_launch(no_launch):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import GenerationConfig, SamplingParams, generate_many, generate_stream
    model, seen = no_launch
    cfg = GenerationConfig(max_new_tokens=8, eos_id=2)
    c = D(no_repeat_ngram_size=3, min_new_tokens=4, bad_token_ids=(1, 2, 3), logit_bias={5: 1.0, 6: 2.0})
    on = dict(per_request_constraints=True, max_bad_token_ids=3, max_logit_bias=2)
    ok = [(_text(4), 5, None, c), _text(5), (_text(4), None, None, None)]
    assert list(generate_stream(model, ok, cfg, **on)) == [] and [r.constraints for r in seen["reqs"]] == [c, None, None]
    refused = [
        (ok, dict(on, per_request_constraints=False)),                                         # a fourth element with the flag off
        ([(_text(4), 5, None, "no_repeat_ngram_size=3")], on),                                 # not a DecodingConstraints
        ([(_text(4), 3, None, c)], on),                                                        # min_new_tokens above the request's own limit
        (ok, dict(on, max_bad_token_ids=2)), (ok, dict(on, max_logit_bias=1)),                 # more ids / biases than the capacities
        (ok, dict(on, max_bad_token_ids=1025)), (ok, dict(on, max_logit_bias=-1)), (ok, dict(on, max_bad_token_ids=2.5)),
        (ok, dict(on, max_logit_bias=True)),
        ([(_text(4), 5, SamplingParams(greedy=True), c)], on),                                 # a third element without per_request
        ([_text(4)], dict(on, constraints=D(bad_token_ids=(1, 2, 3, 4)))),                     # the stream's own object beyond the capacities
        ([(_text(4), 2)], dict(on, constraints=D(min_new_tokens=3))),
    ]
    for reqs, kw in refused:
        with pytest.raises(ValueError):
            generate_stream(model, reqs, cfg, **kw)
        with pytest.raises(ValueError):
            generate_many(model, tuple(reqs), cfg, **kw)
    # a shape the _supported query refuses: max_new_tokens beyond the staged history
    with pytest.raises(ValueError, match="db1_constrain_logits_slots_per"):
        generate_stream(model, [_text(4)], GenerationConfig(max_new_tokens=4097), **on)
    generate_stream(model, [_text(4)], GenerationConfig(max_new_tokens=4097))                  # (the flag off: not asked)


def test_the_cache_key_changes_only_with_the_flag(no_launch):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import GenerationConfig, generate_stream
    import dataclasses
    import inspect
    from bdm_db1_amd import answer_stream, caption_stream, generate_many, serving
    from bdm_db1_amd.generation import DecodeKey
    model, seen = no_launch
    cfg = GenerationConfig(max_new_tokens=8)
    c = D(repetition_penalty=1.2)
    key = lambda constraints, per_request, caps: DecodeKey(rows=3, cfg=cfg, V=V, hi=V, constraints=constraints, n=None, per_request=per_request,
                                                           caps=caps)
    keys = {}
    for name, kw in (("plain", {}), ("cons", dict(constraints=c)), ("per", dict(per_request=True)), ("noop", dict(constraints=D())),
                     ("caps_ignored", dict(max_bad_token_ids=7, max_logit_bias=9)), ("bad_caps_ignored", dict(max_bad_token_ids=5000))):
        generate_stream(model, [_text(4)], cfg, slots=3, **kw)
        keys[name] = seen["key"]
    assert keys["plain"] == key(None, False, None) == keys["noop"] == keys["caps_ignored"] == keys["bad_caps_ignored"]
    assert keys["cons"] == key(c, False, None) and keys["per"] == key(None, True, None)
    on = dict(per_request_constraints=True)
    for name, kw in (("on", on), ("on_cons", dict(on, constraints=c)), ("on_per", dict(on, per_request=True)),
                     ("on_caps", dict(on, max_bad_token_ids=7, max_logit_bias=0)), ("on_noop", dict(on, constraints=D()))):
        generate_stream(model, [_text(4)], cfg, slots=3, **kw)
        keys[name] = seen["key"]
    assert keys["on"] == key(None, False, (64, 64)) == keys["on_noop"] and keys["on_cons"] == key(c, False, (64, 64))
    assert keys["on_per"] == key(None, True, (64, 64)) and keys["on_caps"] == key(None, False, (7, 0))
    distinct = []
    for k in keys.values():
        if k not in distinct:
            distinct.append(k)
    assert len(distinct) == 7
    # the key's fields are exactly these, every state is built from (model, key), and the public entry points take the keywords
    assert [f.name for f in dataclasses.fields(DecodeKey)] == ["rows", "cfg", "V", "hi", "constraints", "n", "per_request", "caps"]
    assert all(type(k) is DecodeKey for k in keys.values()) and len(set(keys.values())) == 7           # (hashable, compared by value)
    assert list(inspect.signature(serving._SlotState.__init__).parameters) == ["self", "model", "key"]
    sig = inspect.signature(generate_stream).parameters
    assert (sig["per_request_constraints"].default, sig["max_bad_token_ids"].default, sig["max_logit_bias"].default) == (False, 64, 64)
    for fn in (generate_many, caption_stream, answer_stream):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(fn).parameters.values())


# --------------------------------------------------------------------------------------------------------------------------- prototypes
def test_prototypes_are_declared_and_exported():
    from bdm_db1_amd import lib
    protos = lib.parse_header()
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    ret, args = protos["db1_constrain_logits_slots_per"]
    # logits M V ld dt | t hist max_new finished status row_map n_slots | cons | bad bad_cap bias_ids bias_val bias_cap | eos_id ws ws_bytes stream
    assert ret is ci and args == [vp, ci, ci, i64, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, ci, ci, vp, i64, vp]
    assert protos["db1_constrain_logits_slots_supported"] == (ci, [ci, i64, ci, ci, ci, ci])
    assert protos["db1_constrain_logits_slots_workspace_bytes"] == (i64, [ci, ci, ci, ci, ci, ci])
    ret, args = protos["db1_stop_match_per"]
    old = protos["db1_stop_match"][1]
    assert ret is ci and args == old[:2] + old[3:] and len(args) == len(old) - 1                # db1_stop_match's arguments without n_stop
    names = ("db1_constrain_logits_slots_per", "db1_constrain_logits_slots_supported", "db1_constrain_logits_slots_workspace_bytes",
             "db1_stop_match_per")
    assert all(n in lib.declared_symbols() for n in names)
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    so = ctypes.CDLL(lib.LIB_PATH)
    assert all(getattr(so, n) is not None for n in names)
    so.db1_constrain_logits_slots_supported.argtypes = [ci, i64, ci, ci, ci, ci]
    assert so.db1_constrain_logits_slots_supported(V, V, 4096, 1024, 1024, 1) == 1 and so.db1_constrain_logits_slots_supported(V, V, 16, 1025, 0, 1) == 0
    assert so.db1_constrain_logits_slots_supported(V, V, 16, 0, 1025, 1) == 0 and so.db1_constrain_logits_slots_supported(V, V, 4097, 0, 0, 1) == 0


# ------------------------------------------------------------------------------------------------- the rule against the scalar rules
def _case(rng, dtype, S=6, Vs=67, ld=72, mx=40, bad_cap=4, bias_cap=3):
    x = (rng.standard_normal((S, ld)) * 4).astype(np.float32)
    l = C.bf16_bits(x) if dtype == C.BF16 else x
    hist = rng.integers(-2, Vs + 2, (S, mx)).astype(np.int32)
    hist[rng.random((S, mx)) < 0.4] = 5
    t = rng.integers(0, mx, S).astype(np.int32)
    cons = np.stack([Q.record(theta=rng.choice([1.0, 1.3, 0.8]), ngram=int(rng.integers(0, 4)), min_new=int(rng.integers(0, mx)),
                              freq=rng.choice([0.0, 0.4, -0.2]), pres=rng.choice([0.0, 0.5]), n_bad=int(rng.integers(0, bad_cap + 1)),
                              n_bias=int(rng.integers(0, bias_cap + 1))) for _ in range(S)])
    bad = rng.integers(-1, Vs + 2, (S, bad_cap)).astype(np.int32)
    bias_ids = np.stack([rng.permutation(Vs + 3)[:bias_cap] - 1 for _ in range(S)]).astype(np.int32)
    bias_val = (rng.standard_normal((S, bias_cap)) * 2).astype(np.float32)
    return l, hist, t, cons, bad, bias_ids, bias_val


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_the_rule_agrees_slot_by_slot_with_the_scalar_rules(dtype):
    Vs, eos = 67, 3
    rng = np.random.default_rng(5 + (dtype == C.BF16))
    same = lambda a, b: (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all()
    edited = 0
    for k in range(12):
        l, hist, t, cons, bad, bi, bv = _case(rng, dtype)
        S = l.shape[0]
        finished = (rng.random(S) < 0.2).astype(np.int32)
        if k % 3 == 0:
            t[1] = 40                                                     # a counter at max_new
            cons[2] = Q.record()                                          # a no-op record
            cons[3] = Q.record(theta=float("nan"))                        # an invalid one
        row_map = None if k % 2 else rng.permutation(S + 1)[:S]           # (one entry may be S: no such slot)
        got, fin, st = Q.constrain(l, hist, t, finished, np.zeros(S, np.int32), cons, bad, bi, bv, V=Vs, dtype=dtype, eos_id=eos, row_map=row_map)
        for r in range(S):
            s = r if row_map is None else int(row_map[r])
            dead = not 0 <= s < S or finished[s] or t[s] >= 40
            if dead or Q.invalid(cons[s], 4, 3) or Q.noop(cons[s], eos):
                assert same(got[r], l[r])
                if not dead and Q.invalid(cons[s], 4, 3):
                    assert st[s] == Q.BAD_RECORD and fin[s] == 1
                continue
            p = Q.unpack(cons[s])
            kw = dict(theta=float(p["theta"]), ngram=p["ngram"], bad=bad[s, :p["n_bad"]].tolist(), eos_id=eos, min_new=p["min_new"])
            more = dict(freq=float(p["freq"]), pres=float(p["pres"]), bias=[(int(i), v) for i, v in zip(bi[s, :p["n_bias"]], bv[s, :p["n_bias"]])])
            one = P.apply(l[r:r + 1], hist[s:s + 1], int(t[s]), V=Vs, dtype=dtype, **kw, **more)[0]         # db1_constrain_logits_pen's rule
            assert same(got[r], one)
            if p["freq"] == 0 and p["pres"] == 0 and p["n_bias"] == 0:                                      # ... and db1_constrain_logits'
                assert same(got[r], C.apply(l[r:r + 1], hist[s:s + 1], int(t[s]), V=Vs, dtype=dtype, **kw)[0])
            edited += int(not same(got[r], l[r]))
        untouched = [s for s in range(S) if row_map is not None and s not in row_map]
        assert all(fin[s] == finished[s] and st[s] == 0 for s in untouched)
    assert edited >= 20


def test_the_stop_rule_agrees_slot_by_slot_with_the_scalar_rule():
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import ops
    rng = np.random.default_rng(9)
    S, mx, pad = 6, 12, 9
    lists = [((5, 6, 7),), (), ((7,), (6, 7), (5, 6, 7)), ((6, 7), (7, 7), (6, 7)), ((1,),), tuple((4 + k % 4, 7) for k in range(16))]
    rows = [ops.pack_slot_constraints(D(stop_sequences=q) if q else None, 2, 0, 0) for q in lists]
    tok, n = np.stack([r[4] for r in rows]), np.stack([r[5] for r in rows])
    st = dict(lengths=np.full(S, 8, np.int32), checked=np.zeros(S, np.int32), finished=np.zeros(S, np.int32), stop_hit=np.zeros(S, np.int32),
              out=rng.integers(0, 4, (S, mx)).astype(np.int32), next_ids=np.zeros(S, np.int64), logprob=-rng.random((S, mx)).astype(np.float32),
              sum_logprob=np.zeros(S, np.float32))
    st["out"][:, 5:8] = (5, 6, 7)
    got = Q.stop(st, tok, n, pad)
    assert got["stop_hit"].tolist() == [1, 0, 3, 1, 0, 3] and got["lengths"].tolist() == [5, 8, 5, 6, 8, 6] and got["checked"].tolist() == [5, 8, 5, 6, 8, 6]
    for s in range(S):                                                    # the scalar rule on that slot alone with its own list
        one = R.step(st, list(lists[s]), pad, row_map=[s])
        for k in got:
            a, b = got[k][s], one[k][s]
            assert (np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)).all() if np.asarray(a).dtype == np.float32 else (a == b).all()
    assert all((st[k] == Q.stop(st, tok, n, pad, row_map=[9])[k]).all() for k in st)           # no such slot: nothing moves
