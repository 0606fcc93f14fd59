"""Frequency / presence penalties, logit bias and stop sequences without a GPU: the two NumPy rules (tests/penalty_rule.py,
tests/stop_rule.py) against second, independent formulations; the new ``DecodingConstraints`` fields (defaults, equality, hash,
normalisation, every refusal, ``applies``); the refusals of ``beam_search`` / ``sample_best_of``; the prototypes; the packed layout; the
cache key of an object that edits nothing."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constraint_rule as C  # noqa: E402
import penalty_rule as P  # noqa: E402
import stop_rule as S  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------- the penalty rule
def _second_penalty(l, H, t, V, dtype, theta, freq, pres, bias, ngram, bad, eos, min_new):
    """the rule again, vectorised over the distinct tokens (np.unique counts, array arithmetic in float32) instead of a walk of the history"""
    x = C.widen(l, dtype).astype(np.float32)
    Hin = np.asarray([c for c in H[:t] if 0 <= c < V], np.int64)
    cols, counts = np.unique(Hin, return_counts=True) if Hin.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    v = x[cols]
    fin = np.isfinite(v)
    th = np.float32(theta)
    with np.errstate(over="ignore", invalid="ignore"):
        if th != 1:
            v = np.where(v > 0, v * np.float32(1.0 / float(th)), v * th).astype(np.float32)
        if np.float32(freq) != 0 or np.float32(pres) != 0:
            p = (counts.astype(np.float32) * np.float32(freq)).astype(np.float32)
            p = (p + np.float32(pres)).astype(np.float32)
            v = (v - p).astype(np.float32)
    store = (lambda a: C.bf16_widen(C.bf16_bits(a))) if dtype == C.BF16 else (lambda a: np.asarray(a, np.float32))
    x[cols[fin]] = store(v[fin])
    for c, b in (bias.items() if hasattr(bias, "items") else bias):
        if 0 <= c < V and np.isfinite(x[c]):
            with np.errstate(over="ignore"):
                x[c] = store(np.array([x[c] + np.float32(b)], np.float32))[0]
    for c in C.banned_columns(H, t, ngram, bad, eos, min_new):
        if 0 <= c < V:
            x[c] = -np.inf
    return x


@pytest.mark.parametrize("dtype", [C.F32, C.BF16])
def test_penalty_rule_against_a_second_formulation(dtype):
    rng = np.random.default_rng(5 + (dtype == C.BF16))
    V, ld, mx = 41, 48, 40
    edited = 0
    for k in range(60):
        l = (rng.standard_normal((1, ld)) * 4).astype(np.float32)
        l[0, rng.integers(0, V, 3)] = (np.nan, np.inf, -np.inf)
        lb = C.bf16_bits(l) if dtype == C.BF16 else l
        t = int(rng.integers(0, mx))
        H = rng.choice(np.array([0, 1, 2, 5, 17, V - 1, -1, V, V + 3]), mx)
        theta = (1.0, 1.3, 0.7)[k % 3]
        freq, pres = ((0.4, 0.0), (0.0, -0.3), (0.25, 0.6), (-0.5, 0.1))[k % 4]
        bias = {int(c): float(rng.standard_normal() * 3) for c in rng.choice(V + 4, 5, replace=False)} if k % 2 else {}
        kw = dict(ngram=(0, 2)[k % 2], bad=(3, V + 1) if k % 5 == 0 else (), eos_id=4, min_new=(0, mx)[k % 2])
        got = P.apply(lb, H[None], t, V=V, dtype=dtype, theta=theta, freq=freq, pres=pres, bias=bias, **kw)
        want = _second_penalty(lb[0], H, t, V, dtype, theta, freq, pres, bias, kw["ngram"], kw["bad"], 4, kw["min_new"])
        g = C.widen(got, dtype)[0]
        assert (g[:V].view(np.uint32) == want[:V].view(np.uint32))[~np.isnan(want[:V])].all(), k
        assert (np.isnan(g[:V]) == np.isnan(want[:V])).all()
        assert (got[0, V:] == lb[0, V:]).all()                       # padding keeps its bits
        edited += int((got != lb).any())
    assert edited > 40


def test_penalty_rule_details():
    V = 8
    l = np.array([[2.0, -2.0, 1.0, 1.0, np.inf, 0.5, 0.0, 3.0]], np.float32)
    H = np.array([[0, 1, 0, 0, 4, 9, -1, 5, 0, 0]])
    # n_0 = 3 among the first 8 entries; entries outside [0, V) are neither penalised nor counted; inf stays
    out = P.apply(l, H, 8, V=V, freq=0.5, pres=0.25)
    assert out[0].tolist() == [2.0 - 1.75, -2.0 - 0.75, 1.0, 1.0, np.inf, 0.5 - 0.75, 0.0, 3.0]
    # negative penalties raise the logit; theta first, then the subtraction
    out = P.apply(l, H, 3, V=V, theta=2.0, freq=-1.0)
    assert out[0, 0] == np.float32(2.0) * np.float32(0.5) + 2.0 and out[0, 1] == -4.0 + 1.0
    # the three operations round one by one: values where a fused multiply-add would differ
    f, p0, x = np.float32(0.1), np.float32(1e-8), np.float32(0.3)
    H3 = np.zeros((1, 4), np.int64)
    out = P.apply(np.array([[x]], np.float32), H3, 3, V=1, freq=float(f), pres=float(p0))
    assert out[0, 0] == np.float32(x - np.float32(np.float32(np.float32(3) * f) + p0))
    # the bias reads what the penalty stored (bf16: two roundings), and a ban overrides both
    lb = C.bf16_bits(np.array([[1.0, 1.0, 1.0]], np.float32))
    out = P.apply(lb, np.zeros((1, 3), np.int64), 1, V=3, dtype=C.BF16, freq=0.00390625 * 3, bias={0: 0.001, 1: 0.5}, bad=(1,))
    once = C.bf16_bits(np.array([np.float32(1.0) - np.float32(0.00390625 * 3)], np.float32))
    twice = C.bf16_bits(np.array([C.bf16_widen(once)[0] + np.float32(0.001)], np.float32))
    assert out[0, 0] == twice[0] and out[0, 1] == C.NEG_INF_BF16 and out[0, 2] == lb[0, 2]
    # with everything new off it is constraint_rule
    rng = np.random.default_rng(1)
    l = rng.standard_normal((3, 20)).astype(np.float32)
    H = rng.integers(-1, 18, (3, 9))
    kw = dict(V=17, theta=1.3, ngram=2, bad=(2,), eos_id=1, min_new=9)
    assert (P.apply(l, H, 7, **kw).view(np.uint32) == C.apply(l, H, 7, **kw).view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------------------------- the stop rule
def _second_stop(out_row, n, stops):
    """the winner again, on strings: every sequence as text, the row's tail with str.endswith, sorted by (-length, index)"""
    text = "".join(f"<{int(v)}>" for v in out_row[:n])
    hits = sorted((-len(q), k) for k, q in enumerate(stops) if len(q) <= n and text.endswith("".join(f"<{int(v)}>" for v in q)))
    return None if not hits else (hits[0][1], -hits[0][0])


def _stop_state(rng, S_, mx, n_top=0, lp=False):
    st = dict(lengths=rng.integers(0, mx + 1, S_).astype(np.int32), checked=rng.integers(0, mx + 1, S_).astype(np.int32),
              finished=rng.integers(0, 2, S_).astype(np.int32), stop_hit=np.zeros(S_, np.int32),
              out=rng.integers(0, 4, (S_, mx)).astype(np.int32), next_ids=rng.integers(0, 4, S_).astype(np.int64))
    if lp:
        st["logprob"] = -rng.random((S_, mx)).astype(np.float32)
        st["sum_logprob"] = -rng.random(S_).astype(np.float32)
    if n_top:
        st["top_ids"] = rng.integers(0, 4, (S_, mx, n_top)).astype(np.int32)
        st["top_logprob"] = -rng.random((S_, mx, n_top)).astype(np.float32)
    return st


def test_stop_rule_against_a_second_formulation():
    rng = np.random.default_rng(8)
    hits = 0
    for k in range(80):
        S_, mx = 6, int(rng.integers(1, 20))
        stops = [tuple(int(v) for v in rng.integers(0, 4, int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 6)))]
        st = _stop_state(rng, S_, mx, n_top=2, lp=True)
        row_map = None if k % 2 else [3, 0, 7, -1, 5]
        new = S.step(st, stops, 9, row_map)
        for s in range(S_):
            n = int(st["lengths"][s])
            touched = (row_map is None or s in row_map) and n != int(st["checked"][s])
            w = _second_stop(st["out"][s], n, stops) if touched and 1 <= n <= mx else None
            if w is None:
                for key in st:
                    if key != "checked":
                        assert (new[key][s] == st[key][s]).all(), (k, s, key)
                assert new["checked"][s] == (n if touched else st["checked"][s])
                continue
            hits += 1
            kk, L = w
            m = n - L
            assert new["lengths"][s] == new["checked"][s] == m and new["finished"][s] == 1 and new["stop_hit"][s] == kk + 1
            assert new["next_ids"][s] == 9 and (new["out"][s, m:n] == 9).all()
            assert (new["out"][s, :m] == st["out"][s, :m]).all() and (new["out"][s, n:] == st["out"][s, n:]).all()
            assert (new["logprob"][s, m:n] == 0).all() and (new["logprob"][s, n:] == st["logprob"][s, n:]).all()
            acc = np.float32(0)
            for v in st["logprob"][s, :m]:
                acc = np.float32(acc + v)
            assert new["sum_logprob"][s].view(np.uint32) == acc.view(np.uint32)
            assert (new["top_ids"][s, m:n] == -1).all() and np.isneginf(new["top_logprob"][s, m:n]).all()
            assert (new["top_ids"][s, :m] == st["top_ids"][s, :m]).all()
    assert hits > 30


def test_stop_rule_details():
    st = dict(lengths=np.array([3, 2, 0, 4], np.int32), checked=np.array([2, 2, 5, 3], np.int32), finished=np.zeros(4, np.int32),
              stop_hit=np.zeros(4, np.int32), out=np.array([[1, 2, 3, 0], [2, 3, 0, 0], [0, 0, 0, 0], [7, 7, 2, 3]], np.int32),
              next_ids=np.arange(4).astype(np.int64) + 10)
    new = S.step(st, [(3,), (2, 3), (1, 2, 3), (7, 7, 2, 3), (7, 2, 3, 9)], 0)
    # row 0: [3], [2 3] and [1 2 3] all match; the longest wins, the whole output goes; row 1: lengths == checked, its matching tail stays;
    # row 2: a stale checked heals, nothing else; row 3: ends at max_new
    assert new["lengths"].tolist() == [0, 2, 0, 0] and new["checked"].tolist() == [0, 2, 0, 0] and new["stop_hit"].tolist() == [3, 0, 0, 4]
    assert new["out"].tolist() == [[0, 0, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and new["next_ids"].tolist() == [0, 11, 12, 0]
    assert S.winner([5, 5], 2, [(5,), (5,)]) == (0, 1)                 # equal lengths: the lowest index
    assert S.winner([5, 5], 1, [(5, 5)]) is None                       # n < L: nothing before column 0 is read
    # a trimmed row launched again is not trimmed twice: stop [a] on a tail a a
    st = dict(lengths=np.array([3], np.int32), checked=np.array([2], np.int32), finished=np.zeros(1, np.int32), stop_hit=np.zeros(1, np.int32),
              out=np.array([[4, 6, 6]], np.int32), next_ids=np.zeros(1, np.int64))
    one = S.step(st, [(6,)], 0)
    two = S.step(one, [(6,)], 0)
    assert one["out"].tolist() == [[4, 6, 0]] and one["lengths"].tolist() == [2] and all((one[k] == two[k]).all() for k in one)
    # replay_row: the first match ends the row
    assert S.replay_row(np.array([5, 6, 7, 8, 9, 1, 1]), 5, [(7, 8), (8,)], 0)[1:] == (2, 1)
    assert S.replay_row(np.array([5, 6, 7]), 3, [(9,)], 0)[1:] == (3, 0)


def test_pack_stop_sequences_layout():
    from bdm_db1_amd import ops
    tok, n = ops.pack_stop_sequences([(5,), (1, 2, 3), tuple(range(16))])
    assert tok.dtype == np.int32 and tok.shape == (3, 16) and n.dtype == np.int32 and n.tolist() == [1, 3, 16]
    assert tok[0].tolist() == [5] + [-1] * 15 and tok[1, :4].tolist() == [1, 2, 3, -1] and tok[2].tolist() == list(range(16))
    t2, n2 = S.pack([(5,), (1, 2, 3), tuple(range(16))])
    assert (t2 == tok).all() and (n2 == n).all()
    for bad in ([], [()], [tuple(range(17))], [(1,)] * 17, [(-1,)]):
        with pytest.raises(ValueError):
            ops.pack_stop_sequences(bad)


# --------------------------------------------------------------------------------------------------------------------- the interface
def test_defaults_equality_and_hash_are_what_they_were():
    from bdm_db1_amd import DecodingConstraints
    d = DecodingConstraints()
    names = [f.name for f in dataclasses.fields(DecodingConstraints)]
    assert names == ["repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "bad_token_ids", "frequency_penalty", "presence_penalty",
                     "logit_bias", "stop_sequences"]
    assert (d.frequency_penalty, d.presence_penalty, d.logit_bias, d.stop_sequences) == (0.0, 0.0, (), ())
    assert d == DecodingConstraints(1.0, 0, 0, ()) and hash(d) == hash(DecodingConstraints(1.0, 0, 0, ())) == hash((1.0, 0, 0, ()))
    c = DecodingConstraints(1.2, 3, 5, (7, 9))
    assert hash(c) == hash((1.2, 3, 5, (7, 9))) and d.is_noop and not d.applies(None)
    a, b = DecodingConstraints(frequency_penalty=0.5), DecodingConstraints(frequency_penalty=0.5)
    assert a == b and hash(a) == hash(b) and a != d and {a: 1}[b] == 1
    assert DecodingConstraints(stop_sequences=[[1, 2]]) != DecodingConstraints(stop_sequences=[[1, 3]])


def test_normalisation_and_every_refusal():
    from bdm_db1_amd import DecodingConstraints as D
    c = D(frequency_penalty=np.float32(0.5), presence_penalty=-1, logit_bias={9: 1, np.int64(2): np.float32(-0.5)},
          stop_sequences=[[4, np.int32(5)], (6,)])
    assert c.frequency_penalty == 0.5 and c.presence_penalty == -1.0 and isinstance(c.presence_penalty, float)
    assert c.logit_bias == ((2, -0.5), (9, 1.0)) and all(type(k) is int and type(b) is float for k, b in c.logit_bias)
    assert c.stop_sequences == ((4, 5), (6,)) and all(type(v) is int for q in c.stop_sequences for v in q)
    assert D(logit_bias=[(9, 1.0), (2, -0.5)]) == D(logit_bias={2: -0.5, 9: 1.0}) and hash(c) == hash(dataclasses.replace(c))
    assert len(D(logit_bias={i: 0.0 for i in range(1024)}).logit_bias) == 1024
    assert len(D(stop_sequences=[(i,) for i in range(16)]).stop_sequences) == 16 and D(stop_sequences=[tuple(range(16))])
    nan, inf = float("nan"), float("inf")
    for kw in (dict(frequency_penalty=nan), dict(frequency_penalty=inf), dict(presence_penalty=-inf), dict(presence_penalty=nan),
               dict(frequency_penalty="1"), dict(presence_penalty=1e39),
               dict(logit_bias=[(1, 0.5), (1, 0.25)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: nan}),
               dict(logit_bias={1: inf}), dict(logit_bias=[(1, 2, 3)]), dict(logit_bias=5), dict(logit_bias={i: 0.0 for i in range(1025)}),
               dict(stop_sequences=[(i,) for i in range(17)]), dict(stop_sequences=[()]), dict(stop_sequences=[tuple(range(17))]),
               dict(stop_sequences=[(-1,)]), dict(stop_sequences=[(1.5,)]), dict(stop_sequences=[3]), dict(stop_sequences=7)):
        with pytest.raises(ValueError):
            D(**kw)
    with pytest.raises(Exception):
        c.frequency_penalty = 1.0                                 # frozen


def test_applies_for_each_new_field():
    from bdm_db1_amd import DecodingConstraints as D
    for kw in (dict(frequency_penalty=0.1), dict(frequency_penalty=-0.1), dict(presence_penalty=0.1), dict(logit_bias={3: 1.0}),
               dict(stop_sequences=[(3,)])):
        c = D(**kw)
        assert c.applies() and c.applies(None) and c.applies(5) and not c.is_noop, kw      # (stop sequences apply whatever eos_id is)
    assert D(frequency_penalty=0.1).edits_logits(None) and D(logit_bias={3: 0.0}).edits_logits(None)
    assert not D(stop_sequences=[(3,)]).edits_logits(None) and D(stop_sequences=[(3,)], bad_token_ids=(1,)).edits_logits(None)
    assert not D(frequency_penalty=0.0, presence_penalty=-0.0).applies()


def test_no_op_objects_keep_the_cache_key_and_beams_refuse_stop_sequences():
    from bdm_db1_amd import DecodingConstraints as D, GenerationConfig
    from bdm_db1_amd import generation as G
    gc = GenerationConfig(max_new_tokens=8)
    key = G.DecodeKey(rows=2, cfg=gc, V=100, hi=90, constraints=None, n=None, per_request=False, caps=None)
    model = SimpleNamespace(compute_dtype=None)                   # (never looked at: a no-op returns before any query)
    for c in (None, D(), D(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=(), stop_sequences=()), D(min_new_tokens=3)):
        assert G._constrained("generate", model, key, c, 8) is key
    for who in ("beam_search", "sample_best_of"):
        with pytest.raises(ValueError, match="stop_sequences"):
            G._constrained(who, model, key, D(stop_sequences=[(1,)]), 8)


def test_generation_config_did_not_gain_a_field():
    from bdm_db1_amd import GenerationConfig
    assert [f.name for f in dataclasses.fields(GenerationConfig)][-2:] == ["top_logprobs", "logprobs"] and len(dataclasses.fields(GenerationConfig)) == 13


def test_prototypes_are_declared_and_exported():
    from bdm_db1_amd import lib
    from bdm_db1_amd.build import build_lib
    protos = lib.parse_header()
    for n in ("db1_constrain_logits_pen", "db1_constrain_logits_pen_supported", "db1_constrain_logits_pen_workspace_bytes", "db1_stop_match",
              "db1_stop_match_supported"):
        assert n in protos, n
    old, new = protos["db1_constrain_logits"][1], protos["db1_constrain_logits_pen"][1]
    assert len(new) == len(old) + 5 and new[:len(old) - 3] == old[:-3] and new[-3:] == old[-3:]      # the parent's arguments, five more, ws / stream
    assert len(protos["db1_constrain_logits_pen_supported"][1]) == 6 and len(protos["db1_stop_match"][1]) == 21
    build_lib()
    so = lib.load()
    for n in ("db1_constrain_logits_pen", "db1_constrain_logits_pen_supported", "db1_constrain_logits_pen_workspace_bytes", "db1_stop_match",
              "db1_stop_match_supported"):
        assert getattr(so, n) is not None
    assert so.db1_constrain_logits_pen_workspace_bytes(4, 100, 30, 0, 16, 1) == 0
    assert so.db1_constrain_logits_pen_supported(100, 100, 30, 0, 1024, 1) and not so.db1_constrain_logits_pen_supported(100, 100, 30, 0, 1025, 1)
    assert so.db1_stop_match_supported(16, 30) and not so.db1_stop_match_supported(17, 30) and not so.db1_stop_match_supported(0, 30)


def test_entry_points_and_tools_take_the_new_fields():
    import inspect
    import bdm_db1_amd as pkg
    from bdm_db1_amd import ops
    sig = inspect.signature(ops.constrain_logits).parameters
    for name in ("frequency_penalty", "presence_penalty", "bias_ids", "bias_val"):
        assert name in sig and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("generate", "generate_stream", "generate_many", "beam_search", "sample_best_of"):
        assert callable(getattr(pkg, name))
    assert callable(ops.stop_match) and callable(ops.pack_stop_sequences)
