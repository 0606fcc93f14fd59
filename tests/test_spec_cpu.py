"""Speculative decoding without a GPU: the rule of tests/spec_rule.py emits exactly what the one-token loop of select_rule / logprob_rule
emits, whatever the drafts; the step counts of a perfect and of an always-wrong script; the draft rule; the commit's modulo; the refusals
of the config, of generate and of the ops wrappers with the library neither loaded nor called; the prototypes."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_rule as S  # noqa: E402

V, LO, HI = 48, 2, 40        # (tokens in [HI, V) are never chosen: an always-wrong script proposes one of them)
MAX_NEW = 12


def make_model(seed, dead=None):
    """logits float64 [V] as a seeded function of (row, the tokens fed so far); ``dead`` = (row, n): that row has no finite logit in the
    window once n tokens have been fed"""
    cache = {}

    def model(r, prefix):
        key = (r, tuple(int(v) for v in prefix))
        if key not in cache:
            h = hashlib.sha256(repr((seed,) + key).encode()).digest()
            l = np.random.default_rng(int.from_bytes(h[:8], "little")).normal(size=V) * 3.0
            if dead is not None and r == dead[0] and len(prefix) >= dead[1]:
                l[LO:HI] = -np.inf
            cache[key] = l
        return cache[key]
    return model


SAMPLING = {"greedy": dict(greedy=True), "top_p": dict(greedy=False, temperature=0.8, top_p=0.9, seed=1234)}


def _scripts(mode, plain_out, M, rng):
    if mode == "lookup":
        return None
    if mode == "perfect":
        return plain_out.copy()
    if mode == "wrong":
        return np.full((M, MAX_NEW), HI + 1, np.int64)
    s = rng.integers(LO, HI, size=(M, MAX_NEW))          # random: right here and there
    keep = rng.random((M, MAX_NEW)) < 0.6
    return np.where(keep, plain_out, s)


def _same(st, plain):
    out, lengths, logprob, sums, status = plain
    assert np.array_equal(st.out, out) and np.array_equal(st.lengths, lengths)
    assert np.array_equal(st.logprob, logprob) and np.array_equal(st.sums, sums)       # (fp32, added in token order: the same bits)
    assert np.array_equal(st.status, status)


@pytest.mark.parametrize("sampling", sorted(SAMPLING))
@pytest.mark.parametrize("mode", ("random", "perfect", "wrong", "lookup"))
@pytest.mark.parametrize("Q", (2, 5, 16))
@pytest.mark.parametrize("M", (1, 3))
def test_the_loop_emits_what_the_one_token_loop_emits(M, Q, mode, sampling):
    sel = SAMPLING[sampling]
    rng = np.random.default_rng(M * 100 + Q)
    for case in ("plain", "eos", "dead"):
        model = make_model(7 + M, dead=(M - 1, 5) if case == "dead" else None)
        eos = -1
        if case == "eos":      # an EOS that the plain loop meets at position 3 of row 0: inside an accepted run of a perfect script
            eos = int(S.generate_plain(model, M, MAX_NEW, LO, HI, **sel)[0][0, 3])
        plain = S.generate_plain(model, M, MAX_NEW, LO, HI, eos_id=eos, **sel)
        ctx = rng.integers(LO, HI, size=(M, 6))
        st = S.generate(model, M, Q, MAX_NEW, LO, HI, V, eos_id=eos, ctx=ctx, ctx_len=np.array([6, 0, 3][:M]),
                        script=_scripts(mode, plain[0], M, rng), logprobs=True, **sel)
        _same(st, plain)
        if case == "eos":
            assert plain[1][0] <= 3 and st.finished[0]
        if case == "dead":
            assert st.status[M - 1] == 1 and plain[1][M - 1] == 5
        if case == "eos" and M == 3:
            assert len({int(v) for v in plain[1]}) > 1         # the rows end at different times


@pytest.mark.parametrize("Q", (2, 5, 16))
@pytest.mark.parametrize("M", (1, 3))
def test_step_counts(M, Q):
    """a perfect script commits Q tokens per step, ceil((n - 1) / Q) steps after the prefill's token; a wrong one commits one per step"""
    model = make_model(3)
    n = MAX_NEW
    plain = S.generate_plain(model, M, n, LO, HI, greedy=True)
    st = S.generate(model, M, Q, n, LO, HI, V, script=plain[0].copy(), greedy=True)
    assert st.hist[1:].sum() == -(-(n - 1) // Q) and st.hist[0] == 0
    assert st.hist[Q] == (n - 1) // Q and (st.hist * np.arange(Q + 1)).sum() == n - 1
    st = S.generate(model, M, Q, n, LO, HI, V, script=np.full((M, n), HI + 1), greedy=True)
    assert st.hist[1] == n - 1 and st.hist.sum() == n - 1
    _same_tokens = np.array_equal(st.out, plain[0])
    assert _same_tokens


def test_step_counts_helper_matches_the_rule():
    model = make_model(3)
    for Q in (2, 5):
        plain = S.generate_plain(model, 3, MAX_NEW, LO, HI, greedy=True)
        p, w = S.step_counts(MAX_NEW, Q)
        assert np.array_equal(S.generate(model, 3, Q, MAX_NEW, LO, HI, V, script=plain[0].copy(), greedy=True).hist, p)
        assert np.array_equal(S.generate(model, 3, Q, MAX_NEW, LO, HI, V, script=np.full((3, MAX_NEW), HI + 1), greedy=True).hist, w)


@pytest.mark.parametrize("h,lo,hi,k,want", S.DRAFT_CASES)
def test_draft_rule(h, lo, hi, k, want):
    assert S.drafts(h, k, V, 0, ng_min=lo, ng_max=hi) == want


def test_draft_rule_seam_ragged_ctx_script_and_finished():
    # a match across the ctx / out seam: ctx = [.., 8, 9], out = [5, 8, 9] -> the 2-gram [8 9] occurred with its first token in ctx
    st = S.State(2, 4, 8)
    st.t, st.out[0, :3], st.out[1, :3] = 3, [5, 8, 9], [5, 8, 9]
    st.sel[:] = S.SKIP
    ctx = np.array([[7, 8, 9, 5], [7, 8, 9, 5]])
    st.finished[:] = False
    st.sel[:, 0], st.hit[:] = 6, 0
    S.accept(st, 4, V, ctx=ctx, ctx_len=np.array([4, 0]))            # both rows emit 6 at t = 3
    assert st.n_acc == 1 and list(st.out[0, :4]) == [5, 8, 9, 6]
    # row 0: h = [7 8 9 5 | 5 8 9 6]: no earlier 6 -> last token; row 1 (ctx_len 0): h = [5 8 9 6] -> last token
    assert list(st.ids[0]) == [6, 6, 6, 6] and list(st.ids[1]) == [6, 6, 6, 6]
    assert S.drafts([7, 8, 9, 5] + [5, 8, 9], 3, V, 0) == [5, 5, 8]     # [8 9] at p = 1 (in ctx) -> continue with 5, 5, 8
    assert S.drafts([5, 8, 9], 3, V, 0) == [9, 9, 9]                    # the same output without the ctx: nothing to find
    # script: a value outside [0, V) and an index past the end fall back to the last token
    sc = np.array([3, 4, -1, V, 5, 6])
    assert S.drafts([9, 1], 4, V, 0, script_row=sc, t2=1, max_new=6) == [4, 1, 1, 5]
    assert S.drafts([9, 1], 4, V, 0, script_row=sc, t2=4, max_new=6) == [5, 6, 1, 1]
    assert S.drafts([9, 1], 3, V, 11, finished=True) == [11, 11, 11] and S.drafts([], 2, V, 11) == [11, 11]


def test_commit_modulo_and_hist():
    st = S.State(1, 5, 8, ring_state=2, cap=104)
    st.n_acc = 1
    S.commit(st, 5)                      # the forward advanced by 5, one token kept: back by 4, below zero
    assert st.ring_state == 102 and st.t == 1 and list(st.hist) == [0, 1, 0, 0, 0, 0]
    st.n_acc = 5
    S.commit(st, 5)
    assert st.ring_state == 102 and st.t == 6 and st.hist[5] == 1
    st.n_acc, st.ring_state = 0, 3
    S.commit(st, 5, count=False)
    assert st.ring_state == 102 and st.t == 6 and st.hist.sum() == 2


def test_counter_at_the_end_and_out_of_range():
    st = S.State(2, 3, 4)
    st.t = 4
    S.accept(st, 3, V)
    assert st.n_acc == 0 and not st.status.any()
    for t in (-1, 5):
        st.t = t
        S.accept(st, 3, V)
        assert st.n_acc == 0 and (st.status == 2).all()


# ------------------------------------------------------------------------------------------------------------------ config, prototypes, refusals
def test_config_is_exported_frozen_and_checked():
    import dataclasses
    import bdm_db1_amd as B
    c = B.SpeculativeConfig()
    assert (c.num_draft_tokens, c.ngram_max, c.ngram_min, c.use_prompt) == (4, 3, 1, True)
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.num_draft_tokens = 2
    for kw in (dict(num_draft_tokens=0), dict(num_draft_tokens=16), dict(num_draft_tokens=True), dict(num_draft_tokens=2.0), dict(ngram_max=0),
               dict(ngram_max=9), dict(ngram_min=0), dict(ngram_min=9, ngram_max=8), dict(ngram_min=3, ngram_max=2)):
        with pytest.raises(ValueError):
            B.SpeculativeConfig(**kw)
    assert B.SpeculativeConfig(num_draft_tokens=15, ngram_min=8, ngram_max=8).num_draft_tokens == 15


def test_default_keys_are_what_they_were():
    import dataclasses
    from bdm_db1_amd import generation as gen
    cfg = gen.GenerationConfig(max_new_tokens=6)
    key = gen.DecodeKey(rows=2, cfg=cfg, V=100, hi=100)
    assert key.speculative is None and "speculative" not in [f.name for f in dataclasses.fields(key)]
    plan = gen._SpecPlan(gen.SpeculativeConfig(), False, 0)
    sk = gen.DecodeKeySpec(rows=2, cfg=cfg, V=100, hi=100, speculative=plan)
    assert sk != key and sk == gen.DecodeKeySpec(rows=2, cfg=cfg, V=100, hi=100, speculative=plan)
    assert [f.name for f in dataclasses.fields(sk)][-2:] == ["speculative", "kv_cache"]
    assert sk != dataclasses.replace(sk, kv_cache="fp8") and sk != dataclasses.replace(sk, speculative=dataclasses.replace(plan, scripted=True))
    assert gen._SpecState.cache != gen._State.cache


def test_prototypes_are_declared():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for s in ("db1_spec_pick_supported", "db1_spec_pick", "db1_spec_accept_supported", "db1_spec_accept", "db1_spec_commit_supported", "db1_spec_commit"):
        assert s in names, s
    protos = lib.parse_header()
    assert len(protos["db1_spec_pick"][1]) == 26 and len(protos["db1_spec_accept"][1]) == 26 and len(protos["db1_spec_commit"][1]) == 8


def _fake_model(**kw):
    def called(*a, **k):
        raise AssertionError("the model was called")
    m = dict(compute_dtype=torch.float32, use_decode=False, mem_len=40, d_head=128, n_head=2, total_vocab_size=100, text_vocab_size=80,
             training=False, eval=called, train=called, init_mem=called, __call__=called)
    m.update(kw)
    return SimpleNamespace(**m)


def _text_prompt(M=2, L=6):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.zeros(M, L, dtype=torch.long), text_len=None)


def test_generate_refuses_before_anything_is_launched(monkeypatch):
    from bdm_db1_amd import generation as gen, lib

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    sc, cfg = gen.SpeculativeConfig(), gen.GenerationConfig(max_new_tokens=8)
    go = lambda **kw: gen.generate(kw.pop("model", _fake_model()), kw.pop("prompt", _text_prompt()), kw.pop("cfg", cfg),
                                   speculative=kw.pop("sc", sc), **kw)
    good_script = np.zeros((2, 8), np.int32)
    for kw, what in ((dict(sc=4), "SpeculativeConfig expected"),
                     (dict(constraints=gen.DecodingConstraints(repetition_penalty=1.2)), "constraints"),
                     (dict(constraints=gen.DecodingConstraints(stop_sequences=((1, 2),))), "constraints"),
                     (dict(cfg=gen.GenerationConfig(max_new_tokens=8, logprobs=True, top_logprobs=2)), "top_logprobs"),
                     (dict(cfg=gen.BeamSearchConfig(max_new_tokens=8)), "GenerationConfig expected"),
                     (dict(prompt=_text_prompt(M=13)), "> 64"),
                     (dict(sc=gen.SpeculativeConfig(num_draft_tokens=15), prompt=_text_prompt(M=5)), "> 64"),
                     (dict(model=_fake_model(mem_len=4)), "mem_len"),
                     (dict(prompt=_text_prompt(L=4090)), "exceeds 4096"),
                     (dict(cfg=gen.GenerationConfig(max_new_tokens=4097), sc=gen.SpeculativeConfig(use_prompt=False)), "exceeds 4096"),
                     (dict(draft_script=good_script[:1]), "draft_script"), (dict(draft_script=good_script[:, :7]), "draft_script"),
                     (dict(draft_script=good_script.astype(np.float32)), "draft_script"),
                     (dict(kv_cache="fp8"), "kv_cache='fp8' needs the ring path"), (dict(kv_cache="int4"), "kv_cache")):
        with pytest.raises(ValueError, match=what):
            go(**kw)
    with pytest.raises(ValueError, match="draft_script needs speculative"):
        gen.generate(_fake_model(), _text_prompt(), cfg, draft_script=good_script)
    # the wrappers: a BeamSearchConfig, best-of-n and share_prompt
    ic = SimpleNamespace()
    monkeypatch.setattr(gen, "caption_prompt", lambda b: _text_prompt())
    for kw, what in ((dict(cfg=gen.BeamSearchConfig(max_new_tokens=8)), "not to beam search"), (dict(n=4), "best-of-n"),
                     (dict(share_prompt=True), "share_prompt")):
        with pytest.raises(ValueError, match=what):
            gen.generate_captions(_fake_model(), ic, kw.pop("cfg", cfg), speculative=sc, **kw)


def test_none_is_the_call_without_the_keyword(monkeypatch):
    """generate_captions / answer_questions hand speculative=None and draft_script=None to no function that does not know them"""
    from bdm_db1_amd import generation as gen
    seen = {}
    monkeypatch.setattr(gen, "caption_prompt", lambda b: _text_prompt())
    monkeypatch.setattr(gen, "beam_search", lambda model, x, cfg, **kw: seen.update(beam=kw))
    monkeypatch.setattr(gen, "sample_best_of", lambda model, x, cfg, n, **kw: seen.update(best=kw))
    monkeypatch.setattr(gen, "generate", lambda model, x, cfg, **kw: seen.update(gen=kw))
    gen.generate_captions(_fake_model(), None, gen.BeamSearchConfig(max_new_tokens=8), speculative=None, draft_script=None, graphed=False)
    gen.generate_captions(_fake_model(), None, gen.GenerationConfig(greedy=False), n=4, speculative=None)
    gen.generate_captions(_fake_model(), None, gen.GenerationConfig(), speculative=None, draft_script=None)
    assert seen == dict(beam=dict(graphed=False), best={}, gen={})


def _pick_args(M=2, Q=5, q_in=5, Vv=200, mx=8):
    i32 = torch.int32
    z = lambda *s, dt=i32: torch.zeros(*s, dtype=dt)
    return dict(logits2d=z(M * q_in, Vv, dt=torch.float32), t=z(1), finished=z(M), ids=z(M, Q, dt=torch.int64), sel=z(M, Q), hit=z(M, Q), q_in=q_in,
                max_new=mx)


def _accept_args(M=2, Q=5, q_in=5, mx=8):
    i32 = torch.int32
    z = lambda *s, dt=i32: torch.zeros(*s, dtype=dt)
    return dict(t=z(1), sel=z(M, Q), hit=z(M, Q), finished=z(M), lengths=z(M), out=z(M, mx), status=z(M), ids=z(M, Q, dt=torch.int64), n_acc=z(1),
                q_in=q_in, V=200)


def test_ops_refuse_on_the_host_before_the_library_is_loaded(monkeypatch):
    from bdm_db1_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    i32, f32 = torch.int32, torch.float32
    z = lambda *s, dt=i32: torch.zeros(*s, dtype=dt)
    good = _pick_args()
    for kw in (dict(q_in=0), dict(q_in=6), dict(q_in=True), dict(ids=z(2, 1, dt=torch.int64)), dict(ids=z(2, 17, dt=torch.int64)), dict(ids=z(2, 5)),
               dict(ids=z(10, dt=torch.int64)), dict(logits2d=z(9, 200, dt=f32)), dict(logits2d=z(10, 200, dt=torch.float16)),
               dict(logits2d=z(10, 400, dt=f32)[:, ::2]), dict(vocab_lo=5, vocab_hi=5), dict(vocab_hi=201), dict(V=201), dict(max_new=0),
               dict(greedy=False, temperature=0.0), dict(greedy=False, top_p=0.0), dict(greedy=False, top_k=-1), dict(t=z(2)), dict(finished=z(3)),
               dict(finished=z(2, dt=torch.int64)), dict(sel=z(2, 4)), dict(hit=z(2, 5, dt=f32)), dict(lp=z(2, 5)), dict(lp=z(2, 4, dt=f32)),
               dict(stream_id=z(3))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match="spec_pick"):
            ops.spec_pick(**args)
    with pytest.raises(ValueError, match="M \\* Q <= 65535"):
        ops.spec_pick(**_pick_args(M=4096, Q=16, q_in=1, Vv=8))
    good = _accept_args()
    lp3 = dict(lp=z(2, 5, dt=f32), logprob=z(2, 8, dt=f32), sum_logprob=z(2, dt=f32))
    for kw in (dict(q_in=0), dict(q_in=6), dict(ids=z(2, 1, dt=torch.int64)), dict(ids=z(2, 17, dt=torch.int64)), dict(ngram_min=0), dict(ngram_max=9),
               dict(ngram_min=3, ngram_max=2), dict(ngram_min=True), dict(V=0), dict(ctx=z(2, 6)), dict(ctx_len=z(2)),
               dict(ctx=z(2, 4089), ctx_len=z(2)), dict(ctx=z(3, 6), ctx_len=z(2)), dict(ctx=z(2, 6), ctx_len=z(3)), dict(ctx=z(2, 0), ctx_len=z(2)),
               dict(out=z(2, 4097)), dict(lp=lp3["lp"]), dict(lp=lp3["lp"], logprob=lp3["logprob"]), dict(logprob=lp3["logprob"], sum_logprob=lp3["sum_logprob"]),
               dict(lp3, lp=z(2, 4, dt=f32)), dict(lp3, logprob=z(2, 7, dt=f32)), dict(script=z(2, 7)), dict(script=z(2, 8, dt=torch.int64)),
               dict(sel=z(2, 4)), dict(hit=z(3, 5)), dict(finished=z(3)), dict(lengths=z(2, dt=torch.int64)), dict(status=z(1)), dict(t=z(2)),
               dict(n_acc=z(2)), dict(out=z(16)), dict(ids=z(2, 5))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match="spec_accept"):
            ops.spec_accept(**args)
    for kw in (dict(q_in=0, Q=5), dict(q_in=6, Q=5), dict(q_in=1, Q=1), dict(q_in=1, Q=17), dict(q_in=5, Q=5, hist=z(5)), dict(q_in=5, Q=5, hist=z(6, dt=f32)),
               dict(q_in=5, Q=5, ring_state=z(1), cap=0), dict(q_in=5, Q=5, ring_state=z(1), cap=-3), dict(q_in=5, Q=5, ring_state=z(1), cap=4),
               dict(q_in=5, Q=5, ring_state=z(2), cap=104), dict(q_in=5, Q=5, t=z(2))):
        args = dict(t=z(1), n_acc=z(1))
        args.update(kw)
        with pytest.raises(ValueError, match="spec_commit"):
            ops.spec_commit(args.pop("t"), args.pop("n_acc"), **args)
