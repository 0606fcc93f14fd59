"""Decoding constraints end to end: the invariants under ``generate`` on its three paths, the ring path against the eager path's
teacher-forced logits edited by the rule, the fp32 loop against the NumPy oracle with the rule, beam search, the stream against ``generate``
request by request, and the generator's cache key."""
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import beam_rule as B  # noqa: E402
import constraint_rule as C  # noqa: E402
import select_rule as R  # noqa: E402
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401

HI, PAD = 32000, 31999
PATHS = {"replay": dict(), "eager_ring": dict(replay=False), "list": dict(graphed=False)}


@pytest.fixture(scope="module")
def model():
    return _bf16_model()[1]


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _teacher_forced(model, x, ids):
    """the bf16 logits (as fp32) [n, M, V] of the eager list-form path fed the prompt, then ids[:, t] one token per call"""
    out = []
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([x], compute_loss=False, mems=model.init_mem(ids.shape[0]))
        for t in range(ids.shape[1]):
            out.append(logits[:, -1].float().cpu().numpy())
            logits, _, mems = model([_text(ids[:, t:t + 1])], compute_loss=False, mems=mems)
    return np.stack(out)


def _edited(l, H, t, cons, eos=-1, lo=0, hi=HI):
    """row ``l`` (bf16 values held as fp32, [V]) after the rule with history H[:t] -> float64, as the bf16 kernel leaves it"""
    hist = np.zeros((1, max(t, 1) + 1), np.int64)
    hist[0, :t] = H[:t]
    e = C.apply(C.bf16_bits(l[None, :]), hist, t, V=l.shape[0], dtype=C.BF16, theta=cons.repetition_penalty, ngram=cons.no_repeat_ngram_size,
                bad=cons.bad_token_ids, eos_id=eos, min_new=cons.min_new_tokens if eos >= 0 else 0)
    return C.bf16_widen(e)[0].astype(np.float64)


def _bigrams_repeat(row):
    row = [int(v) for v in row]
    pairs = list(zip(row[:-1], row[1:]))
    return len(set(pairs)) < len(pairs)


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("path", list(PATHS))
def test_invariants_hold_on_every_path(model, path, greedy):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate
    kw = PATHS[path]
    M, n = 3, 16
    x = _text(np.random.default_rng(2).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=n, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=HI, pad_id=PAD)

    def run(cfg, cons=None):
        stats = {}
        ids, lengths = generate(model, x, cfg, stats=stats, constraints=cons, **kw)
        assert stats["path"] == ("eager" if path == "list" else "ring")
        return ids.numpy(), lengths.numpy()

    # no bigram twice.  A window of 3 tokens: the 15 bigrams of an unconstrained row cannot all differ (9 exist), so the unconstrained run
    # violates the invariant whatever the model; a constrained row runs until every continuation is banned and then ends (no candidate)
    small = dataclasses.replace(gc, vocab_lo=100, vocab_hi=103)
    base, blen = run(small)
    assert (blen == n).all() and all(_bigrams_repeat(r) for r in base)
    ids, lengths = run(small, DecodingConstraints(no_repeat_ngram_size=2))
    for r in range(M):
        assert lengths[r] >= 4 and not _bigrams_repeat(ids[r, :lengths[r]]), (r, ids[r])
        assert ((ids[r, :lengths[r]] >= 100) & (ids[r, :lengths[r]] < 103)).all() and (ids[r, lengths[r]:] == PAD).all()
    # a wider window (12 tokens, 144 bigrams): the rows run to the end without a repeat
    wide = dataclasses.replace(gc, vocab_lo=100, vocab_hi=112)
    ids, lengths = run(wide, DecodingConstraints(no_repeat_ngram_size=2))
    assert (lengths == n).all() and not any(_bigrams_repeat(r) for r in ids)
    # banned ids: the tokens the unconstrained run chose at token 0 and token 1 of every row
    base, _ = run(gc)
    bad = tuple(sorted(set(int(v) for v in base[:, :2].reshape(-1))))
    assert np.isin(base, bad).any()
    ids, lengths = run(gc, DecodingConstraints(bad_token_ids=bad))
    assert (lengths == n).all() and not np.isin(ids, bad).any()
    # minimum length: EOS = what row 0 picks first
    eos = int(base[0, 0])
    ge = dataclasses.replace(gc, eos_id=eos)
    _, blen = run(ge)
    assert blen[0] == 0
    ids, lengths = run(ge, DecodingConstraints(min_new_tokens=6))
    assert (lengths >= 6).all() and not (ids[:, :6] == eos).any()


@pytest.mark.parametrize("greedy", [True, False])
def test_ring_matches_the_eager_loop_under_the_rule(model, greedy):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate
    M, n = 3, 16
    x = _text(np.random.default_rng(2).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=n, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=HI)
    plain, _ = generate(model, x, gc)
    cons = DecodingConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_token_ids=(int(plain[0, 0]), int(plain[1, 1]), HI + 5))
    st_r, st_e = {}, {}
    ring, _ = generate(model, x, gc, stats=st_r, constraints=cons)
    eager, _ = generate(model, x, gc, graphed=False, stats=st_e, constraints=cons)
    assert st_r["path"] == "ring" and st_e["path"] == "eager"
    ring, eager = ring.numpy(), eager.numpy()
    assert not np.isin(ring, cons.bad_token_ids).any() and not any(_bigrams_repeat(r) for r in ring)
    tf = _teacher_forced(model, x, ring)
    assert (ring[:, 0] == eager[:, 0]).all()          # (the same prefill call)
    for r in range(M):
        for t in range(n):
            raw = tf[t, r]
            l = _edited(raw, ring[r], t, cons)[:HI]
            assert np.isneginf(l[list(cons.bad_token_ids[:2])]).all()
            scale = np.abs(raw[:HI]).max()
            noise = 2e-2 * scale
            fin = l[np.isfinite(l)]
            if greedy:
                assert l[ring[r, t]] >= fin.max() - noise, (r, t)
            else:   # inside the edited eager logits' top-p set, up to bf16 noise at its boundary
                kept = R.kept_set(l, 0, HI, 1.0, 0, 0.9)[0]
                assert l[ring[r, t]] >= l[kept].min() - noise, (r, t)
            if ring[r, t] != eager[r, t]:     # the paths may only part at a near tie of the edited eager logits
                srt = np.sort(fin)
                if greedy:
                    assert srt[-1] - srt[-2] < noise, (r, t)
                break


@pytest.mark.parametrize("theta", [1.3, 5.0])
def test_fp32_greedy_with_a_repetition_penalty_follows_the_oracle(theta):
    """theta = 1.3: this model's greedy loop repeats one token whose lead (> 0.3 of the logits' scale in the oracle) the penalty never
    closes, so the tokens stay; theta = 5: under the oracle the penalty moves the arg-max at 22 of the 24 (row, step) pairs, every winner
    clear by > 5e-3 of the scale"""
    from oracle import db1_oracle as O
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate
    cfg, model, oracle = _fp32_model()
    M, n, hi = 2, 12, cfg["text_vocab_size"]
    x, fields = _prompt(np.random.default_rng(1), "nlp", M, hi)
    xo = O.TaskBatch(kind="nlp", **fields)
    stats = {}
    cons = DecodingConstraints(repetition_penalty=theta)
    ids, lengths = generate(model, x, GenerationConfig(max_new_tokens=n, vocab_hi=hi), stats=stats, constraints=cons)
    assert stats["path"] == "eager" and stats["token_calls"] == n - 1
    ids = ids.numpy()
    assert ids.shape == (M, n) and (lengths.numpy() == n).all()
    # the oracle's loop, teacher-forced on the GPU's tokens, its logits edited by the rule in fp32
    mems = [np.zeros((M, cfg["mem_len"], cfg["n_embed"])) for _ in range(cfg["n_layer"])]
    logits, _, mems = oracle.forward([xo], compute_loss=False, mems=mems)
    changed = 0
    for t in range(n):
        raw = logits[:, -1, :].astype(np.float32)
        l = C.apply(raw, ids, t, V=raw.shape[1], dtype=C.F32, theta=theta)[:, :hi].astype(np.float64)
        scale = np.abs(raw[:, :hi]).max()
        assert t == 0 or (l != raw[:, :hi]).any(axis=1).all()                      # (every row's history is penalised)
        srt = np.sort(l, axis=1)
        for r in range(M):
            assert l[r, ids[r, t]] >= srt[r, -1] - 1e-4 * scale, (t, r)
            if srt[r, -1] - srt[r, -2] > 1e-4 * scale:                           # (a clear winner: the tokens must be equal)
                assert ids[r, t] == np.argmax(l[r]), (t, r)
                changed += int(np.argmax(l[r]) != np.argmax(raw[r, :hi]))
        logits, _, mems = oracle.forward([O.TaskBatch(kind="nlp", text_seq=ids[:, t:t + 1].astype(np.int64))], compute_loss=False, mems=mems)
    print("theta", theta, "steps whose arg-max the penalty moved:", changed)
    assert theta < 5.0 or changed > 0                                              # (the penalty decides tokens)


def _constrained_list_form_score(model, x, g, toks, n, cons, eos, lo, hi, alpha):
    """a fresh batch-1 list-form pass over prompt g plus the hypothesis' tokens, every step's logits edited by the rule: float64 window
    log-probs of its tokens (EOS included) -> the normalised score"""
    from bdm_db1_amd.data import NLPTaskInput
    xg = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=x.text_seq[g:g + 1].clone(), text_len=None)
    seq = [int(c) for c in toks[:n]] + ([eos] if n < len(toks) else [])
    total = 0.0
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([xg], compute_loss=False, mems=model.init_mem(1))
        for i, c in enumerate(seq):
            l = _edited(logits[0, -1].float().cpu().numpy(), np.array(seq), i, cons, eos=eos)[lo:hi]
            f = l[np.isfinite(l)]
            total += l[c - lo] - (f.max() + np.log(np.exp(f - f.max()).sum()))
            logits, _, mems = model([_text(np.array([[c]]))], compute_loss=False, mems=mems)
    return total / len(seq) ** alpha


def test_beam_search_keeps_the_constraints(model):
    from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, beam_search
    G, W, mx, lo, hi = 2, 3, 12, 200, 208
    x = _text(np.random.default_rng(14).integers(0, HI, (G, 6)))
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_lo=lo, vocab_hi=hi, pad_id=PAD,
                          length_penalty=0.0)      # (unnormalised scores: a short hypothesis that ends in EOS stays in the pool)
    first = beam_search(model, x, bc)[0].numpy()
    eos = int(first[0, 0, 0])                                   # group 0's best first token becomes EOS
    bc = dataclasses.replace(bc, eos_id=eos)
    ids, lengths, _ = beam_search(model, x, bc)
    ids, lengths = ids.numpy(), lengths.numpy()
    assert (lengths < 4).any()                                  # (unconstrained: a hypothesis ends before 4 tokens)
    cons = DecodingConstraints(no_repeat_ngram_size=2, min_new_tokens=4)
    stats = {}
    ids, lengths, scores = beam_search(model, x, bc, stats=stats, constraints=cons)
    assert stats["path"] == "ring"
    e_ids, e_len, e_sc = beam_search(model, x, bc, replay=False, constraints=cons)
    assert torch.equal(ids, e_ids) and torch.equal(lengths, e_len) and torch.equal(scores.view(torch.int32), e_sc.view(torch.int32))
    st_l = {}
    l_ids, l_len, l_sc = beam_search(model, x, bc, graphed=False, stats=st_l, constraints=cons)
    assert st_l["path"] == "eager"
    errs = []
    for got_ids, got_len, got_sc in ((ids, lengths, scores), (l_ids, l_len, l_sc)):
        for g in range(G):
            assert torch.isfinite(got_sc[g]).all() and (np.diff(got_sc[g].numpy()) <= 0).all()
            for r in range(W):
                n = int(got_len[g, r])
                row = got_ids[g, r].numpy()
                assert n >= 4 and eos not in row[:n].tolist() and not _bigrams_repeat(row[:n]), (g, r, row)
                assert ((row[:n] >= lo) & (row[:n] < hi)).all()
                want = _constrained_list_form_score(model, x, g, row, n, cons, eos, lo, hi, 0.0)
                errs.append(abs(float(got_sc[g, r]) - want))
    # bf16: per-token log-prob noise of the ring path against fresh list-form passes (the bound of the unconstrained beam test)
    print("constrained beam score |err| max", max(errs))
    assert max(errs) < 2e-2, max(errs)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_one_constrained_beam_step_equals_the_two_rules(dt):
    from bdm_db1_amd import ops
    from beam_kernel_common import _compare, _download, _upload
    G, W, V, mx, t, lo, hi, eos, pad = 3, 3, 500, 8, 4, 2, 480, 5, 479
    M = G * W
    rng = np.random.default_rng(9)
    kind = C.BF16 if dt == torch.bfloat16 else C.F32
    S = B.new_state(G, W, mx, pad)
    S["tokens"][:, :t] = rng.integers(6, 12, (M, t))            # every beam its own history, from few tokens (repeats, shared bigrams)
    S["beam_score"][:] = -rng.random(M).astype(np.float32) * 3
    l = (rng.standard_normal((M, V)) * 3).astype(np.float32)
    l[:, 6:12] += 6.0                                           # the history's tokens lead: the constraints decide the step
    l[:, eos] += 9.0
    lt = torch.from_numpy(l).to(DEV).to(dt)
    host = C.bf16_bits(lt.float().cpu().numpy()) if kind == C.BF16 else l
    kw = dict(theta=1.3, ngram=2, bad=(7, V + 1), eos_id=eos, min_new=t + 1)
    e = C.apply(host, S["tokens"], t, V=V, dtype=kind, **kw)
    want, amb = B.step(S, C.widen(e, kind), t, W, lo, hi, eos, pad, 0.8)
    plain, _ = B.step(S, C.widen(host, kind), t, W, lo, hi, eos, pad, 0.8)
    assert (plain["tokens"][:, t] != want["tokens"][:, t]).any() and plain["pool_count"].sum() > 0 and want["pool_count"].sum() == 0
    D = _upload(S)
    ids = torch.full((M, 2), -5, dtype=torch.long, device=DEV)
    tt = torch.tensor([t], dtype=torch.int32, device=DEV)
    ops.constrain_logits(lt, tt, D["tokens"], V=V, repetition_penalty=1.3, no_repeat_ngram_size=2, bad=_tdev(np.array([7, V + 1], np.int32)),
                         eos_id=eos, min_new=t + 1)
    got_l = lt.view(torch.int16).cpu().numpy().view(np.uint16) if kind == C.BF16 else lt.cpu().numpy().view(np.uint32)
    assert (got_l == (e if kind == C.BF16 else e.view(np.uint32))).all()
    ops.beam_step(lt, tt, D["beam_score"], D["parent"], D["tokens"], D["pool_tokens"], D["pool_len"], D["pool_score"], D["pool_slot"],
                  D["pool_count"], D["done"], D["switches"], ids[:, 0], D["status"], W=W, V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, pad_id=pad,
                  length_penalty=0.8)
    torch.cuda.synchronize()
    assert not amb.all()
    _compare(_download(D, ids), want, amb, W, 1, t)


def test_stream_requests_equal_generate_alone(model):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate, generate_stream
    rng = np.random.default_rng(21)
    lens, limits = [5, 9, 5, 9, 5, 9, 5], [4, 12, 6, 8, 12, 4, 10]
    prompts = [rng.integers(0, HI, (1, n)) for n in lens]
    gc = GenerationConfig(max_new_tokens=12, vocab_lo=300, vocab_hi=310, pad_id=PAD, sync_every=2)
    plain = {i: ids for i, ids, _ in generate_stream(model, [(_text(p), lim) for p, lim in zip(prompts, limits)], gc, slots=3)}
    bad = tuple(sorted({int(plain[i][0]) for i in (0, 1)}))
    cons = DecodingConstraints(no_repeat_ngram_size=2, bad_token_ids=bad)
    stats = {}
    got = {i: (ids.numpy(), n) for i, ids, n in
           generate_stream(model, [(_text(p), lim) for p, lim in zip(prompts, limits)], gc, slots=3, stats=stats, constraints=cons)}
    assert sorted(got) == list(range(7)) and stats["admitted"] == 7 and stats["replays"] < sum(limits)
    for i, (ids, length) in got.items():
        assert ids.shape == (limits[i],) and length == limits[i]
        assert not np.isin(ids, bad).any() and not _bigrams_repeat(ids), (i, ids)
        alone, alen = generate(model, _text(prompts[i]), dataclasses.replace(gc, max_new_tokens=limits[i]), graphed=None, constraints=cons)
        alone = alone.numpy()[0]
        assert int(alen[0]) == length
        if (alone != ids).any():      # the slot's decode batch and the request alone may part only at a near tie of the edited logits
            t = int(np.nonzero(alone != ids)[0][0])
            raw = _teacher_forced(model, _text(prompts[i]), ids[None, :t + 1])[t, 0]
            l = _edited(raw, ids, t, cons)[300:310]
            noise = 2e-2 * np.abs(raw[:HI]).max()
            assert l[ids[t] - 300] >= l.max() - noise and l[alone[t] - 300] >= l.max() - noise, (i, t)
    # a request whose limit is below the minimum length, and a minimum above max_new_tokens: refused before any launch
    with pytest.raises(ValueError):
        generate_stream(model, [(_text(prompts[0]), 3)], gc, slots=3, constraints=DecodingConstraints(min_new_tokens=4))
    with pytest.raises(ValueError):
        generate_stream(model, [_text(prompts[0])], gc, slots=3, constraints=DecodingConstraints(min_new_tokens=13))
    with pytest.raises(ValueError):
        generate(model, _text(prompts[0]), gc, constraints=DecodingConstraints(min_new_tokens=13))
    with pytest.raises(TypeError):
        generate(model, _text(prompts[0]), gc, constraints=dict(min_new_tokens=1))


def test_cache_key_and_the_unconstrained_path():
    from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, GenerationConfig, beam_search, generate, generate_many
    model = _bf16_model()[1]
    x = _text(np.random.default_rng(2).integers(0, HI, (3, 6)))
    gc = GenerationConfig(max_new_tokens=8, greedy=False, top_p=0.9, seed=7, vocab_hi=HI, pad_id=PAD)
    bc = BeamSearchConfig(num_beams=2, max_new_tokens=6, vocab_hi=HI)
    before = generate(model, x, gc)                              # before any constrained call in this process's model
    b_before = beam_search(model, x, bc)
    s_before = generate_many(model, [x], gc, slots=2)
    gen, bgen, sgen = model._generator, model._beam_generator, model._slot_generator
    k = gen.key
    assert k.constraints is None and not k.per_request and k.caps is None and k.n is None and gen.state.con is None
    same = generate(model, x, gc, constraints=None)
    noop = generate(model, x, gc, constraints=DecodingConstraints())
    assert model._generator is gen                               # None, then a no-op object: the cached generator is reused
    beam_search(model, x, bc, constraints=DecodingConstraints())
    generate_many(model, [x], gc, slots=2, constraints=DecodingConstraints())
    assert model._beam_generator is bgen and model._slot_generator is sgen
    for a in (same, noop):
        assert torch.equal(a[0], before[0]) and torch.equal(a[1], before[1])
    cons = DecodingConstraints(repetition_penalty=1.2)
    generate(model, x, gc, constraints=cons)
    real = model._generator
    k = real.key
    assert real is not gen and k.constraints == cons and not k.per_request and k.caps is None and k.n is None and real.state.con is not None
    generate(model, x, gc, constraints=DecodingConstraints(repetition_penalty=1.2))
    assert model._generator is real                              # an equal constraint: the same graph
    generate(model, x, gc, constraints=DecodingConstraints(repetition_penalty=1.2, bad_token_ids=(5,)))
    assert model._generator is not real                          # a changed one: captured again
    beam_search(model, x, bc, constraints=DecodingConstraints(no_repeat_ngram_size=2))
    generate_many(model, [x], gc, slots=2, constraints=cons)
    assert model._beam_generator is not bgen and model._slot_generator is not sgen
    # after constrained calls, constraints=None gives what it gave before them
    after, b_after, s_after = generate(model, x, gc), beam_search(model, x, bc), generate_many(model, [x], gc, slots=2)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    assert all(torch.equal(p, q) for p, q in zip(b_after, b_before))
    assert all(torch.equal(p, q) for p, q in zip(s_after[0], s_before[0])) and s_after[1] == s_before[1]
    # min_new_tokens without an EOS edits nothing: the unconstrained generator is reused, no graph is captured for it
    plain_gen = model._generator
    k = plain_gen.key
    assert k.constraints is None and not k.per_request and k.caps is None and k.n is None
    generate(model, x, gc, constraints=DecodingConstraints(min_new_tokens=3))
    assert model._generator is plain_gen and plain_gen.state.con is None
    assert not DecodingConstraints(min_new_tokens=3).applies(None) and DecodingConstraints(min_new_tokens=3).applies(5)


def test_the_task_helpers_forward_the_keyword(model):
    """generate_captions, answer_questions, caption_stream and answer_stream hand ``constraints`` on: the tokens the unconstrained call
    picks first are banned, and none of them comes back"""
    from bdm_db1_amd import (DecodingConstraints, GenerationConfig, answer_questions, answer_stream, caption_stream, generate_captions)
    rng = np.random.default_rng(31)
    ic, _ = _prompt(rng, "ic", 2, HI)
    vqa, _ = _prompt(rng, "vqa", 2, HI)
    gc = GenerationConfig(max_new_tokens=6, pad_id=PAD, sync_every=2)
    for fn, batch in ((generate_captions, ic), (answer_questions, vqa)):
        base = fn(model, batch, gc)[0].numpy()
        bad = tuple(sorted(set(int(v) for v in base[:, 0])))
        ids, lengths = fn(model, batch, gc, constraints=DecodingConstraints(bad_token_ids=bad, no_repeat_ngram_size=1))
        ids = ids.numpy()
        assert (lengths.numpy() == 6).all() and not np.isin(ids, bad).any() and all(len(set(r.tolist())) == 6 for r in ids), fn.__name__
    for fn, batch in ((caption_stream, ic), (answer_stream, vqa)):
        base = {i: t for i, t, _ in fn(model, [batch], gc, slots=2)}
        bad = tuple(sorted(set(int(t[0]) for t in base.values())))
        got = {i: t.numpy() for i, t, _ in fn(model, [batch], gc, slots=2, constraints=DecodingConstraints(bad_token_ids=bad, no_repeat_ngram_size=1))}
        assert sorted(got) == [0, 1], fn.__name__
        for t in got.values():
            assert t.shape == (6,) and not np.isin(t, bad).any() and len(set(t.tolist())) == 6, fn.__name__
