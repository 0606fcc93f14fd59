"""Diverse beam search end to end (``BeamSearchConfig(num_beam_groups=D, diversity_penalty=...)``): the fp32 eager loop against the NumPy rule
(tests/diverse_beam_rule.py) under the oracle's log-probs, the bf16 ring path against fresh list-form passes, graph replay against eager
launches, the fp8 ring, the shared prompt, the ring prefill and a Prefixed prompt against the default path, the first tokens under a
penalty above every score difference, ``result_groups``, the default call untouched, and the refusals."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import diverse_beam_rule as DR  # noqa: E402
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401

MLEN, LP = 96, 40


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _same(a, b):
    return all(torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------- 1. fp32 against the rule
class _OracleLM:
    """the oracle's next-token logits after (prompt g, tokens), one token per call like the generation loop, memoised per prefix"""

    def __init__(self, cfg, oracle, prompts):
        from oracle import db1_oracle as O
        self.O, self.oracle = O, oracle
        self.cache = {}
        for g, p in enumerate(prompts):
            mems = [np.zeros((1, cfg["mem_len"], cfg["n_embed"])) for _ in range(cfg["n_layer"])]
            logits, _, mems = oracle.forward([p], compute_loss=False, mems=mems)
            self.cache[(g,)] = (logits[0, -1], mems)

    def get(self, g, toks):
        key = (g,) + tuple(int(x) for x in toks)
        if key not in self.cache:
            _, mems = self.get(g, toks[:-1])
            logits, _, mems = self.oracle.forward([self.O.TaskBatch(kind="nlp", text_seq=np.array([[key[-1]]], np.int64))], compute_loss=False,
                                                  mems=mems)
            self.cache[key] = (logits[0, -1], mems)
        return self.cache[key]

    def rows(self, hist, W):
        return np.stack([self.get(b // W, h)[0] for b, h in enumerate(hist)]).astype(np.float32)


def _oracle_score(lm, g, toks, n, lo, hi, alpha):
    """sum of the window log-probs (float64) of the hypothesis' n tokens over n^alpha (no EOS here)"""
    seq = [int(c) for c in toks[:n]]
    total = 0.0
    for i, c in enumerate(seq):
        l = lm.get(g, seq[:i])[0].astype(np.float64)[lo:hi]
        f = l[np.isfinite(l)]
        total += l[c - lo] - (f.max() + np.log(np.exp(f - f.max()).sum()))
    return total / len(seq) ** alpha


@pytest.mark.parametrize("D", [2, 4])
def test_fp32_diverse_beams_follow_the_rule_under_the_oracle(D):
    from oracle import db1_oracle as O
    from bdm_db1_amd import BeamSearchConfig, beam_search
    cfg, model, oracle = _fp32_model()
    G, W, mx, hi, lam, alpha = 2, 4, 6, cfg["text_vocab_size"], 0.5, 0.9
    x, fields = _prompt(np.random.default_rng(21), "ic", G, hi)
    xo = [O.TaskBatch(kind="ic", **{k: v[g:g + 1] for k, v in fields.items()}) for g in range(G)]
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_hi=hi, length_penalty=alpha, num_beam_groups=D,
                          diversity_penalty=lam)
    stats = {}
    ids, lengths, scores = beam_search(model, x, bc, stats=stats)
    assert stats["path"] == "eager" and stats["token_calls"] == mx - 1
    assert tuple(ids.shape) == (G, W, mx) and tuple(scores.shape) == (G, W) and tuple(stats["result_groups"].shape) == (G, W)
    lm = _OracleLM(cfg, oracle, xo)
    rid, rlen, rsc, rgr, _, amb = DR.search(lambda hist: lm.rows(hist, W), G, W, D, lam, mx, 0, hi, -1, 0, alpha, R=W, tol=1e-4)
    assert not amb.all()
    for g in range(G):
        assert (np.diff(scores[g].numpy()) <= 0).all()
        for r in range(W):      # ambiguous or not: every score is the returned ids' own (unpenalised) score
            want = _oracle_score(lm, g, ids[g, r].numpy(), int(lengths[g, r]), 0, hi, alpha)
            assert abs(float(scores[g, r]) - want) <= 1e-4 * max(1.0, abs(want)), (g, r)
        if not amb[g]:
            assert (ids[g].numpy() == rid[g]).all() and (lengths[g].numpy() == rlen[g]).all(), g
            assert np.allclose(scores[g].numpy(), rsc[g], rtol=1e-4, atol=1e-4), g
            assert (stats["result_groups"][g].numpy() == rgr[g]).all(), g


# ------------------------------------------------------------------------------------------------------------------- 2. the bf16 ring path
def _list_form_score(model, x, g, toks, n, lo, hi, alpha):
    """a fresh batch-1 list-form pass over prompt g plus the hypothesis' tokens: float64 window log-probs -> the normalised score"""
    total = 0.0
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([_text(x[g:g + 1])], compute_loss=False, mems=model.init_mem(1))
        for i in range(n):
            l = logits[0, -1].double().cpu().numpy()[lo:hi]
            total += l[int(toks[i]) - lo] - (l.max() + np.log(np.exp(l - l.max()).sum()))
            logits, _, mems = model([_text(np.array([[int(toks[i])]]))], compute_loss=False, mems=mems)
    return total / n ** alpha


def _check_groups(model, stats, scores, D, R):
    """``result_groups`` against the pools the search left on the device"""
    st = model._beam_generator.state
    G = scores.shape[0]
    ps, pc = st.pool_score.cpu().numpy().reshape(G, D, -1), st.pool_count.cpu().numpy().reshape(G, D)
    for g in range(G):
        order = DR.merge_order(ps[g], pc[g])[:R]
        assert [d for d, _ in order] == stats["result_groups"][g].tolist()[:len(order)], g
        assert [float(ps[g, d, k]) for d, k in order] == scores[g].tolist()[:len(order)], g


def test_bf16_ring_scores_replay_and_result_groups():
    from bdm_db1_amd import BeamSearchConfig, beam_search
    _, model = _bf16_model(seed=8)
    G, W, D, mx, hi = 3, 4, 2, 12, 32000
    x = np.random.default_rng(14).integers(0, hi, (G, 6))
    plain_cfg = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_hi=hi)
    before = beam_search(model, _text(x), plain_cfg)
    bc = dataclasses.replace(plain_cfg, num_beam_groups=D, diversity_penalty=0.5)
    stats = {}
    ids, lengths, scores = beam_search(model, _text(x), bc, stats=stats)
    assert stats["path"] == "ring" and stats["token_calls"] == mx - 1 and (lengths == mx).all()
    assert model._beam_generator.state.done.numel() == G * D
    _check_groups(model, stats, scores, D, W)
    assert sorted(stats["result_groups"][0].tolist()) == [0, 0, 1, 1]       # (no EOS: every pool is offered its W' beams at the last step)
    errs = []
    for g in range(G):
        assert (np.diff(scores[g].numpy()) <= 0).all()
        for r in range(W):
            errs.append(abs(float(scores[g, r]) - _list_form_score(model, x, g, ids[g, r].numpy(), mx, 0, hi, 1.0)))
    print("bf16 ring diverse beam score |err| max", max(errs))
    assert max(errs) < 2e-2, max(errs)
    assert _same((ids, lengths, scores), beam_search(model, _text(x), bc)), "two runs differ"
    assert _same((ids, lengths, scores), beam_search(model, _text(x), bc, replay=False)), "graph replay and eager launches differ"
    # a default-config call after the diverse ones returns the bits it returned before
    assert _same(before, beam_search(model, _text(x), plain_cfg)), "the default call changed after a diverse one"
    assert model._beam_generator.state.done.numel() == G


def test_distinct_first_tokens_under_a_large_penalty():
    from bdm_db1_amd import BeamSearchConfig, beam_search
    _, model = _bf16_model(seed=8)
    G, W, mx, hi = 2, 4, 10, 32000
    x = np.random.default_rng(15).integers(0, hi, (G, 6))
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_hi=hi)
    p_ids, _, p_sc = beam_search(model, _text(x), bc)
    d_ids, _, d_sc = beam_search(model, _text(x), dataclasses.replace(bc, num_beam_groups=W, diversity_penalty=1e4))
    shared = [g for g in range(G) if len(set(p_ids[g, :, 0].tolist())) < W]
    assert shared, "plain beam search shares no first token on these prompts"
    for g in range(G):
        assert len(set(d_ids[g, :, 0].tolist())) == W, (g, d_ids[g, :, 0])
    assert torch.isfinite(d_sc).all() and (d_sc > -100).all()              # the penalty never enters a score


# ------------------------------------------------------------------------------------------- 3. fp8 ring, shared prompt, ring prefill, Prefixed
@pytest.fixture(scope="module")
def d128():
    """the mems_d128 configuration widened to n_position = 128, mem_len = 96: a bf16 model and an fp32 model on the same parameters"""
    from golden_util import case_cfg, make_params
    from bdm_db1_amd import TransformerXL
    cfg = case_cfg("mems_d128")
    cfg.update(n_position=128, mem_len=MLEN)
    params = make_params(cfg, 128)
    models = []
    for dt in (torch.bfloat16, torch.float32):
        m = TransformerXL(SimpleNamespace(**cfg), device=DEV, compute_dtype=dt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        m.eval()
        models.append(m)
    return cfg, models[0], models[1]


def _fp32_scores(m32, segments, ids, hi, alpha):
    """teacher-forced under the fp32 model: the prompt ``segments`` (arrays [L_i], fed one after the other) then the R continuations
    ``ids`` [R, n] -> sum_t log softmax(logits_t[:hi])[ids[r, t]] / n^alpha"""
    R, n = ids.shape
    idt = torch.as_tensor(np.asarray(ids, np.int64), device=DEV)
    with torch.no_grad():
        m32._dec_state = None
        mems = m32.init_mem(R)
        for seg in segments:
            logits, _, mems = m32([_text(np.repeat(seg[None], R, 0))], compute_loss=False, mems=mems)
        total = torch.zeros(R, dtype=torch.float64, device=DEV)
        for t in range(n):
            total += logits[:, -1, :hi].double().log_softmax(-1).gather(1, idt[:, t:t + 1])[:, 0]
            if t + 1 < n:
                logits, _, mems = m32([_text(ids[:, t:t + 1])], compute_loss=False, mems=mems)
    return (total / float(n) ** alpha).cpu().numpy()


def _distance(m32, segments, out, hi, alpha):
    ids, lengths, scores = (x.numpy() for x in out)
    assert (lengths == ids.shape[2]).all()            # (no EOS: every hypothesis runs to the end)
    want = np.stack([_fp32_scores(m32, [s[g] for s in segments], ids[g], hi, alpha) for g in range(ids.shape[0])])
    return float(np.abs(scores - want).max())


def test_fp8_shared_prompt_ring_prefill_and_prefixed_against_the_default_path(d128):
    """each path runs the diverse search and its scores lie as close to the fp32 model's teacher-forced scores of the ids it returned as the
    path's own test asks of plain beam search: the shared prompt and the ring prefill within 2x the default path's distance
    (test_group_ring_generation_gpu.py), the fp8 ring within 16x (test_kv8_generation_gpu.py: e4m3's rounding step against bf16's), a
    Prefixed prompt within 2x the distance of the default path on the concatenated prompt"""
    from bdm_db1_amd import BeamSearchConfig, PrefixCache, Prefixed, beam_search
    cfg, model, m32 = d128
    hi = cfg["text_vocab_size"]
    G, W, D = 2, 4, 2
    prompt = np.random.default_rng(21).integers(0, hi, (G, 70))
    bc = BeamSearchConfig(max_new_tokens=7, num_beams=W, num_return_sequences=W, vocab_hi=hi, num_beam_groups=D, diversity_penalty=0.5)
    off = beam_search(model, _text(prompt), bc)
    e_off = _distance(m32, [prompt], off, hi, bc.length_penalty)
    assert e_off > 0
    for name, kw, gate in (("share_prompt", dict(share_prompt=True), 2), ("fp8", dict(kv_cache="fp8"), 16)):
        stats = {}
        on = beam_search(model, _text(prompt), bc, stats=stats, **kw)
        assert stats["path"] == "ring" and tuple(on[0].shape) == tuple(off[0].shape) and tuple(stats["result_groups"].shape) == (G, W)
        if name == "share_prompt":
            assert model._beam_generator.ring.is_group_ring and model._beam_generator.ring.kv[0].shape[0] == G * W
        _check_groups(model, stats, on[2], D, W)
        e_on = _distance(m32, [prompt], on, hi, bc.length_penalty)
        print(f"diverse beam search, {name}: |score - fp32 score of the returned ids| {e_on:.3e}, default {e_off:.3e}")
        assert e_on <= gate * e_off, (name, e_on, e_off)
        assert _same(on, beam_search(model, _text(prompt), bc, replay=False, **kw)), (name, "graph replay and eager launches differ")
    model.use_ring_prefill = True
    try:
        assert model.ring_prefill_supported
        direct = beam_search(model, _text(prompt), bc)
    finally:
        model.use_ring_prefill = False
    e_direct = _distance(m32, [prompt], direct, hi, bc.length_penalty)
    print(f"diverse beam search, ring prefill: {e_direct:.3e}, default {e_off:.3e}")
    assert e_direct <= 2 * e_off
    cache = PrefixCache(model, 2)
    h = cache.put(_text(prompt[:, :LP]))
    pre = beam_search(model, Prefixed(cache, h, _text(prompt[:, LP:])), bc)
    e_pre = _distance(m32, [prompt[:, :LP], prompt[:, LP:]], pre, hi, bc.length_penalty)
    print(f"diverse beam search, Prefixed: {e_pre:.3e}, default {e_off:.3e}")
    assert e_pre <= 2 * e_off
    assert _same(off, beam_search(model, _text(prompt), bc)), "the default path changed"


def test_constraints_and_the_caption_helper_take_the_config(d128):
    from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, beam_search, generate_captions
    from bdm_db1_amd.data import ICTaskInput
    cfg, model, _ = d128
    hi = cfg["text_vocab_size"]
    G, W, D, mx = 2, 4, 2, 6
    prompt = np.random.default_rng(22).integers(0, hi, (G, 9))
    bc = BeamSearchConfig(max_new_tokens=mx, num_beams=W, num_return_sequences=W, vocab_hi=hi, num_beam_groups=D, diversity_penalty=0.5)
    free = beam_search(model, _text(prompt), bc)
    banned = sorted(set(free[0][:, :, 0].flatten().tolist()))
    ids, _, sc = beam_search(model, _text(prompt), bc, constraints=DecodingConstraints(bad_token_ids=tuple(banned), no_repeat_ngram_size=1))
    assert not np.isin(ids.numpy(), banned).any() and torch.isfinite(sc).all()
    for row in ids.reshape(-1, mx).tolist():
        assert len(set(row)) == mx                                          # (no token twice in a hypothesis)
    with pytest.raises(ValueError, match="stop_sequences"):
        beam_search(model, _text(prompt), bc, constraints=DecodingConstraints(stop_sequences=((1, 2),)))
    rng = np.random.default_rng(23)
    batch = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(rng.integers(0, hi, (G, 3))),
                        img_seq=_tdev(rng.standard_normal((G, 3, 32, 32)).astype(np.float32)), text_seq=None)
    stats = {}
    c_ids, c_len, c_sc = generate_captions(model, batch, dataclasses.replace(bc, num_return_sequences=3), stats=stats)
    assert tuple(c_ids.shape) == (G, 3, mx) and tuple(stats["result_groups"].shape) == (G, 3) and (c_sc[:, :-1] >= c_sc[:, 1:]).all()


# ------------------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_never_call_the_model(d128, monkeypatch):
    from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, beam_search
    cfg, model, m32 = d128
    hi = cfg["text_vocab_size"]
    prompt = _text(np.random.default_rng(24).integers(0, hi, (2, 9)))

    def called(*a, **k):
        raise AssertionError("the model was called")
    for m in (model, m32):
        monkeypatch.setattr(m, "forward", called)
    for bad in (dict(num_beam_groups=3), dict(num_beam_groups=0), dict(num_beam_groups=8), dict(num_beam_groups=2, diversity_penalty=-1.0),
                dict(num_beam_groups=2, diversity_penalty=float("inf")), dict(num_beam_groups=2, diversity_penalty=float("nan")),
                dict(num_beam_groups=1, diversity_penalty=0.5)):
        with pytest.raises(ValueError):
            beam_search(model, prompt, BeamSearchConfig(num_beams=4, max_new_tokens=4, vocab_hi=hi, **bad))
    bc = BeamSearchConfig(num_beams=4, max_new_tokens=4, vocab_hi=hi, num_beam_groups=2, diversity_penalty=0.5)
    for kw in (dict(constraints=DecodingConstraints(stop_sequences=((3,),))), dict(kv_cache="fp8", graphed=False), dict(share_prompt=True, graphed=False),
               dict(kv_cache="int4")):
        with pytest.raises(ValueError):
            beam_search(model, prompt, bc, **kw)
    with pytest.raises(ValueError):
        beam_search(m32, prompt, bc, graphed=True)                          # (fp32: no ring path)
    with pytest.raises(ValueError):
        beam_search(model, prompt, dataclasses.replace(bc, max_new_tokens=MLEN + 1))
