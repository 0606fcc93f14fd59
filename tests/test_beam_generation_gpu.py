"""Beam search end to end (bdm_db1_amd.generation.beam_search): the fp32 eager loop against the NumPy rule under the oracle's log-probs, one
beam against greedy generation, the bf16 ring path (the beams' K / V histories reordered in the ring) against fresh list-form passes, the
graphed ring path against the same kernels launched eagerly, EOS and the early stop, captions at the DB1-1.3B geometry, and the pinned flag
words of dropped graphed steps."""
import dataclasses
import gc
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
DEV = "cuda"

import beam_rule as B  # noqa: E402
from gpu_common import _bf16_model, _fp32_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401


def _prompts(rng, kind, G, vocab):
    from oracle import db1_oracle as O
    x, fields = _prompt(rng, kind, G, vocab)
    return x, [O.TaskBatch(kind=kind, **{k: v[g:g + 1] for k, v in fields.items()}) for g in range(G)]


class _OracleLM:
    """the oracle's next-token logits after (prompt g, tokens), one token per call like the generation loop, memoised per prefix"""

    def __init__(self, cfg, oracle, prompts):
        from oracle import db1_oracle as O
        self.O, self.cfg, self.oracle = O, cfg, oracle
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


def _oracle_search(lm, G, W, mx, lo, hi, eos, pad, alpha, tol):
    """the rule's search under the oracle's logits -> (ids, lengths, scores, ambiguous groups)"""
    S = B.new_state(G, W, mx, pad)
    amb = np.zeros(G, bool)
    for t in range(mx):
        hist = [list(S["tokens"][b, :t]) for b in range(G * W)]
        S, a = B.step(S, lm.rows(hist, W), t, W, lo, hi, eos, pad, alpha, tol=tol)
        amb |= a
        if S["done"].all():
            break
    return B.results(S, W, W, pad) + (amb,)


def _oracle_score(lm, g, toks, n, lo, hi, eos, alpha):
    """sum of the window log-probs (float64) of the hypothesis' tokens (its EOS included) over its length^alpha"""
    seq = [int(c) for c in toks[:n]] + ([eos] if eos >= 0 and n < len(toks) else [])
    total = 0.0
    for i, c in enumerate(seq):
        l = lm.get(g, seq[:i])[0].astype(np.float64)[lo:hi]
        f = l[np.isfinite(l)]
        total += l[c - lo] - (f.max() + np.log(np.exp(f - f.max()).sum()))
    return total / len(seq) ** alpha


@pytest.mark.parametrize("kind", ["nlp", "ic"])
def test_fp32_beams_follow_the_rule_under_the_oracle(kind):
    from bdm_db1_amd import BeamSearchConfig, beam_search
    cfg, model, oracle = _fp32_model()
    G, W, mx, hi = 2, 3, 7, cfg["text_vocab_size"]
    x, xo = _prompts(np.random.default_rng(11), kind, G, hi)
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_hi=hi, length_penalty=0.9)
    stats = {}
    ids, lengths, scores = beam_search(model, x, bc, stats=stats)
    assert stats["path"] == "eager" and stats["token_calls"] == mx - 1
    assert tuple(ids.shape) == (G, W, mx) and tuple(scores.shape) == (G, W)
    lm = _OracleLM(cfg, oracle, xo)
    rid, rlen, rsc, amb = _oracle_search(lm, G, W, mx, 0, hi, -1, 0, 0.9, tol=1e-4)
    assert not amb.all()
    for g in range(G):
        for r in range(W):
            want = _oracle_score(lm, g, ids[g, r].numpy(), int(lengths[g, r]), 0, hi, -1, 0.9)
            assert abs(float(scores[g, r]) - want) <= 1e-4 * max(1.0, abs(want)), (g, r)
        if not amb[g]:
            assert (ids[g].numpy() == rid[g]).all() and (lengths[g].numpy() == rlen[g]).all(), g
            assert np.allclose(scores[g].numpy(), rsc[g], rtol=1e-4, atol=1e-4), g


def test_one_beam_equals_greedy_fp32_and_bf16_ring():
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search, generate
    cfg, model, _ = _fp32_model()
    hi = cfg["text_vocab_size"]
    x, _ = _prompts(np.random.default_rng(12), "ic", 3, hi)
    g_ids, g_len = generate(model, x, GenerationConfig(max_new_tokens=9, vocab_hi=hi))
    b_ids, b_len, _ = beam_search(model, x, BeamSearchConfig(num_beams=1, max_new_tokens=9, vocab_hi=hi))
    assert torch.equal(b_ids[:, 0], g_ids) and torch.equal(b_len[:, 0], g_len)
    _, model = _bf16_model()
    x, _ = _prompts(np.random.default_rng(13), "nlp", 3, 32000)
    st_g, st_b = {}, {}
    g_ids, g_len = generate(model, x, GenerationConfig(max_new_tokens=14, vocab_hi=32000), stats=st_g)
    b_ids, b_len, _ = beam_search(model, x, BeamSearchConfig(num_beams=1, max_new_tokens=14, vocab_hi=32000), stats=st_b)
    assert st_g["path"] == st_b["path"] == "ring"
    assert torch.equal(b_ids[:, 0], g_ids) and torch.equal(b_len[:, 0], g_len)


def _list_form_score(model, x, g, toks, n, lo, hi, alpha):
    """a fresh batch-1 list-form pass over prompt g plus the hypothesis' tokens: float64 window log-probs -> the normalised score"""
    from bdm_db1_amd.data import NLPTaskInput
    xg = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=x.text_seq[g:g + 1].clone(), text_len=None)
    total = 0.0
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([xg], compute_loss=False, mems=model.init_mem(1))
        for i in range(n):
            l = logits[0, -1].double().cpu().numpy()[lo:hi]
            total += l[int(toks[i]) - lo] - (l.max() + np.log(np.exp(l - l.max()).sum()))
            y = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.array([[int(toks[i])]])),
                             text_len=None)
            logits, _, mems = model([y], compute_loss=False, mems=mems)
    return total / n ** alpha


def test_bf16_ring_beams_switch_lineage_and_score_like_fresh_passes():
    from bdm_db1_amd import BeamSearchConfig, beam_search
    _, model = _bf16_model(seed=8)
    G, W, mx, hi = 3, 4, 12, 32000
    x, _ = _prompts(np.random.default_rng(14), "nlp", G, hi)
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_hi=hi)
    stats = {}
    ids, lengths, scores = beam_search(model, x, bc, stats=stats)
    assert stats["path"] == "ring" and stats["token_calls"] == mx - 1
    assert stats["parent_switches"] > 0
    assert (lengths == mx).all()
    errs = []
    for g in range(G):
        assert (np.diff(scores[g].numpy()) <= 0).all()
        for r in range(W):
            want = _list_form_score(model, x, g, ids[g, r].numpy(), mx, 0, hi, 1.0)
            errs.append(abs(float(scores[g, r]) - want))
    # bf16: per-token log-prob noise of the ring path against the list-form path, averaged over the 12 tokens of a hypothesis
    print("bf16 ring beam score |err| max", max(errs))
    assert max(errs) < 2e-2, max(errs)
    # the graphed ring path and the same kernels launched eagerly over the same ring: identical bits
    e_ids, e_len, e_sc = beam_search(model, x, bc, replay=False)
    assert torch.equal(ids, e_ids) and torch.equal(lengths, e_len) and torch.equal(scores.view(torch.int32), e_sc.view(torch.int32))


def test_eos_pool_and_early_stop():
    from bdm_db1_amd import BeamSearchConfig, beam_search
    from bdm_db1_amd.data import NLPTaskInput
    cfg, model, oracle = _fp32_model()
    G, W, mx, lo, hi = 3, 2, 20, 0, 6
    x, xo = _prompts(np.random.default_rng(15), "nlp", G, cfg["text_vocab_size"])
    lm = _OracleLM(cfg, oracle, xo)
    # the EOS: the token the oracle's beams pick most often at step 0 (the model reaches it)
    eos = int(np.argmax(np.bincount([int(np.argmax(lm.get(g, [])[0][lo:hi])) for g in range(G)], minlength=hi)))
    bc = BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=W, vocab_lo=lo, vocab_hi=hi, eos_id=eos, pad_id=hi + 3,
                          sync_every=2, length_penalty=0.0)
    ids, lengths, scores = beam_search(model, x, bc)
    rid, rlen, rsc, amb = _oracle_search(lm, G, W, mx, lo, hi, eos, hi + 3, 0.0, tol=1e-4)
    assert not amb.all() and (rlen < mx).any()          # (some hypothesis ends in EOS)
    ids, lengths = ids.numpy(), lengths.numpy()
    for g in range(G):
        for r in range(W):
            n = int(lengths[g, r])
            if n < mx:
                assert ids[g, r, n] == eos and (ids[g, r, n + 1:] == hi + 3).all()
            want = _oracle_score(lm, g, ids[g, r], n, lo, hi, eos, 0.0)
            assert abs(float(scores[g, r]) - want) <= 1e-4 * max(1.0, abs(want)), (g, r)
        if not amb[g]:
            assert (ids[g] == rid[g]).all() and (lengths[g] == rlen[g]).all(), g
    # early stop: prompts whose first choice is the EOS; one beam, no length normalisation -> every group is done at step 0, and the host
    # (looking every 2 tokens) stops after one call instead of mx - 1
    rng = np.random.default_rng(16)
    cands = rng.integers(0, cfg["text_vocab_size"], (40, 6))
    from oracle import db1_oracle as O
    lm40 = _OracleLM(cfg, oracle, [O.TaskBatch(kind="nlp", text_seq=cands[i:i + 1]) for i in range(40)])
    first = np.array([int(np.argmax(lm40.get(i, [])[0][lo:hi])) for i in range(40)])
    eos = int(np.argmax(np.bincount(first, minlength=hi)))
    pick = np.nonzero(first == eos)[0][:3]
    assert pick.size == 3
    xp = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(cands[pick]), text_len=None)
    stats = {}
    ids, lengths, scores = beam_search(model, xp, dataclasses.replace(bc, num_beams=1, num_return_sequences=1, eos_id=eos), stats=stats)
    assert stats["token_calls"] == 1 < mx - 1, stats
    assert (lengths.numpy() == 0).all() and (ids.numpy()[:, 0, 0] == eos).all() and (ids.numpy()[:, 0, 1:] == hi + 3).all()


def test_bf16_ring_holds_each_beams_own_history():
    """after a ring beam search, every row's last t keys / values equal those of a batch-1 ring fed the prompt and that beam's own tokens
    (wrong lineage -> keys of other tokens: an O(1) relative difference)"""
    from bdm_db1_amd import BeamSearchConfig, RingMemory, beam_search
    from bdm_db1_amd.data import NLPTaskInput
    _, model = _bf16_model(seed=8)
    G, W, mx, hi = 2, 4, 10, 32000
    x, _ = _prompts(np.random.default_rng(17), "nlp", G, hi)
    stats = {}
    beam_search(model, x, BeamSearchConfig(num_beams=W, max_new_tokens=mx, vocab_hi=hi), stats=stats)
    assert stats["path"] == "ring" and stats["parent_switches"] > 0
    gen = model._beam_generator
    toks, ring = gen.state.tokens.cpu().numpy(), gen.ring
    mlen, cap, t = int(model.mem_len), ring.cap, mx - 1
    s0 = int(ring.state.item())
    slots = torch.tensor([(s0 + mlen - t + i) % cap for i in range(t)], device=DEV)
    worst = 0.0
    with torch.no_grad():
        for g in range(G):
            xg = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=x.text_seq[g:g + 1].clone(), text_len=None)
            model._dec_state = None
            _, _, mems = model([xg], compute_loss=False, mems=model.init_mem(1))
            one = RingMemory(model, 1)
            for j in range(W):
                b = g * W + j
                one.load(mems)
                for i in range(t):
                    y = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(toks[b:b + 1, i:i + 1].astype(np.int64)),
                                     text_len=None)
                    model([y], compute_loss=False, mems=one)
                for layer in range(model.n_layer):
                    want = one.kv[layer][0, mlen:mlen + t].float()
                    got = ring.kv[layer][b, slots].float()
                    for i in range(t):
                        err = float((got[i] - want[i]).abs().max() / want[i].abs().max())
                        worst = max(worst, err)
    print("ring history rel err max", worst)
    assert worst < 5e-2, worst


@pytest.mark.parametrize("G", [1, 16])
def test_beam_captions_at_db1_1p3b_geometry(G):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, TransformerXL, generate_captions, synth
    from bdm_db1_amd.data import ICTaskInput
    cfg = synth.db1_config("1.3B")
    torch.manual_seed(11)
    model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)
    model.eval()
    rng = np.random.default_rng(7)
    batch = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(rng.integers(0, 32000, (G, 4))),
                        img_seq=_tdev(rng.standard_normal((G, 3, 224, 224)).astype(np.float32)), text_seq=None)
    stats = {}
    ids, lengths, scores = generate_captions(model, batch, BeamSearchConfig(num_beams=4, max_new_tokens=30, num_return_sequences=2), stats=stats)
    assert stats["path"] == "ring" and tuple(ids.shape) == (G, 2, 30) and tuple(scores.shape) == (G, 2)
    assert ((ids >= 0) & (ids < cfg.text_vocab_size)).all() and (lengths == 30).all()
    assert (scores[:, 0] >= scores[:, 1]).all() and torch.isfinite(scores).all()
    model._beam_generator = None
    b_ids, b_len, _ = generate_captions(model, batch, BeamSearchConfig(num_beams=1, max_new_tokens=30))
    model._beam_generator = None
    g_ids, g_len = generate_captions(model, batch, GenerationConfig(max_new_tokens=30))
    assert torch.equal(b_ids[:, 0], g_ids) and torch.equal(b_len[:, 0], g_len)


def test_dropped_graphed_steps_return_their_pinned_words():
    from bdm_db1_amd import GraphedRingStep, ops
    _, model = _bf16_model()
    for i in range(300):
        s = ops.new_chain_scratch(DEV)
        del s
    for i in range(260):
        step = GraphedRingStep(model, 1, 1)
        step(step.ids)
        del step
        if i % 64 == 0:
            gc.collect()
    step = GraphedRingStep(model, 1, 1)
    step(step.ids)
    step.check(synchronize=True)


def test_beam_search_rejects_bad_arguments():
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search
    cfg, model, _ = _fp32_model()
    x, _ = _prompts(np.random.default_rng(16), "nlp", 2, 300)
    with pytest.raises(ValueError):
        beam_search(model, x, BeamSearchConfig(max_new_tokens=cfg["mem_len"] + 1))
    with pytest.raises(ValueError):
        beam_search(model, x, BeamSearchConfig(vocab_hi=10 ** 6))
    with pytest.raises(ValueError):
        beam_search(model, x, BeamSearchConfig(), graphed=True)       # (fp32: no ring path)
    with pytest.raises(TypeError):
        beam_search(model, x, GenerationConfig())
    assert dataclasses.replace(BeamSearchConfig(), num_beams=2).num_beams == 2
