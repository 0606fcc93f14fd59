"""Generation (bdm_db1_amd.generation): the fp32 eager loop against the NumPy oracle's own greedy loop, the bf16 hipGraph ring loop against
the eager bf16 loop, RingMemory.load, seeds / stream ids, EOS and the early stop, and captions at the DB1-1.3B geometry."""
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
DEV = "cuda"

import select_rule as R  # noqa: E402
from gpu_common import _bf16_model, _fp32_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401


def _prompts(rng, kind, M, vocab):
    from oracle import db1_oracle as O
    x, fields = _prompt(rng, kind, M, vocab)
    return x, O.TaskBatch(kind=kind, **fields)


@pytest.mark.parametrize("kind", ["nlp", "ic"])
def test_fp32_greedy_generation_follows_the_oracle(kind):
    from oracle import db1_oracle as O
    from bdm_db1_amd import GenerationConfig, generate
    cfg, model, oracle = _fp32_model()
    M, n, hi = 2, 12, cfg["text_vocab_size"]
    x, xo = _prompts(np.random.default_rng(1), kind, M, hi)
    stats = {}
    ids, lengths = generate(model, x, GenerationConfig(max_new_tokens=n, vocab_hi=hi), stats=stats)
    assert stats["path"] == "eager" and stats["token_calls"] == n - 1
    ids = ids.numpy()
    assert ids.shape == (M, n) and (lengths.numpy() == n).all()
    # the oracle's loop, teacher-forced on the GPU's tokens: one token per call over its own memory
    mems = [np.zeros((M, cfg["mem_len"], cfg["n_embed"])) for _ in range(cfg["n_layer"])]
    logits, _, mems = oracle.forward([xo], compute_loss=False, mems=mems)
    for t in range(n):
        l = logits[:, -1, :hi]
        scale = np.abs(l).max()
        srt = np.sort(l, axis=1)
        for r in range(M):
            assert l[r, ids[r, t]] >= srt[r, -1] - 1e-4 * scale, (t, r)
            if t < 8:
                assert srt[r, -1] - srt[r, -2] > 1e-4 * scale, (t, r)   # (a clear winner: the tokens must be equal)
                assert ids[r, t] == np.argmax(l[r]), (t, r)
        logits, _, mems = oracle.forward([O.TaskBatch(kind="nlp", text_seq=ids[:, t:t + 1].astype(np.int64))], compute_loss=False, mems=mems)


def _teacher_forced(model, x, ids):
    """float64 logits [n, M, V] of the eager list-form path fed the prompt, then ids[:, t] one token per call"""
    from bdm_db1_amd.data import NLPTaskInput
    out = []
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([x], compute_loss=False, mems=model.init_mem(ids.shape[0]))
        for t in range(ids.shape[1]):
            out.append(logits[:, -1].double().cpu().numpy())
            y = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(ids[:, t:t + 1].astype(np.int64)),
                             text_len=None)
            logits, _, mems = model([y], compute_loss=False, mems=mems)
    return np.stack(out)


@pytest.mark.parametrize("greedy", [True, False])
def test_bf16_ring_generation_matches_the_eager_loop(greedy):
    from bdm_db1_amd import GenerationConfig, generate
    cfg, model = _bf16_model()
    M, n = 3, 16
    x, _ = _prompts(np.random.default_rng(2), "nlp", M, 32000)
    gc = GenerationConfig(max_new_tokens=n, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=32000)
    st_r, st_e = {}, {}
    ring, _ = generate(model, x, gc, stats=st_r)
    eager, _ = generate(model, x, gc, graphed=False, stats=st_e)
    assert st_r["path"] == "ring" and st_e["path"] == "eager"
    ring, eager = ring.numpy(), eager.numpy()
    tf = _teacher_forced(model, x, ring)
    assert (ring[:, 0] == eager[:, 0]).all()          # (the same prefill call)
    for r in range(M):
        for t in range(n):
            l = tf[t, r, :32000]
            scale = np.abs(l).max()
            noise = 2e-2 * scale
            if greedy:
                assert l[ring[r, t]] >= l.max() - noise, (r, t)
            else:   # inside the eager logits' top-p set, up to bf16 noise at its boundary
                kept = R.kept_set(l, 0, 32000, 1.0, 0, 0.9)[0]
                assert l[ring[r, t]] >= l[kept].min() - noise, (r, t)
            if ring[r, t] != eager[r, t]:     # the paths may only part at a near tie of the eager path
                srt = np.sort(l)
                if greedy:
                    assert srt[-1] - srt[-2] < noise, (r, t)
                break


def test_ring_memory_load_continues_a_prefill():
    """RingMemory.load(mems) after a 70-token prefill through the list-form path == the same 70 tokens fed through the ring in chunks of
    <= 64 (the next token's logits)"""
    from bdm_db1_amd import RingMemory
    from bdm_db1_amd.data import NLPTaskInput
    cfg, model = _bf16_model(mem_len=100)
    rng = np.random.default_rng(3)
    M = 2
    ids = rng.integers(0, 32000, (M, 70))
    nxt = rng.integers(0, 32000, (M, 1))
    mk = lambda a: NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(a), text_len=None)
    with torch.no_grad():
        model._dec_state = None
        _, _, mems = model([mk(ids)], compute_loss=False, mems=model.init_mem(M))
        loaded = RingMemory(model, M)
        loaded.load(mems)
        a = model([mk(nxt)], compute_loss=False, mems=loaded)[0].float().cpu().numpy()
        chunked = RingMemory(model, M)
        for c0 in (0, 64):
            model([mk(ids[:, c0:c0 + 64])], compute_loss=False, mems=chunked)
        b = model([mk(nxt)], compute_loss=False, mems=chunked)[0].float().cpu().numpy()
    err = np.abs(a - b).max() / np.abs(b).max()
    assert err < 1e-2, err
    with pytest.raises(ValueError):
        loaded.load(mems[:1])


def test_seeds_and_stream_ids():
    from bdm_db1_amd import GenerationConfig, generate
    cfg, model, _ = _fp32_model()
    hi = cfg["text_vocab_size"]
    x, _ = _prompts(np.random.default_rng(4), "nlp", 4, hi)
    gc = GenerationConfig(max_new_tokens=10, greedy=False, temperature=1.5, top_p=0.95, seed=77, vocab_hi=hi)
    a, _ = generate(model, x, gc, stream_ids=[10, 11, 12, 13])
    b, _ = generate(model, x, gc, stream_ids=[10, 11, 12, 13])
    c, _ = generate(model, x, dataclasses.replace(gc, seed=78), stream_ids=[10, 11, 12, 13])
    assert torch.equal(a, b) and not torch.equal(a, c)
    from bdm_db1_amd.data import NLPTaskInput
    one = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=x.text_seq[2:3].clone(), text_len=None)
    s, _ = generate(model, one, gc, stream_ids=[12])
    assert torch.equal(s[0], a[2])


def test_eos_pads_the_rest_and_stops_early():
    """EOS at a known step: the token greedy generation picks at step 2 of row 0 becomes eos_id"""
    from bdm_db1_amd import GenerationConfig, clip_at_eos, generate
    cfg, model = _bf16_model()
    x, _ = _prompts(np.random.default_rng(6), "nlp", 3, 32000)
    base, _ = generate(model, x, GenerationConfig(max_new_tokens=12, vocab_hi=32000))
    base = base.numpy()
    eos, pad = int(base[0, 2]), 31999
    stats = {}
    ids, lengths = generate(model, x, GenerationConfig(max_new_tokens=12, vocab_hi=32000, eos_id=eos, pad_id=pad), stats=stats)
    ids, lengths = ids.numpy(), lengths.numpy()
    for r in range(3):
        hit = np.nonzero(base[r] == eos)[0]
        n = int(hit[0]) if hit.size else 12
        assert lengths[r] == n
        assert (ids[r, :n] == base[r, :n]).all()
        if n < 12:
            assert ids[r, n] == eos and (ids[r, n + 1:] == pad).all()
    assert clip_at_eos(ids, lengths)[0] == base[0, :lengths[0]].tolist()
    # one row alone: EOS at step <= 2, the host looks every 4 tokens -> 3 replays instead of 11
    from bdm_db1_amd.data import NLPTaskInput
    one = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=x.text_seq[:1].clone(), text_len=None)
    stats = {}
    ids1, len1 = generate(model, one, GenerationConfig(max_new_tokens=12, vocab_hi=32000, eos_id=eos, pad_id=pad, sync_every=4), stats=stats)
    assert stats["path"] == "ring" and stats["token_calls"] == 3 < 11
    assert int(len1[0]) == lengths[0] and (ids1.numpy()[0] == ids[0]).all()


@pytest.mark.parametrize("M", [1, 16])
def test_captions_at_db1_1p3b_geometry(M):
    from bdm_db1_amd import GenerationConfig, TransformerXL, generate_captions, synth
    from bdm_db1_amd.data import ICTaskInput
    cfg = synth.db1_config("1.3B")
    torch.manual_seed(11)
    model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)
    model.eval()
    rng = np.random.default_rng(7)
    batch = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(rng.integers(0, 32000, (M, 4))),
                        img_seq=_tdev(rng.standard_normal((M, 3, 224, 224)).astype(np.float32)), text_seq=None)
    stats = {}
    ids, lengths = generate_captions(model, batch, GenerationConfig(max_new_tokens=30), stats=stats)   # (the ring chain is checked inside)
    assert stats["path"] == "ring" and tuple(ids.shape) == (M, 30)
    assert ((ids >= 0) & (ids < cfg.text_vocab_size)).all() and (lengths == 30).all()
    first, _ = generate_captions(model, batch, GenerationConfig(max_new_tokens=1), graphed=False)
    assert torch.equal(first[:, 0], ids[:, 0])
