"""share_prompt=True in the model and in generation (decode.GroupedRingMemory, db1_relattn_decode_group_fwd): the launches it makes and no
longer makes, six hand-driven steps of both memories against an fp32 model, beam search and best-of-n scores against an fp32
teacher-forced score of the returned ids, graph replay against eager launches, the default path untouched, and the refusals -- on the
2-layer d_head = 128 model of the ring-prefill tests (n_position 128, mem_len 96) with an fp32 model on the same parameters."""
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

from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

MLEN = 96


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


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _prompt_ids(cfg, rows, L, seed):
    return np.random.default_rng(seed).integers(0, cfg["text_vocab_size"], (rows, L))


class _Count:
    def __init__(self, monkeypatch):
        from bdm_db1_amd import ops
        self.group, self.ring = [], 0
        real_group, real_ring = ops.relattn_decode_group_fwd, ops.relattn_decode_ring_fwd

        def group(*a, **k):
            self.group.append((int(a[3].shape[0]), int(a[5].shape[0])))       # (base rows, tail rows)
            return real_group(*a, **k)

        def ring(*a, **k):
            self.ring += 1
            return real_ring(*a, **k)
        monkeypatch.setattr(ops, "relattn_decode_group_fwd", group)
        monkeypatch.setattr(ops, "relattn_decode_ring_fwd", ring)

    def reset(self):
        self.group, self.ring = [], 0


# ------------------------------------------------------------------------------------------------------------------------------ 1. launches
@pytest.mark.parametrize("ring_prefill", [False, True])
def test_launches_with_and_without_the_flag(d128, monkeypatch, ring_prefill):
    from bdm_db1_amd import BeamSearchConfig, beam_search
    from bdm_db1_amd.decode import GroupedRingMemory, RingMemory
    cfg, model, _ = d128
    nl, G, W, n = cfg["n_layer"], 2, 4, 5
    prompt = _text(_prompt_ids(cfg, G, 70, 3))
    bc = BeamSearchConfig(max_new_tokens=n, num_beams=W, vocab_hi=cfg["text_vocab_size"])
    model.use_ring_prefill = ring_prefill
    try:
        for share in (True, False):
            beam_search(model, prompt, bc, share_prompt=share)          # (builds the cached generator: warm-up and capture launch too)
            cnt = _Count(monkeypatch)
            stats = {}
            beam_search(model, prompt, bc, share_prompt=share, replay=False, stats=stats)
            mem = model._beam_generator.ring
            assert stats["path"] == "ring" and stats["token_calls"] == n - 1
            if share:
                assert cnt.group == [(G, G * W)] * (nl * (n - 1)) and cnt.ring == 0
                assert isinstance(mem, GroupedRingMemory) and mem.base.B == G and all(k.shape[0] == G for k in mem.base.kv)
                assert all(tuple(k.shape[:2]) == (G * W, mem.cap_t) for k in mem.kv) and mem.cap_t >= n + 1 and mem.Lt == n
                assert int(mem.n_tail.cpu()) == n - 1 and int(mem.state.cpu()) == n - 1 and int(mem.status.cpu()) == 0
            else:
                assert cnt.group == [] and cnt.ring == nl * (n - 1)
                assert isinstance(mem, RingMemory) and mem.B == G * W
            monkeypatch.undo()
    finally:
        model.use_ring_prefill = False


# ------------------------------------------------------------------------------------------------------------------------------ 2. by hand
def test_six_steps_by_hand_against_the_fp32_model(d128):
    """the same ids and parents through a GroupedRingMemory, a RingMemory and the fp32 model's list-form memory: next-token logits of both
    bf16 paths against fp32, e_shared <= 2 e_default and below 3e-2 (the neighbouring tests' gate)"""
    from bdm_db1_amd import generation
    from bdm_db1_amd.decode import GroupedRingMemory, RingMemory
    cfg, model, m32 = d128
    G, W, steps = 2, 3, 6
    M = G * W
    rng = np.random.default_rng(11)
    prompt = _prompt_ids(cfg, G, 70, 12)
    ids = rng.integers(0, cfg["text_vocab_size"], (steps, M, 1))
    parents = [(np.arange(M) // W) * W + rng.integers(0, W, M) for _ in range(steps)]
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)
    with torch.no_grad():
        _, mems = generation._prefill(model, _text(prompt), G)
        shared = GroupedRingMemory(model, G, W, steps)
        shared.base.load(mems)
        shared.begin()
        plain = RingMemory(model, M)
        plain.load([m.repeat_interleave(W, 0) for m in mems])
        m32._dec_state = None
        _, _, mems32 = m32([_text(prompt)], compute_loss=False, mems=m32.init_mem(G))
        mems32 = [m.repeat_interleave(W, 0) for m in mems32]
        e_shared = e_plain = 0.0
        for s in range(steps):
            x = _text(ids[s])
            ref, _, mems32 = m32([x], compute_loss=False, mems=mems32)
            a, _, back = model([x], compute_loss=False, mems=shared)
            assert back is shared
            b, _, _ = model([x], compute_loss=False, mems=plain)
            ref = ref.double().cpu().numpy()
            e_shared = max(e_shared, float(np.abs(a.double().cpu().numpy() - ref).max() / np.abs(ref).max()))
            e_plain = max(e_plain, float(np.abs(b.double().cpu().numpy() - ref).max() / np.abs(ref).max()))
            t, par = i32([s + 1]), i32(parents[s])
            shared.reorder(par, t, max_t=steps, group=W)
            plain.reorder(par, t, max_t=steps, group=W)
            mems32 = [m.index_select(0, par.long()) for m in mems32]
        assert int(shared.n_tail.cpu()) == steps and int(shared.status.cpu()) == 0
        shared.check()
    print(f"next-token logits against fp32 over {steps} steps: e_shared = {e_shared:.3e}, e_default = {e_plain:.3e}")
    assert e_shared <= 2 * e_plain and e_shared < 3e-2


# ------------------------------------------------------------------------------------------------------------------------------ 3. the calls
def _fp32_scores(m32, prompt_row, ids, hi, alpha):
    """teacher-forced: sum_t log softmax(logits_t[:hi])[ids[r, t]] / n^alpha for the R continuations ``ids`` [R, n] of one prompt"""
    R, n = ids.shape
    idt = torch.as_tensor(np.asarray(ids, np.int64), device=DEV)
    with torch.no_grad():
        m32._dec_state = None
        logits, _, mems = m32([_text(np.repeat(prompt_row[None], R, 0))], compute_loss=False, mems=m32.init_mem(R))
        total = torch.zeros(R, dtype=torch.float64, device=DEV)
        for t in range(n):
            total += logits[:, -1, :hi].double().log_softmax(-1).gather(1, idt[:, t:t + 1])[:, 0]
            if t + 1 < n:
                logits, _, mems = m32([_text(ids[:, t:t + 1])], compute_loss=False, mems=mems)
    return (total / float(n) ** alpha).cpu().numpy()


def _distance(m32, prompt, out, hi, alpha):
    ids, lengths, scores = (x.numpy() for x in out)
    assert (lengths == ids.shape[2]).all()            # (no EOS: every hypothesis runs to the end)
    want = np.stack([_fp32_scores(m32, prompt[g], ids[g], hi, alpha) for g in range(ids.shape[0])])
    return float(np.abs(scores - want).max())


def _same(a, b):
    return all(torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_beam_search_scores_against_fp32_and_replay(d128):
    from bdm_db1_amd import BeamSearchConfig, beam_search
    cfg, model, m32 = d128
    hi = cfg["text_vocab_size"]
    G, W = 2, 4
    prompt = _prompt_ids(cfg, G, 70, 21)
    bc = BeamSearchConfig(max_new_tokens=7, num_beams=W, num_return_sequences=W, vocab_hi=hi)
    off = beam_search(model, _text(prompt), bc)
    stats = {}
    on = beam_search(model, _text(prompt), bc, share_prompt=True, stats=stats)
    assert stats["path"] == "ring" and tuple(on[0].shape) == tuple(off[0].shape) and tuple(on[2].shape) == (G, W)
    e_on, e_off = _distance(m32, prompt, on, hi, bc.length_penalty), _distance(m32, prompt, off, hi, bc.length_penalty)
    print(f"beam search W = {W}: |score - fp32 score of the returned ids| shared {e_on:.3e}, default {e_off:.3e}")
    assert e_on <= 2 * e_off
    assert _same(on, beam_search(model, _text(prompt), bc, share_prompt=True)), "two runs differ"
    assert _same(on, beam_search(model, _text(prompt), bc, share_prompt=True, replay=False)), "graph replay and eager launches differ"
    assert _same(off, beam_search(model, _text(prompt), bc)), "the default path changed after a shared call"
    assert _same(off, beam_search(model, _text(prompt), bc, share_prompt=False))


@pytest.mark.parametrize("n", [4, 17])
def test_best_of_scores_against_fp32(d128, n):
    from bdm_db1_amd import GenerationConfig, sample_best_of
    cfg, model, m32 = d128
    hi = cfg["text_vocab_size"]
    G = 2
    prompt = _prompt_ids(cfg, G, 70, 31)
    gc = GenerationConfig(max_new_tokens=6, greedy=False, top_k=50, seed=5, vocab_hi=hi)
    kw = dict(num_return_sequences=n, length_penalty=1.0)
    off = sample_best_of(model, _text(prompt), gc, n, **kw)
    stats = {}
    on = sample_best_of(model, _text(prompt), gc, n, share_prompt=True, stats=stats, **kw)
    assert stats["path"] == "ring" and model._best_of_generator.ring.W == n and model._best_of_generator.ring.base.B == G
    e_on, e_off = _distance(m32, prompt, on, hi, 1.0), _distance(m32, prompt, off, hi, 1.0)
    print(f"best of n = {n}: |score - fp32 score of the returned ids| shared {e_on:.3e}, default {e_off:.3e}")
    assert e_on <= 2 * e_off
    assert _same(on, sample_best_of(model, _text(prompt), gc, n, share_prompt=True, **kw)), "two runs differ"
    assert _same(off, sample_best_of(model, _text(prompt), gc, n, **kw)), "the default path changed after a shared call"


def test_captions_pass_the_keyword_on(d128):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, generation
    cfg, model, _ = d128
    seen = []
    real = generation._ring_generator

    def spy(model_, State, key):
        seen.append(key)
        return real(model_, State, key)
    generation._ring_generator = spy
    try:
        x = _text(_prompt_ids(cfg, 2, 20, 41))
        generation._run(model, x, BeamSearchConfig(max_new_tokens=3, num_beams=2, vocab_hi=cfg["text_vocab_size"]), share_prompt=True)
        generation._run(model, x, GenerationConfig(max_new_tokens=3, greedy=False, vocab_hi=cfg["text_vocab_size"]), n=3, share_prompt=True)
    finally:
        generation._ring_generator = real
    assert [type(k).__name__ for k in seen] == ["DecodeKeyShared", "DecodeKeyShared"]


# ------------------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(d128, monkeypatch):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search, generation, sample_best_of
    cfg, model, m32 = d128
    hi = cfg["text_vocab_size"]
    prompt = _text(_prompt_ids(cfg, 2, 20, 51))
    bc = BeamSearchConfig(max_new_tokens=3, num_beams=2, vocab_hi=hi)
    gc = GenerationConfig(max_new_tokens=3, greedy=False, vocab_hi=hi)
    cache = generation.PrefixCache(model, 2)
    handles = cache.put(prompt)
    prefixed = generation.Prefixed(cache, handles, _text(_prompt_ids(cfg, 2, 3, 52)))

    def no_model(*a, **k):
        raise AssertionError("the model was called")
    for m in (model, m32):
        monkeypatch.setattr(m, "_forward", no_model)
    with pytest.raises(ValueError, match="share_prompt"):
        beam_search(m32, prompt, bc, share_prompt=True)
    for kw in (dict(graphed=False), dict(kv_cache="fp8")):
        with pytest.raises(ValueError, match="share_prompt"):
            beam_search(model, prompt, bc, share_prompt=True, **kw)
        with pytest.raises(ValueError, match="share_prompt"):
            sample_best_of(model, prompt, gc, 3, share_prompt=True, **kw)
    with pytest.raises(ValueError, match="Prefixed"):
        beam_search(model, prefixed, bc, share_prompt=True)
    with pytest.raises(ValueError, match="Prefixed"):
        sample_best_of(model, prefixed, gc, 3, share_prompt=True)
    with pytest.raises(ValueError, match="mem_len"):
        sample_best_of(model, prompt, GenerationConfig(max_new_tokens=MLEN + 1, greedy=False, vocab_hi=hi), 3, share_prompt=True)
    with pytest.raises(ValueError, match="mem_len"):
        beam_search(model, prompt, BeamSearchConfig(max_new_tokens=MLEN + 1, num_beams=2, vocab_hi=hi), share_prompt=True)
    with pytest.raises(ValueError, match="G = W = 1"):
        sample_best_of(model, _text(_prompt_ids(cfg, 1, 20, 53)), gc, 1, share_prompt=True)
    from bdm_db1_amd import ops
    monkeypatch.setattr(ops, "relattn_decode_group_supported", lambda *a: False)
    with pytest.raises(ValueError, match="not supported for this model"):
        beam_search(model, prompt, bc, share_prompt=True)
    from bdm_db1_amd.decode import GroupedRingMemory
    with pytest.raises(ValueError):
        GroupedRingMemory(m32, 2, 2, 4)
    with pytest.raises(ValueError):
        GroupedRingMemory(model, 1, 1, 4)
