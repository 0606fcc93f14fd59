"""The prefix cache (generation.PrefixCache / Prefixed) in the model, in generation and in the streams, on the 2-layer d_head = 128 model of the
ring-prefill tests (n_position 128, mem_len 96) with an fp32 model on the same parameters: a 40-token prefix (or the image prompt) cached
once and continued by suffixes of 1, 7 and 70 tokens against the fp32 list-form chain ``model(prefix, mems=init)``, ``model(suffix, mems=...)``;
the forked ring rows; sharing; the cache stays as it was; the launches; the W-fold / n-fold expansion; mixed streams; the refusals."""
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

MLEN, LP = 96, 40


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
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids)), text_len=None)


def _image(cfg, G, seed):
    from bdm_db1_amd.data import ICTaskInput
    rng = np.random.default_rng(seed)
    return ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(rng.integers(0, cfg["text_vocab_size"], (G, 3))),
                       img_seq=_tdev(rng.standard_normal((G, 3, 32, 32)).astype(np.float32)), text_seq=_tdev(np.zeros((G, 0), np.int64)))


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _ids(cfg, rows, L, seed):
    return np.random.default_rng(seed).integers(0, cfg["text_vocab_size"], (rows, L))


def _rows_kv(ring, i, rows, H):
    """the K/V [len(rows), mlen, 2, H, D] of ring rows ``rows`` of layer i at origin 0 as float64 (an fp8 ring: through ops.kv8_unpack)"""
    from bdm_db1_amd import ops
    x = ring.kv[i].cpu()[rows][:, :MLEN]
    if ring.kv_dtype == "fp8":
        x = ops.kv8_unpack(x, H)[0]
    return x.double().numpy()


def _chain32(model32, prefix, suffix):
    """the fp32 model's list-form chain -> (last-position logits float64 [G, V], per layer the K/V [G, mlen, 2, H, D] it projects from
    the memory after the suffix)"""
    d, H, D = model32.d_model, model32.n_head, model32.d_head
    G = suffix.text_seq.shape[0]
    with torch.no_grad():
        _, _, mems = model32([prefix], compute_loss=False, mems=model32.init_mem(G))
        logits, _, mems = model32([suffix], compute_loss=False, mems=mems)
    kv = []
    for i, m in enumerate(mems):
        W = model32.W(f"h.{i}.dec_attn.qkv_net.weight").double().cpu().numpy()
        kv.append((m.double().cpu().numpy() @ W.T)[:, :, d:].reshape(G, MLEN, 2, H, D))
    return logits[:, -1].double().cpu().numpy(), kv


# ------------------------------------------------------------------------------------------------ 1. next token, forked rows, read-only cache
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("Ls", [1, 7, 70])
@pytest.mark.parametrize("kind", ["text", "image"])
def test_continuation_against_the_fp32_chain(d128, kind, Ls, kv):
    """next-token logits within 3e-2 of max (the ring-prefill tests' gate; measured 2e-3 .. 4e-3 on both formats) and the forked rows' K/V
    no further from fp32 than twice what the list-form chain + load_rows leaves in a ring of the same format"""
    from bdm_db1_amd import PrefixCache, Prefixed, RingMemory, generation
    cfg, model, model32 = d128
    nl, H, G = cfg["n_layer"], cfg["n_head"], 2
    pre_ids = _ids(cfg, G, LP, 11)
    prefix = _text(pre_ids) if kind == "text" else _image(cfg, G, 12)
    suffix = _text(_ids(cfg, G, Ls, 13 + Ls))
    cache = PrefixCache(model, 3, kv_cache=kv)
    handles = cache.put(prefix)
    assert [h.row for h in handles] == [0, 1] and cache.free == 1
    snap = [k.clone() for k in cache.ring.kv]
    with torch.no_grad():
        ring = RingMemory(model, 4, kv_dtype=kv)
        before = [k.clone() for k in ring.kv]
        p = Prefixed(cache, [handles[1], handles[0]], suffix)              # (call row 0 continues cache row 1)
        logits = generation._prefill_ring(model, p, ring, _i32(3, 1))
        torch.cuda.synchronize()
        assert tuple(logits.shape) == (G, Ls, model.total_vocab_size) and int(ring.load_status.cpu()) == 0 and int(ring.state.cpu()) == 0
        assert int(cache.ring.state.cpu()) == 0 and all(torch.equal(a, b) for a, b in zip(cache.ring.kv, snap)), "the cache ring changed"
        for i in range(nl):
            assert torch.equal(ring.kv[i][[0, 2]], before[i][[0, 2]]) and torch.equal(ring.kv[i][[3, 1], MLEN:], before[i][[3, 1], MLEN:])
        # the chain the continuation replaces, on the bf16 model: list-form prefix, list-form suffix, load_rows
        old = RingMemory(model, 4, kv_dtype=kv)
        pick = lambda t: generation._take(prefix, t, G, [1, 0])
        swapped = _text(pre_ids[[1, 0]]) if kind == "text" else type(prefix)(position_id=None, attention_mask=None, loss_mask=None, label=None,
                                                                                     prompt_seq=pick("prompt_seq"), img_seq=pick("img_seq"),
                                                                                     text_seq=prefix.text_seq)
        _, mems = generation._prefill(model, swapped, G)
        lo, _, mems = model([suffix], compute_loss=False, mems=mems)
        old.load_rows(mems, _i32(3, 1))
        torch.cuda.synchronize()
    ref_logits, ref_kv = _chain32(model32, swapped, suffix)
    new = logits[:, -1].double().cpu().numpy()
    e_log = float(np.abs(new - ref_logits).max() / np.abs(ref_logits).max())
    e_log_old = float(np.abs(lo[:, -1].double().cpu().numpy() - ref_logits).max() / np.abs(ref_logits).max())
    e_new = e_old = 0.0
    for i in range(nl):
        scale = np.abs(ref_kv[i]).max()
        e_new = max(e_new, float(np.abs(_rows_kv(ring, i, [3, 1], H) - ref_kv[i]).max() / scale))
        e_old = max(e_old, float(np.abs(_rows_kv(old, i, [3, 1], H) - ref_kv[i]).max() / scale))
    print(f"{kind} prefix, suffix {Ls}, {kv} cache: last logits vs fp32 chain {e_log:.3e} (bf16 list-form chain {e_log_old:.3e}); "
          f"forked K/V e_new = {e_new:.3e}, e_old = {e_old:.3e}")
    assert e_log < 3e-2
    assert e_new <= 2 * e_old


# -------------------------------------------------------------------------------------------------------------------------------- 2. sharing
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_three_requests_sharing_one_handle(d128, kv):
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, generate
    cfg, model, _ = d128
    one = _ids(cfg, 1, LP, 21)
    cache = PrefixCache(model, 4, kv_cache=kv)
    h = cache.put(_text(np.repeat(one, 4, 0)))               # four copies of one prefix, each in a row of its own
    for i in range(len(cache.ring.kv)):
        assert all(torch.equal(cache.ring.kv[i][0, :MLEN], cache.ring.kv[i][r, :MLEN]) for r in (1, 2, 3))
    snap = [k.clone() for k in cache.ring.kv]
    suffix = _text(_ids(cfg, 3, 7, 22))
    gcfg = GenerationConfig(max_new_tokens=4, logprobs=True)
    shared = generate(model, Prefixed(cache, [h[3]] * 3, suffix), gcfg, kv_cache=kv)
    ring_shared = [k.clone() for k in model._generator.ring.kv]
    copies = generate(model, Prefixed(cache, h[:3], suffix), gcfg, kv_cache=kv)
    for a, b in zip(shared, copies):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(ring_shared, model._generator.ring.kv)), "the requests' ring rows differ"
    assert all(torch.equal(a, b) for a, b in zip(cache.ring.kv, snap)), "the cache ring changed"


# ------------------------------------------------------------------------------------------------------------------------------- 3. launches
class _Count:
    """calls of the two new ops (and of the two they stand in for), input rows of every ops.gemm, entries into model._decode_begin"""

    def __init__(self, monkeypatch, model):
        from bdm_db1_amd import ops
        self.n = dict(relattn_mem_ring_fwd=0, ring_fork_rows=0, relattn_mem_kv_fwd=0, ring_prefill_rows=0, begin=0)
        self.gemm_rows = []

        def wrap(name, real):
            def f(*a, **k):
                self.n[name] += 1
                return real(*a, **k)
            return f
        for name in ("relattn_mem_ring_fwd", "ring_fork_rows", "relattn_mem_kv_fwd", "ring_prefill_rows"):
            monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
        real_gemm = ops.gemm

        def gemm(*a, **k):
            self.gemm_rows.append(int(a[0].shape[0]))
            return real_gemm(*a, **k)
        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(model, "_decode_begin", wrap("begin", model._decode_begin))

    def reset(self):
        self.n = {k: 0 for k in self.n}
        self.gemm_rows = []


def test_launches_of_a_continuation(d128, monkeypatch):
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, generate
    cfg, model, _ = d128
    nl, G, Ls = cfg["n_layer"], 3, 7
    cache = PrefixCache(model, 2)
    h = cache.put(_text(_ids(cfg, 1, LP, 31)))
    p = Prefixed(cache, h * G, _text(_ids(cfg, G, Ls, 32)))
    gcfg = GenerationConfig(max_new_tokens=3)
    generate(model, p, gcfg)                                 # (builds the cached generator)
    cnt = _Count(monkeypatch, model)
    out = generate(model, p, gcfg)
    assert tuple(out[0].shape) == (G, 3)
    assert cnt.n == dict(relattn_mem_ring_fwd=nl, ring_fork_rows=nl, relattn_mem_kv_fwd=0, ring_prefill_rows=0, begin=0)
    # no projection over the prefix's rows or the memory's: every GEMM of the prefill has the suffix's G * Ls rows
    assert cnt.gemm_rows.count(G * Ls) >= nl and not {G * (LP + Ls), G * LP, G * MLEN, G * (MLEN + Ls), LP, MLEN} & set(cnt.gemm_rows)
    cnt.reset()
    cache.put(_text(_ids(cfg, 1, LP, 33)))                   # put is the existing ring prefill, whatever model.use_ring_prefill says
    assert model.use_ring_prefill is False and cnt.n["relattn_mem_kv_fwd"] == nl and cnt.n["ring_prefill_rows"] == nl and cnt.n["ring_fork_rows"] == 0
    with pytest.raises(RuntimeError):
        cache.put(_text(_ids(cfg, 1, LP, 34)))               # no free row


# ------------------------------------------------------------------------------------------------------------------------------ 4. expansion
def test_expansion_to_beams_and_samples(d128, monkeypatch):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, PrefixCache, Prefixed, RingMemory, beam_search, generation, sample_best_of
    cfg, model, _ = d128
    G, W, mx = 2, 3, 4
    cache = PrefixCache(model, 2)
    h = cache.put(_text(_ids(cfg, 2, LP, 41)))
    p = Prefixed(cache, [h[1], h[1]], _text(_ids(cfg, G, 7, 42)))
    with torch.no_grad():
        plain = RingMemory(model, G)
        plain_logits = generation._prefill_ring(model, p, plain)              # the non-expanded continuation: row g from call row g
    seen = []
    real = generation._prefill_ring

    def recorded(model_, prompt, ring, rows=None, expand=None):
        out = real(model_, prompt, ring, rows, expand)
        seen.append((expand, int(ring.state.cpu()), [k[:, :MLEN].clone() for k in ring.kv], out.clone()))
        return out
    monkeypatch.setattr(generation, "_prefill_ring", recorded)
    b_ids, b_len, b_sc = beam_search(model, p, BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=2))
    assert tuple(b_ids.shape) == (G, 2, mx) and tuple(b_len.shape) == (G, 2) and tuple(b_sc.shape) == (G, 2)
    s_ids, s_len, s_sc = sample_best_of(model, p, GenerationConfig(max_new_tokens=mx, greedy=False, seed=5), n=W)
    assert tuple(s_ids.shape) == (G, 1, mx) and tuple(s_len.shape) == (G, 1) and tuple(s_sc.shape) == (G, 1)
    assert [e for e, _, _, _ in seen] == [W, W]
    for _, origin, kv, logits in seen:
        assert origin == 0 and torch.equal(logits, plain_logits)
        for i, k in enumerate(kv):
            assert k.shape[0] == G * W
            for g in range(G):
                for w in range(W):
                    assert torch.equal(k[g * W + w], plain.kv[i][g, :MLEN]), ("row", g * W + w, "is not the continuation of call row", g, "layer", i)


# --------------------------------------------------------------------------------------------------------------------------------- 5. stream
def _teacher_forced(model32, prompt_ids, gen_ids):
    """log-probabilities (over the whole vocabulary) of ``gen_ids`` after ``prompt_ids`` under the fp32 model's list-form path, one call"""
    seq = np.concatenate([prompt_ids, gen_ids[:-1]])[None]
    with torch.no_grad():
        logits, _, _ = model32([_text(seq)], compute_loss=False, mems=model32.init_mem(1))
    lp = torch.log_softmax(logits[0, len(prompt_ids) - 1:].double(), -1).cpu().numpy()
    return lp[np.arange(len(gen_ids)), gen_ids]


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_stream_mixes_prefixed_and_plain_requests(d128, kv):
    """the existing stream gate: the log-probs' largest deviation from the fp32 model teacher-forced on the same ids is at most twice that of
    the same requests as plain prompts (prefix ++ suffix) through the list-form admissions, on a ring of the same format"""
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, generate_many
    cfg, model, model32 = d128
    gcfg = GenerationConfig(max_new_tokens=5, logprobs=True)
    pre = _ids(cfg, 2, LP, 51)
    cache = PrefixCache(model, 2, kv_cache=kv)
    h = cache.put(_text(pre))
    snap = [k.clone() for k in cache.ring.kv]
    s7, s9, plain40, plain9 = _ids(cfg, 3, 7, 52), _ids(cfg, 1, 9, 53), _ids(cfg, 1, 40, 54), _ids(cfg, 1, 9, 55)
    which = [0, 0, 1]                                        # the handles of the three 7-token suffixes
    reqs = [Prefixed(cache, [h[w] for w in which[:2]], _text(s7[:2])), _text(plain40), Prefixed(cache, [h[1]], _text(s9)), _text(plain9),
            Prefixed(cache, [h[which[2]]], _text(s7[2:]))]
    full = [np.concatenate([pre[which[0]], s7[0]]), np.concatenate([pre[which[1]], s7[1]]), plain40[0], np.concatenate([pre[1], s9[0]]), plain9[0],
            np.concatenate([pre[which[2]], s7[2]])]
    as_plain = [_text(f[None]) for f in full]

    def run(items, slots):
        stats = {}
        return generate_many(model, items, gcfg, slots=slots, stats=stats, kv_cache=kv), stats

    def deviation(out):
        worst = 0.0
        for f, ids, n, lp in zip(full, *out):
            g = ids.numpy().astype(np.int64)
            assert int(n) == len(g) == 5
            worst = max(worst, float(np.abs(lp.numpy().astype(np.float64) - _teacher_forced(model32, f, g)).max()))
        return worst

    (a, sa), (b, sb), (base, sbase) = run(reqs, 6), run(reqs, 6), run(as_plain, 6)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) if torch.is_tensor(u) else u == v for u, v in zip(x, y)), "two runs differ"
    # six slots, six requests: one admission; the three 7-token suffixes share one continuation call, the 9-token one has its own
    assert sa["prefixed"] == 4 and sa["admitted"] == 6 and sa["prefill_calls"] == 4 and sbase["prefixed"] == 0 and sbase["admitted"] == 6
    d_new, d_base = deviation(a), deviation(base)
    print(f"stream logprobs vs the fp32 model teacher-forced on the same ids, {kv} ring: prefixed + plain {d_new:.3e}, all plain {d_base:.3e}")
    assert d_new <= 2 * d_base
    (c, sc) = run(reqs, 2)                                   # two slots: the requests come in over several admissions
    assert sc["prefixed"] == 4 and sc["admitted"] == 6 and len(c[0]) == 6
    assert all(torch.equal(x, y) for x, y in zip(cache.ring.kv, snap)), "the cache ring changed"


def test_answer_stream_takes_the_vqa_helpers_pair(d128):
    """image_prefix + question_suffixes through answer_stream: the requests of generate_many over the same Prefixed prompts, and as many
    prefixed admissions as questions"""
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, answer_stream, generate_many, image_prefix, question_suffixes
    from bdm_db1_amd.data import VQATaskInput
    from bdm_db1_amd.generation import _text_window
    cfg, model, _ = d128
    rng = np.random.default_rng(71)
    vqa = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(rng.integers(0, cfg["text_vocab_size"], (3, 3))),
                       img_seq=_tdev(rng.standard_normal((3, 3, 32, 32)).astype(np.float32)), text_seq=_tdev(rng.integers(1, cfg["text_vocab_size"], (3, 9))),
                       ques_len=torch.tensor([9, 4, 9]))
    cache = PrefixCache(model, 3)
    h = cache.put(image_prefix(vqa))
    items = [Prefixed(cache, [h[int(r)] for r in rows], suffix) for suffix, rows in question_suffixes(vqa)]
    assert [len(p.handles) for p in items] == [1, 2] and [p.suffix_len for p in items] == [4, 9]
    gcfg, stats = GenerationConfig(max_new_tokens=4), {}
    got = sorted(answer_stream(model, items, gcfg, slots=2, stats=stats), key=lambda r: r[0])
    want = generate_many(model, items, _text_window(model, gcfg), slots=2)
    assert stats["prefixed"] == 3 and [r[0] for r in got] == [0, 1, 2]
    assert all(torch.equal(r[1], ids) and r[2] == n for r, ids, n in zip(got, *want))


# ------------------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(d128, monkeypatch):
    from bdm_db1_amd import (BeamSearchConfig, GenerationConfig, PrefixCache, Prefixed, RingMemory, RingPrefill, beam_search, generate, generate_many,
                             rank_candidates, sample_best_of, score_document)
    cfg, model, model32 = d128
    with pytest.raises(ValueError):
        PrefixCache(model32, 2)                              # an fp32 model has no ring prefill
    cache, cache8 = PrefixCache(model, 2), PrefixCache(model, 2, kv_cache="fp8")
    h, h8 = cache.put(_text(_ids(cfg, 1, LP, 61))), cache8.put(_text(_ids(cfg, 1, LP, 61)))
    p, p8 = Prefixed(cache, h * 2, _text(_ids(cfg, 2, 7, 62))), Prefixed(cache8, h8 * 2, _text(_ids(cfg, 2, 7, 62)))
    gcfg = GenerationConfig(max_new_tokens=3)
    with torch.no_grad():
        ring = RingMemory(model, 2)
    cnt = _Count(monkeypatch, model)
    for call in (lambda: generate(model32, p, gcfg), lambda: generate(model, p, gcfg, graphed=False), lambda: generate(model, p, gcfg, kv_cache="fp8"),
                 lambda: generate(model, p8, gcfg), lambda: beam_search(model, p8, BeamSearchConfig(num_beams=2, max_new_tokens=3)),
                 lambda: sample_best_of(model, p, GenerationConfig(max_new_tokens=3, greedy=False), n=2, graphed=False),
                 lambda: generate_many(model, [p, p8], gcfg, slots=2), lambda: generate_many(model, [p], gcfg, slots=2, kv_cache="fp8"),
                 lambda: rank_candidates(model, p, [[1, 2]]), lambda: score_document(model, p), lambda: cache.put(p),
                 lambda: Prefixed(cache, h, _text(_ids(cfg, 1, 0, 63)))):
        with pytest.raises(ValueError):
            call()
    with torch.no_grad():
        for bad in (dict(base=ring), dict(base=cache8.ring), dict(base=cache.ring, base_rows=torch.tensor([0, 0], device=DEV)),
                    dict(base=cache.ring, base_rows=_i32(0, 0, 0))):
            with pytest.raises(ValueError):
                model([p.suffix], compute_loss=False, mems=RingPrefill(ring, **bad))
    torch.cuda.synchronize()
    assert not any(cnt.n.values()) and cnt.gemm_rows == []
    model._wversion += 1                                     # a weight change: the handles are stale
    try:
        with pytest.raises(RuntimeError):
            generate(model, p, gcfg)
    finally:
        model._wversion -= 1
    assert tuple(generate(model, p, gcfg)[0].shape) == (2, 3)
