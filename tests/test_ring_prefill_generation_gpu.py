"""The prefill straight into the K/V ring (decode.RingPrefill, model.use_ring_prefill) in the model and in generation: the launches it makes
and no longer makes, the ring content against an fp32 model (and against the list-form prefill + load_rows it replaces), the next token, the
W-fold / n-fold expansion, the stream's admissions, and the refusals -- on a 2-layer d_head = 128 model (n_position 128, mem_len 96) with an
fp32 model on the same parameters."""
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


@pytest.fixture
def flag(d128):
    """model.use_ring_prefill = True for one test"""
    model = d128[1]
    model.use_ring_prefill = True
    yield model
    model.use_ring_prefill = False


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids)), text_len=None)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _prompt_ids(cfg, rows, L, seed):
    return np.random.default_rng(seed).integers(0, cfg["text_vocab_size"], (rows, L))


class _Count:
    """calls of the new ops, input rows of every ops.gemm, entries into model._decode_begin"""

    def __init__(self, monkeypatch, model):
        from bdm_db1_amd import ops
        self.kv, self.fill, self.gemm_rows, self.begin = [], 0, [], 0
        real_kv, real_fill, real_gemm, real_begin = ops.relattn_mem_kv_fwd, ops.ring_prefill_rows, ops.gemm, model._decode_begin

        def kv(*a, **k):
            self.kv.append((a[9], a[10], a[11]))           # (B, q, mlen)
            return real_kv(*a, **k)

        def fill(*a, **k):
            self.fill += 1
            return real_fill(*a, **k)

        def gemm(*a, **k):
            self.gemm_rows.append(int(a[0].shape[0]))
            return real_gemm(*a, **k)

        def begin(*a, **k):
            self.begin += 1
            return real_begin(*a, **k)
        monkeypatch.setattr(ops, "relattn_mem_kv_fwd", kv)
        monkeypatch.setattr(ops, "ring_prefill_rows", fill)
        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(model, "_decode_begin", begin)

    def reset(self):
        self.kv, self.fill, self.gemm_rows, self.begin = [], 0, [], 0


# ------------------------------------------------------------------------------------------------------------------------------ 1. launches
def test_launches_with_and_without_the_flag(d128, monkeypatch):
    from bdm_db1_amd import GenerationConfig, RingMemory, RingPrefill, generate, generation
    cfg, model, _ = d128
    nl, L, n = cfg["n_layer"], 70, 2
    prompt = _text(_prompt_ids(cfg, n, L, 70))
    gcfg = GenerationConfig(max_new_tokens=3)
    assert model.use_ring_prefill is False and model.ring_prefill_supported and model.ring_prefill_ok(L)
    with torch.no_grad():
        ring = RingMemory(model, n)
        RingPrefill(ring).zero_kv()                       # (the zero-memory K/V row: once per weight version, not part of a prefill)
        cnt = _Count(monkeypatch, model)
        logits = generation._prefill_ring(model, prompt, ring)
        assert tuple(logits.shape) == (n, L, model.total_vocab_size)
        assert cnt.kv == [(n, L, MLEN)] * nl and cnt.fill == nl and cnt.begin == 0
        assert n * (MLEN + L) not in cnt.gemm_rows and n * MLEN not in cnt.gemm_rows and cnt.gemm_rows.count(n * L) >= nl
        assert int(ring.state.cpu()) == 0 and int(ring.load_status.cpu()) == 0
        # the list-form prefill + load it replaces: what it launches today
        cnt.reset()
        _, mems = generation._prefill(model, prompt, n)
        ring.load(mems)
        assert cnt.kv == [] and cnt.fill == 0
        assert cnt.gemm_rows.count(n * (MLEN + L)) == nl and cnt.gemm_rows.count(n * MLEN) == nl and cnt.begin == 2
    # through generate: flag off -- none of the new functions; flag on -- n_layer each, no projection of memory rows
    generate(model, prompt, gcfg)                         # (builds the cached generator)
    cnt.reset()
    off = generate(model, prompt, gcfg)
    assert cnt.kv == [] and cnt.fill == 0 and cnt.gemm_rows.count(n * (MLEN + L)) == nl and cnt.gemm_rows.count(n * MLEN) == nl and cnt.begin == 2
    gen_before = model._generator
    model.use_ring_prefill = True
    try:
        generate(model, prompt, gcfg)                     # (the zero-memory row of the generator's own ring)
        cnt.reset()
        on = generate(model, prompt, gcfg)
    finally:
        model.use_ring_prefill = False
    assert model._generator is gen_before                 # the flag joins no cache key: the same ring, the same captured graph
    assert cnt.kv == [(n, L, MLEN)] * nl and cnt.fill == nl and cnt.begin == 0
    assert n * (MLEN + L) not in cnt.gemm_rows and n * MLEN not in cnt.gemm_rows
    assert tuple(on[0].shape) == tuple(off[0].shape) == (n, 3)


# -------------------------------------------------------------------------------------------------------------------------- 2. ring content
def _ring_rows_kv(ring, i, rows, origin, H):
    """the K/V [len(rows), mlen, 2, H, D] of ring rows ``rows`` of layer i as float64 (an fp8 ring: dequantised through ops.kv8_unpack)"""
    from bdm_db1_amd import ops
    slots = (origin + torch.arange(MLEN)) % ring.cap
    x = ring.kv[i].cpu()[rows][:, slots]
    if ring.kv_dtype == "fp8":
        x = ops.kv8_unpack(x, H)[0]
    return x.double().numpy()


def _fp32_kv(model32, ids):
    """per layer the K/V [rows, mlen, 2, H, D] (float64) the fp32 model projects from its own list-form memory after the prompt ``ids``"""
    d, H, D = model32.d_model, model32.n_head, model32.d_head
    with torch.no_grad():
        _, _, mems = model32([_text(ids)], compute_loss=False, mems=model32.init_mem(ids.shape[0]))
    out = []
    for i, m in enumerate(mems):
        W = model32.W(f"h.{i}.dec_attn.qkv_net.weight").double().cpu().numpy()
        out.append((m.double().cpu().numpy() @ W.T)[:, :, d:].reshape(ids.shape[0], MLEN, 2, H, D))
    return out


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_ring_content_after_an_admission(d128, kv_dtype):
    from bdm_db1_amd import RingMemory, RingPrefill, generation
    cfg, model, model32 = d128
    nl, H = cfg["n_layer"], cfg["n_head"]
    ids = _prompt_ids(cfg, 2, 70, 271)
    rows = [3, 1]
    with torch.no_grad():
        ring = RingMemory(model, 4, kv_dtype=kv_dtype)
        for s in range(3):                                 # a few decode calls: the origin moves to 6
            model([_text(_prompt_ids(cfg, 4, 2, 900 + s))], compute_loss=False, mems=ring)
        origin = int(ring.state.cpu())
        assert origin == 6
        snap = [k.clone() for k in ring.kv]
        logits, none, back = model([_text(ids)], compute_loss=False, mems=RingPrefill(ring, _i32(*rows)))
        torch.cuda.synchronize()
        assert none is None and isinstance(back, RingPrefill) and tuple(logits.shape) == (2, 70, model.total_vocab_size)
        assert int(ring.state.cpu()) == origin and int(ring.load_status.cpu()) == 0
        covered = ((origin + torch.arange(MLEN)) % ring.cap).tolist()
        uncovered = [s for s in range(ring.cap) if s not in covered]
        assert len(uncovered) == 64
        for i in range(nl):
            assert torch.equal(ring.kv[i][[0, 2]], snap[i][[0, 2]]), "a row that was not admitted changed"
            assert torch.equal(ring.kv[i][rows][:, uncovered], snap[i][rows][:, uncovered]), "a slot outside the window changed"
            assert not torch.equal(ring.kv[i][rows][:, covered], snap[i][rows][:, covered])
        # the old path into a second ring: list-form prefill, then load_rows
        old = RingMemory(model, 4, kv_dtype=kv_dtype)
        _, mems = generation._prefill(model, _text(ids), 2)
        old.load_rows(mems, _i32(*rows))
        torch.cuda.synchronize()
    ref = _fp32_kv(model32, ids)
    e_new = e_old = 0.0
    for i in range(nl):
        scale = np.abs(ref[i]).max()
        en = float(np.abs(_ring_rows_kv(ring, i, rows, origin, H) - ref[i]).max() / scale)
        eo = float(np.abs(_ring_rows_kv(old, i, rows, 0, H) - ref[i]).max() / scale)
        print(f"ring K/V vs fp32, {kv_dtype} ring, layer {i}: max-norm rel err new path {en:.3e}, old path {eo:.3e}")
        e_new, e_old = max(e_new, en), max(e_old, eo)
    print(f"ring K/V vs fp32, {kv_dtype} ring: e_new = {e_new:.3e}, e_old = {e_old:.3e}")
    assert e_new <= 2 * e_old


# ---------------------------------------------------------------------------------------------------------------------------- 3. next token
def test_next_token_after_either_prefill(d128):
    from bdm_db1_amd import RingMemory, RingPrefill, generation
    cfg, model, model32 = d128
    ids, nxt = _prompt_ids(cfg, 2, 70, 33), _prompt_ids(cfg, 2, 2, 34)
    last = lambda t: t[:, -1].double().cpu().numpy()
    with torch.no_grad():
        ring = RingMemory(model, 2)
        model([_text(ids)], compute_loss=False, mems=RingPrefill(ring))
        new = last(model([_text(nxt)], compute_loss=False, mems=ring)[0])
        _, mems = generation._prefill(model, _text(ids), 2)
        ring.load(mems)
        old = last(model([_text(nxt)], compute_loss=False, mems=ring)[0])
        _, _, mems32 = model32([_text(ids)], compute_loss=False, mems=model32.init_mem(2))
        ref = last(model32([_text(nxt)], compute_loss=False, mems=mems32)[0])
    e_new, e_old = (float(np.abs(x - ref).max() / np.abs(ref).max()) for x in (new, old))
    print(f"last-position logits of the call after the prefill vs fp32: new path {e_new:.3e}, old path {e_old:.3e}; "
          f"new vs old {float(np.abs(new - old).max() / np.abs(old).max()):.3e}")
    assert e_new < 3e-2 and e_old < 3e-2


# ------------------------------------------------------------------------------------------------------------------------------ 4. expansion
def test_expansion_to_beams_and_samples(d128, flag, monkeypatch):
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, RingMemory, RingPrefill, beam_search, generation, sample_best_of
    cfg, model = d128[0], flag
    G, W, mx = 2, 3, 4
    ids = _prompt_ids(cfg, G, 70, 44)
    with torch.no_grad():
        plain = RingMemory(model, G)
        model([_text(ids)], compute_loss=False, mems=RingPrefill(plain))        # the non-expanded prefill: row g from prompt g
    seen = []
    real = generation._prefill_ring

    def recorded(model_, prompt, ring, rows=None, expand=None):
        out = real(model_, prompt, ring, rows, expand)
        seen.append((expand, int(ring.state.cpu()), [k[:, :MLEN].clone() for k in ring.kv]))
        return out
    monkeypatch.setattr(generation, "_prefill_ring", recorded)
    b_ids, b_len, b_sc = beam_search(model, _text(ids), BeamSearchConfig(num_beams=W, max_new_tokens=mx, num_return_sequences=2))
    assert tuple(b_ids.shape) == (G, 2, mx) and tuple(b_len.shape) == (G, 2) and tuple(b_sc.shape) == (G, 2)
    s_ids, s_len, s_sc = sample_best_of(model, _text(ids), GenerationConfig(max_new_tokens=mx, greedy=False, seed=5), n=W)
    assert tuple(s_ids.shape) == (G, 1, mx) and tuple(s_len.shape) == (G, 1) and tuple(s_sc.shape) == (G, 1)
    assert [e for e, _, _ in seen] == [W, W]
    for _, origin, kv in seen:
        assert origin == 0
        for i, k in enumerate(kv):
            assert k.shape[0] == G * W
            for g in range(G):
                for w in range(W):
                    assert torch.equal(k[g * W + w], plain.kv[i][g, :MLEN]), ("row", g * W + w, "is not the prefill of prompt", g, "layer", i)


# --------------------------------------------------------------------------------------------------------------------------------- 5. stream
def _teacher_forced(model32, prompt_ids, gen_ids):
    """log-probabilities (over the whole vocabulary) of ``gen_ids`` after ``prompt_ids`` under the fp32 model's list-form path, one call"""
    seq = np.concatenate([prompt_ids, gen_ids[:-1]])[None]
    with torch.no_grad():
        logits, _, _ = model32([_text(seq)], compute_loss=False, mems=model32.init_mem(1))
    lp = torch.log_softmax(logits[0, len(prompt_ids) - 1:].double(), -1).cpu().numpy()
    return lp[np.arange(len(gen_ids)), gen_ids]


def test_stream_admissions(d128):
    from bdm_db1_amd import GenerationConfig, generate_many
    cfg, model, model32 = d128
    gcfg = GenerationConfig(max_new_tokens=5, logprobs=True)
    prompts = [_prompt_ids(cfg, 1, L, 500 + k)[0] for k, L in enumerate((70, 9, 40, 70, 40, 9))]
    reqs = [_text(p[None]) for p in prompts]

    def run(on, **kw):
        stats = {}
        model.use_ring_prefill = on
        try:
            out = generate_many(model, reqs, gcfg, slots=2, stats=stats, **kw)
        finally:
            model.use_ring_prefill = False
        return out, stats

    def deviation(out):
        worst = 0.0
        for p, ids, n, lp in zip(prompts, *out):
            g = ids.numpy().astype(np.int64)
            assert int(n) == len(g) == 5                   # (no eos_id: every request runs to its limit)
            worst = max(worst, float(np.abs(lp.numpy().astype(np.float64) - _teacher_forced(model32, p, g)).max()))
        return worst

    (off, s_off), (on, s_on), (on2, s_on2) = run(False), run(True), run(True)
    for a, b in zip(on, on2):
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b)), "two runs with the flag on differ"
    assert s_on["prefill_calls"] == s_off["prefill_calls"] and s_on["admitted"] == s_off["admitted"] == len(reqs)
    d_off, d_on = deviation(off), deviation(on)
    print(f"stream logprobs vs the fp32 model teacher-forced on the same ids: flag off {d_off:.3e}, flag on {d_on:.3e}")
    assert d_on <= 2 * d_off
    (f8, _), (f8b, _) = run(True, kv_cache="fp8"), run(True, kv_cache="fp8")
    for a, b, c in zip(f8, f8b, on):
        assert len(a) == len(c)
        for x, y, z in zip(a, b, c):
            assert (torch.equal(x, y) and x.shape == z.shape and x.dtype == z.dtype) if torch.is_tensor(x) else (x == y and type(x) is type(z))


# ------------------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(d128, monkeypatch):
    from bdm_db1_amd import GenerationConfig, RingMemory, RingPrefill, generate
    cfg, model, model32 = d128
    ids = _prompt_ids(cfg, 2, 70, 61)
    with pytest.raises(ValueError):
        RingMemory(model32, 2)                             # an fp32 model has no ring ...
    with torch.no_grad():
        ring = RingMemory(model, 4)
        RingPrefill(ring).zero_kv()
        before = [k.clone() for k in ring.kv]
        cnt = _Count(monkeypatch, model)
        with pytest.raises(ValueError):
            model32([_text(ids)], compute_loss=False, mems=RingPrefill(ring))        # ... and takes no RingPrefill of another model's
        for bad in (dict(rows=torch.tensor([3, 1], device=DEV)), dict(rows=_i32(3, 1).cpu()), dict(rows=_i32(0, 1, 2, 3, 0)),
                    dict(src=torch.tensor([0, 0, 1, 1], device=DEV)), dict(src=_i32(0, 1))):
            with pytest.raises(ValueError):
                RingPrefill(ring, **bad)
        with pytest.raises(ValueError):
            model([_text(ids)], compute_loss=False, mems=RingPrefill(ring))          # four destinations, two call rows, no src map
        model.train()
        try:
            with pytest.raises(ValueError):
                model([_text(ids)], compute_loss=False, mems=RingPrefill(ring, _i32(0, 1)))      # training mode
        finally:
            model.eval()
    with pytest.raises(ValueError):
        model([_text(ids)], compute_loss=False, mems=RingPrefill(ring, _i32(0, 1)))              # gradients enabled
    torch.cuda.synchronize()
    assert cnt.kv == [] and cnt.fill == 0 and all(torch.equal(a, b) for a, b in zip(ring.kv, before)) and int(ring.load_status.cpu()) == 0
    # the flag on a model that cannot take the path changes nothing
    gcfg = GenerationConfig(max_new_tokens=3)
    assert not model32.ring_prefill_supported
    a = generate(model32, _text(ids), gcfg)
    model32.use_ring_prefill = True
    try:
        b = generate(model32, _text(ids), gcfg)
    finally:
        model32.use_ring_prefill = False
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and cnt.kv == [] and cnt.fill == 0
