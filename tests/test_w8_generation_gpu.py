"""fp8 decode weights through the model and the decoding loops (``model.set_decode_weights("fp8")``): the launches a decode step makes, the
logits bit for bit against a model that holds the dequantised weights in bf16, the accuracy against fp32 models, the caches a switch
invalidates, the loops, the untouched default and the setter's refusals."""
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

HI, PAD, MLEN = 32000, 31999, 40
MAPS = ("dec_attn.qkv_net.weight", "dec_attn.o_net.weight", "pos_ff.CoreNet.0.weight", "pos_ff.CoreNet.2.weight")


def _cfg(**kw):
    from bdm_db1_amd import synth
    return synth.db1_config("tiny", **{**dict(n_embed=512, n_head=4, n_layer=2, n_position=64, mem_len=MLEN, fp16=True), **kw})


def _build(dtype=torch.bfloat16, seed=11, **kw):
    from bdm_db1_amd import TransformerXL
    torch.manual_seed(seed)
    m = TransformerXL(_cfg(**kw), device=torch.device(DEV), compute_dtype=dtype)
    m.eval()
    return m


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _names(model):
    return [f"h.{i}.{m}" for i in range(model.n_layer) for m in MAPS]


def _with_dequantised_maps(src, dtype):
    """a model of ``dtype`` with ``src``'s parameters, the four linear maps of every layer replaced by w8_unpack(w8_pack(W)) of src's bf16 W"""
    from bdm_db1_amd import ops
    m = _build(dtype)
    m.load_state_dict(src.state_dict(), strict=False)
    with torch.no_grad():
        for name in _names(src):
            W = src.W(name)
            deq = ops.w8_unpack(ops.w8_pack(W.cpu()), *W.shape)[0]
            m.arena.view(m.arena.master, name).copy_(deq.to(DEV).float())
    m.sync_work_params()
    return m


@pytest.fixture(scope="module")
def models():
    """A: the model under test (the flag is switched by the tests, and left off); B: bf16, the dequantised maps, flag off, no chain"""
    A = _build()
    assert A.d_head == 128 and A._decode_fused_ok(1, False, None)
    B = _with_dequantised_maps(A, torch.bfloat16)
    B.use_decode_chain = False
    for name in _names(A):
        assert not torch.equal(A.W(name), B.W(name))                 # (the quantisation is not a no-op on these weights)
    return A, B


@pytest.fixture
def fp8(models):
    A = models[0]
    A.set_decode_weights("fp8")
    yield A
    A.set_decode_weights("bf16")


class _Count:
    """counts the launches of the fused decode branch's linear maps, by entry point; of db1_linear_decode only those over one of the layers'
    four matrices (the head streams its bf16 weight through the same entry point under either flag)"""

    def __init__(self, monkeypatch, model):
        from bdm_db1_amd import ops
        self.n = dict(w8=0, attn_w8=0, bf16=0, attn_bf16=0, chain=0)
        four = {model.W(n).data_ptr() for n in _names(model)}

        def wrap(name, key, own=lambda a: True):
            orig = getattr(ops, name)

            def f(*a, **k):
                if own(a):
                    self.n[key] += 1
                return orig(*a, **k)
            monkeypatch.setattr(ops, name, f)
        wrap("linear_decode_w8", "w8")
        wrap("linear_decode_attn_w8", "attn_w8")
        wrap("linear_decode", "bf16", lambda a: a[1].data_ptr() in four)
        wrap("linear_decode_attn", "attn_bf16")
        wrap("decode_chain", "chain")

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.n, 0)
        return n


@pytest.mark.parametrize("M", [1, 2, 4, 17])
def test_decode_steps_are_the_bf16_steps_over_the_dequantised_weights(models, fp8, monkeypatch, M):
    """six one-token calls of M rows from ring.reset() over the same forced ids: 4 n_layer fp8 launches per step (M <= 2: one of them the
    attention-merge form), none of the bf16 four, no chain; logits bit-equal at every step, the rings byte-equal at the end.
    M = 1, 2: the partials path; 4: the LayerNorm prologue; 17: the LayerNorm launches"""
    from bdm_db1_amd import RingMemory, ops
    A, B = models
    nl = A.n_layer
    assert A.decode_weights == "fp8" and B.decode_weights == "bf16" and A._decode_fused_ok(M, False, None)
    rng = np.random.default_rng(M)
    ids = rng.integers(0, HI, (6, M, 1))
    ra, rb = RingMemory(A, M), RingMemory(B, M)
    ra.reset(), rb.reset()
    cnt = _Count(monkeypatch, A)
    with torch.no_grad():
        for t in range(6):
            la = A([_text(ids[t])], compute_loss=False, mems=ra)[0].clone()
            n = cnt.take()
            assert n["w8"] + n["attn_w8"] == 4 * nl and n["attn_w8"] == (nl if M <= 2 else 0) and n["bf16"] == n["attn_bf16"] == n["chain"] == 0, (t, n)
            lb = B([_text(ids[t])], compute_loss=False, mems=rb)[0].clone()
            n = cnt.take()                                               # (B's own launches: the bf16 entry points, none of the fp8 ones)
            assert n["w8"] == n["attn_w8"] == n["chain"] == 0 and n["attn_bf16"] == (nl if M <= 2 else 0), (t, n)
            assert bool(torch.isfinite(la.float()).all())
            assert torch.equal(la.view(torch.int16), lb.view(torch.int16)), (M, t)
    for name in _names(A):      # the copies the steps streamed are the rule applied to the bf16 weights
        assert torch.equal(A.W8(name).cpu(), ops.w8_pack(A.W(name).cpu())), name
    for ka, kb in zip(ra.kv, rb.kv):
        assert torch.equal(ka.view(torch.int16), kb.view(torch.int16))
    assert int(ra.state[0]) == int(rb.state[0]) == 6


def _fed(model, prompt, fed):
    """logits [rows, HI] float64 after ``prompt`` (one call) and the tokens ``fed`` (one call each) over the list-form memory"""
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([_text(prompt)], compute_loss=False, mems=model.init_mem(prompt.shape[0]))
        for t in range(fed.shape[1]):
            logits, _, mems = model([_text(fed[:, t:t + 1])], compute_loss=False, mems=mems)
    return logits[:, -1, :HI].double().cpu().numpy()


def test_accuracy_against_fp32_models(models, monkeypatch):
    """e8 = the fp8 model against an fp32 model ON THE DEQUANTISED WEIGHTS, e16 = the flag-off model against an fp32 model on the original
    weights, both max|dlogits| / max|logits| at the last step: bf16 arithmetic against fp32 on equal weights either way, so e8 <= 2 e16.
    The distance between the fp8 and the original-weight logits is printed, not gated (the figures: README, "fp8 decode weights")."""
    A, B = models
    ref8, ref16 = _with_dequantised_maps(A, torch.float32), _build(torch.float32)
    ref16.load_state_dict(A.state_dict(), strict=False)
    rng = np.random.default_rng(7)
    prompt, fed = rng.integers(0, HI, (2, 20)), rng.integers(0, HI, (2, 6))
    l16 = _fed(A, prompt, fed)
    A.set_decode_weights("fp8")
    try:
        cnt = _Count(monkeypatch, A)
        l8 = _fed(A, prompt, fed)
        n = cnt.take()
        assert n["w8"] == 7 * 4 * A.n_layer and n["bf16"] == 0, n          # (every call of the run took the fused branch on the fp8 copies)
    finally:
        A.set_decode_weights("bf16")
    r8, r16 = _fed(ref8, prompt, fed), _fed(ref16, prompt, fed)
    e8 = np.abs(l8 - r8).max() / np.abs(r8).max()
    e16 = np.abs(l16 - r16).max() / np.abs(r16).max()
    d = np.abs(l8 - l16).max() / np.abs(l16).max()
    print(f"w8 accuracy: e16 = {e16:.3e}, e8 = {e8:.3e}, e8 / e16 = {e8 / e16:.2f}; fp8 against original-weight logits = {d:.3e}")
    assert e16 > 0 and d > 0 and e8 <= 2 * e16, (e8, e16)


def test_switching_rebuilds_generators_and_invalidates_prefix_handles(models):
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, generate
    A = models[0]
    rng = np.random.default_rng(3)
    cfg = GenerationConfig(max_new_tokens=4, vocab_hi=HI, pad_id=PAD)
    x = _text(rng.integers(0, HI, (2, 7)))
    ids16 = generate(A, x, cfg)[0]
    gen, v = A._generator, A._wversion
    cache = PrefixCache(A, 2)
    h = cache.put(_text(rng.integers(0, HI, (1, 12))))
    suffix = _text(rng.integers(0, HI, (1, 5)))
    generate(A, Prefixed(cache, h, suffix), cfg)
    A.set_decode_weights("bf16")                                     # (no change: nothing is invalidated)
    assert A._wversion == v
    A.set_decode_weights("fp8")
    try:
        assert A._wversion == v + 1 and A.decode_weights == "fp8"
        with pytest.raises(RuntimeError):
            generate(A, Prefixed(cache, h, suffix), cfg)
        ids8 = generate(A, x, cfg)[0]
        assert A._generator is not gen and A._generator.step._version == A._wversion
        gen8 = A._generator
        assert torch.equal(generate(A, x, cfg)[0], ids8) and A._generator is gen8
    finally:
        A.set_decode_weights("bf16")
    assert A._wversion == v + 2 and A._w8 is None
    assert torch.equal(generate(A, x, cfg)[0], ids16) and A._generator is not gen8


def test_loops_run_with_the_flag(fp8, monkeypatch):
    """generate (replay == eager, token for token), a stream and get_action under the flag, each twice with equal results; the replays'
    graphs were captured after an eager warm-up packed the copies"""
    from bdm_db1_amd import GenerationConfig, RingMemory, generate, generate_many
    from bdm_db1_amd.evaluation import get_action
    from bdm_db1_amd.tokenizer import ContinuousScalarTokenizer
    A = fp8
    rng = np.random.default_rng(5)
    prompts = rng.integers(0, HI, (3, 9))
    cfg = GenerationConfig(max_new_tokens=6, vocab_hi=HI, pad_id=PAD, sync_every=2)
    cnt = _Count(monkeypatch, A)
    stats = {}
    ids, lengths = generate(A, _text(prompts), cfg, stats=stats)
    n = cnt.take()
    assert stats["path"] == "ring" and n["w8"] > 0 and n["bf16"] == n["attn_bf16"] == n["chain"] == 0, n
    again = generate(A, _text(prompts), cfg)
    eager = generate(A, _text(prompts), cfg, replay=False)
    assert torch.equal(ids, again[0]) and torch.equal(ids, eager[0]) and torch.equal(lengths, eager[1])
    one = generate(A, _text(prompts[:1]), cfg)                           # one row: the per-layer launches, not the chain
    n = cnt.take()
    assert n["attn_w8"] > 0 and n["chain"] == n["bf16"] == 0 and torch.equal(one[0], generate(A, _text(prompts[:1]), cfg, replay=False)[0])
    reqs = [_text(prompts[i:i + 1]) for i in range(3)]
    s1, s2 = generate_many(A, reqs, cfg, slots=2), generate_many(A, reqs, cfg, slots=2)
    assert all(torch.equal(a, b) for a, b in zip(s1[0], s2[0])) and s1[1] == s2[1] == [6, 6, 6]
    c = _cfg()
    args = SimpleNamespace(overlap_with_text=c.overlap_with_text, text_vocab_size=c.text_vocab_size, num_discrete_values=c.num_discrete_values,
                           n_position=c.n_position, use_prompt=False)
    tok = ContinuousScalarTokenizer(c.num_continuous_bin)
    obs = [torch.from_numpy(rng.integers(HI, HI + 1024, 5)) for _ in range(2)]

    def episode():
        memory, acts = RingMemory(A, 1), []
        with torch.no_grad():
            for o in obs:
                act, _, memory = get_action(args, A, o, None, tok, 0, 0, 5, 2, False, None, memory, prompt_strategy="none")
                acts.append(np.asarray(act, np.float64))
        return np.stack(acts), [k.clone() for k in memory.kv]
    cnt.take()
    (a1, k1), (a2, k2) = episode(), episode()
    n = cnt.take()
    assert n["w8"] + n["attn_w8"] == 2 * 2 * 3 * 4 * A.n_layer and n["bf16"] == n["chain"] == 0, n      # 2 episodes x 2 steps x 3 calls (observation, action token, memorise)
    assert np.array_equal(a1, a2) and all(torch.equal(u, v) for u, v in zip(k1, k2))


def test_first_use_under_a_capture_raises(fp8):
    from bdm_db1_amd import RingMemory
    A = fp8
    assert A._w8 is None
    ring = RingMemory(A, 1)
    x = _text(np.zeros((1, 1), np.int64))
    A._decode_R()                                                        # (everything else the call caches exists before the capture)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="eagerly"):
        with torch.cuda.graph(g):
            with torch.no_grad():
                A([x], compute_loss=False, mems=ring)
    torch.cuda.synchronize()


def test_default_takes_the_launches_it_took(monkeypatch):
    """a model whose flag was never set: generate makes no fp8 launch, one row still decodes through the persistent chain, the replayed ids
    are the eager ones, and setting "bf16" explicitly changes nothing (no version bump, the cached generator stays)"""
    from bdm_db1_amd import GenerationConfig, generate, ops
    m = _build(seed=12)
    assert m.decode_weights == "bf16" and m._w8 is None
    rng = np.random.default_rng(8)
    prompts = rng.integers(0, HI, (2, 9))
    cfg = GenerationConfig(max_new_tokens=5, vocab_hi=HI, pad_id=PAD)
    cnt = _Count(monkeypatch, m)
    ids = generate(m, _text(prompts), cfg)[0]
    n2 = cnt.take()
    assert n2["w8"] == n2["attn_w8"] == n2["chain"] == 0 and n2["bf16"] > 0 and n2["attn_bf16"] > 0, n2
    one = generate(m, _text(prompts[:1]), cfg)[0]
    n1 = cnt.take()
    chain = ops.decode_chain_supported(m.d_model, m.d_ff, m.n_head, m.d_head, MLEN + 1)      # (the 1.3B geometry: the test below)
    assert n1["w8"] == n1["attn_w8"] == 0 and (n1["chain"] > 0) == chain and (chain or n1["attn_bf16"] > 0), n1
    m.check_decode_chain(synchronize=True)
    gen, v = m._generator, m._wversion
    m.set_decode_weights("bf16")
    assert m._wversion == v and m._w8 is None
    assert torch.equal(generate(m, _text(prompts[:1]), cfg)[0], one) and m._generator is gen
    assert torch.equal(generate(m, _text(prompts), cfg, replay=False)[0], ids)
    n = cnt.take()
    assert n["w8"] == n["attn_w8"] == 0 and n["bf16"] > 0, n


def test_one_token_call_leaves_the_chain_at_1p3b_geometry(monkeypatch):
    """where the model has the persistent one-token chain (the 1.3B layer geometry, two layers here): flag off, the one-token call is the
    chain's launches; flag on, the per-layer launches with the attention-merge prologue -- 4 n_layer fp8 launches, no chain launch"""
    from bdm_db1_amd import RingMemory, TransformerXL, ops, synth
    torch.manual_seed(13)
    m = TransformerXL(synth.db1_config("1.3B", n_layer=2, mem_len=1024, n_position=1024), device=torch.device(DEV), compute_dtype=torch.bfloat16)
    m.eval()
    assert m.use_decode_chain and ops.decode_chain_supported(m.d_model, m.d_ff, m.n_head, m.d_head, 1025)
    cnt = _Count(monkeypatch, m)
    x = _text(np.full((1, 1), 17, np.int64))
    with torch.no_grad():
        l16 = m([x], compute_loss=False, mems=RingMemory(m, 1))[0].float().cpu().numpy()
        m.check_decode_chain(synchronize=True)
        n = cnt.take()
        assert n["chain"] == m.n_layer and n["w8"] == n["attn_w8"] == n["attn_bf16"] == 0, n
        m.set_decode_weights("fp8")
        l8 = m([x], compute_loss=False, mems=RingMemory(m, 1))[0].float().cpu().numpy()
        n = cnt.take()
    assert n["chain"] == n["bf16"] == n["attn_bf16"] == 0 and n["attn_w8"] == m.n_layer and n["w8"] == 3 * m.n_layer, n
    assert np.isfinite(l8).all() and np.isfinite(l16).all() and not np.array_equal(l8, l16)


def test_setter_refusals(models):
    A = models[0]
    v = A._wversion
    for bad in ("fp16", "e5m2", None, "FP8"):
        with pytest.raises(ValueError):
            A.set_decode_weights(bad)
    A.use_decode = False
    try:
        with pytest.raises(ValueError, match="use_decode"):
            A.set_decode_weights("fp8")
    finally:
        A.use_decode = True
    with pytest.raises(ValueError, match="bf16"):
        _build(torch.float32, n_layer=1).set_decode_weights("fp8")
    with pytest.raises(ValueError, match="128"):
        _build(n_embed=192, n_head=3, n_layer=1).set_decode_weights("fp8")            # d_model % 128 != 0
    with pytest.raises(ValueError, match="post-LN"):
        _build(pre_lnorm=True, n_layer=1).set_decode_weights("fp8")
    with pytest.raises(ValueError, match="GEGLU"):
        _build(activation_fn="gelu", n_layer=1).set_decode_weights("fp8")
    assert A._wversion == v and A.decode_weights == "bf16"
