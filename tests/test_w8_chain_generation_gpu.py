"""fp8 weights in the persistent one-token chain through the model (``model.set_decode_weights("fp8", chain=True)``) at the 1.3B layer geometry
with two layers: the launches a call makes, the logits against the fp8 per-layer launches on the same copies, the graphed step against the
eager call, the accuracy gate of the fp8-weights section, generate, the flag's plumbing and the failed-hand-off path."""
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

from gpu_common import DEV, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD = 32000, 31999
MAPS = ("dec_attn.qkv_net.weight", "dec_attn.o_net.weight", "pos_ff.CoreNet.0.weight", "pos_ff.CoreNet.2.weight")


def _build(mem_len=1024, dtype=torch.bfloat16, seed=13, n_layer=2):
    from bdm_db1_amd import TransformerXL, synth
    torch.manual_seed(seed)
    m = TransformerXL(synth.db1_config("1.3B", n_layer=n_layer, mem_len=mem_len, n_position=max(1024, mem_len)), device=torch.device(DEV), compute_dtype=dtype)
    m.eval()
    return m


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _names(model):
    return [f"h.{i}.{m}" for i in range(model.n_layer) for m in MAPS]


def _supported(mem_len=1024):
    from bdm_db1_amd import ops
    return ops.decode_chain_w8_supported(2048, 4096, 16, 128, mem_len + 1)


@pytest.fixture(scope="module")
def model():
    """the model under test, mem_len 1024 (the tests switch the flag, and leave it off)"""
    if not _supported():
        pytest.skip("db1_decode_chain_w8 needs 256 CUs")
    m = _build()
    assert m.use_decode_chain and m.decode_weights == "bf16" and m.decode_chain_w8 is False
    return m


@pytest.fixture
def chain8(model):
    model.use_decode_chain = True
    model.set_decode_weights("fp8", chain=True)
    yield model
    model.set_decode_weights("bf16")
    model.use_decode_chain = True


class _Count:
    """counts the launches over the layers' four linear maps, by entry point; of db1_linear_decode and the GEMM only those whose weight is one
    of the four bf16 matrices (the head and the embedders stream their own bf16 weights under either flag)"""

    def __init__(self, monkeypatch, model):
        from bdm_db1_amd import ops
        self.n = dict(w8=0, attn_w8=0, bf16=0, attn_bf16=0, gemm=0, chain=0, chain_w8=0)
        four = {model.W(n).data_ptr() for n in _names(model)}
        of_four = lambda a: len(a) > 1 and isinstance(a[1], torch.Tensor) and a[1].data_ptr() in four

        def wrap(name, key, own=lambda a: True):
            orig = getattr(ops, name)

            def f(*a, **k):
                if own(a):
                    self.n[key] += 1
                return orig(*a, **k)
            monkeypatch.setattr(ops, name, f)
        wrap("linear_decode_w8", "w8")
        wrap("linear_decode_attn_w8", "attn_w8")
        wrap("linear_decode", "bf16", of_four)
        wrap("linear_decode_attn", "attn_bf16")
        wrap("gemm", "gemm", of_four)
        wrap("decode_chain", "chain")
        wrap("decode_chain_w8", "chain_w8")

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.n, 0)
        return n


def test_launch_counts(model, monkeypatch):
    """chain=True: a one-token call over RingMemory(m, 1) is n_layer db1_decode_chain_w8 launches and ONE db1_linear_decode_w8 (layer 0's own
    projection) -- no bf16 chain, no launch or GEMM over a bf16 copy of the four maps, no per-layer fp8 merge launch; a call of 2 rows still
    makes the 4 n_layer per-layer fp8 launches.  chain=False: the counts tests/test_w8_generation_gpu.py states."""
    from bdm_db1_amd import RingMemory
    m, nl = model, model.n_layer
    cnt = _Count(monkeypatch, m)
    x1, x2 = _text(np.full((1, 1), 17)), _text(np.full((2, 1), 17))
    m.set_decode_weights("fp8", chain=True)
    try:
        assert m.decode_weights == "fp8" and m.decode_chain_w8 is True
        with torch.no_grad():
            r1, r2, r3 = RingMemory(m, 1), RingMemory(m, 2), RingMemory(m, 1)
            cnt.take()                                                   # (a new ring projects the zero memory: bf16 GEMMs, not part of a call)
            l8c = m([x1], compute_loss=False, mems=r1)[0].float().cpu().numpy()
            m.check_decode_chain(synchronize=True)
            n = cnt.take()
            assert n == dict(w8=1, attn_w8=0, bf16=0, attn_bf16=0, gemm=0, chain=0, chain_w8=nl), n
            m([x2], compute_loss=False, mems=r2)
            n = cnt.take()
            assert n["w8"] + n["attn_w8"] == 4 * nl and n["attn_w8"] == nl and n["bf16"] == n["attn_bf16"] == n["gemm"] == n["chain"] == n["chain_w8"] == 0, n
            m.set_decode_weights("fp8")
            assert m.decode_chain_w8 is False
            l8 = m([x1], compute_loss=False, mems=r3)[0].float().cpu().numpy()
            n = cnt.take()
            assert n == dict(w8=3 * nl, attn_w8=nl, bf16=0, attn_bf16=0, gemm=0, chain=0, chain_w8=0), n
    finally:
        m.set_decode_weights("bf16")
    assert np.isfinite(l8c).all() and np.abs(l8c - l8).max() / np.abs(l8).max() < 1e-2


@pytest.mark.parametrize("mem_len", [1024, 1400])
def test_logits_against_the_fp8_per_layer_launches(model, mem_len):
    """calls of q = 22, 1, 1, 1, 9, 1, 1 tokens: chain=True against chain=False on the same model (the same packed copies), max|d| / max|ref| < 1e-2
    -- the bound tests/test_decode_gpu.py holds the bf16 chain to against its launches; no hand-off poll ran out.  mem_len 1400: 12 chunks"""
    from bdm_db1_amd import RingMemory
    if not _supported(mem_len):
        pytest.skip("db1_decode_chain_w8 needs 256 CUs")
    m = model if mem_len == 1024 else _build(mem_len)
    rng = np.random.default_rng(4)
    calls = [rng.integers(0, HI, (1, q)) for q in (22, 1, 1, 1, 9, 1, 1)]

    def run(chain):
        m.set_decode_weights("fp8", chain=chain)
        m._chain_watch = None
        mems, outs = RingMemory(m, 1), []
        with torch.no_grad():
            for ids in calls:
                logits, _, mems = m([_text(ids)], compute_loss=False, mems=mems)
                outs.append(logits.float().cpu().numpy())
        return outs
    try:
        ref = run(False)
        assert m._chain_watch is None, "chain=False went through a persistent launch"
        got = run(True)
        assert m._chain_watch is not None, "the one-token calls did not go through db1_decode_chain_w8"
        m.check_decode_chain(synchronize=True)
    finally:
        m.set_decode_weights("bf16")
    for step, (a, b) in enumerate(zip(got, ref)):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"w8 chain against the fp8 launches, mem_len {mem_len}, call {step} (q = {calls[step].shape[1]}): {err:.3e}")
        assert err < 1e-2, f"call {step} (q = {calls[step].shape[1]}): rel err {err:.3e}"


def test_graphed_step_equals_the_eager_call(chain8, monkeypatch):
    from bdm_db1_amd import GraphedRingStep, RingMemory
    m = chain8
    ids = _tdev(np.random.default_rng(6).integers(0, HI, (1, 1)))
    cnt = _Count(monkeypatch, m)
    g = GraphedRingStep(m, 1, 1)
    n = cnt.take()
    assert n["chain_w8"] > 0 and n["chain"] == n["attn_w8"] == n["bf16"] == n["attn_bf16"] == 0, n   # (warm-up and capture: the fp8 chain)
    mem_e = RingMemory(m, 1)
    with torch.no_grad():
        for _ in range(3):
            lg_g, _ = g(ids)
            lg_e, _, mem_e = m([_text(ids.cpu().numpy())], compute_loss=False, mems=mem_e)
            assert lg_g.dtype == lg_e.dtype and torch.equal(lg_g, lg_e)
    g.check(synchronize=True)
    m.check_decode_chain(synchronize=True)


def _forced_ring(m, prompt, fed):
    """logits [HI] float64 after ``prompt`` (one call) and the tokens ``fed`` (one call each) over a RingMemory"""
    from bdm_db1_amd import RingMemory
    with torch.no_grad():
        mems = RingMemory(m, 1)
        logits, _, mems = m([_text(prompt)], compute_loss=False, mems=mems)
        for t in range(fed.shape[1]):
            logits, _, mems = m([_text(fed[:, t:t + 1])], compute_loss=False, mems=mems)
    return logits[0, -1, :HI].double().cpu().numpy()


def _forced_list(m, prompt, fed):
    """the same run over the list-form memory (an fp32 model has no ring)"""
    with torch.no_grad():
        m._dec_state = None
        logits, _, mems = m([_text(prompt)], compute_loss=False, mems=m.init_mem(1))
        for t in range(fed.shape[1]):
            logits, _, mems = m([_text(fed[:, t:t + 1])], compute_loss=False, mems=mems)
    return logits[0, -1, :HI].double().cpu().numpy()


def test_accuracy_against_fp32_models(model, monkeypatch):
    """the gate of the fp8-weights section at this geometry: e16 = the bf16 chain against an fp32 model on the original weights, e8 = the fp8 chain
    against an fp32 model on the DEQUANTISED weights, both max|dlogits| / max|logits| at the last step of a teacher-forced run: e8 <= 2 e16"""
    from bdm_db1_amd import ops
    m = model
    rng = np.random.default_rng(7)
    prompt, fed = rng.integers(0, HI, (1, 20)), rng.integers(0, HI, (1, 6))
    cnt = _Count(monkeypatch, m)
    l16 = _forced_ring(m, prompt, fed)
    n = cnt.take()
    assert n["chain"] == 6 * m.n_layer and n["chain_w8"] == 0, n
    m.set_decode_weights("fp8", chain=True)
    try:
        l8 = _forced_ring(m, prompt, fed)
        n = cnt.take()
        assert n["chain_w8"] == 6 * m.n_layer and n["chain"] == 0, n
        m.check_decode_chain(synchronize=True)
        deq = {name: ops.w8_unpack(m.W8(name), *m.W(name).shape)[0] for name in _names(m)}
    finally:
        m.set_decode_weights("bf16")
    ref = _build(dtype=torch.float32)
    ref.load_state_dict(m.state_dict(), strict=False)
    r16 = _forced_list(ref, prompt, fed)
    with torch.no_grad():
        for name, w in deq.items():
            ref.arena.view(ref.arena.master, name).copy_(w.to(DEV).float())
    ref.sync_work_params()
    r8 = _forced_list(ref, prompt, fed)
    e8 = np.abs(l8 - r8).max() / np.abs(r8).max()
    e16 = np.abs(l16 - r16).max() / np.abs(r16).max()
    d = np.abs(l8 - l16).max() / np.abs(l16).max()
    print(f"w8 chain accuracy: e16 = {e16:.3e}, e8 = {e8:.3e}, e8 / e16 = {e8 / e16:.2f}; fp8 chain against bf16 chain logits = {d:.3e}")
    assert e16 > 0 and d > 0 and e8 <= 2 * e16, (e8, e16)


def test_generate_one_row_takes_the_fp8_chain(chain8, monkeypatch):
    from bdm_db1_amd import GenerationConfig, generate
    m = chain8
    prompt = np.random.default_rng(5).integers(0, HI, (1, 9))
    cfg = GenerationConfig(max_new_tokens=6, vocab_hi=HI, pad_id=PAD, sync_every=2)
    cnt = _Count(monkeypatch, m)
    stats = {}
    ids, lengths = generate(m, _text(prompt), cfg, stats=stats)
    n = cnt.take()
    assert stats["path"] == "ring" and n["chain_w8"] > 0 and n["chain"] == n["attn_w8"] == n["bf16"] == n["attn_bf16"] == 0, (stats, n)
    eager = generate(m, _text(prompt), cfg, replay=False)
    n = cnt.take()
    assert n["chain_w8"] > 0 and n["chain"] == n["attn_w8"] == 0, n
    assert torch.equal(ids, eager[0]) and torch.equal(lengths, eager[1])


def test_flag_plumbing(model):
    from bdm_db1_amd import GenerationConfig, generate
    m = model
    cfg = GenerationConfig(max_new_tokens=3, vocab_hi=HI, pad_id=PAD)
    x = _text(np.random.default_rng(3).integers(0, HI, (1, 7)))
    m.set_decode_weights("fp8")
    try:
        generate(m, x, cfg)
        gen, v = m._generator, m._wversion
        m.set_decode_weights("fp8")                                      # (no change: nothing is invalidated)
        assert m._wversion == v and m.decode_chain_w8 is False
        m.set_decode_weights("fp8", chain=True)
        assert m._wversion == v + 1 and m.decode_chain_w8 is True and m.decode_weights == "fp8" and m._w8 is None
        generate(m, x, cfg)
        assert m._generator is not gen and m._generator.step._version == m._wversion
        gen8 = m._generator
        m.set_decode_weights("fp8", chain=True)                          # (no change)
        assert m._wversion == v + 1
        generate(m, x, cfg)
        assert m._generator is gen8
        m.set_decode_weights("fp8", chain=False)
        assert m._wversion == v + 2 and m.decode_chain_w8 is False
        with pytest.raises(AttributeError):
            m.decode_chain_w8 = True                                     # read-only
        with pytest.raises(TypeError):
            m.set_decode_weights("fp8", True)                            # keyword only
    finally:
        m.set_decode_weights("bf16")
    assert m.decode_weights == "bf16" and m.decode_chain_w8 is False


def test_fp8_alone_on_a_fresh_model_leaves_the_chain(monkeypatch):
    from bdm_db1_amd import RingMemory
    if not _supported():
        pytest.skip("db1_decode_chain_w8 needs 256 CUs")
    m = _build(seed=14)
    m.set_decode_weights("fp8")
    assert m.decode_chain_w8 is False
    cnt = _Count(monkeypatch, m)
    with torch.no_grad():
        lg = m([_text(np.full((1, 1), 5))], compute_loss=False, mems=RingMemory(m, 1))[0]
    n = cnt.take()
    assert n["chain"] == n["chain_w8"] == 0 and n["attn_w8"] == m.n_layer and n["w8"] == 3 * m.n_layer and bool(torch.isfinite(lg.float()).all()), n


def test_setter_refusals(model):
    from bdm_db1_amd import TransformerXL, synth
    m = model
    v = m._wversion
    with pytest.raises(ValueError, match="fp8"):
        m.set_decode_weights("bf16", chain=True)
    assert m._wversion == v and m.decode_weights == "bf16" and m.decode_chain_w8 is False
    with pytest.raises(ValueError, match="n_layer"):
        _build(n_layer=1).set_decode_weights("fp8", chain=True)
    with pytest.raises(ValueError, match="geometry"):
        _build(mem_len=1536).set_decode_weights("fp8", chain=True)      # 1537 keys: 13 chunks, more than the merge is unrolled for
    torch.manual_seed(1)
    tiny = TransformerXL(synth.db1_config("tiny", n_embed=512, n_head=4, n_layer=2, n_position=64, mem_len=40, fp16=True), device=torch.device(DEV),
                         compute_dtype=torch.bfloat16)
    tiny.set_decode_weights("fp8")                                       # (fp8 alone is fine there)
    with pytest.raises(ValueError, match="geometry"):
        tiny.set_decode_weights("fp8", chain=True)
    assert tiny.decode_weights == "fp8" and tiny.decode_chain_w8 is False


def test_failed_hand_off_falls_back_to_the_fp8_launches(chain8, monkeypatch):
    """as tests/test_decode_gpu.py does it for the bf16 chain: the error word of the eager stream's scratch is set by hand (no kernel is made to
    fail).  The next forward raises, use_decode_chain goes False, and the same call then runs through the fp8 per-layer launches"""
    from bdm_db1_amd import RingMemory, lib, ops
    m = chain8
    off = int(lib.load().db1_decode_chain_error_offset())
    x = _text(np.full((1, 1), 9))
    mem = RingMemory(m, 1)
    cnt = _Count(monkeypatch, m)
    with torch.no_grad():
        m([x], compute_loss=False, mems=mem)
        m.check_decode_chain(synchronize=True)
        ops.decode_chain_scratch(m.dev)[off:off + 4].view(torch.int32).fill_(1)
        lg_bad, _, mem = m([x], compute_loss=False, mems=mem)              # this call's flag copy carries the 1
        lg_bad.float().cpu()
        with pytest.raises(lib.Db1Error, match="hand-off poll"):
            m([x], compute_loss=False, mems=mem)
        assert m.use_decode_chain is False and m._chain_watch is None and m.decode_chain_w8 is True
        cnt.take()
        lg_ok, _, mem = m([x], compute_loss=False, mems=mem)               # the fp8 per-layer launches
        n = cnt.take()
    assert n["chain_w8"] == n["chain"] == n["bf16"] == n["attn_bf16"] == n["gemm"] == 0 and n["attn_w8"] == m.n_layer and n["w8"] == 3 * m.n_layer, n
    assert bool(torch.isfinite(lg_ok.float()).all()) and m._chain_watch is None
    assert not ops.decode_chain_error(m.dev)
