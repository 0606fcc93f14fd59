"""The fp8 K/V ring through the model and the decoding loops (``RingMemory(kv_dtype="fp8")``, ``kv_cache="fp8"``): one token step bit for bit
against a bf16 ring that holds the dequantised values, the loops' own exactness (replay against eager, beams, a stream), the one-token chain
path, the accuracy against an fp32 model, and the untouched default."""
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

import kv8_rule as K8  # noqa: E402
from gpu_common import DEV, _bf16_model, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD, MLEN = 32000, 31999, 100


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


@pytest.fixture(scope="module")
def model():
    return _bf16_model(mem_len=MLEN)[1]


def _prefill(model, ids):
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([_text(ids)], compute_loss=False, mems=model.init_mem(ids.shape[0]))
    return logits, mems


def _dequantised_twin(model, ring8):
    """a bf16 RingMemory whose rows hold what the fp8 ring ``ring8`` holds, dequantised; same origin"""
    from bdm_db1_amd import RingMemory, ops
    ring16 = RingMemory(model, ring8.B)
    for dst, src in zip(ring16.kv, ring8.kv):
        dst.copy_(ops.kv8_unpack(src.cpu(), model.n_head)[0].to(DEV))
    ring16.state.copy_(ring8.state)
    return ring16


@pytest.mark.parametrize("rows,new", [(3, 1), (1, 1), (2, 5), (1, 2)])
def test_one_step_is_the_bf16_step_over_the_dequantised_ring(model, rows, new):
    """prefill, load the fp8 ring (its slots are the rule applied to the bf16 ring's rows), one call: the logits bit for bit those of the same
    call over a bf16 RingMemory overwritten with the dequantised values -- through the plain path (3 rows; 5 tokens), the partials path and,
    where the model has one, the chain (1 row, 1 token)"""
    from bdm_db1_amd import RingMemory
    rng = np.random.default_rng(rows * 10 + new)
    _, mems = _prefill(model, rng.integers(0, HI, (rows, 70)))
    ring8, ring16 = RingMemory(model, rows, kv_dtype="fp8"), RingMemory(model, rows)
    assert ring8.kv_dtype == "fp8" and ring16.kv_dtype == "bf16" and ring8.kv[0].dtype == torch.uint8
    assert tuple(ring8.kv[0].shape) == (rows, MLEN + 64, K8.slot_bytes(model.n_head))
    ring8.load(mems)
    ring16.load(mems)
    for a, b in zip(ring8.kv, ring16.kv):
        assert np.array_equal(a[:, :MLEN].cpu().numpy(), K8.pack(b[:, :MLEN].to(torch.float64).cpu().numpy()))
        assert not bool(a[:, MLEN:].any())
    twin = _dequantised_twin(model, ring8)
    x = _text(rng.integers(0, HI, (rows, new)))
    with torch.no_grad():
        got = model([x], compute_loss=False, mems=ring8)[0].clone()
        want = model([x], compute_loss=False, mems=twin)[0].clone()
        plain = model([x], compute_loss=False, mems=ring16)[0].clone()
    model.check_decode_chain(synchronize=True)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not torch.equal(got.view(torch.int16), plain.view(torch.int16))       # (the quantisation is not a no-op on these keys / values)
    assert int(ring8.state[0]) == int(twin.state[0]) == new
    # the call appended its own keys / values quantised by the rule: the twin holds them unquantised
    for a, b in zip(ring8.kv, twin.kv):
        assert np.array_equal(a[:, MLEN:MLEN + new].cpu().numpy(), K8.pack(b[:, MLEN:MLEN + new].to(torch.float64).cpu().numpy()))


def test_load_rows_quantises_into_the_rows_it_is_given(model):
    from bdm_db1_amd import RingMemory
    rng = np.random.default_rng(2)
    _, mems = _prefill(model, rng.integers(0, HI, (2, 30)))
    whole = RingMemory(model, 2, kv_dtype="fp8")
    whole.load(mems)
    ring = RingMemory(model, 4, kv_dtype="fp8")
    with torch.no_grad():
        for _ in range(3):
            model([_text(rng.integers(0, HI, (4, 50)))], compute_loss=False, mems=ring)
    origin = int(ring.state[0])
    before = [k.clone() for k in ring.kv]
    ring.load_rows(mems, _tdev(np.asarray([3, 1], np.int32)))
    assert origin == 150 and int(ring.state[0]) == origin and int(ring.load_status[0]) == 0
    slots = (origin + np.arange(MLEN)) % ring.cap
    for k, k0, w in zip(ring.kv, before, whole.kv):
        assert torch.equal(k[[3, 1]][:, slots], w[:, :MLEN]) and torch.equal(k[[0, 2]], k0[[0, 2]])


def _fed_logits(model, prompt, fed, memory):
    """[steps, rows, HI] float64: the logits after the prompt and after every fed token, one token per call, over ``memory`` (a RingMemory loaded
    from the prefill, or None: the list-form memory)"""
    out = []
    with torch.no_grad():
        logits, mems = _prefill(model, prompt)
        if memory is not None:
            memory.load(mems)
            mems = memory
        for t in range(fed.shape[1]):
            out.append(logits[:, -1, :HI].double().cpu().numpy())
            logits, _, mems = model([_text(fed[:, t:t + 1])], compute_loss=False, mems=mems)
        out.append(logits[:, -1, :HI].double().cpu().numpy())
    return np.stack(out)


def _check_greedy(model, prompt, ids, who):
    """every greedy token against the fp8 ring teacher-forced on the request alone: chosen logit >= max - 2e-2 max|l| (what the bf16 stream
    tests ask of a stream)"""
    from bdm_db1_amd import RingMemory
    ids = np.asarray(ids)
    tf = _fed_logits(model, prompt, ids[None, :-1], RingMemory(model, 1, kv_dtype="fp8"))
    for t in range(ids.shape[0]):
        l = tf[t, 0]
        assert l[ids[t]] >= l.max() - 2e-2 * np.abs(l).max(), (who, t)


def test_loops_over_the_fp8_ring(model):
    """generate: replay == eager over the same ring, token for token; a greedy stream over the same requests follows the fp8 ring
    teacher-forced on each request alone; beam_search: replay == eager; the stats say ring"""
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, beam_search, generate, generate_many
    from bdm_db1_amd.generation import DecodeKeyFp8
    rng = np.random.default_rng(31)
    prompts = rng.integers(0, HI, (3, 9))
    cfg = GenerationConfig(max_new_tokens=8, vocab_hi=HI, pad_id=PAD, sync_every=2)
    stats = {}
    ids, lengths = generate(model, _text(prompts), cfg, kv_cache="fp8", stats=stats)
    assert stats["path"] == "ring" and stats["token_calls"] == 7
    assert type(model._generator.key) is DecodeKeyFp8 and model._generator.ring.kv_dtype == "fp8" and model._generator.ring.kv[0].dtype == torch.uint8
    e_ids, e_len = generate(model, _text(prompts), cfg, kv_cache="fp8", replay=False)
    assert torch.equal(ids, e_ids) and torch.equal(lengths, e_len)
    s_ids, s_len = generate_many(model, [_text(prompts[i:i + 1]) for i in range(3)], cfg, slots=2, kv_cache="fp8")
    assert model._slot_generator.ring.kv_dtype == "fp8" and s_len == [8, 8, 8]
    for i in range(3):
        _check_greedy(model, prompts[i:i + 1], s_ids[i].numpy(), ("stream", i))
        _check_greedy(model, prompts[i:i + 1], ids[i].numpy(), ("generate", i))
    sampled = GenerationConfig(max_new_tokens=8, greedy=False, top_p=0.9, seed=77, vocab_hi=HI, pad_id=PAD)
    a, b = generate(model, _text(prompts), sampled, kv_cache="fp8"), generate(model, _text(prompts), sampled, kv_cache="fp8", replay=False)
    assert torch.equal(a[0], b[0])
    bc = BeamSearchConfig(max_new_tokens=6, num_beams=3, num_return_sequences=2, vocab_hi=HI, pad_id=PAD)
    bstats = {}
    g = beam_search(model, _text(prompts[:2]), bc, kv_cache="fp8", stats=bstats)
    e = beam_search(model, _text(prompts[:2]), bc, kv_cache="fp8", replay=False)
    assert bstats["path"] == "ring" and model._beam_generator.ring.kv_dtype == "fp8"
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])


def test_default_is_the_call_without_the_keyword(model):
    from bdm_db1_amd import GenerationConfig, generate
    from bdm_db1_amd.generation import DecodeKey
    rng = np.random.default_rng(32)
    x = _text(rng.integers(0, HI, (2, 7)))
    cfg = GenerationConfig(max_new_tokens=6, greedy=False, top_p=0.9, seed=5, vocab_hi=HI, pad_id=PAD, logprobs=True)
    plain = generate(model, x, cfg)
    gen = model._generator
    assert type(gen.key) is DecodeKey and gen.ring.kv_dtype == "bf16" and gen.ring.kv[0].dtype == torch.bfloat16
    kw = generate(model, x, cfg, kv_cache="bf16")
    assert model._generator is gen                                          # (the same key: nothing was rebuilt)
    for u, v in zip(plain, kw):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)


def test_fp8_ring_accuracy_against_an_fp32_model(model):
    """e = max|logits - reference| / max|reference| at the last step of a teacher-forced run, the reference an fp32 model on the same
    parameters, prompt and fed tokens: e8 (fp8 ring) <= 16 e16 (bf16 ring).  e4m3 keeps 3 mantissa bits where bf16 keeps 7 -- a rounding
    step 2^4 times larger -- and touches only the memory's keys / values, where bf16 rounds every activation."""
    from bdm_db1_amd import RingMemory, TransformerXL, synth
    cfg = synth.db1_config("tiny", n_embed=256, n_head=2, n_layer=2, n_position=128, mem_len=MLEN, fp16=True)
    ref_model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.float32)
    ref_model.load_state_dict(model.state_dict(), strict=False)
    ref_model.eval()
    rng = np.random.default_rng(33)
    prompt, fed = rng.integers(0, HI, (2, 60)), rng.integers(0, HI, (2, 12))
    ref = _fed_logits(ref_model, prompt, fed, None)[-1]
    l16 = _fed_logits(model, prompt, fed, RingMemory(model, 2))[-1]
    l8 = _fed_logits(model, prompt, fed, RingMemory(model, 2, kv_dtype="fp8"))[-1]
    e16 = np.abs(l16 - ref).max() / np.abs(ref).max()
    e8 = np.abs(l8 - ref).max() / np.abs(ref).max()
    print(f"kv8 accuracy: e16 = {e16:.3e}, e8 = {e8:.3e}, e8 / e16 = {e8 / e16:.2f}")
    assert e16 > 0 and e8 <= 16 * e16, (e8, e16)
    # the maximum sits on one bf16 logit and hardly moves with the keys' rounding; the root-mean-square distance does.  The same bound, for
    # the same reason (a rounding step 2^4 times larger, on the memory's K / V only), and the fp8 run must differ from the bf16 one at all
    r16 = np.sqrt(np.mean((l16 - ref) ** 2)) / np.abs(ref).max()
    r8 = np.sqrt(np.mean((l8 - ref) ** 2)) / np.abs(ref).max()
    d = np.sqrt(np.mean((l8 - l16) ** 2)) / np.abs(ref).max()
    print(f"kv8 accuracy (rms): r16 = {r16:.3e}, r8 = {r8:.3e}, r8 / r16 = {r8 / r16:.2f}, fp8 against bf16 ring = {d:.3e}")
    assert d > 0 and r8 <= 16 * r16, (r8, r16, d)


def test_one_token_chain_over_the_fp8_ring_at_1p3b_geometry():
    """M = 1 at the 1.3B layer geometry (3 layers, 16 heads, mem_len 1024), where the one-token call is db1_decode_chain fed by the attention's
    partials: the fp8 ring's logits bit for bit those over the dequantised bf16 ring, the chain against the per-launch path as the bf16 test
    asks it (1e-2 of max|logits|), and greedy tokens of ``generate`` that are the per-launch path's up to that noise"""
    from bdm_db1_amd import GenerationConfig, RingMemory, TransformerXL, generate, synth
    cfg = synth.db1_config("1.3B", n_layer=3, mem_len=1024, n_position=1024)
    torch.manual_seed(11)
    model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)
    model.eval()
    rng = np.random.default_rng(4)
    calls = [rng.integers(0, HI, (1, q)) for q in (22, 1, 1)]

    def run(chain, memory):
        model.use_decode_chain = chain
        outs = []
        with torch.no_grad():
            for ids in calls:
                outs.append(model([_text(ids)], compute_loss=False, mems=memory)[0].clone())
        model.check_decode_chain(synchronize=True)
        return outs

    ring_a, ring_b = RingMemory(model, 1, kv_dtype="fp8"), RingMemory(model, 1, kv_dtype="fp8")
    assert tuple(ring_a.kv[0].shape) == (1, 1088, 4224)
    model._chain_watch = None
    got = run(True, ring_a)
    assert model._chain_watch is not None, "the one-token calls did not go through db1_decode_chain"
    ref = run(False, ring_b)
    for a, b in zip(got, ref):
        a, b = a.float().cpu().numpy(), b.float().cpu().numpy()
        assert np.abs(a - b).max() / np.abs(b).max() < 1e-2
    # one more token through the chain: over the fp8 ring and over its dequantised twin
    twin = _dequantised_twin(model, ring_a)
    x = _text(rng.integers(0, HI, (1, 1)))
    model.use_decode_chain = True
    with torch.no_grad():
        l8 = model([x], compute_loss=False, mems=ring_a)[0].clone()
        l16 = model([x], compute_loss=False, mems=twin)[0].clone()
    model.check_decode_chain(synchronize=True)
    assert torch.equal(l8.view(torch.int16), l16.view(torch.int16))
    # generate, one row: the graph replays the chain; its greedy tokens against the per-launch path teacher-forced on them
    gc = GenerationConfig(max_new_tokens=5, vocab_hi=HI, pad_id=PAD)
    prompt = rng.integers(0, HI, (1, 12))
    stats = {}
    ids, _ = generate(model, _text(prompt), gc, kv_cache="fp8", stats=stats)
    assert stats["path"] == "ring" and model._generator.step._watch is not None
    model.use_decode_chain = False
    try:
        tf = _fed_logits(model, prompt, ids.numpy()[:, :-1].astype(np.int64), RingMemory(model, 1, kv_dtype="fp8"))
    finally:
        model.use_decode_chain = True
    for t in range(ids.shape[1]):
        l = tf[t, 0]
        assert l[int(ids[0, t])] >= l.max() - 2e-2 * np.abs(l).max(), t
