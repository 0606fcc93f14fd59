"""Speculative decoding end to end on the small test models.  fp32 eager list-form loop: ids, lengths and log-probs are those of plain
``generate`` for lookup drafts, a perfect script and an always-wrong one, and the accepted histogram is the rule's.  bf16 ring: graph replay
against eager launches bit for bit, the teacher-forced gate of tests/test_logprob_generation_gpu.py, EOS inside an accepted run, the fp8
ring, the ring prefill and a Prefixed prompt, and the default call untouched by speculative ones.  Then the refusals."""
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

import logprob_rule as L  # noqa: E402
import select_rule as R  # noqa: E402
import spec_rule as S  # noqa: E402
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD = 32000, 31999
M, N = 3, 12


@pytest.fixture(scope="module")
def bf16():
    return _bf16_model()[1]


@pytest.fixture(scope="module")
def fp32():
    cfg, model, _ = _fp32_model()
    return cfg, model


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _teacher_forced(model, x, ids):
    """the logits [n, M, V] (float64) of the eager list-form path fed the prompt, then ids[:, t] one token per call"""
    out = []
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([x], compute_loss=False, mems=model.init_mem(ids.shape[0]))
        for t in range(ids.shape[1]):
            out.append(logits[:, -1].double().cpu().numpy())
            logits, _, mems = model([_text(ids[:, t:t + 1])], compute_loss=False, mems=mems)
    return np.stack(out)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------ fp32 eager
_PLAIN = {}


def _fp32_plain(fp32, greedy):
    """plain ``generate`` with log-probs, its teacher-forced float64 logits and, per row, the first token whose top-2 gap is below
    1e-3 max|l| (n: none) -- computed once per sampling mode and shared"""
    from bdm_db1_amd import GenerationConfig, generate
    if greedy not in _PLAIN:
        cfg, model = fp32
        hi = cfg["text_vocab_size"]
        prompt = np.random.default_rng(41).integers(0, hi, (M, 6))
        gc = GenerationConfig(max_new_tokens=N, greedy=greedy, top_p=0.9, seed=99, vocab_hi=hi, logprobs=True)
        stats = {}
        ids, lengths, lps, sums = generate(model, _text(prompt), gc, stats=stats)
        assert stats["path"] == "eager"
        tf = _teacher_forced(model, _text(prompt), ids.numpy())
        first = np.full(M, N)
        for r in range(M):
            for t in range(N):
                top = np.sort(tf[t, r, :hi])[-2:]
                if top[1] - top[0] < 1e-3 * np.abs(tf[t, r, :hi]).max():
                    first[r] = t
                    break
        want = np.array([[L.logprob(tf[t, r], int(ids[r, t]), 0, hi) for t in range(N)] for r in range(M)])
        err = max([abs(float(lps[r, t]) - want[r, t]) for r in range(M) for t in range(first[r])], default=0.0)
        print(f"plain generate (greedy={greedy}): compared {first.sum()} of {M * N} pairs, max |lp - lp64| = {err:.3e}")
        assert 4 * first.sum() >= 3 * M * N, first         # the condition on the seeds: plain generate alone meets it
        _PLAIN[greedy] = dict(prompt=prompt, gc=gc, ids=ids, lengths=lengths, lps=lps, first=first, want=want, err=err, hi=hi)
    return _PLAIN[greedy]


@pytest.mark.parametrize("mode", ["lookup", "perfect", "wrong", "partial"])
@pytest.mark.parametrize("Q", [2, 5])
@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "top_p"])
def test_fp32_eager_equals_plain_generate(fp32, greedy, Q, mode):
    from bdm_db1_amd import SpeculativeConfig, generate
    cfg, model = fp32
    p = _fp32_plain(fp32, greedy)
    V, hi = int(model.total_vocab_size), p["hi"]
    bad = hi + (V - hi) // 2
    partial = np.where(np.arange(N) % 3 == 2, bad, p["ids"].numpy())          # every third proposal is wrong: calls commit 1 .. 3 tokens
    script = {"lookup": None, "perfect": p["ids"].numpy(), "wrong": np.full((M, N), bad, np.int32), "partial": partial.astype(np.int32)}[mode]
    stats = {}
    ids, lengths, lps, sums = generate(model, _text(p["prompt"]), p["gc"], speculative=SpeculativeConfig(num_draft_tokens=Q - 1), draft_script=script,
                                       stats=stats)
    assert stats["path"] == "eager" and ids.dtype == torch.int32 and tuple(ids.shape) == (M, N) and tuple(lps.shape) == (M, N)
    first = p["first"]
    err = 0.0
    for r in range(M):
        k = int(first[r])
        assert torch.equal(ids[r, :k], p["ids"][r, :k]), (r, ids[r], p["ids"][r])
        err = max([err] + [abs(float(lps[r, t]) - p["want"][r, t]) for t in range(k)])
        if k == N:
            assert int(lengths[r]) == int(p["lengths"][r])
    print(f"speculative (greedy={greedy}, Q={Q}, {mode}): max |lp - lp64| = {err:.3e}; plain {p['err']:.3e}; accepted {stats['accepted']}, "
          f"tokens per call {stats['tokens_per_call']:.2f}")
    assert err <= max(4 * p["err"], 1e-5), (err, p["err"])
    assert sum(stats["accepted"]) == stats["token_calls"] and len(stats["accepted"]) == Q + 1
    assert stats["accepted"][0] == 0         # no row ends early here: the host never runs a call past the end of the output
    if (first == N).all() and mode in ("perfect", "wrong"):      # (one shared counter: the histogram is the rule's when no row has an excluded token)
        perfect, wrong = S.step_counts(N, Q)
        assert stats["accepted"] == list(perfect if mode == "perfect" else wrong), stats["accepted"]


# ------------------------------------------------------------------------------------------------------------------------------- bf16 ring
def _check_teacher_forced(model, prompt, ids, lps, greedy, who):
    """the gate of test_bf16_ring_logprobs_...: up to each row's first token outside the list-form arg-max / kept set, every log-prob lies
    within 2 * 2e-2 max|l| of the teacher-forced value -> the number of (row, token) pairs compared"""
    tf = _teacher_forced(model, _text(prompt), ids)
    checked, worst = 0, 0.0
    for r in range(ids.shape[0]):
        for t in range(ids.shape[1]):
            l = tf[t, r, :HI]
            inside = ids[r, t] == int(np.argmax(l)) if greedy else R.kept_set(l, 0, HI, 1.0, 0, 0.9)[0][ids[r, t]]
            if not inside:
                break
            d = abs(lps[r, t] - L.logprob(l, int(ids[r, t]), 0, HI))
            worst = max(worst, d / (2 * 2e-2 * np.abs(l).max()))
            assert d <= 2 * 2e-2 * np.abs(l).max(), (who, r, t)
            checked += 1
    print(f"{who}: {checked} of {ids.size} pairs compared, worst |lp - lp_tf| = {worst:.3f} of the bound")
    return checked


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "top_p"])
def test_bf16_ring_replay_equals_eager_launches_and_follows_the_list_form(bf16, greedy):
    from bdm_db1_amd import GenerationConfig, SpeculativeConfig, generate
    model = bf16
    prompt = np.random.default_rng(42).integers(0, HI, (M, 6))
    gc = GenerationConfig(max_new_tokens=N, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=HI, logprobs=True)
    sc = SpeculativeConfig(num_draft_tokens=4)
    plain = generate(model, _text(prompt), gc)
    s1, s2, s3 = {}, {}, {}
    a = generate(model, _text(prompt), gc, speculative=sc, stats=s1)
    b = generate(model, _text(prompt), gc, speculative=sc, stats=s2, replay=False)
    c = generate(model, _text(prompt), gc, speculative=sc, stats=s3)
    assert s1["path"] == "ring" and _same_bits(a, b) and _same_bits(a, c)
    assert s1["accepted"] == s2["accepted"] == s3["accepted"] and sum(s1["accepted"]) == s1["token_calls"]
    # a perfect script from the plain ring run
    s4 = {}
    ids, lengths, lps, sums = generate(model, _text(prompt), gc, speculative=sc, draft_script=plain[0].numpy(), stats=s4)
    checked = _check_teacher_forced(model, prompt, ids.numpy(), lps.numpy(), greedy, f"perfect script (greedy={greedy})")
    assert 4 * checked >= 3 * M * N, checked
    print(f"accepted (lookup) {s1['accepted']}, (perfect script) {s4['accepted']}, tokens per call {s4['tokens_per_call']:.2f}")
    assert sum(s4["accepted"]) == s4["token_calls"] and s4["token_calls"] < N - 1         # fewer calls than tokens
    if checked == M * N and torch.equal(ids, plain[0]):      # the script was this path's own continuation: accepted in full
        assert s4["accepted"] == list(S.step_counts(N, 5)[0]), s4["accepted"]
    assert 4 * _check_teacher_forced(model, prompt, a[0].numpy(), a[2].numpy(), greedy, f"lookup (greedy={greedy})") >= 3 * M * N
    # the default call after the speculative ones: the bits it returned before, over the generator it had
    gen = model._generator
    assert _same_bits(generate(model, _text(prompt), gc), plain) and model._generator is gen and model._spec_generator is not None


def test_bf16_ring_over_several_key_chunks():
    """mem_len 300: a call's 305 keys span three 128-key chunks of the ring attention, and the rejected positions of 23 calls take the
    origin back around the ring's end -- the teacher-forced gate on a run that never accepts, on lookup drafts and on a script of the
    path's own tokens, and replay against eager launches"""
    from bdm_db1_amd import GenerationConfig, SpeculativeConfig, generate
    model = _bf16_model(mem_len=300)[1]
    n = 24
    prompt = np.random.default_rng(45).integers(0, HI, (2, 6))
    gc = GenerationConfig(max_new_tokens=n, greedy=False, top_p=0.9, seed=9, vocab_hi=HI, logprobs=True)
    sc = SpeculativeConfig(num_draft_tokens=4)
    s1, s2 = {}, {}
    wrong = generate(model, _text(prompt), gc, speculative=sc, draft_script=np.full((2, n), HI, np.int32), stats=s1)
    assert s1["path"] == "ring" and s1["accepted"][1] == n - 1
    own = generate(model, _text(prompt), gc, speculative=sc, draft_script=wrong[0].numpy(), stats=s2)
    eager = generate(model, _text(prompt), gc, speculative=sc, draft_script=wrong[0].numpy(), replay=False)
    look = generate(model, _text(prompt), gc, speculative=sc)
    print(f"several chunks: accepted with the path's own tokens as the script {s2['accepted']}")
    assert _same_bits(own, eager)
    for who, got in (("never accepts", wrong), ("own script", own), ("lookup", look)):
        assert 4 * _check_teacher_forced(model, prompt, got[0].numpy(), got[2].numpy(), False, f"several chunks, {who}") >= 3 * 2 * n


def test_bf16_ring_eos_inside_an_accepted_run(bf16):
    from bdm_db1_amd import GenerationConfig, SpeculativeConfig, generate
    model = bf16
    prompt = np.random.default_rng(43).integers(0, HI, (M, 6))
    gc = GenerationConfig(max_new_tokens=N, greedy=False, top_p=0.9, seed=77, vocab_hi=HI, pad_id=PAD, logprobs=True)      # (sampled: distinct tokens)
    base = generate(model, _text(prompt), gc)[0]
    eos = int(base[0, 3])
    first = int(np.nonzero(base[0].numpy() == eos)[0][0])
    gc = dataclasses.replace(gc, eos_id=eos)
    plain = generate(model, _text(prompt), gc)
    stats = {}
    ids, lengths, lps, sums = generate(model, _text(prompt), gc, speculative=SpeculativeConfig(num_draft_tokens=4), draft_script=base.numpy(), stats=stats)
    assert first == 3 and int(lengths[0]) == 3 and int(ids[0, 3]) == eos and (ids[0, 4:] == PAD).all() and (lps[0, 4:] == 0).all()
    assert stats["accepted"][3] >= 1                 # the first step kept tokens 1 .. 3 of its five positions: the EOS sat inside the run
    assert torch.equal(ids[0], plain[0][0]) and int(plain[1][0]) == 3


def test_bf16_ring_fp8_prefill_and_prefixed(bf16):
    from bdm_db1_amd import GenerationConfig, PrefixCache, Prefixed, SpeculativeConfig, generate
    model = bf16
    rng = np.random.default_rng(44)
    prompt = rng.integers(0, HI, (M, 9))
    gc = GenerationConfig(max_new_tokens=N, vocab_hi=HI, pad_id=PAD, logprobs=True)
    sc = SpeculativeConfig(num_draft_tokens=4)
    # the fp8 ring: replay == eager launches, and every token within 2e-2 max|l| of the list-form arg-max (the fp8 loops' own gate)
    s = {}
    a = generate(model, _text(prompt), gc, speculative=sc, kv_cache="fp8", stats=s)
    b = generate(model, _text(prompt), gc, speculative=sc, kv_cache="fp8", replay=False)
    assert s["path"] == "ring" and model._spec_generator.ring.kv_dtype == "fp8" and _same_bits(a, b)
    tf = _teacher_forced(model, _text(prompt), a[0].numpy())
    for r in range(M):
        for t in range(N):
            l = tf[t, r, :HI]
            assert l[int(a[0][r, t])] >= l.max() - 2e-2 * np.abs(l).max(), ("fp8", r, t)
    # the ring prefill and a Prefixed prompt only change the prefill
    was = model.use_ring_prefill
    try:
        model.use_ring_prefill = True
        c = generate(model, _text(prompt), gc, speculative=sc)
        assert 4 * _check_teacher_forced(model, prompt, c[0].numpy(), c[2].numpy(), True, "ring prefill") >= 3 * M * N
    finally:
        model.use_ring_prefill = was
    cache = PrefixCache(model, 2)
    handles = cache.put(_text(prompt[:2, :5]))
    d = generate(model, Prefixed(cache, [handles[0], handles[1], handles[0]], _text(np.concatenate([prompt[:2, 5:], prompt[:1, 5:]]))), gc, speculative=sc)
    whole = np.concatenate([prompt[:2], prompt[:1]])
    assert 4 * _check_teacher_forced(model, whole, d[0].numpy(), d[2].numpy(), True, "Prefixed") >= 3 * M * N
    assert torch.equal(d[0][0], d[0][2])             # two continuations of one handle with one suffix


def test_refusals_leave_the_model_alone(bf16):
    from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, GenerationConfig, SpeculativeConfig, generate
    model = bf16
    calls = []
    hook = model.register_forward_pre_hook(lambda m, a: calls.append(1))
    x = _text(np.zeros((M, 6), np.int64))
    gc, sc = GenerationConfig(max_new_tokens=N, vocab_hi=HI), SpeculativeConfig()
    try:
        for kw in (dict(constraints=DecodingConstraints(no_repeat_ngram_size=2)), dict(constraints=DecodingConstraints(stop_sequences=((5,),))),
                   dict(config=dataclasses.replace(gc, logprobs=True, top_logprobs=3)), dict(config=BeamSearchConfig(max_new_tokens=N)),
                   dict(speculative=SpeculativeConfig(num_draft_tokens=15), prompt=_text(np.zeros((5, 6), np.int64))),
                   dict(prompt=_text(np.zeros((13, 6), np.int64))), dict(draft_script=np.zeros((M, N + 1), np.int32)),
                   dict(draft_script=np.zeros((M, N), np.float32)), dict(config=dataclasses.replace(gc, max_new_tokens=4097)),
                   dict(prompt=_text(np.zeros((M, 4090), np.int64))), dict(kv_cache="fp8", graphed=False), dict(speculative=7)):
            args = dict(prompt=x, config=gc, speculative=sc)
            args.update(kw)
            with pytest.raises(ValueError):
                generate(model, args.pop("prompt"), args.pop("config"), **args)
        with pytest.raises(ValueError):
            generate(model, x, gc, draft_script=np.zeros((M, N), np.int32))
    finally:
        hook.remove()
    assert not calls
