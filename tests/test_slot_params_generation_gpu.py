"""Per-request sampling parameters end to end (``generate_stream(..., per_request=True)``): the 2-layer bf16 model, the eight text prompts
and limits, 3 slots and ``sync_every=2`` of tests/test_serving_gpu.py.  With no params on any request the stream is the shared-config
stream bit for bit; with mixed params every request follows the eager path on its own prompt under its OWN parameters."""
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

import select_rule as R  # noqa: E402
from gpu_common import DEV, _bf16_model, _need_gpu, _tdev  # noqa: E402,F401
from test_serving_gpu import HI, LENS, LIMITS, PAD, SLOTS, _cfg, _static_replays, _teacher_forced, _text  # noqa: E402

WIN = (1000, 3000)


@pytest.fixture(scope="module")
def model():
    return _bf16_model(mem_len=100)[1]


@pytest.fixture(scope="module")
def prompts():
    rng = np.random.default_rng(21)
    return [rng.integers(0, HI, (1, n)) for n in LENS]


def _sampled(seed=77):
    from bdm_db1_amd import SamplingParams
    return SamplingParams(greedy=False, top_p=0.9, temperature=0.8, seed=seed)


def _mixed(prompts, seed1=77):
    """requests alternate: the config's default (greedy), sampled at top-p 0.9 / T 0.8 / seed 77, greedy in the narrow window [1000, 3000)"""
    from bdm_db1_amd import SamplingParams
    kinds = [None, _sampled(), SamplingParams(vocab_lo=WIN[0], vocab_hi=WIN[1])]
    reqs = []
    for i, (p, lim) in enumerate(zip(prompts, LIMITS)):
        sp = _sampled(seed1) if i == 1 else kinds[i % 3]
        reqs.append((_text(p), lim) if sp is None else (_text(p), lim, sp))
    return reqs


def _check_request(model, x, ids, length, limit, v, who=None):
    """the request's tokens against the eager path on its own prompt under its own resolved parameters ``v``: chosen logit >= max of its
    window (greedy) / >= min of its kept set (sampling), minus 2e-2 * max|l| over the window (the bf16 allowance of test_serving_gpu.py);
    no EOS in these streams: every request runs to its limit"""
    ids = ids.numpy() if torch.is_tensor(ids) else np.asarray(ids)
    lo, hi = v["vocab_lo"], v["vocab_hi"]
    assert ids.shape == (limit,) and ids.dtype == np.int32 and length == limit, who
    tf = _teacher_forced(model, x, ids[None, :])
    for t in range(limit):
        l = tf[t, 0]
        noise = 2e-2 * np.abs(l[lo:hi]).max()
        assert lo <= ids[t] < hi, (who, t)
        if v["greedy"]:
            assert l[ids[t]] >= l[lo:hi].max() - noise, (who, t)
        else:
            kept = R.kept_set(l, lo, hi, v["temperature"], v["top_k"], v["top_p"])[0]
            assert l[ids[t]] >= l[kept].min() - noise, (who, t)


@pytest.mark.parametrize("kind", ["greedy", "sampled", "logprobs"])
def test_the_flag_alone_changes_nothing(model, prompts, kind):
    from bdm_db1_amd import generate_many
    from bdm_db1_amd.generation import DecodeKey
    cfg = _cfg(kind != "sampled", **(dict(logprobs=True, top_logprobs=3) if kind == "logprobs" else {}))
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    s0, s1 = {}, {}
    want = generate_many(model, reqs, cfg, slots=SLOTS, stats=s0)
    key0 = model._slot_generator.key
    got = generate_many(model, reqs, cfg, slots=SLOTS, stats=s1, per_request=True)
    assert len(got) == len(want) == (5 if kind == "logprobs" else 2)
    for a, b in zip(got, want):             # ids, lengths (, logprobs, top_ids, top_logprobs): bit for bit
        assert len(a) == len(b) == 8
        for x, y in zip(a, b):
            assert (x == y) if isinstance(x, int) else (x.dtype == y.dtype and x.numpy().tobytes() == y.numpy().tobytes())
    assert s0 == s1
    # the flag is part of the generator's key, and only when it is set
    plain = DecodeKey(rows=SLOTS, cfg=cfg, V=model.total_vocab_size, hi=HI, constraints=None, n=None, per_request=False, caps=None)
    assert key0 == plain and model._slot_generator.key == DecodeKey(rows=SLOTS, cfg=cfg, V=model.total_vocab_size, hi=HI, constraints=None,
                                                                    n=None, per_request=True, caps=None)
    assert model._slot_generator.state.params.shape == (SLOTS, 8)


@pytest.fixture(scope="module")
def mixed_run(model, prompts):
    from bdm_db1_amd import generate_stream
    stats = {}
    got = list(generate_stream(model, _mixed(prompts), _cfg(True), slots=SLOTS, stats=stats, per_request=True))
    return got, stats


def test_mixed_requests_follow_the_eager_path_each_under_its_own_parameters(model, prompts, mixed_run):
    got, stats = mixed_run
    cfg, V = _cfg(True), model.total_vocab_size
    assert sorted(i for i, _, _ in got) == list(range(8))                   # every index exactly once
    reqs = _mixed(prompts)
    from bdm_db1_amd import SamplingParams
    for i, ids, length in got:
        sp = reqs[i][2] if len(reqs[i]) == 3 else SamplingParams()
        v = sp.resolve(cfg, V, HI)
        assert v["greedy"] == (i % 3 != 1) and (v["vocab_lo"], v["vocab_hi"]) == (WIN if i % 3 == 2 else (0, HI))
        _check_request(model, _text(prompts[i]), ids, length, LIMITS[i], v, who=i)
        if i % 3 == 2:
            assert ((ids.numpy() >= WIN[0]) & (ids.numpy() < WIN[1])).all(), i
    assert stats["replays"] < _static_replays(LIMITS, SLOTS)
    assert stats["admitted"] == 8 and stats["no_candidate"] == 0
    # the windowed requests are not what the config alone would have given them
    from bdm_db1_amd import generate_many
    plain, _ = generate_many(model, [(_text(p), lim) for p, lim in zip(prompts, LIMITS)], cfg, slots=SLOTS)
    by_index = {i: ids for i, ids, _ in got}
    assert any(not torch.equal(by_index[i], plain[i]) for i in (2, 5))


def test_token_0_is_the_requests_own(model, prompts):
    """the two prompts whose length nobody shares are prefilled alone: token 0 under given SamplingParams and stream id is token 0 of
    ``generate`` under a GenerationConfig of those values and that stream id, whatever the request order and the slot count"""
    from bdm_db1_amd import GenerationConfig, SamplingParams, generate, generate_many
    own = {3: SamplingParams(greedy=False, top_p=0.9, temperature=0.8, seed=77),
           6: SamplingParams(greedy=False, top_k=20, temperature=1.5, seed=(1 << 40) + 9, vocab_lo=WIN[0], vocab_hi=WIN[1])}
    reqs = [(_text(p), lim) + ((own[i],) if i in own else ()) for i, (p, lim) in enumerate(zip(prompts, LIMITS))]
    cfg = _cfg(True)
    a, _ = generate_many(model, reqs, cfg, slots=SLOTS, per_request=True)
    order = [3, 7, 0, 5, 1, 6, 2, 4]
    d, _ = generate_many(model, [reqs[i] for i in order], cfg, slots=2, stream_ids=order, per_request=True)
    for i, sp in own.items():
        v = sp.resolve(cfg, model.total_vocab_size, HI)
        lock = GenerationConfig(max_new_tokens=2, pad_id=PAD, **v)
        ids, _ = generate(model, _text(prompts[i]), lock, stream_ids=[i])
        assert int(ids[0, 0]) == int(a[i][0]) == int(d[order.index(i)][0]), i
        assert v["vocab_lo"] <= int(a[i][0]) < v["vocab_hi"]


def test_a_requests_seed_is_its_own(model, prompts, mixed_run):
    from bdm_db1_amd import generate_many
    base = {i: ids for i, ids, _ in mixed_run[0]}
    other, _ = generate_many(model, _mixed(prompts, seed1=78), _cfg(True), slots=SLOTS, per_request=True)
    assert not torch.equal(other[1], base[1])                               # request 1: another seed, other draws
    for i in range(8):
        if i != 1:
            assert int(other[i][0]) == int(base[i][0]), i                   # everybody else's token 0 is what it was


def test_refusals_come_before_any_launch(model, prompts):
    from bdm_db1_amd import DecodingConstraints, SamplingParams, generate_many, generate_stream
    model._slot_generator = None
    x = _text(prompts[0])
    with pytest.raises(ValueError, match="per_request"):
        generate_stream(model, [(x, 4), (x, 4, _sampled())], _cfg(True), slots=SLOTS)                      # params with the flag off
    with pytest.raises(ValueError):
        generate_stream(model, [(x, 4, SamplingParams(vocab_hi=model.total_vocab_size + 1))], _cfg(True), slots=SLOTS, per_request=True)
    with pytest.raises(ValueError):
        generate_stream(model, [(x, 4, _sampled())], _cfg(True), slots=SLOTS, per_request=True,
                        constraints=DecodingConstraints(min_new_tokens=5))                                # limit 4 < min_new_tokens 5
    with pytest.raises(ValueError):
        generate_stream(model, [(x, 4, SamplingParams(top_p=0.0))], _cfg(True), slots=SLOTS, per_request=True)
    assert model._slot_generator is None                                     # nothing was built, nothing launched
    with pytest.raises(ValueError, match="per_request"):                     # a lazy iterable: refused when the request is reached
        generate_many(model, iter([(x, 4, _sampled())]), _cfg(True), slots=SLOTS)


def test_constraints_work_with_mixed_parameters(model, prompts):
    from bdm_db1_amd import DecodingConstraints, generate_many
    ids, lengths = generate_many(model, _mixed(prompts), _cfg(True), slots=SLOTS, per_request=True,
                                 constraints=DecodingConstraints(no_repeat_ngram_size=2))
    assert lengths == LIMITS
    for i, row in enumerate(ids):
        toks = row.tolist()
        bigrams = list(zip(toks, toks[1:]))
        assert len(set(bigrams)) == len(bigrams), i
        if i % 3 == 2:
            assert all(WIN[0] <= t < WIN[1] for t in toks), i
