"""Continuous batching end to end (bdm_db1_amd.serving): every request of a stream over 3 recycled slots against the eager list-form path,
teacher-forced on the request's own prompt ALONE; limits, EOS, determinism, the recycling itself, mixed prompt kinds and the refusals."""
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
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD, SLOTS = 32000, 31999, 3
LENS = [5, 9, 5, 70, 9, 5, 12, 9]
LIMITS = [4, 16, 4, 6, 16, 4, 4, 8]


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


@pytest.fixture(scope="module")
def model():
    return _bf16_model(mem_len=100)[1]


@pytest.fixture(scope="module")
def prompts():
    rng = np.random.default_rng(21)
    return [rng.integers(0, HI, (1, n)) for n in LENS]


def _cfg(greedy, **kw):
    from bdm_db1_amd import GenerationConfig
    return GenerationConfig(max_new_tokens=16, greedy=greedy, top_p=0.9, seed=4321, vocab_hi=HI, pad_id=PAD, sync_every=2, **kw)


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


def _check_request(model, x, ids, length, limit, greedy, eos=None, who=None):
    """the request's tokens against the eager path on its own prompt: chosen logit >= max (greedy) / >= min of the kept set (top-p 0.9),
    minus 2e-2 * max|l|, token 0 included; then the bookkeeping: length, EOS, pad_id after the end"""
    ids = ids.numpy() if torch.is_tensor(ids) else np.asarray(ids)
    assert ids.shape == (limit,) and ids.dtype == np.int32, who
    n = length if length == limit else length + 1           # the tokens picked: those before EOS, and EOS
    assert 0 <= length <= limit
    if eos is None:
        assert length == limit, who
    elif length < limit:
        assert ids[length] == eos, who
    assert eos is None or eos not in ids[:length].tolist(), who
    assert (ids[n:] == PAD).all(), who
    tf = _teacher_forced(model, x, ids[None, :n])
    for t in range(n):
        l = tf[t, 0, :HI]
        noise = 2e-2 * np.abs(l).max()
        assert 0 <= ids[t] < HI
        if greedy:
            assert l[ids[t]] >= l.max() - noise, (who, t)
        else:
            kept = R.kept_set(l, 0, HI, 1.0, 0, 0.9)[0]
            assert l[ids[t]] >= l[kept].min() - noise, (who, t)


def _static_replays(limits, slots):
    return sum(max(limits[i:i + slots]) - 1 for i in range(0, len(limits), slots))


@pytest.fixture(scope="module")
def greedy_run(model, prompts):
    from bdm_db1_amd import generate_stream
    stats = {}
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    got = list(generate_stream(model, reqs, _cfg(True), slots=SLOTS, stats=stats))
    return got, stats


@pytest.mark.parametrize("greedy", [True, False])
def test_stream_follows_the_eager_path_request_by_request(model, prompts, greedy, greedy_run):
    from bdm_db1_amd import generate_many, generate_stream
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    stats = {}
    got, stats = greedy_run if greedy else (list(generate_stream(model, reqs, _cfg(False), slots=SLOTS, stats=stats)), stats)
    assert sorted(i for i, _, _ in got) == list(range(8))                   # every index exactly once
    for i, ids, length in got:
        _check_request(model, _text(prompts[i]), ids, length, LIMITS[i], greedy, who=i)
    # recycling is real: fewer token steps than the same list in lockstep batches of ``slots``
    assert stats["replays"] < _static_replays(LIMITS, SLOTS)
    assert stats["replays"] * SLOTS >= sum(l - 1 for l in LIMITS)
    assert stats["admitted"] == 8 and 0 < stats["occupancy"] <= 1 and stats["no_candidate"] == 0
    assert 1 <= stats["prefill_calls"] <= 8
    assert abs(stats["occupancy"] - sum(l - 1 for l in LIMITS) / (stats["replays"] * SLOTS)) < 1e-12
    # the same call twice: identical results, in request order from generate_many
    ids2, len2 = generate_many(model, reqs, _cfg(greedy), slots=SLOTS)
    by_index = {i: (ids, n) for i, ids, n in got}
    for i in range(8):
        assert torch.equal(ids2[i], by_index[i][0]) and len2[i] == by_index[i][1]


def test_stream_ids_select_the_draws(model, prompts):
    """sampling: the default stream ids are the request indices; other ids give other draws; and a request's token 0 -- the prefill's logits,
    its stream id, token index 0 -- does not depend on its slot, on the requests before it or on when it was admitted.  (Checked bit for bit
    on the two requests whose prompt length nobody shares, so that they are prefilled alone in every run; the later tokens' logits come from
    decode batches of other sizes and may differ in bf16 noise, their draws are pinned by the kernel test.)"""
    from bdm_db1_amd import generate_many
    cfg = _cfg(False)
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    a, _ = generate_many(model, reqs, cfg, slots=SLOTS)
    b, _ = generate_many(model, reqs, cfg, slots=SLOTS, stream_ids=list(range(8)))
    c, _ = generate_many(model, reqs, cfg, slots=SLOTS, stream_ids=[100 + i for i in range(8)])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert sum(int((x != y).sum()) for x, y in zip(a, c)) > 0
    order = [3, 7, 0, 5, 1, 6, 2, 4]
    d, _ = generate_many(model, [reqs[i] for i in order], cfg, slots=2, stream_ids=order)
    for i in (3, 6):
        alone, _ = generate_many(model, [reqs[i]], cfg, slots=1, stream_ids=[i])
        assert int(alone[0][0]) == int(a[i][0]) == int(d[order.index(i)][0]), i


def test_one_stream_at_a_time(model, prompts, greedy_run):
    from bdm_db1_amd import generate_stream
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    first = generate_stream(model, reqs, _cfg(True), slots=SLOTS)
    got = [next(first)]
    second = generate_stream(model, reqs, _cfg(True), slots=SLOTS)
    with pytest.raises(RuntimeError):
        next(second)                                  # the first stream's slots are not touched
    got += list(first)
    want = {i: (ids, n) for i, ids, n in greedy_run[0]}
    assert sorted(i for i, _, _ in got) == list(range(8))
    for i, ids, n in got:
        assert torch.equal(ids, want[i][0]) and n == want[i][1]
    third = generate_stream(model, reqs, _cfg(True), slots=SLOTS)
    next(third)
    third.close()                                     # an abandoned stream gives the model back
    assert len(list(generate_stream(model, reqs, _cfg(True), slots=SLOTS))) == 8


def test_eos_frees_the_slot_early(model, prompts, greedy_run):
    from bdm_db1_amd import generate_stream
    base = {i: ids for i, ids, _ in greedy_run[0]}
    eos = int(base[1][5])
    first = int(np.nonzero(base[1].numpy() == eos)[0][0])
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    stats = {}
    got = {i: (ids, n) for i, ids, n in generate_stream(model, reqs, _cfg(True, eos_id=eos), slots=SLOTS, stats=stats)}
    assert sorted(got) == list(range(8))
    assert got[1][1] == first and int(got[1][0][first]) == eos and (got[1][0][first + 1:] == PAD).all()
    if first == 5:
        assert got[1][1] == 5
    for i, (ids, n) in got.items():
        _check_request(model, _text(prompts[i]), ids, n, LIMITS[i], True, eos=eos, who=i)
    assert stats["replays"] <= greedy_run[1]["replays"]


def test_eager_launches_over_the_same_ring(model, prompts):
    from bdm_db1_amd import generate_stream
    reqs = [(_text(p), lim) for p, lim in zip(prompts, LIMITS)]
    stats = {}
    got = list(generate_stream(model, reqs, _cfg(True), slots=SLOTS, stats=stats, replay=False))
    assert sorted(i for i, _, _ in got) == list(range(8)) and stats["replays"] < _static_replays(LIMITS, SLOTS)
    for i, ids, length in got:
        _check_request(model, _text(prompts[i]), ids, length, LIMITS[i], True, who=i)


def _image_batches(rng):
    from bdm_db1_amd.data import ICTaskInput, VQATaskInput
    ic = dict(prompt_seq=rng.integers(0, HI, (2, 3)), img_seq=rng.standard_normal((2, 3, 32, 32)).astype(np.float32))
    vqa = dict(prompt_seq=rng.integers(0, HI, (3, 3)), img_seq=rng.standard_normal((3, 3, 32, 32)).astype(np.float32),
               text_seq=rng.integers(1, HI, (3, 7)), ques_len=np.array([5, 3, 5]))
    mk_ic = lambda f, rows: ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(f["prompt_seq"][rows]),
                                        img_seq=_tdev(f["img_seq"][rows]), text_seq=_tdev(np.zeros((len(rows), 0), np.int64)))
    mk_vqa = lambda f, rows, n: VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None,
                                             prompt_seq=_tdev(f["prompt_seq"][rows]), img_seq=_tdev(f["img_seq"][rows]),
                                             text_seq=_tdev(f["text_seq"][rows][:, :n]), img_id_seq=None, ques_id_seq=None, ques_len=None)
    return ic, vqa, mk_ic, mk_vqa


def test_mixed_kinds_and_a_ragged_vqa_batch(model):
    from bdm_db1_amd import answer_stream, caption_stream, generate_stream, question_prompts
    from bdm_db1_amd.data import VQATaskInput
    from bdm_db1_amd.generation import caption_prompt
    rng = np.random.default_rng(33)
    ic, vqa, mk_ic, mk_vqa = _image_batches(rng)
    text = rng.integers(0, HI, (2, 6))
    batch = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(vqa["prompt_seq"]),
                         img_seq=_tdev(vqa["img_seq"]), text_seq=_tdev(vqa["text_seq"]), img_id_seq=None, ques_id_seq=None,
                         ques_len=_tdev(vqa["ques_len"]))
    cfg = dataclasses.replace(_cfg(True), max_new_tokens=6)
    # one list: two text rows, a caption batch of 2, the VQA batch split by question length (rows [1], then rows [0, 2])
    parts = question_prompts(batch)
    assert [r.tolist() for _, r in parts] == [[1], [0, 2]]
    items = [_text(text), (caption_prompt(mk_ic(ic, [0, 1])), 4)] + [p for p, _ in parts]
    stats = {}
    got = {i: (ids, n) for i, ids, n in generate_stream(model, items, cfg, slots=SLOTS, stats=stats)}
    assert sorted(got) == list(range(7)) and stats["admitted"] == 7 and stats["prefill_calls"] >= 4
    own = [(_text(text[[0]]), 6), (_text(text[[1]]), 6), (mk_ic(ic, [0]), 4), (mk_ic(ic, [1]), 4), (mk_vqa(vqa, [1], 3), 6),
           (mk_vqa(vqa, [0], 5), 6), (mk_vqa(vqa, [2], 5), 6)]
    for i, (x, lim) in enumerate(own):
        _check_request(model, x, got[i][0], got[i][1], lim, True, who=i)
    # answer_stream takes the ragged batch as it is; the indices are the batch's rows
    ans = {i: (ids, n) for i, ids, n in answer_stream(model, [batch], cfg, slots=2)}
    assert sorted(ans) == [0, 1, 2]
    for i, n in enumerate([5, 3, 5]):
        _check_request(model, mk_vqa(vqa, [i], n), ans[i][0], ans[i][1], 6, True, who=("vqa", i))
    cap = {i: (ids, n) for i, ids, n in caption_stream(model, [(mk_ic(ic, [0, 1]), 3)], cfg, slots=2)}
    assert sorted(cap) == [0, 1]
    for i in range(2):
        _check_request(model, mk_ic(ic, [i]), cap[i][0], cap[i][1], 3, True, who=("ic", i))
    from bdm_db1_amd import answer_questions
    with pytest.raises(ValueError):
        answer_questions(model, batch, cfg)          # (the lockstep entry point still asks for one length)


def test_refusals_come_before_any_launch(model, prompts):
    from bdm_db1_amd import GenerationConfig, generate_many, generate_stream
    cfg32, fp32, _ = _fp32_model()
    x = _text(np.zeros((1, 4), np.int64))
    with pytest.raises(ValueError):
        generate_stream(fp32, [x], GenerationConfig(max_new_tokens=4, vocab_hi=cfg32["text_vocab_size"]), slots=2)
    assert getattr(fp32, "_slot_generator", None) is None
    model._slot_generator = None
    with pytest.raises(ValueError):
        generate_stream(model, [(_text(prompts[0]), 4), (_text(prompts[1]), 17)], _cfg(True), slots=SLOTS)       # limit > max_new_tokens = 16
    assert model._slot_generator is None                                     # nothing was built, nothing launched
    with pytest.raises(ValueError):
        generate_many(model, iter([(_text(prompts[0]), 0)]), _cfg(True), slots=SLOTS)
    with pytest.raises(ValueError):
        generate_stream(model, [x], _cfg(True), slots=0)


def test_one_generator_class_serves_the_stream_and_generate():
    from bdm_db1_amd import GenerationConfig, generate, generate_many, generate_stream
    model = _bf16_model()[1]
    rng = np.random.default_rng(8)
    cfg = GenerationConfig(max_new_tokens=4, vocab_hi=HI, pad_id=PAD, sync_every=2)
    reqs = [_text(rng.integers(0, HI, (1, n))) for n in (5, 7, 5)]
    ids, lengths = generate_many(model, reqs, cfg, slots=2)
    assert len(ids) == 3 and lengths == [4, 4, 4]
    generate(model, reqs[0], cfg)
    assert type(model._slot_generator) is type(model._generator) and model._slot_generator is not model._generator
    gen = model._slot_generator
    first = generate_stream(model, reqs, cfg, slots=2)
    next(first)
    with pytest.raises(RuntimeError):
        next(generate_stream(model, reqs, cfg, slots=2))
    assert model._slot_generator is gen and gen.busy              # nothing was rebuilt, the first stream still holds the slots
    assert len(list(first)) == 2 and not gen.busy
