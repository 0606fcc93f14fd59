"""Token log-probs from generation, end to end on the small test models: the fp32 eager loop against the rule on its own teacher-forced
logits, the bf16 ring path (graph replay against eager launches bit for bit, and against the eager list-form logits within bf16 noise), EOS,
constraints, the slot stream against ``generate``, and best-of-n sampling against ``generate`` over the repeated prompt."""
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

import constraint_rule as C  # noqa: E402
import logprob_rule as L  # noqa: E402
import select_rule as R  # noqa: E402
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD = 32000, 31999


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
    """the logits [n, M, V] (as stored, widened to float64) of the eager list-form path fed the prompt, then ids[:, t] one token per call"""
    out = []
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([x], compute_loss=False, mems=model.init_mem(ids.shape[0]))
        for t in range(ids.shape[1]):
            out.append(logits[:, -1].double().cpu().numpy())
            logits, _, mems = model([_text(ids[:, t:t + 1])], compute_loss=False, mems=mems)
    return np.stack(out)


def _f32_sum(row):
    s = np.float32(0.0)
    for v in row:
        s = np.float32(s + np.float32(v))
    return s


def test_fp32_eager_logprobs_follow_the_rule(fp32):
    from bdm_db1_amd import GenerationConfig, generate
    cfg, model = fp32
    hi, M, n = cfg["text_vocab_size"], 2, 8
    x = _text(np.random.default_rng(1).integers(0, hi, (M, 6)))
    gc = GenerationConfig(max_new_tokens=n, greedy=False, top_p=0.9, seed=99, vocab_hi=hi)
    ids0, len0 = generate(model, x, gc)
    stats = {}
    ids, lengths, lps, sums = generate(model, x, dataclasses.replace(gc, logprobs=True), stats=stats)
    assert stats["path"] == "eager" and torch.equal(ids, ids0) and torch.equal(lengths, len0)
    assert lps.dtype == torch.float32 and tuple(lps.shape) == (M, n) and sums.dtype == torch.float32 and tuple(sums.shape) == (M,)
    tf = _teacher_forced(model, x, ids.numpy())
    want = np.array([[L.logprob(tf[t, r], int(ids[r, t]), 0, hi) for t in range(n)] for r in range(M)])
    err = np.abs(lps.numpy() - want).max()
    print(f"max |lp - lp64| = {err:.3e}")
    assert err <= 1e-5, err
    assert (lps.numpy() < 0).all()
    for r in range(M):
        assert sums.numpy()[r] == _f32_sum(lps.numpy()[r])                 # bit for bit: one fp32 add per token, in order


@pytest.mark.parametrize("greedy", [True, False])
def test_bf16_ring_logprobs_replay_equals_eager_launches_and_follow_the_eager_logits(bf16, greedy):
    from bdm_db1_amd import GenerationConfig, generate
    model, M, n = bf16, 3, 8
    x = _text(np.random.default_rng(2).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=n, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=HI, logprobs=True)
    stats = {}
    ids, lengths, lps, sums = generate(model, x, gc, stats=stats)
    ids_e, len_e, lps_e, sums_e = generate(model, x, gc, replay=False)
    assert stats["path"] == "ring"
    assert torch.equal(ids, ids_e) and torch.equal(lengths, len_e)
    assert torch.equal(lps.view(torch.int32), lps_e.view(torch.int32)) and torch.equal(sums.view(torch.int32), sums_e.view(torch.int32))
    plain, plen = generate(model, x, dataclasses.replace(gc, logprobs=False))
    assert torch.equal(plain, ids) and torch.equal(plen, lengths)        # the flag does not change a token
    ids, lps = ids.numpy(), lps.numpy()
    tf = _teacher_forced(model, x, ids)
    checked = 0
    for r in range(M):
        for t in range(n):
            l = tf[t, r, :HI]
            inside = ids[r, t] == int(np.argmax(l)) if greedy else R.kept_set(l, 0, HI, 1.0, 0, 0.9)[0][ids[r, t]]
            if not inside:      # the ring's token left the eager arg-max / kept set (bf16 noise at a near tie): the row is compared up to here
                break
            bound = 2 * 2e-2 * np.abs(l).max()
            assert abs(lps[r, t] - L.logprob(l, int(ids[r, t]), 0, HI)) <= bound, (r, t)
            checked += 1
    assert checked >= M                                                   # (token 0 comes from the same prefill call)
    for r in range(M):
        assert sums.numpy()[r] == _f32_sum(lps[r])


def test_eos_is_scored_and_the_rest_is_zero(bf16):
    from bdm_db1_amd import GenerationConfig, generate
    model = bf16
    x = _text(np.random.default_rng(6).integers(0, HI, (3, 6)))
    gc = GenerationConfig(max_new_tokens=8, vocab_hi=HI, seed=5)
    base, _ = generate(model, x, gc)
    eos = int(base[0, 2])
    ids, lengths, lps, sums = generate(model, x, dataclasses.replace(gc, eos_id=eos, pad_id=PAD, logprobs=True))
    ids, lengths, lps, sums = ids.numpy(), lengths.numpy(), lps.numpy(), sums.numpy()
    first = int(np.nonzero(base[0].numpy() == eos)[0][0])
    assert first <= 2 and lengths[0] == first and ids[0, first] == eos
    assert lps[0, first] != 0.0 and (lps[0, :first + 1] < 0).all() and (lps[0, first + 1:] == 0.0).all()
    assert sums[0] == _f32_sum(lps[0, :first + 1])
    for r in range(3):
        k = lengths[r] + 1 if lengths[r] < 8 else 8
        assert (lps[r, :k] != 0.0).all() and (lps[r, k:] == 0.0).all() and sums[r] == _f32_sum(lps[r])


def test_logprobs_under_constraints_follow_the_edited_logits(fp32):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate
    cfg, model = fp32
    hi, M, n = cfg["text_vocab_size"], 2, 8
    V = int(model.total_vocab_size)
    x = _text(np.random.default_rng(3).integers(0, hi, (M, 6)))
    gc = GenerationConfig(max_new_tokens=n, greedy=False, top_p=0.9, seed=7, vocab_hi=hi, logprobs=True)
    plain = generate(model, x, gc)[0]
    bad = int(plain[0, 0])
    cons = DecodingConstraints(repetition_penalty=1.3, bad_token_ids=(bad,))
    ids, lengths, lps, sums = generate(model, x, gc, constraints=cons)
    ids, lps = ids.numpy(), lps.numpy()
    assert not (ids == bad).any() and np.isfinite(lps).all()
    tf = _teacher_forced(model, x, ids)
    for t in range(n):
        e = C.apply(tf[t].astype(np.float32), ids, t, V=V, dtype=C.F32, theta=1.3, bad=(bad,)).astype(np.float64)
        assert np.isneginf(e[:, bad]).all()                               # a banned token has no finite log-prob to get
        for r in range(M):
            assert abs(lps[r, t] - L.logprob(e[r], int(ids[r, t]), 0, hi)) <= 1e-5, (r, t)


def test_stream_logprobs_equal_those_of_generate(bf16):
    """5 requests over 2 slots.  Every look of the host (``sync_every`` 8 > the longest limit) finds both slots done, so the requests move in
    as the pairs (0, 1), (2, 3) and then 4 alone: ``generate`` over the same pair, with the same stream ids, runs the same prefill and the
    same two-row token steps."""
    from bdm_db1_amd import GenerationConfig, generate, generate_many, generate_stream
    model = bf16
    rng = np.random.default_rng(12)
    prompts = [rng.integers(0, HI, (1, 6)) for _ in range(5)]
    limits = [3, 5, 6, 4, 5]
    cfg = GenerationConfig(max_new_tokens=6, greedy=False, top_p=0.9, seed=31, vocab_hi=HI, pad_id=PAD, logprobs=True)
    reqs = [(_text(p), lim) for p, lim in zip(prompts, limits)]
    stats = {}
    got = {i: (ids, n, lp) for i, ids, n, lp in generate_stream(model, reqs, cfg, slots=2, stats=stats, replay=False)}
    assert sorted(got) == list(range(5)) and stats["prefill_calls"] == 3
    state = model._slot_generator.state
    slot_sums = state.sum_logprob.cpu().numpy()
    for pair in ([0, 1], [2, 3], [4, 4]):
        x = _text(np.concatenate([prompts[i] for i in pair]))
        sid = [pair[0], pair[1] if pair[1] != pair[0] else 1000]
        ids, lengths, lps, sums = generate(model, x, cfg, stream_ids=sid, replay=False)
        for row, i in enumerate(pair[:1] if pair[0] == pair[1] else pair):
            lim = limits[i]
            assert tuple(got[i][2].shape) == (lim,) and got[i][2].dtype == torch.float32
            assert torch.equal(got[i][0], ids[row, :lim]), i
            assert torch.equal(got[i][2].view(torch.int32), lps[row, :lim].contiguous().view(torch.int32)), i
    # a slot's second (third) tenant does not inherit the sum: slot 0 ends with request 4's sum alone, slot 1 with request 3's
    assert slot_sums[0] == _f32_sum(got[4][2].numpy()) and slot_sums[1] == _f32_sum(got[3][2].numpy())
    # generate_many: a third list, in request order; without the flag the stream's tuples are what they were
    ids3, len3, lp3 = generate_many(model, reqs, cfg, slots=2, replay=False)
    assert all(torch.equal(lp3[i].view(torch.int32), got[i][2].view(torch.int32)) and torch.equal(ids3[i], got[i][0]) for i in range(5))
    plain = list(generate_stream(model, reqs, dataclasses.replace(cfg, logprobs=False), slots=2, replay=False))
    assert all(len(r) == 3 for r in plain) and all(torch.equal(ids, got[i][0]) for i, ids, _ in plain)


def test_sample_best_of_ranks_the_rows_generate_samples(bf16):
    from bdm_db1_amd import GenerationConfig, generate, sample_best_of
    model, G, n, Rn, mx = bf16, 2, 4, 2, 8
    p = np.random.default_rng(15).integers(0, HI, (G, 6))
    gc = GenerationConfig(max_new_tokens=mx, greedy=False, top_p=0.9, seed=17, vocab_hi=HI, pad_id=PAD)
    free = generate(model, _text(np.repeat(p, n, 0)), gc)[0].numpy()
    eos = int(free[1, 2])                                                  # (so that at least one row ends early)
    gc = dataclasses.replace(gc, eos_id=eos)
    ids, lengths, lps, sums = generate(model, _text(np.repeat(p, n, 0)), dataclasses.replace(gc, logprobs=True), stream_ids=list(range(G * n)))
    ids, lengths, sums = ids.numpy().reshape(G, n, mx), lengths.numpy().reshape(G, n), sums.numpy().reshape(G, n)
    assert (lengths < mx).any()
    for pen in (1.0, 0.0):
        stats, prompts_run = {}, []       # every model call that carries more than one position is a prefill: (rows, positions)
        hook = model.register_forward_pre_hook(
            lambda m, a: prompts_run.append(tuple(a[0][0].text_seq.shape)) if a[0][0].text_seq.shape[1] > 1 else None)
        try:
            b_ids, b_len, b_sc = sample_best_of(model, _text(p), gc, n, length_penalty=pen, num_return_sequences=Rn, stats=stats)
        finally:
            hook.remove()
        assert prompts_run == [(G, 6)]                                     # ONE prefill of the G prompts, not n of them and not G * n rows
        assert tuple(b_ids.shape) == (G, Rn, mx) and tuple(b_len.shape) == (G, Rn) and tuple(b_sc.shape) == (G, Rn)
        assert b_ids.dtype == torch.int32 and b_len.dtype == torch.int32 and b_sc.dtype == torch.float32
        assert stats["path"] == "ring" and stats["token_calls"] <= mx - 1   # then one call per token for all G * n rows
        want = L.best_of_scores(sums, lengths, lengths < mx, np.zeros((G, n), bool), pen)
        order = L.best_of_order(want.astype(np.float32), Rn)
        for g in range(G):
            for r, j in enumerate(order[g]):
                assert np.array_equal(b_ids[g, r].numpy(), ids[g, j]) and int(b_len[g, r]) == lengths[g, j], (g, r, j)
                assert abs(float(b_sc[g, r]) - want[g, j]) <= 1e-6 * abs(want[g, j]), (g, r)
            assert float(b_sc[g, 0]) >= float(b_sc[g, 1])
    given = sample_best_of(model, _text(p), gc, n, num_return_sequences=n, stream_ids=np.arange(G * n).reshape(G, n) + 500)
    assert not torch.equal(given[0][:, :Rn], b_ids) or not torch.equal(given[2][:, :Rn], b_sc)      # other streams, other draws
    with pytest.raises(ValueError):
        sample_best_of(model, _text(p), gc, n, stream_ids=np.arange(G * n))
