"""The top-n alternatives end to end on the small test models: ``generate`` with ``top_logprobs`` against the same call without it (bit for
bit), graph replay against eager launches, the greedy token at the head of its alternatives, banned ids, the slot stream against lockstep
``generate`` (tenant reset included), and ``score`` with ``ScoreConfig.top_n`` against ``top_n=0`` and across chunkings."""
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

from gpu_common import DEV, _bf16_model, _need_gpu, _tdev  # noqa: E402,F401

HI, PAD, N = 32000, 31999, 4


@pytest.fixture(scope="module")
def bf16():
    return _bf16_model()[1]


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check_shape_and_order(ids, lengths, lps, top_ids, top_lp, eos=None):
    """shapes and dtypes; written positions hold n real alternatives in never increasing order, the chosen token's entry carries its log-prob
    bit for bit; the positions after a row's last written token hold -1 / -inf"""
    M, mx = ids.shape
    assert top_ids.dtype == torch.int32 and top_lp.dtype == torch.float32 and tuple(top_ids.shape) == (M, mx, N) == tuple(top_lp.shape)
    for r in range(M):
        k = min(int(lengths[r]) + (1 if eos is not None else 0), mx)
        assert (top_ids[r, :k] >= 0).all() and torch.isfinite(top_lp[r, :k]).all()
        assert (top_lp[r, :k, 1:] <= top_lp[r, :k, :-1]).all()
        assert (top_ids[r, k:] == -1).all() and torch.isneginf(top_lp[r, k:]).all()
        for t in range(k):
            hit = (top_ids[r, t] == ids[r, t]).nonzero()
            if hit.numel():
                assert _bits(top_lp)[r, t, int(hit[0])] == _bits(lps)[r, t], (r, t)


@pytest.mark.parametrize("greedy", [True, False])
def test_generate_with_top_logprobs_keeps_the_other_outputs_and_replay_equals_eager(bf16, greedy):
    from bdm_db1_amd import GenerationConfig, generate
    model, M, mx = bf16, 3, 8
    x = _text(np.random.default_rng(2).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=mx, greedy=greedy, top_p=0.9, seed=1234, vocab_hi=HI, logprobs=True)
    base = generate(model, x, gc)
    stats = {}
    got = generate(model, x, dataclasses.replace(gc, top_logprobs=N), stats=stats)
    assert stats["path"] == "ring" and len(base) == 4 and len(got) == 6
    for a, b in zip(base, got[:4]):                                                  # ids, lengths, logprobs, sum_logprob: bit for bit
        assert torch.equal(_bits(a), _bits(b))
    eager = generate(model, x, dataclasses.replace(gc, top_logprobs=N), replay=False)
    for a, b in zip(got, eager):                                                     # graphed equals eager on all six
        assert torch.equal(_bits(a), _bits(b))
    ids, lengths, lps, _, top_ids, top_lp = got
    _check_shape_and_order(ids, lengths, lps, top_ids, top_lp)
    if greedy:
        assert torch.equal(top_ids[:, :, 0], ids)
    # an EOS: written with its alternatives, -1 / -inf after it
    eos = int(ids[0, 2])
    e = generate(model, x, dataclasses.replace(gc, top_logprobs=N, eos_id=eos, pad_id=PAD))
    assert int(e[1][0]) <= 2
    _check_shape_and_order(e[0], e[1], e[2], e[4], e[5], eos=eos)
    if greedy:
        for r in range(M):
            k = min(int(e[1][r]) + 1, mx)
            assert torch.equal(e[4][r, :k, 0], e[0][r, :k])                          # the EOS included


def test_eager_list_form_path_returns_the_alternatives_too(bf16):
    from bdm_db1_amd import GenerationConfig, generate
    model, M, mx = bf16, 2, 5
    x = _text(np.random.default_rng(3).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=mx, vocab_hi=HI, logprobs=True, top_logprobs=N)
    stats = {}
    ids, lengths, lps, sums, top_ids, top_lp = generate(model, x, gc, graphed=False, stats=stats)
    assert stats["path"] == "eager"
    _check_shape_and_order(ids, lengths, lps, top_ids, top_lp)
    assert torch.equal(top_ids[:, :, 0], ids)


def test_a_banned_id_is_never_an_alternative(bf16):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate
    model, M, mx = bf16, 3, 6
    x = _text(np.random.default_rng(4).integers(0, HI, (M, 6)))
    gc = GenerationConfig(max_new_tokens=mx, vocab_hi=HI, logprobs=True, top_logprobs=N)
    free = generate(model, x, gc)[4]
    bad = tuple(sorted({int(v) for v in free[:, 0].reshape(-1)}))                   # every alternative of the first step
    top_ids = generate(model, x, gc, constraints=DecodingConstraints(bad_token_ids=bad))[4]
    assert not np.isin(top_ids.numpy(), bad).any() and (top_ids >= 0).all()


def test_stream_alternatives_equal_those_of_generate(bf16):
    """5 requests of mixed limits over 2 slots, as tests/test_logprob_generation_gpu.py runs them: the requests move in as the pairs (0, 1),
    (2, 3) and then 4 alone, and ``generate`` over the same pair runs the same prefill and the same two-row token steps.  Slot 0's third
    tenant (request 4, limit 5) follows one of limit 6, slot 1's second (request 3, limit 4) one of limit 5: what the earlier tenant wrote
    beyond the new one's tokens must be gone."""
    from bdm_db1_amd import GenerationConfig, generate, generate_many, generate_stream
    model = bf16
    rng = np.random.default_rng(12)
    prompts = [rng.integers(0, HI, (1, 6)) for _ in range(5)]
    limits = [3, 5, 6, 4, 5]
    cfg = GenerationConfig(max_new_tokens=6, greedy=False, top_p=0.9, seed=31, vocab_hi=HI, pad_id=PAD, logprobs=True, top_logprobs=N)
    reqs = [(_text(p), lim) for p, lim in zip(prompts, limits)]
    got = {r[0]: r[1:] for r in generate_stream(model, reqs, cfg, slots=2, replay=False)}
    assert sorted(got) == list(range(5)) and all(len(v) == 5 for v in got.values())
    # an EOS for the second run: request 2's second token
    eos = int(got[2][0][1])
    cfg_e = dataclasses.replace(cfg, eos_id=eos)
    got_e = {r[0]: r[1:] for r in generate_stream(model, reqs, cfg_e, slots=2, replay=False)}
    for c, g in ((cfg, got), (cfg_e, got_e)):
        for pair in ([0, 1], [2, 3], [4, 4]):
            x = _text(np.concatenate([prompts[i] for i in pair]))
            sid = [pair[0], pair[1] if pair[1] != pair[0] else 1000]
            ids, lengths, lps, sums, top_ids, top_lp = generate(model, x, c, stream_ids=sid, replay=False)
            for row, i in enumerate(pair[:1] if pair[0] == pair[1] else pair):
                lim = limits[i]
                s_ids, s_len, s_lp, s_ti, s_tl = g[i]
                assert tuple(s_ti.shape) == (lim, N) == tuple(s_tl.shape) and s_ti.dtype == torch.int32 and s_tl.dtype == torch.float32
                assert torch.equal(s_ids, ids[row, :lim]) and int(s_len) == min(int(lengths[row]), lim), i
                assert torch.equal(s_ti, top_ids[row, :lim]), i                      # written positions and -1 / -inf tails alike
                assert torch.equal(_bits(s_tl), _bits(top_lp[row, :lim])), i
    assert any((v[3] == -1).any() for v in got_e.values())                           # (the EOS run has tails to compare)
    many = generate_many(model, reqs, cfg, slots=2, replay=False)
    assert len(many) == 5 and all(torch.equal(many[3][i], got[i][3]) and torch.equal(_bits(many[4][i]), _bits(got[i][4])) for i in range(5))
    plain = list(generate_stream(model, reqs, dataclasses.replace(cfg, top_logprobs=0), slots=2, replay=False))
    assert all(len(r) == 4 for r in plain)


def test_score_with_top_n_keeps_the_other_fields_and_any_chunking(bf16):
    from bdm_db1_amd.scoring import ScoreConfig, score
    model = bf16
    rng = np.random.default_rng(21)
    from bdm_db1_amd.data import NLPTaskInput
    B, Lq = 3, 10
    seq = rng.integers(0, HI, (B, Lq))
    mask = np.ones((B, Lq), np.float32)
    mask[:, -1] = 0

    def task(label):
        return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=_tdev(mask), label=_tdev(label.astype(np.int64)), text_seq=_tdev(seq),
                            text_len=None)

    # labels the model ranks first, second, ... (so that labels are among the alternatives), one ignored, one far down
    pre = score(model, [task(np.roll(seq, -1, 1))], ScoreConfig(vocab_hi=HI, top_n=N))
    label = np.take_along_axis(pre.top_ids[0], (np.arange(B * Lq).reshape(B, Lq, 1) % N), 2)[..., 0].astype(np.int64)
    label[0, 4] = -100                                                               # an ignored position still gets its alternatives
    label[1, 2] = seq[1, 3]
    x = task(label)
    base = score(model, [x], ScoreConfig(vocab_hi=HI))
    base1 = score(model, [x], ScoreConfig(vocab_hi=HI, chunk_rows=1))
    got = score(model, [x], ScoreConfig(vocab_hi=HI, top_n=N))
    one = score(model, [x], ScoreConfig(vocab_hi=HI, top_n=N, chunk_rows=1))
    assert base.top_ids is None and base.top_logprob is None
    for r, b in ((got, base), (one, base1)):                                         # the same sweep with and without the alternatives
        assert r.loss == b.loss and r.status == b.status
        for name in ("sum_logprob", "tokens", "hits"):
            assert np.array_equal(getattr(r, name).view(np.int32), getattr(b, name).view(np.int32)), name
        for name in ("logprob", "top1", "rank"):
            assert np.array_equal(getattr(r, name)[0].view(np.int32), getattr(b, name)[0].view(np.int32)), name
        assert r.top_ids[0].shape == (B, Lq, N) == r.top_logprob[0].shape and r.top_ids[0].dtype == np.int32
        assert np.array_equal(r.top_ids[0][..., 0], r.top1[0])
        assert (r.top_ids[0] >= 0).all() and (r.top_ids[0] < HI).all() and (r.top_logprob[0][..., 1:] <= r.top_logprob[0][..., :-1]).all()
        # a label among the alternatives carries the bits of its log-prob, and sits at its rank
        hit = r.top_ids[0] == label[..., None]
        assert hit.sum() >= B * Lq - 3
        assert np.array_equal(r.top_logprob[0].view(np.int32)[hit], np.broadcast_to(r.logprob[0].view(np.int32)[..., None], hit.shape)[hit])
    assert np.array_equal(got.top_ids[0][0, 4], pre.top_ids[0][0, 4])                # (the ignored position: the label plays no part)
    # one row of logits at a time equals the default chunking
    diff = np.abs(one.top_logprob[0] - got.top_logprob[0]).max()
    print(f"chunk_rows=1 vs default: ids differ at {(one.top_ids[0] != got.top_ids[0]).sum()} places, max |top_logprob diff| = {diff:.3e}")
    assert np.array_equal(one.top_ids[0], got.top_ids[0]) and np.array_equal(one.top_logprob[0].view(np.int32), got.top_logprob[0].view(np.int32))
    assert score(model, [x], ScoreConfig(vocab_hi=HI, top_n=N, return_tokens=False)).top_ids is None
