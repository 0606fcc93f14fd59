"""Penalties, bias and stop sequences end to end.  Stop sequences alone edit no logit, so a run under them is DETERMINED by the unconstrained
run: tests/stop_rule.py applied token by token to that run's rows gives the ids, lengths and hits exactly -- checked for ``generate`` on the
ring path, with ``replay=False`` and on the fp32 eager path, for a stream over fewer slots than requests, and through the task helpers.
Penalties and bias: a host-driven loop over the same ring -- the step's logits brought to the host, edited by tests/penalty_rule.py and
written back before the selection -- must pick the same tokens as the device's own launch, for ``generate``, a stream and ``beam_search``.
With every new field at its default nothing changes: the cached generator, the keys of ``stats``, the tensors."""
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

import penalty_rule as P  # noqa: E402
import stop_rule as S  # noqa: E402
from gpu_common import DEV, _bf16_model, _fp32_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401

HI, PAD = 32000, 31999


@pytest.fixture(scope="module")
def model():
    return _bf16_model()[1]


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


def _fresh_pair(row, lo=2, strict=True):
    """the first j >= lo where neither row[j] nor row[j + 1] occurs earlier in the row: the pair first ends at token j + 2.  A row without one
    (a greedy row that settled on one token): the middle, unless ``strict``"""
    row = [int(v) for v in row]
    for j in range(lo, len(row) - 1):
        if row[j] not in row[:j] and row[j + 1] not in row[:j + 1]:
            return j
    if strict:
        pytest.fail(f"no fresh pair of tokens in {row}")
    return len(row) // 2


def _bits(x):
    return x.numpy().view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------------- stop sequences
def _check_generate_under_stops(model, x, gc, **path):
    from bdm_db1_amd import DecodingConstraints, generate
    base = generate(model, x, gc, **path)
    b_ids, b_len = base[0].numpy(), base[1].numpy()
    M, n = b_ids.shape
    j = _fresh_pair(b_ids[0], strict=False)
    stops = [tuple(int(v) for v in b_ids[0, j:j + 2]), (int(b_ids[1, n // 2]),)]
    stats = {}
    got = generate(model, x, gc, stats=stats, constraints=DecodingConstraints(stop_sequences=stops), **path)
    ids, lengths = got[0].numpy(), got[1].numpy()
    want = [S.replay_row(b_ids[r], b_len[r], stops, gc.pad_id) for r in range(M)]
    for r in range(M):
        assert (ids[r] == want[r][0]).all() and lengths[r] == want[r][1], (r, ids[r], want[r], b_ids[r])
    assert stats["stop_hits"] == [w[2] for w in want]
    assert want[0][1] <= j and want[0][2] >= 1 and want[1][2] >= 1 and want[1][1] <= n // 2       # (rows 0 and 1 do stop, mid-way at the latest)
    if gc.logprobs:
        lp, sm, tid, tlp = got[2:]
        for r in range(M):
            m = int(lengths[r])
            hit = want[r][2] > 0
            end = m if hit else n
            assert (_bits(lp)[r, :end] == _bits(base[2])[r, :end]).all() and (tid.numpy()[r, :end] == base[4].numpy()[r, :end]).all()
            assert (_bits(tlp)[r, :end] == _bits(base[5])[r, :end]).all()
            if hit:      # the removed positions, and everything after them
                assert (lp.numpy()[r, m:] == 0).all() and (tid.numpy()[r, m:] == -1).all() and np.isneginf(tlp.numpy()[r, m:]).all()
                assert _bits(sm)[r] == S.seq_sum(base[2].numpy()[r, :m]).view(np.uint32)
            else:
                assert _bits(sm)[r] == _bits(base[3])[r]
    return stats


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("path", ["replay", "eager_ring"])
def test_generate_under_stop_sequences_is_the_rule_applied_to_the_unconstrained_run(model, path, greedy):
    from bdm_db1_amd import GenerationConfig
    gc = GenerationConfig(max_new_tokens=16, greedy=greedy, top_p=0.9, seed=77, vocab_hi=HI, pad_id=PAD, sync_every=4, logprobs=True, top_logprobs=3)
    x = _text(np.random.default_rng(2).integers(0, HI, (3, 6)))
    stats = _check_generate_under_stops(model, x, gc, **({} if path == "replay" else dict(replay=False)))
    assert stats["path"] == "ring"


def test_generate_under_stop_sequences_on_the_fp32_eager_path():
    from bdm_db1_amd import GenerationConfig
    cfg, model, _ = _fp32_model()
    hi = cfg["text_vocab_size"]
    x, _ = _prompt(np.random.default_rng(1), "nlp", 3, hi)
    gc = GenerationConfig(max_new_tokens=12, greedy=False, seed=5, vocab_hi=hi, pad_id=hi - 1, logprobs=True, top_logprobs=3)
    stats = _check_generate_under_stops(model, x, gc)
    assert stats["path"] == "eager"


def test_stream_under_stop_sequences_over_fewer_slots_than_requests(model):
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate_many
    rng = np.random.default_rng(21)
    n = 12
    prompts = [_text(rng.integers(0, HI, (1, k))) for k in (5, 6, 7, 8, 9)]       # five shapes: every request is prefilled alone in both runs
    gc = GenerationConfig(max_new_tokens=n, greedy=False, top_p=0.9, seed=3, vocab_hi=HI, pad_id=PAD, sync_every=2, logprobs=True, top_logprobs=3)
    s0 = {}
    base = generate_many(model, prompts, gc, slots=2, stats=s0)
    assert "stopped" not in s0
    b_ids = [t.numpy() for t in base[0]]
    j = _fresh_pair(b_ids[0])
    stops = [tuple(int(v) for v in b_ids[0][j:j + 2]), (int(b_ids[1][6]),)]
    limits = [j + 2, n, n, n, n]                   # request 0's match completes exactly on its last allowed token
    reqs = [(p, lim) for p, lim in zip(prompts, limits)]
    stats = {}
    ids, lengths, lp, tid, tlp = generate_many(model, reqs, gc, slots=2, stats=stats, constraints=DecodingConstraints(stop_sequences=stops))
    want = [S.replay_row(b_ids[i][:limits[i]], min(int(base[1][i]), limits[i]), stops, PAD) for i in range(5)]
    assert want[0][1:] == (j, 1) and want[1][2] >= 1
    for i in range(5):
        m = int(lengths[i])
        assert ids[i].shape == (limits[i],) and (ids[i].numpy() == want[i][0]).all() and m == want[i][1], (i, ids[i], want[i])
        end = m if want[i][2] else limits[i]
        assert (_bits(lp[i])[:end] == _bits(base[2][i])[:end]).all() and (tid[i].numpy()[:end] == base[3][i].numpy()[:end]).all()
        assert (_bits(tlp[i])[:end] == _bits(base[4][i])[:end]).all()
        if want[i][2]:
            assert (lp[i].numpy()[m:] == 0).all() and (tid[i].numpy()[m:] == -1).all() and np.isneginf(tlp[i].numpy()[m:]).all()
    assert stats["stopped"] == sum(w[2] > 0 for w in want) and stats["admitted"] == 5
    assert set(stats) == set(s0) | {"stopped"}


def test_the_task_helpers_forward_stop_sequences_and_beams_refuse_them(model):
    from bdm_db1_amd import (BeamSearchConfig, DecodingConstraints, GenerationConfig, answer_questions, answer_stream, beam_search, caption_stream,
                             generate_captions, sample_best_of)
    rng = np.random.default_rng(31)
    ic, _ = _prompt(rng, "ic", 2, HI)
    vqa, _ = _prompt(rng, "vqa", 2, HI)
    gc = GenerationConfig(max_new_tokens=8, greedy=False, seed=11, pad_id=PAD, sync_every=2)
    for fn, batch in ((generate_captions, ic), (answer_questions, vqa)):
        b_ids, b_len = (a.numpy() for a in fn(model, batch, gc))
        stops = [(int(b_ids[0, 3]),), (int(b_ids[1, 4]), int(b_ids[1, 5]))]
        ids, lengths = fn(model, batch, gc, constraints=DecodingConstraints(stop_sequences=stops))
        for r in range(2):
            w = S.replay_row(b_ids[r], b_len[r], stops, PAD)
            assert (ids.numpy()[r] == w[0]).all() and int(lengths[r]) == w[1] and w[2] > 0, (fn.__name__, r)
    for fn, batch in ((caption_stream, ic), (answer_stream, vqa)):
        base = {i: t.numpy() for i, t, _ in fn(model, [batch], gc, slots=2)}
        stops = [(int(base[0][3]),), (int(base[1][4]), int(base[1][5]))]
        got = {i: (t.numpy(), k) for i, t, k in fn(model, [batch], gc, slots=2, constraints=DecodingConstraints(stop_sequences=stops))}
        for i in range(2):
            w = S.replay_row(base[i], 8, stops, PAD)
            assert (got[i][0] == w[0]).all() and got[i][1] == w[1] and w[2] > 0, (fn.__name__, i)
    x = _text(rng.integers(0, HI, (2, 6)))
    cons = DecodingConstraints(stop_sequences=[(5,)])
    with pytest.raises(ValueError, match="stop_sequences"):
        beam_search(model, x, BeamSearchConfig(num_beams=2, max_new_tokens=4, vocab_hi=HI), constraints=cons)
    with pytest.raises(ValueError, match="stop_sequences"):
        sample_best_of(model, x, GenerationConfig(max_new_tokens=4, greedy=False, vocab_hi=HI), 2, constraints=cons)


# ---------------------------------------------------------------------------------------------------------------------- penalties and bias
def _host_apply(logits2d, hist, t, finished, row_map, V, rule):
    """the rule on the host, in place on the step's bf16 logits: what the device launch does"""
    if torch.cuda.is_current_stream_capturing():      # (the generator's graph is captured but never replayed in a host-driven run)
        return
    bits = logits2d.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    tt = t.cpu().numpy()
    e = P.apply(bits, hist.cpu().numpy(), int(tt[0]) if tt.size == 1 else tt, V=V, dtype=P.BF16,
                finished=None if finished is None else finished.cpu().numpy(), row_map=None if row_map is None else row_map.cpu().numpy(), **rule)
    logits2d.copy_(torch.from_numpy(e.view(np.int16)).to(DEV).view(torch.bfloat16))


def _rule_kw(cons):
    return dict(theta=cons.repetition_penalty, ngram=cons.no_repeat_ngram_size, bad=cons.bad_token_ids, freq=cons.frequency_penalty,
                pres=cons.presence_penalty, bias=cons.logit_bias)


def _host_states(rule):
    from bdm_db1_amd import generation as G, serving

    class HostState(G._State):
        cache = "_host_generator"

        def epilogue(self, logits2d, next_ids, ring=None):
            _host_apply(logits2d, self.out, self.t, self.finished, None, self.V, rule)
            super().epilogue(logits2d, next_ids, ring)

    class HostBeamState(G._BeamState):
        cache = "_host_beam_generator"

        def select(self, logits2d, next_ids):
            _host_apply(logits2d, self.tokens, self.t, None, None, self.V, rule)
            super().select(logits2d, next_ids)

    class HostSlotState(serving._SlotState):
        cache = "_host_slot_generator"

        def select(self, logits2d, next_ids, row_map=None):
            _host_apply(logits2d, self.out, self.t, self.finished, row_map, self.V, rule)
            super().select(logits2d, next_ids, row_map)

    return HostState, HostBeamState, HostSlotState


def _cons_from(base_ids):
    """constraints that move this run: the tokens it picks most get penalised, its first tokens get a negative bias, one a positive one"""
    from bdm_db1_amd import DecodingConstraints
    flat = [int(v) for v in np.asarray(base_ids).reshape(-1)]
    bias = {flat[0]: -4.0, flat[1]: -2.5, flat[-1]: 1.5, HI + 7: 3.0, 123: 0.75}
    return DecodingConstraints(repetition_penalty=1.1, frequency_penalty=0.6, presence_penalty=0.4, logit_bias=bias, bad_token_ids=(flat[2],))


def test_generate_equals_a_host_driven_loop_under_the_rule(model):
    from bdm_db1_amd import GenerationConfig, generate
    from bdm_db1_amd import generation as G
    x = _text(np.random.default_rng(2).integers(0, HI, (3, 6)))
    gc = GenerationConfig(max_new_tokens=14, vocab_lo=500, vocab_hi=540, pad_id=PAD)
    base = generate(model, x, gc)[0].numpy()
    cons = _cons_from(base)
    stats = {}
    ids, lengths = generate(model, x, gc, stats=stats, constraints=cons)
    assert stats["path"] == "ring" and "frequency_penalty" in model._generator.state.con and "stop_hits" not in stats
    e_ids, _ = generate(model, x, gc, replay=False, constraints=cons)
    HostState = _host_states(_rule_kw(cons))[0]
    with torch.no_grad():
        h_ids, h_len = G._decode(model, x, HostState, G.DecodeKey(rows=3, cfg=gc, V=int(model.total_vocab_size), hi=540, constraints=None, n=None,
                                                                   per_request=False, caps=None), True, False, None, start=(None,))
    assert torch.equal(ids, h_ids) and torch.equal(lengths, h_len) and torch.equal(ids, e_ids)
    assert (ids.numpy() != base).any() and not np.isin(ids.numpy(), cons.bad_token_ids).any()
    model._host_generator = None


def test_stream_equals_a_host_driven_stream_under_the_rule(model, monkeypatch):
    from bdm_db1_amd import GenerationConfig, generate_many, serving
    rng = np.random.default_rng(23)
    reqs = [(_text(rng.integers(0, HI, (1, k))), lim) for k, lim in ((5, 10), (6, 4), (5, 10), (7, 7), (6, 10))]
    gc = GenerationConfig(max_new_tokens=10, vocab_lo=500, vocab_hi=540, pad_id=PAD, sync_every=2)
    base = generate_many(model, reqs, gc, slots=2)[0]
    cons = _cons_from(np.concatenate([b.numpy() for b in base]))
    ids, lengths = generate_many(model, reqs, gc, slots=2, constraints=cons)
    monkeypatch.setattr(serving, "_SlotState", _host_states(_rule_kw(cons))[2])
    h_ids, h_len = generate_many(model, reqs, gc, slots=2, replay=False)
    monkeypatch.undo()
    assert h_len == lengths and all(torch.equal(a, b) for a, b in zip(ids, h_ids))
    assert any((a.numpy() != b.numpy()).any() for a, b in zip(ids, base))
    model._host_slot_generator = None


def test_beam_search_equals_a_host_driven_search_under_the_rule(model):
    from bdm_db1_amd import BeamSearchConfig, beam_search
    from bdm_db1_amd import generation as G
    x = _text(np.random.default_rng(14).integers(0, HI, (2, 6)))
    bc = BeamSearchConfig(num_beams=3, max_new_tokens=10, num_return_sequences=3, vocab_lo=500, vocab_hi=540, pad_id=PAD)
    base = beam_search(model, x, bc)[0].numpy()
    cons = _cons_from(base[:, 0])
    stats = {}
    ids, lengths, scores = beam_search(model, x, bc, stats=stats, constraints=cons)
    assert stats["path"] == "ring"
    HostBeam = _host_states(_rule_kw(cons))[1]
    with torch.no_grad():
        h_ids, h_len, h_sc = G._decode(model, x, HostBeam, G.DecodeKey(rows=2, cfg=bc, V=int(model.total_vocab_size), hi=540, constraints=None, n=None,
                                                                        per_request=False, caps=None), True, False, None)
    assert torch.equal(ids, h_ids) and torch.equal(lengths, h_len) and (_bits(scores) == _bits(h_sc)).all()
    assert (ids.numpy() != base).any()
    model._host_beam_generator = None


# ---------------------------------------------------------------------------------------------------------------------------------- defaults
def test_defaults_change_nothing():
    from bdm_db1_amd import DecodingConstraints, GenerationConfig, generate, generate_many
    model = _bf16_model()[1]
    x = _text(np.random.default_rng(2).integers(0, HI, (3, 6)))
    gc = GenerationConfig(max_new_tokens=8, greedy=False, top_p=0.9, seed=7, vocab_hi=HI, pad_id=PAD)
    s0, t0 = {}, {}
    before = generate(model, x, gc, stats=s0)
    s_before = generate_many(model, [x], gc, slots=2, stats=t0)
    gen, sgen = model._generator, model._slot_generator
    off = DecodingConstraints(frequency_penalty=0.0, presence_penalty=0.0, logit_bias={}, stop_sequences=[])
    s1, t1 = {}, {}
    same = generate(model, x, gc, stats=s1, constraints=off)
    s_same = generate_many(model, [x], gc, slots=2, stats=t1, constraints=off)
    assert model._generator is gen and model._slot_generator is sgen          # the cached generators are reused: the key is what it was
    k = gen.key
    assert k.constraints is None and not k.per_request and k.caps is None and k.n is None
    assert gen.state.con is None and gen.state.stop is None and gen.state.checked is None and gen.state.stop_hit is None
    assert torch.equal(same[0], before[0]) and torch.equal(same[1], before[1])
    assert all(torch.equal(p, q) for p, q in zip(s_same[0], s_before[0])) and s_same[1] == s_before[1]
    assert set(s1) == set(s0) == {"path", "token_calls"} and set(t1) == set(t0) and "stopped" not in t0
    # the old fields alone still go to the old entry point, and build no stop state
    generate(model, x, gc, constraints=DecodingConstraints(repetition_penalty=1.2))
    st = model._generator.state
    assert st.con is not None and "frequency_penalty" not in st.con and "bias_ids" not in st.con and st.stop is None
    # stop sequences alone: a new key, no constrain launch, the stop state exists
    generate(model, x, gc, constraints=DecodingConstraints(stop_sequences=[(5,)]))
    st = model._generator.state
    k = model._generator.key
    assert k.constraints == DecodingConstraints(stop_sequences=[(5,)]) and not k.per_request and k.caps is None and k.n is None
    assert st.con is None and st.stop is not None and st.checked.shape == (3,)
    after = generate(model, x, gc)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
