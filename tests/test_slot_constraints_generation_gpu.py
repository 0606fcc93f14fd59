"""Per-request decoding constraints in a stream, end to end on the 2-layer bf16 model, the eight text prompts, 3 slots and sync_every=2 of
tests/test_serving_gpu.py.  The flag alone changes nothing; every request carrying one object equals the stream-level form of that object;
a mixed stream equals a host-driven stream in which the two per-slot launches are replaced by the NumPy rule
(tests/slot_constraints_rule.py); a neighbour's constraints touch nobody else; a slot's next tenant inherits nothing; the flag works with
``per_request=True``; the caption and VQA wrappers forward the fourth element."""
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
import slot_constraints_rule as Q  # noqa: E402
from gpu_common import DEV, _bf16_model, _need_gpu, _prompt, _tdev  # noqa: E402,F401

HI, PAD, SLOTS = 32000, 31999, 3
LO, WIN = 500, 540                       # a window of 40 tokens: rows repeat themselves, so penalties and n-gram bans move them
LENS = [5, 9, 5, 70, 9, 5, 12, 9]
LIMITS = [4, 16, 4, 6, 16, 4, 4, 8]
ON = dict(per_request_constraints=True, max_bad_token_ids=32, max_logit_bias=4)


def _text(ids):
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(np.asarray(ids, np.int64)), text_len=None)


@pytest.fixture(scope="module")
def model():
    return _bf16_model(mem_len=100)[1]


@pytest.fixture(scope="module")
def prompts():
    rng = np.random.default_rng(21)
    return [_text(rng.integers(0, HI, (1, n))) for n in LENS]


def _cfg(**kw):
    from bdm_db1_amd import GenerationConfig
    kw = {**dict(max_new_tokens=16, greedy=False, top_p=0.9, seed=4321, vocab_lo=LO, vocab_hi=WIN, pad_id=PAD, sync_every=2, logprobs=True), **kw}
    return GenerationConfig(**kw)


def _run(model, reqs, cfg, **kw):
    from bdm_db1_amd import generate_many
    stats = {}
    out = generate_many(model, reqs, cfg, slots=SLOTS, stats=stats, **kw)
    return [[t.numpy() if torch.is_tensor(t) else t for t in col] for col in out], stats


def _equal(a, b, only=None):
    """ids, lengths and (when there) log-probs bit for bit, request by request"""
    assert len(a) == len(b)
    for col_a, col_b in zip(a, b):
        assert len(col_a) == len(col_b)
        for i, (x, y) in enumerate(zip(col_a, col_b)):
            if only is not None and i not in only:
                continue
            if isinstance(x, np.ndarray):
                x, y = (x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else (x, y)
                assert x.shape == y.shape and (x == y).all(), (i, x, y)
            else:
                assert x == y, (i, x, y)


@pytest.fixture(scope="module")
def base(model, prompts):
    """the fully unconstrained stream, flag off"""
    return _run(model, list(zip(prompts, LIMITS)), _cfg())


def test_the_flag_alone_changes_nothing(model, prompts, base):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd.generation import DecodeKey
    reqs = list(zip(prompts, LIMITS))
    on, s_on = _run(model, reqs, _cfg(), **ON)
    _equal(on, base[0])
    assert "stopped" not in base[1] and s_on["stopped"] == 0 and set(s_on) == set(base[1]) | {"stopped"}
    assert model._slot_generator.key == DecodeKey(rows=SLOTS, cfg=_cfg(), V=model.total_vocab_size, hi=WIN, constraints=None, n=None,
                                                  per_request=False, caps=(32, 4))
    # ... and with a stream-level object every request runs under
    C = D(repetition_penalty=1.2, no_repeat_ngram_size=2, frequency_penalty=0.3, logit_bias={int(base[0][0][1][0]): -3.0})
    off_c, _ = _run(model, reqs, _cfg(), constraints=C)
    on_c, _ = _run(model, reqs, _cfg(), constraints=C, **ON)
    _equal(on_c, off_c)
    assert any((a != b).any() for a, b in zip(off_c[0], base[0][0]))
    # the four-tuple form with nothing in it is the same request
    on4, _ = _run(model, [(p, lim, None, None) for p, lim in reqs], _cfg(), constraints=C, **ON)
    _equal(on4, off_c)


def test_every_request_carrying_one_object_equals_the_stream_level_form(model, prompts):
    from bdm_db1_amd import DecodingConstraints as D
    import dataclasses
    reqs = list(zip(prompts, LIMITS))
    C0 = D(repetition_penalty=1.2, no_repeat_ngram_size=3, presence_penalty=0.4, bad_token_ids=(LO + 1, LO + 2))
    ids0 = _run(model, reqs, _cfg(), constraints=C0)[0][0]
    C = dataclasses.replace(C0, stop_sequences=((int(ids0[1][5]),), (int(ids0[4][2]), int(ids0[4][3]))))     # (stops edit no logit: both hit)
    off, s_off = _run(model, reqs, _cfg(), constraints=C)
    on, s_on = _run(model, [(p, lim, None, C) for p, lim in reqs], _cfg(), **ON)
    _equal(on, off)
    assert s_on["stopped"] == s_off["stopped"] >= 2 and off[1][1] <= 5 and off[1][4] <= 2
    # the stream's own object is replaced as a whole by a request's
    on2, _ = _run(model, [(p, lim, None, C) for p, lim in reqs], _cfg(), constraints=D(bad_token_ids=tuple(range(LO, LO + 30))), **ON)
    _equal(on2, off)


def _host_slot_state():
    """``_SlotState`` with the two per-slot launches replaced by the NumPy rule on the host"""
    from bdm_db1_amd import serving

    class HostSlotState(serving._SlotState):
        cache = "_host_slot_generator"

        def constrain(self, logits2d, row_map=None):
            if torch.cuda.is_current_stream_capturing():      # (the generator's graph is captured but never replayed in a host-driven run)
                return
            assert self.tables is not None
            bits = logits2d.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            n = lambda x: x.cpu().numpy()
            lg, fin, st = Q.constrain(bits, n(self.out), n(self.t), n(self.finished), n(self.status), n(self.cons_rec), n(self.bad),
                                      n(self.bias_ids), n(self.bias_val), V=self.V, dtype=P.BF16, eos_id=self.eos,
                                      row_map=None if row_map is None else n(row_map))
            logits2d.copy_(torch.from_numpy(lg.view(np.int16)).to(DEV).view(torch.bfloat16))
            self.finished.copy_(torch.from_numpy(fin))
            self.status.copy_(torch.from_numpy(st))

        def stop_match(self, next_ids, row_map=None):
            if torch.cuda.is_current_stream_capturing():
                return
            dev = dict(lengths=self.lengths, checked=self.checked, finished=self.finished, stop_hit=self.stop_hit, out=self.out, next_ids=next_ids)
            if self.logprob is not None:
                dev.update(logprob=self.logprob, sum_logprob=self.sum_logprob)
            if self.top_ids is not None:
                dev.update(top_ids=self.top_ids, top_logprob=self.top_logprob)
            new = Q.stop({k: v.cpu().numpy() for k, v in dev.items()}, self.stop_tok.cpu().numpy(), self.stop_len.cpu().numpy(), int(self.cfg.pad_id),
                         None if row_map is None else row_map.cpu().numpy())
            for k, v in dev.items():
                v.copy_(torch.from_numpy(new[k]))

    return HostSlotState


def test_a_mixed_stream_equals_a_host_driven_stream_under_the_rule(model, prompts, base, monkeypatch):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import serving
    b_ids = base[0][0]
    E = int(b_ids[6][1])                                     # an EOS that request 6 would choose as its second token
    cfg = _cfg(eos_id=E, top_logprobs=2)
    reqs = list(zip(prompts, LIMITS))
    e_ids, e_len = _run(model, reqs, cfg)[0][:2]             # the unconstrained stream under that EOS, flag off
    assert e_len[6] <= 1
    n4 = int(e_len[4])
    stop4 = (int(e_ids[4][max(0, min(3, n4 - 1))]),) if n4 else (E,)
    bad1 = tuple(int(v) for v in e_ids[1][:2] if v not in (E, PAD)) or (LO,)
    cons = [None, D(no_repeat_ngram_size=2, bad_token_ids=bad1), None,
            D(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.25, logit_bias={int(e_ids[3][0]): -4.0, LO + 3: 2.0, HI + 7: 1.0}),
            D(stop_sequences=((LO - 1, LO - 2), stop4)), None, D(min_new_tokens=3),
            D(repetition_penalty=1.1, presence_penalty=-0.3, logit_bias={LO + 5: 1.0}, stop_sequences=((int(e_ids[7][1]),),), bad_token_ids=(LO + 6,))]
    mixed = [(p, lim, None, c) for (p, lim), c in zip(reqs, cons)]
    got, stats = _run(model, mixed, cfg, **ON)
    monkeypatch.setattr(serving, "_SlotState", _host_slot_state())
    want, h_stats = _run(model, mixed, cfg, replay=False, **ON)
    monkeypatch.undo()
    model._host_slot_generator = None
    _equal(got, want)
    assert stats["stopped"] == h_stats["stopped"] >= int(n4 > 0)
    ids, lens = got[0], got[1]
    assert lens[6] >= 3 and not np.isin(ids[1][:lens[1]], bad1).any() and not (ids[7][:lens[7]] == LO + 6).any()
    if n4:
        assert lens[4] <= 3 and (ids[4][:lens[4]] == e_ids[4][:lens[4]]).all()
    _equal(got[:2], [e_ids, e_len], only=(0, 2, 5))             # (the requests without constraints: what they are without the flag)


def test_a_neighbours_constraints_touch_nobody_else_and_a_slot_keeps_nothing_of_its_last_tenant(model, prompts, base):
    from bdm_db1_amd import DecodingConstraints as D
    reqs = list(zip(prompts, LIMITS))
    cfg = _cfg()                                              # no EOS and no stop sequence below: the schedule is the base stream's
    heavy = D(repetition_penalty=1.5, no_repeat_ngram_size=2, frequency_penalty=1.0, bad_token_ids=tuple(range(LO, LO + 30)),
              logit_bias={LO + 31: 5.0, LO + 32: -5.0, LO + 33: 2.0, LO + 34: 1.0})
    light = D(bad_token_ids=(int(base[0][0][6][0]),))
    cons = [heavy, heavy, heavy, None, light, None, light, None]       # 3 slots: requests 3 .. 7 each follow a tenant with other lists
    got, _ = _run(model, [(p, lim, None, c) for (p, lim), c in zip(reqs, cons)], cfg, **ON)
    _equal(got, base[0], only=(3, 5, 7))
    for i in (0, 1, 2):
        assert not np.isin(got[0][i], range(LO, LO + 30)).any() and (got[0][i] != base[0][0][i]).any()
    # the light requests: exactly what they are in a stream of their own that never saw the heavy lists
    alone, _ = _run(model, [(p, lim, None, c) for (p, lim), c in zip(reqs, [None] * 4 + [light, None, light, None])], cfg, **ON)
    _equal(got, alone, only=(4, 6))
    assert got[0][6][0] != base[0][0][6][0]
    # and with a stream-level object: requests without their own run under it, the others under theirs alone
    got2, _ = _run(model, [(p, lim, None, c) for (p, lim), c in zip(reqs, [None, light] * 4)], cfg, constraints=heavy, **ON)
    under, _ = _run(model, reqs, cfg, constraints=heavy)
    _equal(got2, under, only=(0, 2, 4, 6))
    only_light, _ = _run(model, reqs, cfg, constraints=light)
    _equal(got2, only_light, only=(1, 3, 5, 7))


def test_the_flag_works_together_with_per_request_sampling(model, prompts):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd.generation import DecodeKey
    from bdm_db1_amd import SamplingParams as SP
    reqs = list(zip(prompts, LIMITS))
    cfg = _cfg()
    C = D(repetition_penalty=1.2, no_repeat_ngram_size=2, logit_bias={LO + 3: 1.5}, bad_token_ids=(LO + 9,))
    sps = [None, SP(greedy=True), SP(temperature=0.7, top_k=5), None, SP(seed=99, top_p=0.5), SP(greedy=True, vocab_lo=LO + 10, vocab_hi=WIN - 5), None,
           SP(temperature=1.5)]
    both, _ = _run(model, [(p, lim, sp, C) for (p, lim), sp in zip(reqs, sps)], cfg, per_request=True, **ON)
    assert model._slot_generator.key == DecodeKey(rows=SLOTS, cfg=cfg, V=model.total_vocab_size, hi=WIN, constraints=None, n=None,
                                                  per_request=True, caps=(32, 4))
    want, _ = _run(model, [(p, lim, sp) for (p, lim), sp in zip(reqs, sps)], cfg, per_request=True, constraints=C)
    _equal(both, want)
    # constraints per request and params per request, both differing from request to request
    half, _ = _run(model, [(p, lim, sp, C if i % 2 else None) for i, ((p, lim), sp) in enumerate(zip(reqs, sps))], cfg, per_request=True, **ON)
    plain, _ = _run(model, [(p, lim, sp) for (p, lim), sp in zip(reqs, sps)], cfg, per_request=True)
    _equal(half, want, only=(1, 3, 5, 7))
    _equal(half, plain, only=(0, 2, 4, 6))


def test_the_caption_and_vqa_wrappers_forward_the_fourth_element(model):
    from bdm_db1_amd import DecodingConstraints as D
    from bdm_db1_amd import GenerationConfig, answer_stream, caption_stream
    rng = np.random.default_rng(31)
    ic, _ = _prompt(rng, "ic", 2, HI)
    vqa, _ = _prompt(rng, "vqa", 2, HI)
    gc = GenerationConfig(max_new_tokens=8, greedy=False, seed=11, vocab_lo=LO, vocab_hi=WIN, pad_id=PAD, sync_every=2)
    for fn, batch in ((caption_stream, ic), (answer_stream, vqa)):
        base = {i: t.numpy() for i, t, _ in fn(model, [batch], gc, slots=2)}
        C = D(bad_token_ids=(int(base[0][0]), int(base[1][0])), repetition_penalty=1.2)
        want = {i: (t.numpy(), k) for i, t, k in fn(model, [batch], gc, slots=2, constraints=C)}
        got = {i: (t.numpy(), k) for i, t, k in fn(model, [(batch, None, None, C)], gc, slots=2, per_request_constraints=True)}
        for i in range(2):
            assert (got[i][0] == want[i][0]).all() and got[i][1] == want[i][1], (fn.__name__, i)
            assert got[i][0][0] != base[i][0]
        with pytest.raises(ValueError, match="per_request_constraints"):
            list(fn(model, [(batch, None, None, C)], gc, slots=2))

