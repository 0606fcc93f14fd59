"""The host side of continuous batching (bdm_db1_amd.serving) without a GPU: SlotScheduler driven by a fake step that feeds it scripted
``finished`` vectors, the request numbering, the regrouping of rows into one prefill batch, and question_prompts on a ragged VQA batch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch = pytest.importorskip("torch")

from bdm_db1_amd import GenerationConfig, SlotScheduler, question_prompts  # noqa: E402
from bdm_db1_amd import serving  # noqa: E402
from bdm_db1_amd.data import NLPTaskInput, VQATaskInput  # noqa: E402


def _text(ids):
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.as_tensor(np.asarray(ids)), text_len=None)


class _FakeStep:
    """what the device does to ``finished``: a slot ends when its request has ``limit`` tokens, or earlier where ``eos_at`` says so"""

    def __init__(self, slots, eos_at=None):
        self.t, self.limit, self.finished = [0] * slots, [1] * slots, [1] * slots
        self.eos_at = eos_at or {}
        self.index = [None] * slots

    def occupy(self, slot, req):
        assert self.finished[slot] == 1, "a live slot was handed out again"
        self.t[slot], self.limit[slot], self.finished[slot], self.index[slot] = 0, req.limit, 0, req.index
        self._pick(slot)        # (token 0, from the prefill)

    def _pick(self, slot):
        if self.finished[slot]:
            return
        self.t[slot] += 1
        if self.t[slot] == self.limit[slot] or self.eos_at.get(self.index[slot]) == self.t[slot] - 1:
            self.finished[slot] = 1

    def replay(self):
        for s in range(len(self.t)):
            self._pick(s)


def _drive(slots, reqs, every, eos_at=None):
    sched, step = SlotScheduler(slots, iter(reqs)), _FakeStep(slots, eos_at)
    order, groups_seen, replays, occupied_now = [], [], 0, {}
    for _ in range(10_000):
        for key, members in sched.admit():
            groups_seen.append((key, members))
            for slot, req in members:
                assert slot not in occupied_now, "no slot is handed out twice"
                occupied_now[slot] = req.index
                step.occupy(slot, req)
        k = sched.replays_due(every)
        for _ in range(k):
            step.replay()
        sched.advance(k)
        replays += k
        if sched.idle():
            break
        done = sched.harvest(list(step.finished))
        assert [r.index for _, r in done] == sorted(r.index for _, r in done)       # (the yield order of one look)
        for slot, req in done:
            assert occupied_now.pop(slot) == req.index
            order.append(req.index)
    else:
        raise AssertionError("the loop did not end")
    return order, groups_seen, replays, sched


def _reqs(lens, limits):
    items = [(_text(np.zeros((1, n), np.int64)), lim) for n, lim in zip(lens, limits)]
    return list(serving._requests(items, GenerationConfig(max_new_tokens=max(limits))))


LENS, LIMITS = [5, 9, 5, 70, 9, 5, 12, 9], [4, 16, 4, 6, 16, 4, 4, 8]


@pytest.mark.parametrize("slots,every", [(3, 2), (1, 8), (8, 1), (5, 3)])
def test_every_request_finishes_once_and_slots_are_recycled(slots, every):
    reqs = _reqs(LENS, LIMITS)
    order, groups, replays, sched = _drive(slots, reqs, every)
    assert sorted(order) == list(range(8)) and sched.admitted == 8 and sched.idle()
    for key, members in groups:
        assert len({r.key for _, r in members}) == 1 and members[0][1].key == key          # a group shares one shape
        assert len({s for s, _ in members}) == len(members)
    # first come, first served: requests enter in order
    entered = [r.index for _, members in groups for _, r in members]
    assert sorted(entered) == list(range(8))
    assert [min(r.index for _, r in m) for _, m in groups] == sorted(min(r.index for _, r in m) for _, m in groups)
    static = sum(max(LIMITS[i:i + slots]) - 1 for i in range(0, 8, slots))
    lower = -(-sum(l - 1 for l in LIMITS) // slots)
    assert lower <= replays
    if slots == 3:
        assert replays < static       # recycling beats lockstep batches on this list


def test_grouping_by_shape_and_early_eos():
    reqs = _reqs([5, 5, 9, 5], [6, 6, 6, 6])
    order, groups, replays, _ = _drive(4, reqs, 2, eos_at={1: 2})
    assert [[r.index for _, r in m] for _, m in groups] == [[0, 1, 3], [2]]
    assert order[0] == 1 and sorted(order) == [0, 1, 2, 3]        # the request that met EOS comes back first
    assert replays == 5


def test_limit_one_requests_need_no_replay():
    order, _, replays, _ = _drive(2, _reqs([3, 3, 3], [1, 1, 1]), 4)
    assert order == [0, 1, 2] and replays == 0


def test_requests_are_numbered_and_checked():
    cfg = GenerationConfig(max_new_tokens=8)
    items = [_text(np.zeros((2, 4), np.int64)), (_text(np.zeros((3, 6), np.int64)), 5)]
    reqs = list(serving._requests(items, cfg))
    assert [r.index for r in reqs] == [0, 1, 2, 3, 4] and [r.limit for r in reqs] == [8, 8, 5, 5, 5] and [r.row for r in reqs] == [0, 1, 0, 1, 2]
    assert reqs[0].key == reqs[1].key != reqs[2].key
    with pytest.raises(ValueError):
        list(serving._requests([(items[0], 9)], cfg))
    with pytest.raises(ValueError):
        list(serving._requests([(items[0], 0)], cfg))
    with pytest.raises(ValueError):
        SlotScheduler(0, [])


def test_gather_builds_one_batch_in_slot_order():
    a = _text(np.arange(8).reshape(2, 4))
    b = _text(np.arange(100, 112).reshape(3, 4))
    reqs = list(serving._requests([a, b], GenerationConfig()))
    assert serving._gather(reqs[:2]) is a                       # a whole batch is passed through
    x = serving._gather([reqs[1], reqs[4], reqs[0]])
    assert x.text_seq.tolist() == [[4, 5, 6, 7], [108, 109, 110, 111], [0, 1, 2, 3]]


def test_only_the_per_row_fields_are_sliced():
    from bdm_db1_amd.data import ICTaskInput
    G = 2
    x = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=torch.arange(6).reshape(G, 3),
                    img_seq=torch.arange(G * 3 * 4).reshape(G, 3, 2, 2).float(), text_seq=torch.zeros(G, 0, dtype=torch.long), img_id_seq=[7, 8])
    x.vision_row_ids = torch.arange(G * 4)            # (one id per patch, image after image)
    x.vision_col_ids = torch.arange(G * 4).reshape(G, 4) + 10
    reqs = list(serving._requests([x], GenerationConfig()))
    y = serving._gather([reqs[1]])
    assert y.prompt_seq.tolist() == [[3, 4, 5]] and tuple(y.img_seq.shape) == (1, 3, 2, 2) and tuple(y.text_seq.shape) == (1, 0)
    assert y.vision_row_ids.tolist() == [4, 5, 6, 7] and y.vision_col_ids.tolist() == [14, 15, 16, 17]
    assert type(y) is ICTaskInput
    x.vision_row_ids = torch.arange(7)
    with pytest.raises(ValueError):
        serving._gather([reqs[1]])
    x.vision_row_ids = torch.arange(G * 4)
    x.prompt_seq = torch.arange(9).reshape(3, 3)      # (a per-row field of another batch size)
    with pytest.raises(ValueError):
        serving._take(x, "prompt_seq", G, [1])


def test_question_prompts_partition_a_ragged_batch():
    rng = np.random.default_rng(0)
    G, ql = 7, np.array([5, 3, 5, 8, 3, 5, 1])
    text = rng.integers(1, 1000, (G, 12))
    batch = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=torch.as_tensor(rng.integers(0, 9, (G, 3))),
                         img_seq=torch.as_tensor(rng.standard_normal((G, 3, 32, 32)).astype(np.float32)), text_seq=torch.as_tensor(text),
                         img_id_seq=None, ques_id_seq=None, ques_len=torch.as_tensor(ql))
    parts = question_prompts(batch)
    assert [int(p.text_seq.shape[1]) for p, _ in parts] == [1, 3, 5, 8]
    rows = np.concatenate([r for _, r in parts])
    assert sorted(rows.tolist()) == list(range(G))              # every row once
    for p, r in parts:
        n = p.text_seq.shape[1]
        assert (ql[r] == n).all()
        assert np.array_equal(p.text_seq.numpy(), text[r, :n])
        assert torch.equal(p.prompt_seq, batch.prompt_seq[r]) and torch.equal(p.img_seq, batch.img_seq[r])
    # round trip: scattering per-prompt results back by ``rows`` restores the batch order
    back = np.empty(G, np.int64)
    for p, r in parts:
        back[r] = ql[r]
    assert np.array_equal(back, ql)
    # the numbering answer_stream gives the requests: batch rows in their original order, batch after batch
    items = [serving._Item(p, [10 + int(i) for i in r]) for p, r in parts]
    got = sorted(q.index for q in serving._requests(items, GenerationConfig()))
    assert got == list(range(10, 10 + G))
    batch.ques_len = None
    (p, r), = question_prompts(batch)
    assert r.tolist() == list(range(G)) and p.text_seq.shape[1] == 12
    # the one-length entry points still refuse a ragged batch
    from bdm_db1_amd.generation import question_prompt
    batch.ques_len = torch.as_tensor(ql)
    with pytest.raises(ValueError):
        question_prompt(batch)


def _vqa(ques_len):
    G = 4
    x = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=torch.arange(G * 3).reshape(G, 3),
                     img_seq=torch.arange(G * 3 * 4).reshape(G, 3, 2, 2).float(), text_seq=torch.arange(100, 100 + G * 7).reshape(G, 7),
                     img_id_seq=None, ques_id_seq=None, ques_len=None if ques_len is None else torch.as_tensor(ques_len))
    x.vision_row_ids = torch.arange(G * 4)            # (one id per patch, image after image)
    x.vision_col_ids = torch.arange(G * 4) + 50
    return x


def _same_prompt(a, b):
    import dataclasses
    assert type(a) is type(b)
    for name in [f.name for f in dataclasses.fields(a)] + ["vision_row_ids", "vision_col_ids"]:
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None and v is None) or torch.equal(torch.as_tensor(u), torch.as_tensor(v)), name


def test_question_prompt_is_the_one_length_case_of_question_prompts():
    from bdm_db1_amd.generation import question_prompt
    b = _vqa([3, 3, 3, 3])
    (p, rows), = question_prompts(b)
    assert rows.tolist() == [0, 1, 2, 3] and tuple(p.text_seq.shape) == (4, 3)
    _same_prompt(p, question_prompt(b))
    assert torch.equal(p.text_seq, b.text_seq[:, :3]) and torch.equal(p.vision_col_ids, b.vision_col_ids)
    b = _vqa([3, 5, 3, 5])
    with pytest.raises(ValueError):
        question_prompt(b)
    parts = question_prompts(b)
    assert [r.tolist() for _, r in parts] == [[0, 2], [1, 3]]
    for (p, r), n in zip(parts, (3, 5)):
        assert torch.equal(p.text_seq, b.text_seq[r, :n]) and torch.equal(p.prompt_seq, b.prompt_seq[r])
        assert torch.equal(p.vision_row_ids, b.vision_row_ids.reshape(4, -1)[r].reshape(-1))
        assert torch.equal(p.vision_col_ids, b.vision_col_ids.reshape(4, -1)[r].reshape(-1))
    b = _vqa(None)
    (p, rows), = question_prompts(b)
    assert rows.tolist() == [0, 1, 2, 3] and torch.equal(p.text_seq, b.text_seq)
    _same_prompt(p, question_prompt(b))
