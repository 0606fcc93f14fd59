"""Continuous batching for generation: the rows of ONE decode batch are SLOTS that requests pass through.

``generate`` runs M rows in lockstep: they start together, the call lasts as long as its slowest row, and every row has the same prompt shape.
Captioning or answering over a dataset is neither: most captions end long before ``max_new_tokens`` and real VQA batches hold questions of
several lengths.  Here a request that ends (EOS, or its own token limit) frees its slot, and a waiting request takes the slot over while the
other rows go on:

  * the K/V ring advances all rows together from one device-side origin, so a new request moves in by writing its ``mem_len`` projected keys
    and values relative to the current origin (``RingMemory.load_rows``, db1_ring_load_rows): nothing else in the ring moves;
  * waiting requests of one prompt shape are prefilled together through the list-form path (``generation._prefill``), requests of other shapes
    in calls of their own; after a prefill every row holds exactly ``mem_len`` memory entries, whatever its prompt was.  With
    ``model.use_ring_prefill`` the group's prefill writes its keys and values straight into the slots' ring rows instead
    (``generation._prefill_ring``, db1_ring_prefill_rows) and nothing is projected a second time;
  * the per-token graph (one ``GraphedRingStep`` of ``slots`` rows, kept on the model) ends in db1_select_tokens_slots: every slot has its own
    token counter and limit, advanced by the launch itself, and a vacant slot only feeds ``pad_id`` forward.  The same kernel, given the
    slots of the newly admitted rows (``row_map``), picks their token 0 from the prefill's last-position logits straight into their slots;
  * with ``per_request=True`` the graph ends in db1_select_tokens_slots_per instead, which reads greedy / temperature / top-k / top-p / seed
    and the vocabulary window of every slot from a device record the admission writes (``SamplingParams``): requests that are decoded
    differently share one stream, one graph and one batch;
  * with ``per_request_constraints=True`` the selection is framed by db1_constrain_logits_slots_per and db1_stop_match_per, which read every
    slot's penalties, bans, bias and stop sequences from device tables the admission writes (a ``DecodingConstraints`` per request).

A request's tokens depend on its prompt, its stream id, the seed and its token index: not on the slot it got or on when it was admitted.
What the host decides -- which slot, which requests share a prefill, the order results come back in -- is ``SlotScheduler``, plain Python.
"""
from __future__ import annotations

import dataclasses
from collections import OrderedDict
from functools import partial
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .generation import (_PATCH_FIELDS, _PER_ROW_FIELDS, DecodeKey, DecodingConstraints, GenerationConfig, SamplingParams, _batch_size, _constrained,
                         _check_prompt, _need_memory, _prefill, _prefill_ring, Prefixed, _ring_generator, _ring_ok, _SamplingState, _take, _text_window, _use_ring_prefill,
                         _vocab_window, _with_kv_cache, _work, caption_prompt, question_prompts)


# ------------------------------------------------------------------------------------------------------------------------------- requests
@dataclasses.dataclass
class Request:
    """one row of a prompt batch: ``index`` (its place in the results, and its default Philox stream), the batch and the row in it, its
    token limit, and ``key``: requests with equal keys have one prompt shape and can share a prefill; ``params``: its own
    ``SamplingParams`` in a ``per_request`` stream (None: the stream config's); ``constraints``: its own ``DecodingConstraints`` in a
    ``per_request_constraints`` stream (None: the stream's)"""
    index: int
    limit: int
    key: tuple
    prompt: object = None
    row: int = 0
    params: Optional[SamplingParams] = None
    constraints: Optional[DecodingConstraints] = None


@dataclasses.dataclass
class _Item:
    """a prompt batch whose rows carry given result indices (``answer_stream``: the rows of one VQA batch, regrouped by question length)"""
    prompt: object
    indices: object
    limit: Optional[int] = None
    params: Optional[SamplingParams] = None
    constraints: Optional[DecodingConstraints] = None


_SEQ_FIELDS = ("text_seq", "prompt_seq", "img_seq")            # what makes a prompt's shape


def _shape_key(prompt) -> tuple:
    if isinstance(prompt, Prefixed):     # requests over one cache with one suffix length share one continuation call
        return ("Prefixed", id(prompt.cache), prompt.suffix_len)
    key = [type(prompt).__name__]
    for f in _SEQ_FIELDS:
        v = getattr(prompt, f, None)
        if v is not None:
            v = v if torch.is_tensor(v) else np.asarray(v)
            key.append((f,) + tuple(int(n) for n in v.shape[1:]))
    return tuple(key)


def _requests(items: Iterable, cfg: GenerationConfig, min_new: int = 0, per_request: bool = False,
              window: Optional[Tuple[int, int]] = None, caps: Optional[Tuple[int, int]] = None, check_prefixed=None) -> Iterator[Request]:
    """the rows of ``items`` (prompt | (prompt, max_new_tokens) | _Item; ``per_request``: also (prompt, max_new_tokens or None,
    SamplingParams or None); ``caps`` = (max_bad_token_ids, max_logit_bias), the per-request-constraints flag: also (prompt,
    max_new_tokens or None, SamplingParams or None, DecodingConstraints or None)) as Requests, numbered in order; raises ValueError for a
    limit outside [1, cfg.max_new_tokens] or below ``min_new`` (the minimum length of the constraints the request runs under: its own, else
    the stream's), for params when ``per_request`` is off, for params that do not resolve under ``cfg`` and ``window`` = (V, hi)
    (``SamplingParams.resolve``; None: not checked here), for constraints when ``caps`` is None, that are no ``DecodingConstraints`` or
    that hold more banned ids or biases than ``caps``, and what ``generate`` raises for a prompt batch that is not one shape"""
    nxt = 0
    for item in items:
        indices = params = cons = None
        if isinstance(item, _Item):
            prompt, limit, indices, params, cons = item.prompt, item.limit, item.indices, item.params, item.constraints
        elif isinstance(item, tuple):
            if len(item) == 4 and caps is not None:
                prompt, limit, params, cons = item
            elif len(item) == 4 and item[3] is not None:
                raise ValueError("generate_stream: a request with DecodingConstraints needs per_request_constraints=True")
            elif len(item) == 3 and per_request:
                prompt, limit, params = item
            elif len(item) == 3 and item[2] is not None:
                raise ValueError("generate_stream: a request with SamplingParams needs per_request=True")
            elif len(item) != 2:
                raise ValueError("generate_stream: a request is a prompt or (prompt, max_new_tokens)" +
                                 (" or (prompt, max_new_tokens, SamplingParams)" if per_request else ""))
            else:
                prompt, limit = item
        else:
            prompt, limit = item, None
        if params is not None:
            if not per_request:
                raise ValueError("generate_stream: a request with SamplingParams needs per_request=True")
            if not isinstance(params, SamplingParams):
                raise ValueError(f"generate_stream: SamplingParams expected as a request's third element, got {type(params).__name__}")
            if window is not None:
                params.resolve(cfg, *window)
        need = min_new
        if cons is not None:
            if caps is None:
                raise ValueError("generate_stream: a request with DecodingConstraints needs per_request_constraints=True")
            if not isinstance(cons, DecodingConstraints):
                raise ValueError(f"generate_stream: DecodingConstraints expected as a request's fourth element, got {type(cons).__name__}")
            _fits(cons, caps, "a request's")
            need = cons.min_new_tokens     # (the request's object replaces the stream's as a whole)
        limit = int(cfg.max_new_tokens if limit is None else limit)
        if not 1 <= limit <= int(cfg.max_new_tokens):
            raise ValueError(f"generate_stream: a request's max_new_tokens {limit} must lie in [1, config.max_new_tokens = {cfg.max_new_tokens}]")
        if limit < need:
            raise ValueError(f"generate_stream: min_new_tokens {need} exceeds a request's max_new_tokens {limit}")
        G = _batch_size(prompt, prefixed_ok=True)
        if isinstance(prompt, Prefixed) and check_prefixed is not None:     # (``generation._check_prompt`` for the stream's model and kv_cache)
            check_prefixed(prompt)
        key = _shape_key(prompt)
        if indices is None:
            indices = range(nxt, nxt + G)
        elif len(indices) != G:
            raise ValueError(f"generate_stream: {len(indices)} indices for a prompt batch of {G} rows")
        for r, i in enumerate(indices):
            yield Request(index=int(i), limit=limit, key=key, prompt=prompt, row=r, params=params, constraints=cons)
            nxt = max(nxt, int(i) + 1)


def _fits(cons: DecodingConstraints, caps: Tuple[int, int], whose: str):
    """raise ValueError if ``cons`` holds more banned ids or biases than the stream's capacities ``caps``"""
    if len(cons.bad_token_ids) > caps[0]:
        raise ValueError(f"generate_stream: {whose} {len(cons.bad_token_ids)} bad_token_ids exceed max_bad_token_ids = {caps[0]}")
    if len(cons.logit_bias) > caps[1]:
        raise ValueError(f"generate_stream: {whose} {len(cons.logit_bias)} logit_bias entries exceed max_logit_bias = {caps[1]}")


def _gather(reqs: List[Request]):
    """ONE prompt batch holding the rows of ``reqs`` (one shape key), in order"""
    first = reqs[0].prompt
    if isinstance(first, Prefixed):      # the suffix rows gathered like any prompt's, every row with its own handle
        return Prefixed(first.cache, [r.prompt.handles[r.row] for r in reqs], _gather([dataclasses.replace(r, prompt=r.prompt.suffix) for r in reqs]))
    if all(r.prompt is first for r in reqs) and [r.row for r in reqs] == list(range(_batch_size(first))):
        return first
    runs = []    # (consecutive requests of one batch are taken together)
    for r in reqs:
        if runs and runs[-1][0] is r.prompt:
            runs[-1][1].append(r.row)
        else:
            runs.append((r.prompt, [r.row]))

    def field(name):
        parts = [_take(p, name, _batch_size(p), rows) for p, rows in runs]
        if not torch.is_tensor(parts[0]) or not (name in _PER_ROW_FIELDS or name in _PATCH_FIELDS):
            return parts[0]
        return parts[0] if len(parts) == 1 else torch.cat([x.to(parts[0].device) for x in parts], 0)

    x = type(first)(**{f.name: field(f.name) for f in dataclasses.fields(first)})
    for n in _PATCH_FIELDS:
        if hasattr(first, n):
            setattr(x, n, field(n))
    return x


# ------------------------------------------------------------------------------------------------------------- the host's bookkeeping
class SlotScheduler:
    """Which request sits in which slot.  ``requests``: an iterable of objects with ``index``, ``limit`` and ``key``, consumed lazily and in
    order (first come, first served).  The loop of ``generate_stream`` is

        groups = admit()            # free slots -> waiting requests, grouped by key (one prefill each)
        k = replays_due(every)      # how many token steps to run before looking at the device again
        advance(k)
        done = harvest(finished)    # the device's ``finished`` vector -> the (slot, request) pairs that ended, slots freed

    until ``idle()``.  No device, no torch: tests drive it with scripted ``finished`` vectors."""

    def __init__(self, slots: int, requests: Iterable):
        if int(slots) < 1:
            raise ValueError(f"slots {slots} must be >= 1")
        self.slots = int(slots)
        self.owner: List[Optional[object]] = [None] * self.slots
        self.picked = [0] * self.slots       # tokens the slot's request has had picked so far, as far as the host can know (no EOS seen)
        self._it = iter(requests)
        self.admitted = 0

    def free_slots(self) -> List[int]:
        return [s for s in range(self.slots) if self.owner[s] is None]

    def idle(self) -> bool:
        return all(o is None for o in self.owner)

    def admit(self) -> List[Tuple[tuple, List[Tuple[int, object]]]]:
        """the next waiting requests, one per free slot (lowest slot first, in request order) -> [(key, [(slot, request), ...]), ...]: one
        entry per prompt shape, in order of first appearance"""
        groups: "OrderedDict[tuple, list]" = OrderedDict()
        for s in self.free_slots():
            req = next(self._it, None)
            if req is None:
                break
            self.owner[s], self.picked[s] = req, 1     # (the prefill picks token 0)
            self.admitted += 1
            groups.setdefault(req.key, []).append((s, req))
        return list(groups.items())

    def replays_due(self, every: int) -> int:
        """``every``, or fewer when every occupied slot reaches its limit sooner (0: nothing left to run)"""
        left = [self.owner[s].limit - self.picked[s] for s in range(self.slots) if self.owner[s] is not None]
        return max(0, min(int(every), max(left, default=0)))

    def advance(self, k: int):
        for s in range(self.slots):
            if self.owner[s] is not None:
                self.picked[s] = min(self.owner[s].limit, self.picked[s] + int(k))

    def harvest(self, finished) -> List[Tuple[int, object]]:
        """the occupied slots whose ``finished`` entry is set, freed -> [(slot, request)] by ascending request index (the yield order)"""
        done = [(s, self.owner[s]) for s in range(self.slots) if self.owner[s] is not None and int(finished[s]) != 0]
        for s, _ in done:
            self.owner[s] = None
        return sorted(done, key=lambda sr: sr[1].index)


# ----------------------------------------------------------------------------------------------------------------------- the device state
class _SlotState(_SamplingState):
    """the device state of ``key.rows`` slots: per-slot token counter, limit, flags, stream id and output row; ``key.per_request``: also
    every slot's sampling record ``params`` [slots, 8] (``ops.pack_slot_params``), and the selection is db1_select_tokens_slots_per;
    ``key.caps`` = (max_bad_token_ids, max_logit_bias): every slot's constraints live in device tables (``ops.pack_slot_constraints``:
    the record ``cons_rec`` [slots, 8], ``bad`` [slots, caps[0]], ``bias_ids`` / ``bias_val`` [slots, caps[1]], ``stop_tok``
    [slots, 16, 16] and ``stop_len`` [slots, 16]), ``key.constraints`` is only what a slot starts with and a request without its own runs
    under, and the selection is framed by db1_constrain_logits_slots_per and db1_stop_match_per, both always launched"""
    cache = "_slot_generator"

    def __init__(self, model, key: DecodeKey):
        slots, cfg, caps = key.rows, key.cfg, key.caps
        super().__init__(model, key, slots, slots, None if caps is not None else key.constraints)
        self.limit = torch.ones(slots, **self.i32)
        self.finished.fill_(1)       # (vacant)
        state = dict(t=self.t, limit=self.limit, finished=self.finished, lengths=self.lengths, out=self.out, status=self.status)
        self.params = None
        if not key.per_request:
            self._pick = partial(ops.select_tokens_slots, **state, **self.sel)
        else:     # (every slot starts with the config's own record: a vacant slot's is never read, but it is never garbage either)
            rec = ops.pack_slot_params(**SamplingParams().resolve(cfg, key.V, key.hi))
            self.params = torch.from_numpy(np.tile(rec, (slots, 1))).to(self.dev)
            self._pick = partial(ops.select_tokens_slots_per, params=self.params, **state, **self.sel_shared)
        self.caps, self.tables = caps, None
        if caps is not None:     # (every slot starts with the stream's own constraints, as it starts with the config's sampling record)
            self.eos = -1 if cfg.eos_id is None else int(cfg.eos_id)
            self.stream_rows = ops.pack_slot_constraints(key.constraints, cfg.eos_id, *caps)
            self.tables = [torch.from_numpy(np.tile(x, (slots,) + (1,) * x.ndim)).to(self.dev) for x in self.stream_rows]
            self.cons_rec, self.bad, self.bias_ids, self.bias_val, self.stop_tok, self.stop_len = self.tables
            self.checked, self.stop_hit = torch.zeros(slots, **self.i32), torch.zeros(slots, **self.i32)
            self._constrain = partial(ops.constrain_logits_slots_per, cons=self.cons_rec, t=self.t, hist=self.out, finished=self.finished,
                                      status=self.status, V=self.V, bad=self.bad if caps[0] else None, bias_ids=self.bias_ids if caps[1] else None,
                                      bias_val=self.bias_val if caps[1] else None, eos_id=self.eos)
            self._stop = partial(ops.stop_match_per, stop_tok=self.stop_tok, stop_len=self.stop_len, lengths=self.lengths, checked=self.checked,
                                 finished=self.finished, stop_hit=self.stop_hit, out=self.out, pad_id=int(cfg.pad_id), **self.lp_top)

    def start(self):
        self.finished.fill_(1)
        for x in (self.t, self.lengths, self.status) + (() if self.checked is None else (self.checked, self.stop_hit)):
            x.zero_()
        if self.tables is not None:
            for tab, row in zip(self.tables, self.stream_rows):
                tab.copy_(torch.from_numpy(row).to(self.dev).expand_as(tab))

    def occupy(self, slots: List[int], limits: List[int], stream_ids: List[int], records=None, constraints=None) -> torch.Tensor:
        """fresh state for the requests moving into ``slots`` (``records``: int32 [len(slots), 8], their sampling records, in a per-request
        stream; ``constraints``: one ``ops.pack_slot_constraints`` result per request, in a per-request-constraints stream: every table
        row of the slot is overwritten, so nothing of the last tenant's lists stays) -> the slots as the int32 device vector ``select`` and
        ``load_rows`` take"""
        idx = torch.tensor(slots, dtype=torch.int64).to(self.dev)
        for x in (self.t, self.lengths, self.status, self.finished) + (() if self.checked is None else (self.checked, self.stop_hit)):
            x.index_fill_(0, idx, 0)
        self.out.index_fill_(0, idx, self.cfg.pad_id)
        if self.logprob is not None:         # (a new tenant does not inherit the last one's log-probs or their sum)
            self.logprob.index_fill_(0, idx, 0.0)
            self.sum_logprob.index_fill_(0, idx, 0.0)
        self.clear_top(idx)
        self.limit.index_copy_(0, idx, torch.tensor(limits, dtype=torch.int32).to(self.dev))
        self.stream_id.index_copy_(0, idx, torch.from_numpy(np.asarray(stream_ids, dtype=np.int64).astype(np.int32)).to(self.dev))
        if self.params is not None:
            self.params.index_copy_(0, idx, torch.from_numpy(np.ascontiguousarray(records, dtype=np.int32)).to(self.dev))
        if self.tables is not None:     # (the six rows of every new tenant side by side as 32-bit words: ONE copy to the device)
            n = len(slots)
            words = np.concatenate([np.stack([c[k] for c in constraints]).reshape(n, -1).view(np.int32) for k in range(len(self.tables))], 1)
            words, at = torch.from_numpy(words).to(self.dev), 0
            for tab in self.tables:
                w = tab[0].numel()
                if w:
                    tab.index_copy_(0, idx, words[:, at:at + w].contiguous().view(tab.dtype).reshape(n, *tab.shape[1:]))
                at += w
        return idx.to(torch.int32)

    def select(self, logits2d, next_ids, row_map=None):
        """constrain -> select -> stop, all over the same rows: the prefill's token 0 (``row_map``: the new tenants) and every replay"""
        self.constrain(logits2d, row_map)
        self._pick(logits2d, next_ids=next_ids, row_map=row_map)
        self.stop_match(next_ids, row_map)

    def epilogue(self, logits2d, next_ids, ring=None):
        self.select(logits2d, next_ids)      # (the launch advances every live slot's t itself)

    def read(self, slots: List[int]):
        """(out rows, [t, length, status(, stop_hit)] rows, logprob rows or None, (top_ids rows, top_logprob rows) or None) of ``slots`` on the
        host; the fourth column only with stop sequences (per-request constraints: always)"""
        idx = torch.tensor(slots, dtype=torch.int64).to(self.dev)
        cols = (self.t, self.lengths, self.status) + (() if self.checked is None else (self.stop_hit,))
        meta = torch.stack(cols, 1).index_select(0, idx).cpu()
        lp = None if self.logprob is None else self.logprob.index_select(0, idx).cpu()
        top = None if self.top_ids is None else (self.top_ids.index_select(0, idx).cpu(), self.top_logprob.index_select(0, idx).cpu())
        return self.out.index_select(0, idx).cpu(), meta, lp, top


# ------------------------------------------------------------------------------------------------------------------------------ the driver
def generate_stream(model, requests: Iterable, config: Optional[GenerationConfig] = None, slots: int = 8, stream_ids=None,
                    stats: Optional[dict] = None, replay: bool = True,
                    constraints: Optional[DecodingConstraints] = None, per_request: bool = False, per_request_constraints: bool = False,
                    max_bad_token_ids: int = 64, max_logit_bias: int = 64, kv_cache: str = "bf16") -> Iterator[tuple]:
    """Generate for a stream of requests over ``slots`` recycled rows; yields ``(index, ids int32 [limit], length)`` on the host as requests
    finish (requests that are found finished at the same look come in index order).  ``ids[:length]`` are the tokens before EOS, then EOS,
    then ``pad_id``.

    ``requests``: an iterable (consumed lazily) of prompts -- each ONE ``NLPTaskInput`` / ``ICTaskInput`` / ``VQATaskInput`` batch of one or
    more rows of one shape, every row a request -- or ``(prompt, max_new_tokens)`` with ``max_new_tokens <= config.max_new_tokens`` as the
    rows' own limit.  Items may differ in shape and kind.  Requests are numbered in order; ``stream_ids`` (indexable by that number; default:
    the number itself) gives every request its Philox stream.  Ring path only (bf16, ``use_decode``, d_head 128, mem_len > 0): anything else
    raises ValueError here, before anything is launched, and so does a bad first request list when ``requests`` is a list or tuple.
    The host looks at the device every ``config.sync_every`` token steps.  ``replay`` False: the same forward and epilogue launched eagerly
    over the same ring instead of as a graph replay.  ``stats`` (a dict) receives ``replays`` (token steps), ``prefill_calls``,
    ``admitted``, ``occupancy`` = live row-steps / (replays * slots) and ``no_candidate``: the requests that ended early because a step had no
    finite logit in the window (``pad_id`` written, as ``generate`` does; they come back like any other request).  ONE stream at a time per
    model: the slots, the ring and the graph are kept on the model, so a second ``generate_stream`` whose first result is asked for while
    another is still running raises RuntimeError (run the first to its end or ``close()`` it).  ``constraints`` (a ``DecodingConstraints``):
    applied on the device to every step's logits over each request's own tokens so far, whatever slot it sits in; a request whose limit is
    below ``min_new_tokens`` raises ValueError; a request ended by one of the ``stop_sequences`` comes back without the matched tokens and
    frees its slot at the host's next look, and ``stats`` then also receives ``stopped``, their count.  With ``config.logprobs`` the stream yields ``(index, ids, length, logprobs float32 [limit])``:
    every token's log-probability as ``generate`` returns it (EOS included, 0 after it); with ``config.top_logprobs`` n two more fields,
    ``top_ids int32 [limit, n]`` and ``top_logprobs float32 [limit, n]``, as ``generate`` returns them (-1 / -inf after the request's last
    token).  ``per_request`` True: a request may also be ``(prompt, max_new_tokens or None, SamplingParams)`` and is then decoded under its
    own greedy / temperature / top_k / top_p / seed / vocabulary window (fields left None: the config's); a request without params runs under
    the config.  The stream's graph then ends in db1_select_tokens_slots_per, which reads every slot's parameters on the device; the flag is
    needed up front because ``requests`` is consumed lazily and the captured graph holds one kernel or the other, and it joins the
    generator's cache key.  ``eos_id``, ``pad_id``, the constraints and the log-prob switches stay the stream's.  False: nothing changes, and
    a request that carries params raises ValueError (a list or tuple of requests: before any launch).  ``per_request_constraints`` True: a
    request may also be ``(prompt, max_new_tokens or None, SamplingParams or None, DecodingConstraints or None)`` (the third element None
    unless ``per_request`` is set too: the two flags are independent) and then runs under its OWN constraints, which replace the stream's
    ``constraints=`` as a whole (there are no "inherit" fields); a request without one runs under the stream's, or under none.  The
    graph's epilogue is then db1_constrain_logits_slots_per, the selection, db1_stop_match_per, all three always captured, reading every
    slot's record and lists from device tables the admission writes; ``max_bad_token_ids`` / ``max_logit_bias`` (0 .. 1024 each) are the
    tables' widths, the most banned ids / biases ANY request (or the stream's object) may hold.  The flag is needed up front for the
    reason ``per_request`` is and joins the cache key with the two capacities; ``stats["stopped"]`` is then always present.  False: nothing
    changes, and a request that carries constraints raises ValueError.  ``kv_cache`` "fp8": the slots' ring holds e4m3 keys / values, as
    ``generate`` describes it (admissions quantise the prefill's keys / values on their way in); it joins the cache key.  A request's prompt
    may be a ``generation.Prefixed`` (rows that continue prefixes held in a ``PrefixCache`` of this model and ``kv_cache``; ValueError
    otherwise): waiting requests over one cache with one suffix length share one continuation call into their slots
    (db1_relattn_mem_ring_fwd, db1_ring_fork_rows), mix with plain requests, and ``stats["prefixed"]`` counts them."""
    cfg = config or GenerationConfig()
    _need_memory(model, "generate_stream")
    if not _ring_ok(model):
        raise ValueError("generate_stream needs a bf16 model with the K/V-cached decode path (use_decode, d_head 128, mem_len > 0)")
    slots = int(slots)
    if not 1 <= slots <= 65535:
        raise ValueError(f"slots {slots} must lie in [1, 65535]")
    V, hi = _vocab_window(model, cfg)
    if not ops.select_tokens_slots_supported(V, V, model.compute_dtype):
        raise ValueError(f"db1_select_tokens_slots does not support a vocabulary of {V}")
    per_request = bool(per_request)
    key = _constrained("generate_stream", model, DecodeKey(rows=slots, cfg=cfg, V=V, hi=hi, per_request=per_request), constraints, cfg.max_new_tokens)
    key = _with_kv_cache("generate_stream", model, key, kv_cache)
    min_new = 0 if constraints is None else constraints.min_new_tokens
    caps = None
    if per_request_constraints:     # (with the flag off the key is what it was, and neither capacity is looked at)
        caps = _capacities(max_bad_token_ids, max_logit_bias)
        if not ops.constrain_logits_slots_supported(V, V, cfg.max_new_tokens, caps[0], caps[1], model.compute_dtype):
            raise ValueError(f"db1_constrain_logits_slots_per does not support a vocabulary of {V} with max_new_tokens {cfg.max_new_tokens}")
        if constraints is not None:
            _fits(constraints, caps, "the stream's")
        key = dataclasses.replace(key, caps=caps)
    chk = lambda p: _check_prompt("generate_stream", model, p, kv_cache, None)      # (a Prefixed request: its cache's model and K/V format)
    if isinstance(requests, (list, tuple)):
        for _ in _requests(requests, cfg, min_new, per_request, (V, hi), caps, chk):     # (a list can be checked as a whole before the first launch)
            pass
    return _stream(model, _requests(requests, cfg, min_new, per_request, (V, hi), caps, chk), key, stream_ids, stats, replay)


def _capacities(max_bad_token_ids, max_logit_bias) -> Tuple[int, int]:
    for name, v in (("max_bad_token_ids", max_bad_token_ids), ("max_logit_bias", max_logit_bias)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= ops.MAX_SLOT_LIST:
            raise ValueError(f"generate_stream: {name} {v!r} must be an integer in [0, {ops.MAX_SLOT_LIST}]")
    return int(max_bad_token_ids), int(max_logit_bias)


def _stream(model, reqs, key: DecodeKey, stream_ids, stats, replay):
    slots, cfg, V, hi, per, caps = key.rows, key.cfg, key.V, key.hi, key.per_request, key.caps
    inherit = SamplingParams()
    sched = SlotScheduler(slots, reqs)
    counts = dict(replays=0, prefill_calls=0, admitted=0, occupancy=0.0, no_candidate=0, prefixed=0)
    if caps is not None or (key.constraints is not None and key.constraints.stop_sequences):      # (the key set is what it was without stop sequences)
        counts["stopped"] = 0
    live_steps = 0

    def report():
        counts["admitted"] = sched.admitted
        counts["occupancy"] = live_steps / (counts["replays"] * slots) if counts["replays"] else 0.0
        if stats is not None:
            stats.update(counts)

    gen = None
    try:
        while True:
            results = []
            with _work(model):
                if gen is None:
                    held = getattr(model, _SlotState.cache, None)
                    if held is not None and held.busy:
                        raise RuntimeError("generate_stream: another stream is still running on this model (one stream at a time: finish or "
                                           "close() it first)")
                    gen = _ring_generator(model, _SlotState, key)
                    gen.busy = True
                    gen.state.start()
                    gen.ring.load_status.zero_()
                st, step = gen.state, gen.step
                for _, members in sched.admit():
                    rows = [s for s, _ in members]
                    rs = [r for _, r in members]
                    # one prefill for the group; its last position picks token 0 of every request straight into its slot, its memory moves in
                    prefixed = isinstance(rs[0].prompt, Prefixed)     # (the group continues rows of a PrefixCache: one call over its suffixes)
                    direct = prefixed or _use_ring_prefill(model)
                    counts["prefixed"] += len(rs) if prefixed else 0
                    if not direct:
                        logits, mems = _prefill(model, _gather(rs), len(rs))
                    recs = np.stack([ops.pack_slot_params(**(r.params or inherit).resolve(cfg, V, hi)) for r in rs]) if per else None
                    packed = None
                    if caps is not None:     # (packing validates every record on the host before it is written)
                        packed = [st.stream_rows if r.constraints is None else ops.pack_slot_constraints(r.constraints, cfg.eos_id, *caps)
                                  for r in rs]
                    idx = st.occupy(rows, [r.limit for r in rs], [r.index if stream_ids is None else int(stream_ids[r.index]) for r in rs], recs,
                                    packed)
                    if direct:   # (model.use_ring_prefill) the group's keys / values go straight into its slots' ring rows, nothing moves in afterwards
                        logits, mems = _prefill_ring(model, _gather(rs), gen.ring, idx), None
                    st.select(logits[:, -1], step.ids[:, 0], row_map=idx)
                    if not direct:
                        gen.ring.load_rows(mems, idx)
                    del logits, mems
                    counts["prefill_calls"] += 1
                k = sched.replays_due(cfg.sync_every)
                for _ in range(k):
                    gen.token(replay)
                sched.advance(k)
                counts["replays"] += k
                if not sched.idle():
                    done = sched.harvest(st.finished.cpu())          # (the host's look at the device)
                    if done:
                        out, meta, lp, top = st.read([s for s, _ in done])
                        for j, (_, r) in enumerate(done):
                            t, length, status, *hit = (int(v) for v in meta[j])
                            if hit and hit[0]:
                                counts["stopped"] += 1
                            if status & 2:
                                raise RuntimeError("db1_select_tokens_slots: a slot's token counter left [0, limit)")
                            if status & 4:
                                raise RuntimeError("db1_select_tokens_slots_per: a slot's sampling parameters were refused on the device "
                                                   "(SamplingParams.resolve validates every record on the host before it is written, so "
                                                   "this cannot happen unless the slot state was overwritten)")
                            if status & 8:
                                raise RuntimeError("db1_constrain_logits_slots_per: a slot's constraints were refused on the device "
                                                   "(ops.pack_slot_constraints validates every record on the host before it is written, "
                                                   "so this cannot happen unless the slot state was overwritten)")
                            counts["no_candidate"] += status & 1
                            live_steps += t - 1
                            results.append((r.index, out[j, :r.limit].clone(), length) + (() if lp is None else (lp[j, :r.limit].clone(),)) +
                                           (() if top is None else (top[0][j, :r.limit].clone(), top[1][j, :r.limit].clone())))
                finish = sched.idle() and not results
                if finish:     # nothing waits (admit found no request for the free slots) and every slot is vacant
                    gen.check(replay)
                    if int(gen.ring.load_status.cpu()) != 0:
                        raise RuntimeError("db1_ring_load_rows / db1_ring_prefill_rows / db1_ring_fork_rows: a request was given a row outside the "
                                           "ring, or a cache row out of range")
            report()
            for r in results:
                yield r
            if finish:
                return
    finally:
        if gen is not None:
            gen.busy = False


def generate_many(model, requests: Iterable, config: Optional[GenerationConfig] = None, **kw):
    """``generate_stream`` run to its end -> (ids, lengths) in request order: ``ids[i]`` int32 [request i's limit], ``lengths[i]`` an int;
    with ``config.logprobs`` a third list: ``logprobs[i]`` float32 [request i's limit]; with ``config.top_logprobs`` n two more:
    ``top_ids[i]`` int32 and ``top_logprobs[i]`` float32, both [request i's limit, n]"""
    got = {r[0]: r[1:] for r in generate_stream(model, requests, config, **kw)}
    order = sorted(got)
    # as many lists as the stream's tuples have fields after the index; no request at all: what the config says they would have had
    width = len(got[order[0]]) if order else (2 if config is None or not config.logprobs else 5 if config.top_logprobs else 3)
    return tuple([got[i][k] for i in order] for k in range(width))


def _split(item):
    """a stream wrapper's item -> (batch, max_new_tokens or None, what follows: (), (SamplingParams,) or (SamplingParams or None,
    DecodingConstraints or None), passed through as it is)"""
    if not isinstance(item, tuple):
        return item, None, ()
    b, limit, *rest = item
    return b, limit, tuple(rest)


def caption_stream(model, ic_batches: Iterable, cfg: Optional[GenerationConfig] = None, **kw):
    """``generate_stream`` over ``ICTaskInput`` batches (or ``(batch, max_new_tokens)``; ``per_request=True``: or ``(batch, max_new_tokens
    or None, SamplingParams)``, the params of every image of the batch; ``per_request_constraints=True``: with a fourth element, the
    ``DecodingConstraints`` of every image of the batch): the prompts of ``caption_prompt``, tokens in the text vocabulary
    unless ``cfg`` (or a request's own params) says otherwise; every image is one request"""
    cfg = _text_window(model, cfg or GenerationConfig())

    def items():
        for it in ic_batches:
            b, limit, rest = _split(it)
            yield (caption_prompt(b), limit) + rest

    return generate_stream(model, items(), cfg, **kw)


def answer_stream(model, vqa_batches: Iterable, cfg: Optional[GenerationConfig] = None, **kw):
    """``generate_stream`` over ``VQATaskInput`` batches (or ``(batch, max_new_tokens)``; ``per_request=True``: or ``(batch, max_new_tokens
    or None, SamplingParams)``, the params of every question of the batch; ``per_request_constraints=True``: with a fourth element, the
    ``DecodingConstraints`` of every question of the batch) whose questions may differ in length (``question_prompts``),
    tokens in the text vocabulary unless ``cfg`` (or a request's own params) says otherwise; every question is one request, and the
    results' indices number the batches' rows in their original order.  An item's batch may also be a ``Prefixed`` prompt (the questions of
    ``question_suffixes`` over handles of ``PrefixCache.put(image_prefix(batch))``): its rows are requests like any other"""
    cfg = _text_window(model, cfg or GenerationConfig())

    def items():
        base = 0
        for it in vqa_batches:
            b, limit, rest = _split(it)
            if len(rest) > 2:
                raise ValueError("answer_stream: a request is a batch, (batch, max_new_tokens), (batch, max_new_tokens, SamplingParams) or "
                                 "(batch, max_new_tokens, SamplingParams, DecodingConstraints)")
            if isinstance(b, Prefixed):      # questions that continue cached image prefixes (image_prefix / question_suffixes): as they are
                yield _Item(b, [base + r for r in range(len(b.handles))], limit, *rest)
                base += len(b.handles)
                continue
            for prompt, rows in question_prompts(b):
                yield _Item(prompt, [base + int(r) for r in rows], limit, *rest)
            base += _batch_size(b)

    return generate_stream(model, items(), cfg, **kw)
