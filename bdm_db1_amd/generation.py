"""Text generation: captions (IC), answers (VQA) and text continuations, with the next token picked ON THE DEVICE.

The reference trains these three workloads and evaluates IC / VQA by generating text (train.py:24-25,44,146-170: evaluate_ic /
evaluate_vqa with a ``Decoder(max_length=30)`` that keeps the tokens before the first EOS, text_decoder.py:42-62); those evaluation modules
are not part of its release.  Here sampling (``generate``) and beam search (``beam_search``) are ONE driver, ``_decode``, over two kinds of
device state (``_State``, ``_BeamState``), and a generation is

  * one prefill call (``_prefill``): the prompt (``[prompt, image patches, text]``, longer than the 64 new tokens a ring call takes) runs once
    per prompt through the list-form memory path (``model.init_mem``); its last position picks token 0;
  * then one call per token.  bf16 models with the K/V-cached decode path (``model.use_decode``): the list-form memory is projected into a
    ``RingMemory`` and every token is ONE hipGraph replay (``_RingGenerator``) holding the one-token forward and the state's epilogue: the
    selection, which writes the next token straight into the step's static input ids, and the captured ``t += 1`` of the token counter -- no
    host round trip between tokens; the host asks the state every ``sync_every`` tokens whether all rows have finished, to stop early.
    Other models (fp32, no ring) run the same loop eagerly over the list-form memory, with the same epilogue.

Sampling's epilogue is ``db1_select_tokens`` (greedy / temperature / top-k / top-p, Gumbel-max draws from Philox); beam search's is
``db1_beam_step`` (lse, per-row top-2W, the group walk, the hypothesis pool, the next ids) and ``db1_ring_reorder`` (the last t keys of every
beam whose parent is another row), after a prefill whose memory and last logits are expanded to the W beams of each prompt; with
``BeamSearchConfig.num_beam_groups`` > 1 the step is ``db1_beam_step_diverse`` (sub-groups that choose in turn under a Hamming penalty).  The
rules are stated in include/db1_hip.h and restated in NumPy in tests/select_rule.py, tests/beam_rule.py and tests/diverse_beam_rule.py.  With ``constraints=`` (a
``DecodingConstraints``) either epilogue is preceded by ``db1_constrain_logits``, which edits the step's logits in place over each row's own
generated tokens (tests/constraint_rule.py; with a frequency / presence penalty or a logit bias ``db1_constrain_logits_pen``,
tests/penalty_rule.py), and with stop sequences the sampling epilogue is followed by ``db1_stop_match`` (tests/stop_rule.py), which ends a row
whose tokens spell one and removes them; without, nothing is launched.  With ``speculative=`` (a ``SpeculativeConfig``) a token call
carries 1 + k tokens per row, k of them drafts, and the sampling epilogue is ``db1_spec_pick`` / ``db1_spec_accept`` / ``db1_spec_commit``
(``_SpecState``, tests/spec_rule.py): the same tokens in fewer calls where the drafts are right.  scoring.py takes its prefill, its eval-mode switch and its
vocabulary checks from here.
"""
from __future__ import annotations

import contextlib
import dataclasses
from dataclasses import dataclass, field
from functools import partial
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .decode import GraphedRingStep, GroupedRingMemory, RingMemory, RingPrefill, _token_input  # noqa: F401  (scoring.py takes _token_input from here)


@dataclass(frozen=True)
class GenerationConfig:
    """``greedy``: arg-max (``temperature`` / ``top_k`` / ``top_p`` / ``seed`` unused); else Gumbel-max sampling at ``temperature`` after
    top-k (0 = off) and top-p (1 = off).  ``eos_id`` None: no end-of-sequence token.  Tokens are chosen in ``[vocab_lo, vocab_hi)``
    (``vocab_hi`` None: the model's whole vocabulary for ``generate``, the text vocabulary for captions and answers).  The host checks
    whether every row has finished each ``sync_every`` tokens.  ``logprobs``: the selection also returns every chosen token's log-probability
    over the window (``db1_select_tokens_lp``; the model's distribution, before temperature / top-k / top-p) and the row's sum; the tokens
    are the same either way.  ``top_logprobs`` n (keyword-only; 1 .. 16, with ``logprobs``; 0 = off): also the n most likely tokens of every step and their
    log-probabilities under that same distribution (``db1_select_tokens_top``), the most likely first, ties to the lower id."""
    max_new_tokens: int = 30
    greedy: bool = True
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    eos_id: Optional[int] = None
    pad_id: int = 0
    vocab_lo: int = 0
    vocab_hi: Optional[int] = None
    sync_every: int = 8
    # keyword-only: it comes last in the constructor, after every argument a caller could pass by position before it existed; ``logprobs``
    # stays the last of ``dataclasses.fields``
    top_logprobs: int = field(default=0, kw_only=True)
    logprobs: bool = False

    def __post_init__(self):
        n = self.top_logprobs
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= ops.MAX_TOP_N:
            raise ValueError(f"top_logprobs {n!r} must be an integer in [0, {ops.MAX_TOP_N}]")
        if int(n) and not self.logprobs:
            raise ValueError(f"top_logprobs {n} needs logprobs=True")
        if int(self.max_new_tokens) < 1:
            raise ValueError(f"max_new_tokens {self.max_new_tokens} must be >= 1")
        if not self.greedy and not (0.0 < float(self.temperature) < float("inf")):
            raise ValueError(f"temperature {self.temperature} must be > 0 when sampling")
        if not 0.0 < float(self.top_p) <= 1.0:
            raise ValueError(f"top_p {self.top_p} must lie in (0, 1]")
        if int(self.top_k) < 0:
            raise ValueError(f"top_k {self.top_k} must be >= 0")
        if int(self.vocab_lo) < 0 or (self.vocab_hi is not None and int(self.vocab_hi) <= int(self.vocab_lo)):
            raise ValueError(f"vocabulary window [{self.vocab_lo}, {self.vocab_hi}) is empty")
        if int(self.sync_every) < 1:
            raise ValueError(f"sync_every {self.sync_every} must be >= 1")
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"seed {self.seed} must be a 64-bit unsigned integer")


@dataclass(frozen=True)
class SamplingParams:
    """One request's own sampling parameters in a stream run with ``per_request=True`` (serving.py): the fields of ``GenerationConfig`` that
    ``db1_select_tokens_slots_per`` reads per slot.  ``None`` inherits the stream config's value; for the window that is the RESOLVED one
    (``vocab_hi``: the text vocabulary under ``caption_stream`` / ``answer_stream``, else the config's, else the model's whole vocabulary).
    ``eos_id``, ``pad_id`` and the log-prob switches stay the stream's; so do the constraints, unless the stream also sets
    ``per_request_constraints`` (serving.py): then a request may carry its own ``DecodingConstraints`` as a fourth element."""
    greedy: Optional[bool] = None
    temperature: Optional[float] = None
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    seed: Optional[int] = None
    vocab_lo: Optional[int] = None
    vocab_hi: Optional[int] = None

    def resolve(self, cfg: GenerationConfig, V: int, hi: int) -> dict:
        """the concrete values under the stream config ``cfg`` of a model with a vocabulary of ``V``, ``hi`` the end of the config's window
        inside it (``_vocab_window``) -> the keyword arguments of ``ops.pack_slot_params``.  Raises ValueError for what ``GenerationConfig``
        refuses and for a window that is empty or leaves [0, V)."""
        mine = {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if getattr(self, f.name) is not None}
        mine.setdefault("vocab_hi", int(hi))
        c = dataclasses.replace(cfg, **mine)     # (GenerationConfig's own checks, in its own words)
        if int(c.vocab_hi) > int(V):
            raise ValueError(f"vocabulary window [{c.vocab_lo}, {c.vocab_hi}) exceeds the model's vocabulary ({V})")
        return dict(greedy=bool(c.greedy), temperature=float(c.temperature), top_k=int(c.top_k), top_p=float(c.top_p), seed=int(c.seed),
                    vocab_lo=int(c.vocab_lo), vocab_hi=int(c.vocab_hi))


@dataclass(frozen=True)
class BeamSearchConfig:
    """Beam search with ``num_beams`` beams per prompt (1 .. 16), ``max_new_tokens`` new tokens (at most the model's ``mem_len``), scores
    normalised by (length)^``length_penalty``; the best ``num_return_sequences`` (<= num_beams) hypotheses of each prompt come back.
    ``eos_id`` None: no end-of-sequence token (every hypothesis runs ``max_new_tokens``).  Tokens are chosen in ``[vocab_lo, vocab_hi)``
    (``vocab_hi`` None as in ``GenerationConfig``).  The host checks whether every prompt is done each ``sync_every`` tokens.
    ``num_beam_groups`` D > 1: diverse beam search (Vijayakumar et al., 2016; rule in include/db1_hip.h) -- the beams are split into D
    sub-groups of num_beams / D that choose in turn at every step; a token an earlier sub-group chose in this step costs a later one
    ``diversity_penalty`` per earlier choice in its ranking.  The scores that come back stay the model's length-normalised log-probabilities;
    the results are the best of the D merged pools.  D must divide ``num_beams``; the penalty is finite, >= 0, and 0 when D = 1."""
    num_beams: int = 4
    max_new_tokens: int = 30
    length_penalty: float = 1.0
    num_return_sequences: int = 1
    eos_id: Optional[int] = None
    pad_id: int = 0
    vocab_lo: int = 0
    vocab_hi: Optional[int] = None
    sync_every: int = 8
    num_beam_groups: int = 1
    diversity_penalty: float = 0.0

    def __post_init__(self):
        if not 1 <= int(self.num_beams) <= 16:
            raise ValueError(f"num_beams {self.num_beams} must lie in [1, 16]")
        D, lam = self.num_beam_groups, self.diversity_penalty
        if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 1 <= int(D) <= int(self.num_beams) or int(self.num_beams) % int(D):
            raise ValueError(f"num_beam_groups {D!r} must be an integer in [1, num_beams = {self.num_beams}] that divides num_beams")
        if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0 <= float(lam) < float("inf"):
            raise ValueError(f"diversity_penalty {lam!r} must be finite and >= 0")
        if int(D) == 1 and float(lam) != 0:
            raise ValueError(f"diversity_penalty {lam} needs num_beam_groups > 1 (one group has no earlier group to differ from)")
        if int(self.max_new_tokens) < 1:
            raise ValueError(f"max_new_tokens {self.max_new_tokens} must be >= 1")
        if not abs(float(self.length_penalty)) < float("inf"):
            raise ValueError(f"length_penalty {self.length_penalty} must be finite")
        if not 1 <= int(self.num_return_sequences) <= int(self.num_beams):
            raise ValueError(f"num_return_sequences {self.num_return_sequences} must lie in [1, num_beams = {self.num_beams}]")
        if int(self.vocab_lo) < 0 or (self.vocab_hi is not None and int(self.vocab_hi) <= int(self.vocab_lo)):
            raise ValueError(f"vocabulary window [{self.vocab_lo}, {self.vocab_hi}) is empty")
        if self.eos_id is not None and int(self.eos_id) < 0:
            raise ValueError(f"eos_id {self.eos_id} must be >= 0 (or None)")
        if int(self.sync_every) < 1:
            raise ValueError(f"sync_every {self.sync_every} must be >= 1")


@dataclass(frozen=True)
class SpeculativeConfig:
    """Speculative decoding for ``generate`` (``speculative=``): every call feeds a row its last token and ``num_draft_tokens`` k guessed
    next tokens (1 .. 15; Q = 1 + k positions per call) and keeps the model's own choices up to the first wrong guess.  The selection rule is the
    one-token loop's, greedy or sampled (include/db1_hip.h, db1_spec_pick / _accept / _commit): the results are the same in exact arithmetic
    and in fp32 up to the order of the GEMMs' sums; in bf16 the wider call's logits differ in their last bits, and a row can part from the
    one-token loop's at a near tie (``generate`` says more).  The
    guesses come from an n-gram lookup over the row's history on the device: the longest n-gram, ``ngram_max`` down to ``ngram_min`` (1 .. 8),
    that ends the history and occurred before, continued from its latest occurrence; ``use_prompt``: the history starts with the prompt's
    text tokens (``NLPTaskInput`` prompts), not only with the generated ones.  ``draft_script=`` of ``generate`` replaces the lookup."""
    num_draft_tokens: int = 4
    ngram_max: int = 3
    ngram_min: int = 1
    use_prompt: bool = True

    def __post_init__(self):
        for name, lo, hi in (("num_draft_tokens", 1, ops.SPEC_MAX_Q - 1), ("ngram_max", 1, ops.SPEC_MAX_NGRAM), ("ngram_min", 1, ops.SPEC_MAX_NGRAM)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} {v!r} must be an integer in [{lo}, {hi}]")
            object.__setattr__(self, name, int(v))
        if self.ngram_min > self.ngram_max:
            raise ValueError(f"ngram_min {self.ngram_min} exceeds ngram_max {self.ngram_max}")
        object.__setattr__(self, "use_prompt", bool(self.use_prompt))


@dataclass(frozen=True)
class _SpecPlan:
    """what a speculative decoding state is built from besides the config: whether the drafts come from a script, and the row stride of the
    prompt-text buffer (0: none).  The ``speculative`` field of a ``DecodeKey``."""
    config: SpeculativeConfig
    scripted: bool
    ctx_cap: int


MAX_BAD_TOKEN_IDS = 1024
MAX_LOGIT_BIAS = 1024
MAX_STOP_SEQUENCES, MAX_STOP_LEN = ops.MAX_STOP_SEQUENCES, ops.MAX_STOP_LEN


def _is_count(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) < 2 ** 31


@dataclass(frozen=True)
class DecodingConstraints:
    """Edits of every step's logits before the token (or the beams) are chosen, applied on the device by ``db1_constrain_logits`` (rule in
    include/db1_hip.h) over the tokens a row has GENERATED so far (the prompt is not part of the history): ``repetition_penalty`` theta
    (1 = off): the logit of every token already generated is divided by theta if positive, else multiplied; ``no_repeat_ngram_size`` n
    (0 = off): no n-gram occurs twice; ``min_new_tokens``: EOS cannot be chosen before that many tokens (nothing without an ``eos_id``);
    ``bad_token_ids``: never chosen.  ``frequency_penalty`` f / ``presence_penalty`` p (any finite value, 0 = off): f * (the number of times
    a token has been generated) + p is taken off the logit of every token already generated, after the repetition penalty
    (``db1_constrain_logits_pen``, tests/penalty_rule.py).  ``logit_bias`` (a mapping, or pairs, token id -> bias; at most 1024): added to
    those tokens' logits at every step, after the penalties; a ban still overrides it.  ``stop_sequences`` (at most 16 sequences of 1 .. 16
    token ids): a row whose generated tokens end in one of them ends there, and the matched tokens are removed from what comes back
    (``db1_stop_match``, tests/stop_rule.py); the longest match wins, then the first listed.  Passed as ``constraints=`` to ``generate``,
    ``beam_search`` and the streams; ``beam_search`` and ``sample_best_of`` refuse stop sequences.  In a stream with
    ``per_request_constraints=True`` a request may carry an object of its own, which replaces the stream's as a whole
    (``db1_constrain_logits_slots_per`` / ``db1_stop_match_per`` read every slot's values from device tables)."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    bad_token_ids: Tuple[int, ...] = ()
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    logit_bias: Tuple[Tuple[int, float], ...] = ()
    stop_sequences: Tuple[Tuple[int, ...], ...] = ()

    def __hash__(self):
        # (the first four fields alone while the later ones are off: the hash such an object has always had)
        old = (self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens, self.bad_token_ids)
        new = (self.frequency_penalty, self.presence_penalty, self.logit_bias, self.stop_sequences)
        return hash(old if new == (0.0, 0.0, (), ()) else old + new)

    def _check_new_fields(self):
        for name in ("frequency_penalty", "presence_penalty"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not abs(float(v)) < float("inf"):
                raise ValueError(f"{name} {v!r} must be a finite number")
            with np.errstate(over="ignore"):
                if not abs(float(np.float32(v))) < float("inf"):
                    raise ValueError(f"{name} {v!r} must be finite in float32")
            object.__setattr__(self, name, float(v))
        bias = self.logit_bias
        try:
            pairs = [tuple(kv) for kv in (bias.items() if hasattr(bias, "items") else bias)]
        except TypeError:
            raise ValueError(f"logit_bias {bias!r} must be a mapping or an iterable of (token id, bias)") from None
        if len(pairs) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias: {len(pairs)} entries (at most {MAX_LOGIT_BIAS})")
        for kv in pairs:
            if len(kv) != 2 or not _is_count(kv[0]):
                raise ValueError(f"logit_bias: {kv!r} must be (token id, bias) with an integer id >= 0")
            b = kv[1]
            if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)) or not abs(float(np.float32(b))) < float("inf"):
                raise ValueError(f"logit_bias: the bias {b!r} of token {kv[0]} must be a finite number")
        pairs = sorted((int(k), float(b)) for k, b in pairs)
        if len({k for k, _ in pairs}) != len(pairs):
            raise ValueError("logit_bias: the token ids must be distinct")
        object.__setattr__(self, "logit_bias", tuple(pairs))
        try:
            seqs = [tuple(q) for q in self.stop_sequences]
        except TypeError:
            raise ValueError(f"stop_sequences {self.stop_sequences!r} must be sequences of token ids") from None
        if len(seqs) > MAX_STOP_SEQUENCES:
            raise ValueError(f"stop_sequences: {len(seqs)} sequences (at most {MAX_STOP_SEQUENCES})")
        for q in seqs:
            if not 1 <= len(q) <= MAX_STOP_LEN:
                raise ValueError(f"stop_sequences: a sequence of {len(q)} tokens (1 .. {MAX_STOP_LEN})")
            for v in q:
                if not _is_count(v):
                    raise ValueError(f"stop_sequences: {v!r} must be an integer >= 0")
        object.__setattr__(self, "stop_sequences", tuple(tuple(int(v) for v in q) for q in seqs))

    def __post_init__(self):
        self._check_new_fields()
        theta = float(self.repetition_penalty)
        if not 0.0 < theta < float("inf"):
            raise ValueError(f"repetition_penalty {self.repetition_penalty} must be finite and > 0")
        for name in ("no_repeat_ngram_size", "min_new_tokens"):
            v = getattr(self, name)
            if not _is_count(v):
                raise ValueError(f"{name} {v!r} must be an integer >= 0")
        ids = tuple(self.bad_token_ids)
        if len(ids) > MAX_BAD_TOKEN_IDS:
            raise ValueError(f"bad_token_ids: {len(ids)} ids (at most {MAX_BAD_TOKEN_IDS})")
        for v in ids:
            if not _is_count(v):
                raise ValueError(f"bad_token_ids: {v!r} must be an integer >= 0")
        object.__setattr__(self, "repetition_penalty", theta)
        object.__setattr__(self, "no_repeat_ngram_size", int(self.no_repeat_ngram_size))
        object.__setattr__(self, "min_new_tokens", int(self.min_new_tokens))
        object.__setattr__(self, "bad_token_ids", tuple(int(v) for v in ids))

    def applies(self, eos_id: Optional[int] = 0) -> bool:
        """whether anything is edited under a config with this ``eos_id`` (None: no EOS, so the minimum length holds nothing back).  THE
        definition of a no-op: False means no launch, and the generator's cache key stays what it is without constraints"""
        return self.edits_logits(eos_id) or bool(self.stop_sequences)

    @property
    def edits_more(self) -> bool:
        """a frequency or presence penalty or a bias is set: the logits are edited by ``db1_constrain_logits_pen``"""
        return bool(self.frequency_penalty != 0.0 or self.presence_penalty != 0.0 or self.logit_bias)

    def edits_logits(self, eos_id: Optional[int] = 0) -> bool:
        """``applies`` without the stop sequences, which edit no logit: whether a constrain launch precedes the selection"""
        return bool(self.repetition_penalty != 1.0 or self.no_repeat_ngram_size or self.bad_token_ids or
                    (self.min_new_tokens and eos_id is not None) or self.edits_more)

    @property
    def is_noop(self) -> bool:
        """nothing to apply whatever the config (``applies`` also knows the config's ``eos_id``)"""
        return not self.applies()


@dataclass(frozen=True)
class DecodeKey:
    """What a decoding state is built from and its cached ring generator is kept under: ``rows`` prompts (a stream: slots), the config, the
    vocabulary ``V`` and the window's end ``hi`` (``_vocab_window``); ``constraints``: those that apply, None when they edit nothing
    (``_constrained``); ``n``: samples per prompt (best-of-n only); ``per_request``: the slots carry their own ``SamplingParams``; ``caps``:
    (max_bad_token_ids, max_logit_bias) of a stream whose slots carry their own constraints.  Two calls share a state iff their keys are equal."""
    rows: int
    cfg: object
    V: int
    hi: int
    constraints: Optional[DecodingConstraints] = None
    n: Optional[int] = None
    per_request: bool = False
    caps: Optional[Tuple[int, int]] = None
    kv_cache = "bf16"        # (no field: the key of the default ring is what it was; ``DecodeKeyFp8`` carries the other value)
    share_prompt = False     # (no field either: ``DecodeKeyShared`` carries the other value)
    speculative = None       # (nor this: ``DecodeKeySpec`` carries a plan)


@dataclass(frozen=True)
class DecodeKeyFp8(DecodeKey):
    """the key of a decoding state over an fp8 K/V ring (``kv_cache="fp8"``): ``kv_cache`` as the last field.  Keys of different classes
    never compare equal, so an fp8 generator and a bf16 one are never taken for each other.  Created by ``_with_kv_cache`` ONLY, which
    validates the model and the path first: a ``DecodeKeyFp8(kv_cache="bf16")`` built by hand would name the default ring and still never
    equal the plain key."""
    kv_cache: str = "fp8"


@dataclass(frozen=True)
class DecodeKeyShared(DecodeKey):
    """the key of a beam search or a best-of-n sampling whose rows share their group's prompt keys (``share_prompt=True``): a
    ``GroupedRingMemory`` instead of a ``RingMemory``.  A class of its own for the reason ``DecodeKeyFp8`` is one: the default keys compare
    equal to what they were, and a shared generator is never taken for a per-row one.  Created by ``_with_share_prompt`` ONLY."""
    share_prompt: bool = True


@dataclass(frozen=True)
class DecodeKeySpec(DecodeKey):
    """the key of a speculative ``generate`` (``speculative=``): the ``_SpecPlan`` and the K/V format as the last fields.  A class of its own
    for the reason ``DecodeKeyFp8`` is one: the default keys keep their fields and compare equal to what they were.  Created by
    ``_generate_speculative`` ONLY, after ``_with_kv_cache`` has validated the format."""
    speculative: Optional[_SpecPlan] = None
    kv_cache: str = "bf16"


def clip_at_eos(ids, lengths) -> List[List[int]]:
    """the tokens ``Decoder.decode(..., clip_at_eos=True)`` keeps (text_decoder.py:53-58), as id lists: row r's first ``lengths[r]`` ids"""
    ids = np.asarray(ids)
    return [[int(v) for v in row[:int(n)]] for row, n in zip(ids, np.asarray(lengths))]


# ------------------------------------------------------------------------------------ what generation and scoring share around a model call
@contextlib.contextmanager
def _eval_mode(model):
    """the model in eval mode; its mode is restored on the way out"""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


@contextlib.contextmanager
def _work(model):
    """device work between two yields of a stream: eval mode and no autograd, both restored before the caller's code runs again"""
    with torch.no_grad(), _eval_mode(model):
        yield


def _need_memory(model, who: str) -> int:
    mlen = int(model.mem_len or 0)
    if not mlen > 0:
        raise ValueError(f"{who} needs a model with memory (mem_len > 0)")
    return mlen


def _vocab_window(model, cfg) -> Tuple[int, int]:
    """(V, hi): the model's vocabulary and the end of the window ``[cfg.vocab_lo, cfg.vocab_hi)`` inside it (``vocab_hi`` None: V)"""
    V = int(model.total_vocab_size)
    hi = V if cfg.vocab_hi is None else int(cfg.vocab_hi)
    if hi > V:
        raise ValueError(f"vocabulary window [{cfg.vocab_lo}, {hi}) exceeds the model's vocabulary ({V})")
    if int(cfg.vocab_lo) >= V:
        raise ValueError(f"vocabulary window [{cfg.vocab_lo}, {cfg.vocab_hi}) is empty in a vocabulary of {V}")
    return V, hi


def _constrained(who: str, model, key: DecodeKey, constraints, limit: int) -> DecodeKey:
    """the state key ``key`` with ``constraints`` set -- unless they are None or edit nothing under this config
    (``DecodingConstraints.applies``): then the key itself, and with it the state, the launches and the cached generator, is exactly what
    it is without them.  Raises before anything is launched."""
    if constraints is None:
        return key
    if not isinstance(constraints, DecodingConstraints):
        raise TypeError(f"{who}: DecodingConstraints expected, got {type(constraints).__name__}")
    if constraints.min_new_tokens > int(limit):
        raise ValueError(f"{who}: min_new_tokens {constraints.min_new_tokens} exceeds max_new_tokens {limit}")
    if constraints.stop_sequences and who in ("beam_search", "sample_best_of"):
        raise ValueError(f"{who}: stop_sequences are not supported (beams and best-of-n rank whole hypotheses; use generate or a stream)")
    if not constraints.applies(key.cfg.eos_id):
        return key
    V, mx = key.V, key.cfg.max_new_tokens
    if not ops.constrain_logits_supported(V, V, mx, len(constraints.bad_token_ids), model.compute_dtype):
        raise ValueError(f"{who}: db1_constrain_logits does not support max_new_tokens {mx}")
    if constraints.edits_more and not ops.constrain_logits_pen_supported(V, V, mx, len(constraints.bad_token_ids), len(constraints.logit_bias),
                                                                         model.compute_dtype):
        raise ValueError(f"{who}: db1_constrain_logits_pen does not support {len(constraints.logit_bias)} biases")
    if constraints.stop_sequences and not ops.stop_match_supported(len(constraints.stop_sequences), mx):
        raise ValueError(f"{who}: db1_stop_match does not support {len(constraints.stop_sequences)} stop sequences")
    return dataclasses.replace(key, constraints=constraints)


def _constrain_args(cons: Optional[DecodingConstraints], cfg, V: int, dev) -> Optional[dict]:
    """the keyword arguments a state's ``ops.constrain_logits`` call takes from its constraints (the banned ids as a device vector, made
    once); None: no launch"""
    if cons is None or not cons.edits_logits(cfg.eos_id):
        return None
    eos = -1 if cfg.eos_id is None else int(cfg.eos_id)
    min_new = cons.min_new_tokens if eos >= 0 else 0
    bad = torch.tensor(cons.bad_token_ids, dtype=torch.int32).to(dev) if cons.bad_token_ids else None
    args = dict(V=V, repetition_penalty=cons.repetition_penalty, no_repeat_ngram_size=cons.no_repeat_ngram_size, bad=bad, eos_id=eos,
                min_new=min_new)
    if cons.edits_more:      # (only then does the call go to db1_constrain_logits_pen; the bias list is a device vector made once, as ``bad``)
        args.update(frequency_penalty=cons.frequency_penalty, presence_penalty=cons.presence_penalty)
        if cons.logit_bias:
            args.update(bias_ids=torch.tensor([k for k, _ in cons.logit_bias], dtype=torch.int32).to(dev),
                        bias_val=torch.tensor([b for _, b in cons.logit_bias], dtype=torch.float32).to(dev))
    return args


def _stop_args(cons: Optional[DecodingConstraints], cfg, dev, lp_top: dict) -> Optional[dict]:
    """the arguments a state's ``ops.stop_match`` call takes from its constraints (the packed sequences as device tensors, made once) and
    its log-prob / top-n outputs ``lp_top``; None: no stop sequences, no launch and no buffers"""
    if cons is None or not cons.stop_sequences:
        return None
    tok, n = ops.pack_stop_sequences(cons.stop_sequences)
    return dict(stop_tok=torch.from_numpy(tok).to(dev), stop_len=torch.from_numpy(n).to(dev), pad_id=int(cfg.pad_id), **lp_top)


def _text_window(model, cfg):
    """``cfg`` (a GenerationConfig, BeamSearchConfig or ScoreConfig) with the text vocabulary as its window's end unless it names one"""
    return cfg if cfg.vocab_hi is not None else dataclasses.replace(cfg, vocab_hi=int(model.text_vocab_size))


def _batch_size(prompt, prefixed_ok: bool = False) -> int:
    kind = type(prompt).__name__
    if isinstance(prompt, Prefixed):
        if not prefixed_ok:
            raise ValueError("a Prefixed prompt continues a PrefixCache row on the K/V ring: generate, beam_search, sample_best_of and the streams "
                             "take it; rank_candidates and score_document do not")
        return len(prompt.handles)
    if kind == "NLPTaskInput":
        seq = prompt.text_seq
        lens = getattr(prompt, "text_len", None)
        if lens is not None and np.unique(np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)).size > 1:
            raise ValueError("generate: the rows of a prompt batch must share one length (group prompts by length)")
    elif kind in ("ICTaskInput", "VQATaskInput"):
        seq = prompt.prompt_seq
    else:
        raise TypeError(f"generate: NLPTaskInput, ICTaskInput or VQATaskInput expected, got {kind}")
    try:
        arr = seq if torch.is_tensor(seq) else np.asarray(seq)
    except ValueError as e:
        raise ValueError("generate: the rows of a prompt batch must share one length (group prompts by length)") from e
    if arr.ndim != 2 or arr.dtype == object:
        raise ValueError("generate: the prompt ids must form a [batch, length] array (rows of one length)")
    return int(arr.shape[0])


# the fields of a prompt batch that hold one entry per row (first dimension = the batch); every other field is handed on as it is
_PER_ROW_FIELDS = ("position_id", "attention_mask", "loss_mask", "label", "text_seq", "text_len", "prompt_seq", "img_seq", "img_id_seq",
                   "ques_id_seq", "ques_len")
# attributes next to the dataclass fields: one id per patch, image after image
_PATCH_FIELDS = ("vision_row_ids", "vision_col_ids")


def _take(prompt, name: str, G: int, rows):
    """rows ``rows`` of field ``name`` of a prompt batch of G rows: a per-row field is index-selected, a per-patch field row block by row
    block, anything else (and None) is handed on as it is; ``rows`` None: the whole field, as it is"""
    v = getattr(prompt, name, None)
    if v is None or rows is None or not (name in _PER_ROW_FIELDS or name in _PATCH_FIELDS):
        return v
    v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=v.device)
    if name in _PATCH_FIELDS:
        if G == 0 or v.numel() % G:
            raise ValueError(f"generate_stream: {name} holds {v.numel()} ids for a batch of {G} rows")
        return v.reshape(G, -1).index_select(0, idx).reshape(-1)
    if v.dim() < 1 or v.shape[0] != G:
        raise ValueError(f"generate_stream: {name} of shape {tuple(v.shape)} in a batch of {G} rows")
    return v.index_select(0, idx)


def _carry_patch_ids(src, dst, rows=None):
    """the patch ids of the prompt batch ``src`` carried over to ``dst`` (returned): as they are, or those of ``src``'s rows ``rows``"""
    G = None if rows is None else _batch_size(src)
    for f in _PATCH_FIELDS:
        if hasattr(src, f):
            setattr(dst, f, _take(src, f, G, rows))
    return dst


def _questions(vqa_batch):
    """(``text_seq`` as a tensor, ``ques_len`` as a flat int64 array or None) of a ``VQATaskInput`` batch"""
    q = vqa_batch.text_seq
    q = q if torch.is_tensor(q) else torch.as_tensor(np.asarray(q))
    ql = getattr(vqa_batch, "ques_len", None)
    return q, None if ql is None else np.asarray(torch.as_tensor(ql).cpu()).reshape(-1).astype(np.int64)


def _question_rows(vqa_batch, q, n: Optional[int], rows=None):
    """the prompt ``[prompt, image patches, question]`` of a ``VQATaskInput`` batch (of its rows ``rows``, if given): the question is the
    first ``n`` tokens of ``q``, the batch's ``text_seq`` (``n`` None: all of it)"""
    from .data import VQATaskInput
    G = None if rows is None else _batch_size(vqa_batch)
    take = lambda f: _take(vqa_batch, f, G, rows)
    q = q if rows is None else take("text_seq")
    x = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=take("prompt_seq"), img_seq=take("img_seq"),
                     text_seq=q if n is None else q[:, :n])
    return _carry_patch_ids(vqa_batch, x, rows)


def _prefill(model, prompt, G: int, expand: Optional[int] = None):
    """the prompt (G rows) once through the list-form memory path -> (logits [G, L, V], the new memory); ``expand`` given: every row of the
    memory repeated ``expand``-fold (rows g * expand .. of the result descend from prompt g)"""
    model._dec_state = None
    logits, _, mems = model([prompt], compute_loss=False, mems=model.init_mem(G))
    if expand is not None:
        mems = [m.repeat_interleave(expand, 0) for m in mems]
    return logits, mems


def _use_ring_prefill(model) -> bool:
    """``model.use_ring_prefill`` on a model that supports it (an unsupported model with the flag set keeps the list-form prefill)"""
    return bool(getattr(model, "use_ring_prefill", False)) and bool(getattr(model, "ring_prefill_supported", False))


def _prefill_ring(model, prompt, ring, rows=None, expand: Optional[int] = None):
    """the prompt once, straight into ``ring`` (``decode.RingPrefill``): only its own tokens are projected and every layer's last mem_len keys /
    values go to ring rows ``rows`` (int32 device vector; None: all rows) relative to the ring's current origin -> logits [G, L, V].
    ``expand`` given: ring row r descends from prompt r // expand -- nothing is repeated or projected twice."""
    src = None if expand is None else torch.arange(ring.B if rows is None else int(rows.numel()), dtype=torch.int32, device=model.dev) // int(expand)
    if isinstance(prompt, Prefixed):     # the suffix continues cache rows: ``src`` maps destinations to call rows, ``base_rows`` call rows to cache rows
        base_rows = torch.tensor(prompt.cache.rows_of(prompt.handles), dtype=torch.int32).to(model.dev)
        logits, _, _ = model([prompt.suffix], compute_loss=False, mems=RingPrefill(ring, rows, src, prompt.cache.ring, base_rows))
        return logits
    logits, _, _ = model([prompt], compute_loss=False, mems=RingPrefill(ring, rows, src))
    return logits


# ------------------------------------------------------------------------------------------------------------------------------ prefix cache
@dataclass(frozen=True)
class PrefixHandle:
    """one cached prefix: row ``row`` of its cache's ring, as ``put`` number ``serial`` wrote it under weight version ``version``"""
    row: int
    serial: int
    version: int


class PrefixCache:
    """Prefill a shared prompt ONCE and continue it per request: a ``RingMemory`` of ``rows`` rows (``kv_cache`` "bf16" or "fp8") whose
    origin stays 0, and a free list of its rows (plain Python).  ``put(prompt)`` prefills a batch of G prompts from the zero memory into G
    free rows (the ring prefill, db1_ring_prefill_rows) and returns their handles; ``Prefixed(cache, handles, suffix)`` is then a prompt
    for ``generate``, ``beam_search``, ``sample_best_of`` and the streams: only the suffix is embedded and projected, its attention reads
    the prefix in the cache's slots (db1_relattn_mem_ring_fwd) and db1_ring_fork_rows forks (the cache row, the suffix) into the request's
    own ring row -- the cache is only read, so any number of requests, at once or one after another, may share one handle.  Segment-level
    recurrence makes this exact for the model: a position's keys and values depend on earlier positions only, so a cache row holds what a
    list-form call with ``mems=`` would re-project.  ``release(handles)`` returns rows to the free list; a handle from before a weight
    change (``model._wversion``), or a released one, raises RuntimeError when used."""

    def __init__(self, model, rows: int, kv_cache: str = "bf16"):
        if kv_cache not in ("bf16", "fp8"):
            raise ValueError(f"PrefixCache: kv_cache must be 'bf16' or 'fp8' (got {kv_cache!r})")
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or int(rows) < 1:
            raise ValueError(f"PrefixCache: rows {rows!r} must be a positive integer")
        if not getattr(model, "ring_prefill_supported", False):
            raise ValueError("PrefixCache needs the ring prefill (model.ring_prefill_supported: bf16, use_decode, d_head 128, post-LN layers, mem_len > 0)")
        self.model, self.rows, self.kv_cache = model, int(rows), kv_cache
        self._free = list(range(self.rows))
        self._live = {}                 # row -> the handle that holds it
        self._serial = 0
        self._ring = None               # (allocated by the first ``put``)

    @property
    def ring(self) -> RingMemory:
        if self._ring is None:
            self._ring = RingMemory(self.model, self.rows, kv_dtype=self.kv_cache)
        return self._ring

    @property
    def free(self) -> int:
        """the number of free rows"""
        return len(self._free)

    def _take(self, G: int) -> List[PrefixHandle]:
        """G free rows (the lowest first) as new handles; RuntimeError when fewer are free (nothing is taken then)"""
        if G > len(self._free):
            raise RuntimeError(f"PrefixCache: {G} prompts for {len(self._free)} free rows (of {self.rows}): release some handles")
        rows, self._free = self._free[:G], self._free[G:]
        out = []
        for r in rows:
            self._serial += 1
            out.append(PrefixHandle(row=r, serial=self._serial, version=int(self.model._wversion)))
            self._live[r] = out[-1]
        return out

    def rows_of(self, handles) -> List[int]:
        """the cache rows of ``handles`` (repeats allowed); RuntimeError for a released handle or one from before a weight change"""
        out = []
        for h in handles:
            if not isinstance(h, PrefixHandle):
                raise ValueError(f"PrefixCache: a handle returned by put() expected, got {type(h).__name__}")
            if self._live.get(h.row) != h:
                raise RuntimeError(f"PrefixCache: the handle of row {h.row} was released (or belongs to another cache)")
            if h.version != int(self.model._wversion):
                raise RuntimeError("PrefixCache: the weights changed after the prefix was cached: release the handle and put the prompt again")
            out.append(h.row)
        return out

    def release(self, handles):
        """the rows of ``handles`` become free again (each handle once); their contents stay until a later ``put`` overwrites them"""
        handles = list(handles)
        for h in handles:
            if not isinstance(h, PrefixHandle) or self._live.get(h.row) != h:
                raise RuntimeError("PrefixCache.release: a handle that is not live in this cache")
        if len({h.row for h in handles}) != len(handles):
            raise RuntimeError("PrefixCache.release: a handle given twice")
        for h in handles:
            del self._live[h.row]
            self._free.append(h.row)
        self._free.sort()

    @torch.no_grad()
    def put(self, prompt) -> List[PrefixHandle]:
        """prefill ``prompt`` (ONE batch of G rows of one shape, as ``generate`` takes it) from the zero memory into G free rows -> their
        handles, in row order of the batch.  The existing ring prefill, whatever ``model.use_ring_prefill`` says."""
        G = _batch_size(prompt)
        if not self.model.ring_prefill_supported:
            raise ValueError("PrefixCache.put: the model no longer supports the ring prefill")
        handles = self._take(G)
        try:
            ring = self.ring
            with _eval_mode(self.model):
                ring.load_status.zero_()
                _prefill_ring(self.model, prompt, ring, torch.tensor([h.row for h in handles], dtype=torch.int32).to(self.model.dev))
                if int(ring.load_status.cpu()) != 0:
                    raise RuntimeError("db1_ring_prefill_rows: the prefill skipped a cache row")
        except BaseException:
            self.release(handles)
            raise
        return handles


class Prefixed:
    """A prompt that continues cached prefixes: row g is (the prefix behind ``handles[g]``, row g of ``suffix``).  ``suffix``: an
    ``NLPTaskInput`` batch [G, Ls], Ls >= 1, embedded exactly as NLP text; ``handles``: G handles of ``cache`` -- repeats are the point."""

    def __init__(self, cache: PrefixCache, handles, suffix):
        if not isinstance(cache, PrefixCache):
            raise ValueError(f"Prefixed: a PrefixCache expected, got {type(cache).__name__}")
        if type(suffix).__name__ != "NLPTaskInput":
            raise ValueError(f"Prefixed: the suffix must be an NLPTaskInput batch, got {type(suffix).__name__}")
        G = _batch_size(suffix)
        seq = suffix.text_seq
        if int((seq if torch.is_tensor(seq) else np.asarray(seq)).shape[1]) < 1:
            raise ValueError("Prefixed: the suffix must hold at least one token per row (Ls >= 1)")
        handles = list(handles)
        if len(handles) != G:
            raise ValueError(f"Prefixed: {len(handles)} handles for a suffix batch of {G} rows")
        cache.rows_of(handles)
        self.cache, self.handles, self.suffix = cache, handles, suffix

    @property
    def suffix_len(self) -> int:
        seq = self.suffix.text_seq
        return int((seq if torch.is_tensor(seq) else np.asarray(seq)).shape[1])


def _check_prompt(who: str, model, prompt, kv_cache: str, graphed: Optional[bool]):
    """a ``Prefixed`` prompt needs the ring path of the cache's own model and K/V format: ValueError before anything is launched"""
    if not isinstance(prompt, Prefixed):
        return
    if prompt.cache.model is not model:
        raise ValueError(f"{who}: the Prefixed prompt's cache belongs to another model")
    if graphed is False or not _ring_ok(model) or not getattr(model, "ring_prefill_supported", False):
        raise ValueError(f"{who}: a Prefixed prompt needs the ring path (a bf16 model with use_decode, d_head 128, post-LN layers and mem_len > 0; "
                         f"not graphed=False)")
    if prompt.cache.kv_cache != kv_cache:
        raise ValueError(f"{who}: kv_cache={kv_cache!r} over a PrefixCache of kv_cache={prompt.cache.kv_cache!r}")
    if not model.ring_prefill_ok(prompt.suffix_len):
        raise ValueError(f"{who}: a suffix of {prompt.suffix_len} tokens is not supported by the ring prefill")
    prompt.cache.rows_of(prompt.handles)


def _check_chain(model):
    """raise what the hand-off chain of the eager decode launches recorded, if anything"""
    chk = getattr(model, "check_decode_chain", None)
    if chk is not None:
        chk(True)


def _ring_ok(model) -> bool:
    return (model.compute_dtype == torch.bfloat16 and bool(model.use_decode) and int(model.mem_len or 0) > 0 and model.d_head == 128)


def _with_kv_cache(who: str, model, key: DecodeKey, kv_cache: str, graphed: Optional[bool] = None) -> DecodeKey:
    """``key`` for the K/V ring format ``kv_cache``: "bf16" -- the key itself; "fp8" -- a ``DecodeKeyFp8`` of the same fields, for a call that
    takes the ring path on a model the fp8 attention supports.  Raises ValueError before anything is launched."""
    if kv_cache == "bf16":
        return key
    if kv_cache != "fp8":
        raise ValueError(f"{who}: kv_cache must be 'bf16' or 'fp8' (got {kv_cache!r})")
    if graphed is False or not _ring_ok(model):
        raise ValueError(f"{who}: kv_cache='fp8' needs the ring path (a bf16 model with use_decode, d_head 128 and mem_len > 0; not graphed=False)")
    if not ops.relattn_decode_ring_kv8_supported(1, 1, int(model.mem_len) + 1, model.n_head, model.d_head):
        raise ValueError(f"{who}: kv_cache='fp8' needs an even number of heads and mem_len <= 2047 (n_head {model.n_head}, mem_len {model.mem_len})")
    return DecodeKeyFp8(**{f.name: getattr(key, f.name) for f in dataclasses.fields(key)})


def _with_share_prompt(who: str, model, key: DecodeKey, share_prompt: bool, W: int, prompt, kv_cache: str, graphed: Optional[bool] = None) -> DecodeKey:
    """``key`` for a call whose W rows per prompt share the prompt's keys / values: False -- the key itself; True -- a ``DecodeKeyShared`` of
    the same fields, for a call that takes the graphed bf16 ring path on a model db1_relattn_decode_group_fwd supports.  Raises ValueError
    before anything is launched."""
    if not share_prompt:
        return key
    if model.compute_dtype != torch.bfloat16 or not _ring_ok(model):
        raise ValueError(f"{who}: share_prompt=True needs the ring path (a bf16 model with use_decode, d_head 128 and mem_len > 0)")
    if graphed is False:
        raise ValueError(f"{who}: share_prompt=True needs the graphed ring path (not graphed=False)")
    if kv_cache != "bf16":
        raise ValueError(f"{who}: share_prompt=True keeps bf16 keys / values (kv_cache={kv_cache!r} is not supported)")
    if isinstance(prompt, Prefixed):
        raise ValueError(f"{who}: share_prompt=True does not take a Prefixed prompt (the prefix cache's continuations have rows of their own)")
    mlen, mx = int(model.mem_len), int(key.cfg.max_new_tokens)
    if mx > mlen:
        raise ValueError(f"{who}: share_prompt=True with max_new_tokens {mx} above the model's mem_len {mlen}")
    if key.rows * int(W) < 2:
        raise ValueError(f"{who}: share_prompt=True over one row (G = W = 1) has nothing to share")
    if not ops.relattn_decode_group_supported(key.rows, W, mlen, mx, mlen + 64, mx + 1, model.n_head, model.d_head, model.compute_dtype):
        raise ValueError(f"{who}: share_prompt=True is not supported for this model (db1_relattn_decode_group_supported: 1 <= W <= {ops.GROUP_MAX_W}, "
                         f"mem_len <= {ops.GROUP_MAX_KLEN - 1}, max_new_tokens <= {ops.GROUP_MAX_TAIL}; W = {W}, mem_len = {mlen}, max_new_tokens = {mx})")
    return DecodeKeyShared(**{f.name: getattr(key, f.name) for f in dataclasses.fields(key)})


# ----------------------------------------------------------------------------------------------------------------------- the device states
# What ``_decode`` asks of a state: ``M`` rows, ``expand`` (None, or the rows per prompt), ``cache`` (the model attribute its ring generator
# is kept under), ``start(...)``, ``epilogue(logits_last, next_ids, ring=None)`` -- select, reorder ``ring`` if beams, then t += 1 --,
# ``reorder_list(mems, old)``, ``all_done()`` (a host read), ``result()`` and ``stats()``; ``width`` (default 1): the tokens per row of a
# token call -- a wider state's epilogue takes the logits of all positions [M * width, V] and the whole input ids [M, width].  The stream (serving.py) asks its ``_SlotState`` for
# ``M``, ``expand``, ``cache``, ``start()`` and ``epilogue``.
_no_launch = lambda *args, **kw: None      # the step of an epilogue that has nothing to do


class _SamplingState:
    """what the two sampling states (``_State``, serving's ``_SlotState``) share: ``counters`` token counters ``t``, the per-row flags, stream
    ids and output, all zero / pad_id; with ``cfg.logprobs`` the tokens' log-probs ``logprob`` [M, max_new_tokens] and their per-row sum
    ``sum_logprob``; with ``cfg.top_logprobs`` n the alternatives ``top_ids`` / ``top_logprob`` [M, max_new_tokens, n], -1 / -inf where
    nothing was written (each None when off).  ``lp_top``: those outputs as keywords; ``sel``: the keywords of the ``ops.select_*`` call.
    An epilogue is constrain -> select -> stop.  Each step is bound ONCE, here, to its launch and its buffers (``_constrain`` / ``_stop``
    from ``cons``, ``_pick`` by the subclass) or to ``_no_launch``; ``con`` / ``stop`` are the launch's keywords, None for no launch."""
    expand = None

    def __init__(self, model, key: DecodeKey, M: int, counters: int, cons: Optional[DecodingConstraints]):
        cfg, V = key.cfg, key.V
        self.i32 = i32 = dict(dtype=torch.int32, device=model.dev)
        self.M, self.cfg, self.V, self.hi, self.dev = M, cfg, V, key.hi, model.dev
        self.t = torch.zeros(counters, **i32)
        self.finished, self.lengths, self.status, self.stream_id = (torch.zeros(M, **i32) for _ in range(4))
        self.out = torch.full((M, cfg.max_new_tokens), cfg.pad_id, **i32)
        self.lp_top = {}
        self.logprob = self.sum_logprob = None
        if cfg.logprobs:
            self.logprob = torch.zeros(M, cfg.max_new_tokens, dtype=torch.float32, device=model.dev)
            self.sum_logprob = torch.zeros(M, dtype=torch.float32, device=model.dev)
            self.lp_top.update(logprob=self.logprob, sum_logprob=self.sum_logprob)
        self.top_ids = self.top_logprob = None
        if cfg.top_logprobs:
            n = int(cfg.top_logprobs)
            self.top_ids = torch.full((M, cfg.max_new_tokens, n), -1, **i32)
            self.top_logprob = torch.full((M, cfg.max_new_tokens, n), float("-inf"), dtype=torch.float32, device=model.dev)
            self.lp_top.update(top_n=n, top_ids=self.top_ids, top_logprob=self.top_logprob)
        self.sel_shared = dict(V=V, eos_id=-1 if cfg.eos_id is None else cfg.eos_id, pad_id=cfg.pad_id, stream_id=self.stream_id, **self.lp_top)
        self.sel = dict(self.sel_shared, vocab_lo=cfg.vocab_lo, vocab_hi=key.hi, greedy=cfg.greedy, temperature=cfg.temperature, top_k=cfg.top_k,
                        top_p=cfg.top_p, seed=cfg.seed)
        self.con = _constrain_args(cons, cfg, V, model.dev)
        self._constrain = _no_launch if self.con is None else partial(ops.constrain_logits, t=self.t, hist=self.out, finished=self.finished, **self.con)
        # stop sequences: the packed lists and two more vectors per row, only when there are any
        self.stop = _stop_args(cons, cfg, model.dev, self.lp_top)
        self.checked, self.stop_hit, self._stop = None, None, _no_launch
        if self.stop is not None:
            self.checked, self.stop_hit = torch.zeros(M, **i32), torch.zeros(M, **i32)
            self._stop = partial(ops.stop_match, lengths=self.lengths, checked=self.checked, finished=self.finished, stop_hit=self.stop_hit,
                                 out=self.out, **self.stop)

    def stop_match(self, next_ids, row_map=None):
        """the stop sequences, after the selection: rows whose output now ends in one lose it and end (none configured: no launch)"""
        self._stop(next_ids=next_ids, row_map=row_map)

    def clear_top(self, idx=None):
        """-1 / -inf into the alternatives of every row (``idx``: int64 device vector, of those rows): nothing written yet"""
        if self.top_ids is not None:
            if idx is None:
                self.top_ids.fill_(-1)
                self.top_logprob.fill_(float("-inf"))
            else:
                self.top_ids.index_fill_(0, idx, -1)
                self.top_logprob.index_fill_(0, idx, float("-inf"))

    def constrain(self, logits2d, row_map=None):
        """the decoding constraints, in place on the step's logits, over every row's own output so far (no constraints: no launch)"""
        self._constrain(logits2d, row_map=row_map)


class _State(_SamplingState):
    """the device state of one generation: token counter, per-row flags, the output and the stream ids"""
    cache = "_generator"
    width = 1

    def __init__(self, model, key: DecodeKey):
        M = key.rows if key.n is None else key.rows * key.n      # (best-of-n: n rows per prompt)
        super().__init__(model, key, M, 1, key.constraints)
        self._pick = partial(ops.select_tokens, t=self.t, finished=self.finished, lengths=self.lengths, out=self.out, status=self.status, **self.sel)
        self.stream_id.copy_(torch.arange(M, dtype=torch.int32))

    def start(self, stream_ids=None):
        for x in (self.t, self.finished, self.lengths, self.status) + (() if self.stop is None else (self.checked, self.stop_hit)):
            x.zero_()
        self.out.fill_(self.cfg.pad_id)
        if self.logprob is not None:
            self.logprob.zero_()
            self.sum_logprob.zero_()
        self.clear_top()
        if stream_ids is None:
            self.stream_id.copy_(torch.arange(self.M, dtype=torch.int32))
        else:
            s = torch.as_tensor(np.asarray(stream_ids, dtype=np.int64))
            if s.shape != (self.M,):
                raise ValueError(f"stream_ids: {self.M} values expected, got shape {tuple(s.shape)}")
            self.stream_id.copy_(s.to(torch.int32))

    def select(self, logits2d, next_ids):
        """db1_select_tokens on the last-position logits [M, V] of step t; the tokens go to ``next_ids`` (int64 [M])"""
        self._pick(logits2d, next_ids=next_ids)

    def epilogue(self, logits2d, next_ids, ring=None):
        self.constrain(logits2d)
        self.select(logits2d, next_ids)
        self.stop_match(next_ids)
        self.t.add_(1)

    def reorder_list(self, mems, old=None):
        return mems

    def all_done(self) -> bool:
        return bool(self.finished.all())

    def result(self):
        out, lengths, status = self.out.cpu(), self.lengths.cpu(), self.status.cpu()
        if (status & 2).any():
            raise RuntimeError("db1_select_tokens: the token counter left [0, max_new_tokens)")
        if self.logprob is not None:
            top = () if self.top_ids is None else (self.top_ids.cpu(), self.top_logprob.cpu())
            return (out, lengths, self.logprob.cpu(), self.sum_logprob.cpu()) + top
        return out, lengths

    def stats(self) -> dict:
        """``stop_hits`` (with stop sequences only): per row 0, or the index + 1 of the sequence that ended it"""
        return {} if self.stop is None else dict(stop_hits=[int(v) for v in self.stop_hit.cpu()])


class _BestOfState(_State):
    """``_State`` over the G * n rows of a best-of-n sampling: every prompt's prefill expanded n-fold (rows g * n .. g * n + n - 1), the
    log-probs always on; ``result`` adds the status, which the ranking needs"""
    cache = "_best_of_generator"

    def __init__(self, model, key: DecodeKey):
        super().__init__(model, key)
        self.G, self.expand = key.rows, key.n

    def result(self):
        return super().result() + (self.status.cpu(),)


class _SpecState(_State):
    """``_State`` for speculative decoding (``SpeculativeConfig``; include/db1_hip.h, db1_spec_pick / _accept / _commit): a token call
    carries ``width`` Q = 1 + k tokens per row, and the epilogue is the three launches -- pick every position's token, accept the run the
    drafts allow (the books, the next input ids and the next drafts), commit (``t += n_acc``, the ring's origin back over what was not
    kept).  The outputs and ``result()`` are ``_State``'s.  Next to its buffers: the scratch ``sel`` / ``hit`` / ``lp`` [M, Q], ``n_acc`` [1],
    ``hist`` [Q + 1] (steps by accepted count), the prompt's text ``ctx`` [M, ctx_cap] / ``ctx_len`` [M] and the draft ``script`` [M, max_new]."""
    cache = "_spec_generator"

    def __init__(self, model, key: DecodeKey):
        super().__init__(model, key)
        plan, cfg, i32, dev = key.speculative, key.cfg, self.i32, model.dev
        sc = plan.config
        self.width = Q = 1 + sc.num_draft_tokens
        M, mx = self.M, int(cfg.max_new_tokens)
        self.spec_sel, self.spec_hit = torch.zeros(M, Q, **i32), torch.zeros(M, Q, **i32)
        self.spec_lp = torch.zeros(M, Q, dtype=torch.float32, device=dev) if cfg.logprobs else None
        self.n_acc, self.hist = torch.zeros(1, **i32), torch.zeros(Q + 1, **i32)
        self.ctx = torch.zeros(M, plan.ctx_cap, **i32) if plan.ctx_cap else None
        self.ctx_len = torch.zeros(M, **i32) if plan.ctx_cap else None
        self.script = torch.zeros(M, mx, **i32) if plan.scripted else None
        self._mem_idx = None
        self._pick = partial(ops.spec_pick, t=self.t, finished=self.finished, sel=self.spec_sel, hit=self.spec_hit, lp=self.spec_lp, max_new=mx,
                             V=self.V, vocab_lo=cfg.vocab_lo, vocab_hi=key.hi, greedy=cfg.greedy, temperature=cfg.temperature, top_k=cfg.top_k,
                             top_p=cfg.top_p, seed=cfg.seed, pad_id=cfg.pad_id, stream_id=self.stream_id)
        self._accept = partial(ops.spec_accept, self.t, self.spec_sel, self.spec_hit, self.finished, self.lengths, self.out, self.status,
                               n_acc=self.n_acc, V=self.V, eos_id=-1 if cfg.eos_id is None else cfg.eos_id, pad_id=cfg.pad_id, lp=self.spec_lp,
                               logprob=self.logprob, sum_logprob=self.sum_logprob, ctx=self.ctx, ctx_len=self.ctx_len, script=self.script,
                               ngram_min=sc.ngram_min, ngram_max=sc.ngram_max)

    def start(self, stream_ids=None, ctx=None, script=None):
        """``ctx``: the prompt's text tokens (int array [M, L]) or None; ``script``: the draft script (int32 array [M, max_new]) or None"""
        super().start(stream_ids)
        self.n_acc.zero_()
        self.hist.zero_()
        if self.ctx is not None:
            self.ctx_len.zero_()
            if ctx is not None and ctx.shape[1]:
                self.ctx[:, :ctx.shape[1]].copy_(torch.as_tensor(np.ascontiguousarray(ctx, dtype=np.int32)))
                self.ctx_len.fill_(int(ctx.shape[1]))
        if self.script is not None:
            self.script.copy_(torch.as_tensor(np.ascontiguousarray(script, dtype=np.int32)))

    def epilogue(self, logits2d, ids, ring=None):
        """``logits2d`` [M * q_in, V]: q_in = 1 after the prefill (token 0: nothing to verify, nothing to take back, not counted), else Q;
        ``ids`` int64 [M, Q]: the step's input, rewritten for the next one"""
        q_in = logits2d.shape[0] // self.M
        self._pick(logits2d, ids=ids, q_in=q_in)
        self._accept(ids, q_in=q_in)
        ops.spec_commit(self.t, self.n_acc, q_in=q_in, Q=self.width, hist=self.hist if q_in > 1 else None,
                        ring_state=None if ring is None else ring.state, cap=0 if ring is None else ring.cap)

    def reorder_list(self, mems, old=None):
        """the list-form memory after a call of Q tokens of which n_acc were kept: rows [n_acc, n_acc + mem_len) of cat(old[:, :Q], returned)
        per layer -- the old memory without its n_acc oldest rows, then the kept tokens' hidden states; the index is a device tensor"""
        Q, mlen = self.width, int(mems[0].shape[1])
        if self._mem_idx is None or self._mem_idx.numel() != mlen:
            self._mem_idx = torch.arange(mlen, dtype=torch.long, device=self.dev)
        idx = self._mem_idx + self.n_acc.long()
        return [torch.cat([o[:, :Q].to(m.dtype), m], 1).index_select(1, idx) for o, m in zip(old, mems)]

    def all_done(self) -> bool:
        """also notes ``left``, the tokens still to come, from which ``_decode`` works out its next look"""
        self.left = int(self.cfg.max_new_tokens) - int(self.t)
        return self.left <= 0 or bool(self.finished.all())

    def result(self):
        if (self.status.cpu() & 2).any():
            raise RuntimeError("db1_spec_accept: the token counter left [0, max_new_tokens]")
        return super().result()

    def stats(self) -> dict:
        """``accepted``: per accepted count 0 .. Q the number of token calls that committed that many tokens; ``tokens_per_call``"""
        hist = [int(v) for v in self.hist.cpu()]
        calls = sum(hist)
        return dict(super().stats(), accepted=hist, tokens_per_call=(sum(i * n for i, n in enumerate(hist)) / calls) if calls else 0.0)


class _BeamState:
    """the device state of one beam search over G prompts of W beams (include/db1_hip.h, db1_beam_step); with ``cfg.num_beam_groups`` D > 1
    the state of G * D sub-groups of W / D beams, stepped by db1_beam_step_diverse"""
    cache = "_beam_generator"
    width = 1

    def __init__(self, model, key: DecodeKey):
        G, cfg, V, hi, dev = key.rows, key.cfg, key.V, key.hi, model.dev
        W, mx, D = int(cfg.num_beams), int(cfg.max_new_tokens), int(cfg.num_beam_groups)
        Q, Wg = G * D, W // D                    # (D = 1: the G groups of W beams of the plain search)
        i32 = dict(dtype=torch.int32, device=dev)
        self.G, self.W, self.M, self.cfg, self.V, self.hi = G, W, G * W, cfg, V, hi
        self.D, self.Q, self.Wg = D, Q, Wg
        self.expand = W
        self.t = torch.zeros(1, **i32)
        self.beam_score = torch.zeros(G * W, dtype=torch.float32, device=dev)
        self.parent = torch.zeros(G * W, **i32)
        self.tokens = torch.zeros(G * W, mx, **i32)
        self.pool_tokens = torch.zeros(Q, Wg, mx, **i32)
        self.pool_len = torch.zeros(Q, Wg, **i32)
        self.pool_score = torch.zeros(Q, Wg, dtype=torch.float32, device=dev)
        self.pool_slot = torch.zeros(Q, Wg, **i32)
        self.pool_count = torch.zeros(Q, **i32)
        self.done = torch.zeros(Q, **i32)
        self.switches = torch.zeros(Q, **i32)
        self.status = torch.zeros(Q, **i32)
        self.con = _constrain_args(key.constraints, cfg, V, dev)
        # the step, bound ONCE: db1_beam_step, or with sub-groups db1_beam_step_diverse
        kw = dict(W=Wg, V=V, vocab_lo=cfg.vocab_lo, vocab_hi=hi, eos_id=-1 if cfg.eos_id is None else cfg.eos_id, pad_id=cfg.pad_id,
                  length_penalty=cfg.length_penalty)
        self._step = partial(ops.beam_step, **kw) if D == 1 else \
            partial(ops.beam_step_diverse, D=D, diversity_penalty=float(cfg.diversity_penalty), **kw)

    def start(self):
        pad = self.cfg.pad_id
        for x in (self.t, self.beam_score, self.pool_len, self.pool_count, self.done, self.switches, self.status):
            x.zero_()
        self.parent.copy_(torch.arange(self.M, dtype=torch.int32))
        self.tokens.fill_(pad)
        self.pool_tokens.fill_(pad)
        self.pool_score.fill_(float("-inf"))
        self.pool_slot.copy_(torch.arange(self.Wg, dtype=torch.int32).expand(self.Q, self.Wg))

    def select(self, logits2d, next_ids):
        """db1_beam_step (db1_beam_step_diverse) on the last-position logits [M, V] of step t; the next ids go to ``next_ids`` (int64 [M])"""
        if self.con is not None:     # (``tokens``: db1_beam_step has reordered it into every new beam's own history)
            ops.constrain_logits(logits2d, self.t, self.tokens, **self.con)
        self._step(logits2d, self.t, self.beam_score, self.parent, self.tokens, self.pool_tokens, self.pool_len, self.pool_score, self.pool_slot,
                   self.pool_count, self.done, self.switches, next_ids, self.status)

    def epilogue(self, logits2d, next_ids, ring=None):
        """``ring`` None: step 0 (every beam descends from the same prefill, nothing to reorder), or the list-form memory (``reorder_list``)"""
        self.select(logits2d, next_ids)
        if ring is not None:
            ring.reorder(self.parent, self.t, max_t=self.cfg.max_new_tokens, group=self.Wg, done=self.done)
        self.t.add_(1)

    def reorder_list(self, mems, old=None):
        parent = self.parent.long()
        return [m.index_select(0, parent) for m in mems]

    def all_done(self) -> bool:
        return bool(self.done.all())

    def result(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if (self.status.cpu() & 2).any():
            raise RuntimeError("db1_beam_step: the token counter left [0, max_new_tokens)")
        R, mx = int(self.cfg.num_return_sequences), int(self.cfg.max_new_tokens)
        toks, slot, n, sc, count = (x.cpu() for x in (self.pool_tokens, self.pool_slot, self.pool_len, self.pool_score, self.pool_count))
        ids = torch.full((self.G, R, mx), self.cfg.pad_id, dtype=torch.int32)
        lengths = torch.zeros(self.G, R, dtype=torch.int32)
        scores = torch.full((self.G, R), float("-inf"), dtype=torch.float32)
        # step 8 of the diverse rule: a prompt's D pools merged by (score descending, sub-group ascending, position in its pool ascending),
        # the first R (fewer only when its beams ran out of candidates).  D = 1: the pool's own order -- it is sorted, and on equal scores
        # the earlier offer stays ahead
        for g, ent in enumerate(self._merge_order(sc, count)):
            for r, (d, k) in enumerate(ent):
                q = g * self.D + d
                ids[g, r] = toks[q, int(slot[q, k])]
                lengths[g, r] = n[q, k]
                scores[g, r] = sc[q, k]
        return ids, lengths, scores

    def _merge_order(self, sc, count):
        """per prompt the (sub-group, pool position) of its first R merged results (``sc`` [G D, W'] / ``count`` [G D] on the host)"""
        D, R = self.D, int(self.cfg.num_return_sequences)
        out = []
        for g in range(self.G):
            ent = sorted((-float(sc[g * D + d, k]), d, k) for d in range(D) for k in range(int(count[g * D + d])))
            out.append([(d, k) for _, d, k in ent[:R]])
        return out

    def stats(self) -> dict:
        """``parent_switches``; with sub-groups also ``result_groups`` (int32 [G, R]): the sub-group every result came from, -1 where
        there is none"""
        st = dict(parent_switches=int(self.switches.sum()))
        if self.D > 1:
            groups = torch.full((self.G, int(self.cfg.num_return_sequences)), -1, dtype=torch.int32)
            for g, ent in enumerate(self._merge_order(self.pool_score.cpu(), self.pool_count.cpu())):
                for r, (d, _) in enumerate(ent):
                    groups[g, r] = d
            st["result_groups"] = groups
        return st


# ------------------------------------------------------------------------------------------------------------------------------ the driver
class _RingGenerator:
    """a RingMemory of ``state.M`` rows, the state and the captured per-token graph (the one-token forward and the state's epilogue) for one
    (model, ``key`` = what the state was built from); reused across calls"""
    busy = False        # (set while a stream runs over this state: generate_stream refuses a second one)

    def __init__(self, model, state, key):
        self.model, self.key, self.state = model, key, state
        if key.share_prompt:     # one copy of every prompt's keys / values per group, the rows' own tokens in a tail of max_new_tokens
            self.ring = GroupedRingMemory(model, key.rows, state.expand, key.cfg.max_new_tokens)
        else:
            self.ring = RingMemory(model, state.M, kv_dtype=key.kv_cache)
        self.q = int(getattr(state, "width", 1))     # the tokens per row of a token call (a speculative state: 1 + its draft tokens)
        self.step = GraphedRingStep(model, state.M, self.q, memory=self.ring, epilogue=self.epilogue)

    def epilogue(self, step, logits):
        if self.q == 1:
            self.state.epilogue(logits[:, -1], step.ids[:, 0], self.ring)
        else:       # every position's logits [M * q, V] (a view: the rows keep their padded stride) and the whole input ids
            self.state.epilogue(logits.view(self.state.M * self.q, logits.shape[-1]), step.ids, self.ring)

    def token(self, replay: bool):
        """one token step on the ids the last one left in ``step.ids``: a graph replay, or the same forward and epilogue launched eagerly over
        the same ring"""
        if replay:
            self.step(self.step.ids)
        else:
            logits, _, _ = self.model([self.step.x], compute_loss=False, mems=self.ring)
            self.epilogue(self.step, logits)

    def check(self, replay: bool):
        """the end of a run: raise what the token steps recorded (the replays' hand-off flag; the eager launches' chain)"""
        self.step.check(synchronize=True)
        if not replay:
            _check_chain(self.model)


def _ring_generator(model, State, key) -> _RingGenerator:
    """the generator kept on the model under ``State.cache`` if it was built from ``key`` and the weights it captured, else a new one"""
    gen = getattr(model, State.cache, None)
    if gen is None or gen.key != key or gen.step._version != model._wversion:
        setattr(model, State.cache, None)        # (free the old ring before the new one is allocated)
        gen = _RingGenerator(model, State(model, key), key)
        setattr(model, State.cache, gen)
    return gen


def _decode(model, prompt, State, key, graphed: Optional[bool], replay: bool, stats: Optional[dict], start=()):
    """``max_new_tokens`` steps of ``State(model, key)`` after ``prompt`` (``key.rows`` rows) -> ``state.result()``.  On the ring path
    (``graphed``, as ``generate`` documents it): over the cached ring generator, one graph replay per token (``replay`` False: the same forward
    and epilogue launched eagerly over the same ring); else eagerly over the list-form memory.  The callers have validated everything else:
    nothing is launched before that."""
    ring = _ring_ok(model) if graphed is None else bool(graphed)
    if ring and not _ring_ok(model):
        raise ValueError("the graphed ring path needs a bf16 model with the K/V-cached decode path (use_decode, d_head 128, mem_len > 0)")
    with _eval_mode(model):
        if ring:
            gen = _ring_generator(model, State, key)
            st, ids = gen.state, gen.step.ids
        else:
            st = State(model, key)
            ids = torch.zeros(st.M, st.width, dtype=torch.long, device=model.dev)
        wide = st.width > 1
        st.start(*start)
        # prefill: the whole prompt through the list-form memory path; its last position (expanded like the memory) picks token 0
        direct = ring and (_use_ring_prefill(model) or isinstance(prompt, Prefixed))
        # (share_prompt) the prefill fills the G rows of the grouped memory's base ring, unexpanded; the tail starts empty
        shared = ring and key.share_prompt
        dst = gen.ring.base if shared else (gen.ring if ring else None)
        if shared:
            gen.ring.begin()
        if direct:      # (model.use_ring_prefill, or a Prefixed prompt) the prompt's keys / values go straight into every ring row, origin 0
            dst.state.zero_()
            dst.load_status.zero_()
            logits, mems = _prefill_ring(model, prompt, dst, None, None if shared else st.expand), None
        else:
            logits, mems = _prefill(model, prompt, key.rows, None if shared else st.expand)
        last = logits[:, -1]
        st.epilogue(last if st.expand is None else last.repeat_interleave(st.expand, 0), ids if wide else ids[:, 0])
        del logits, last
        calls = 0
        if ring and not direct:
            dst.load(mems)
            del mems
        # (a wide state may reach the end in fewer calls, and a call past the end is a whole forward that commits nothing: the host also
        #  looks after the fewest calls that can get there, and from the counter it reads then, after the fewest that can get there now)
        look = -(-(st.cfg.max_new_tokens - 1) // st.width)
        for i in range(1, st.cfg.max_new_tokens):
            if i % st.cfg.sync_every == 0 or (wide and i - 1 >= look):
                if st.all_done():
                    break
                if wide:
                    look = i - 1 + max(1, -(-st.left // st.width))
            if ring:
                gen.token(replay)
            else:
                old = mems
                logits, _, mems = model([_token_input(ids)], compute_loss=False, mems=mems)
                if wide:
                    st.epilogue(logits.view(st.M * st.width, logits.shape[-1]), ids)
                else:
                    st.epilogue(logits[:, -1], ids[:, 0])
                mems = st.reorder_list(mems, old)
                del old
            calls += 1
        if ring:
            gen.check(replay)
            if direct and int(dst.load_status.cpu()) != 0:
                raise RuntimeError("db1_ring_prefill_rows / db1_ring_fork_rows: the prefill skipped a ring row or read a cache row out of range")
            if shared:
                gen.ring.check()
        else:
            _check_chain(model)
        if stats is not None:
            stats.update(path="ring" if ring else "eager", token_calls=calls, **st.stats())
        return st.result()


@torch.no_grad()
def generate(model, prompt, config: Optional[GenerationConfig] = None, stream_ids=None, graphed: Optional[bool] = None,
             stats: Optional[dict] = None, replay: bool = True,
             constraints: Optional[DecodingConstraints] = None, kv_cache: str = "bf16",
             speculative: Optional[SpeculativeConfig] = None, draft_script=None):
    """Generate ``config.max_new_tokens`` tokens after ``prompt`` -- ONE ``NLPTaskInput`` / ``ICTaskInput`` / ``VQATaskInput`` batch of M rows
    of one shape -> (ids int32 [M, max_new_tokens], lengths int32 [M]) on the host.  ``ids[r, :lengths[r]]`` are the tokens before EOS;
    after EOS a row holds ``pad_id``.  ``stream_ids`` (M ints, default 0 .. M-1): the Philox stream of every row -- a row's draws depend only
    on its logits, its stream id, the seed and the token index, not on the other rows.  ``graphed`` None: the hipGraph ring path where the
    model has one (bf16, ``use_decode``, d_head 128), else the eager list-form loop; False forces the eager loop.  ``stats`` (a dict):
    receives the path taken and the number of per-token calls.  ``replay`` False (ring path): the same forward and epilogue run eagerly over
    the same ring instead of as a graph replay.  ``constraints`` (a ``DecodingConstraints``): applied to every step's logits
    on the device, over the tokens generated so far, before the token is chosen; a row ended by one of its ``stop_sequences`` comes back
    without the matched tokens (``lengths[r]`` counts those before them, ``pad_id`` after; log-probs 0 and alternatives -1 / -inf there,
    ``sum_logprob`` the sum of the kept ones) and ``stats`` then also receives ``stop_hits``: per row 0, or the matched sequence's index + 1.
    With ``config.logprobs``: (ids, lengths, logprobs float32
    [M, max_new_tokens], sum_logprob float32 [M]) -- ``logprobs[r, t]`` is the log-probability of ``ids[r, t]`` under the model's
    distribution over the window (after the constraints, before temperature / top-k / top-p), EOS included, 0 after it; ``sum_logprob[r]``
    their fp32 sum in token order.  With ``config.top_logprobs`` n two more: top_ids int32 and top_logprobs float32, both
    [M, max_new_tokens, n] -- the n most likely tokens of step t under that same distribution, the most likely first (ties: the lower id),
    and their log-probabilities; -1 / -inf where the step had fewer candidates and at every position after a row's last written token
    (where ``logprobs`` holds 0).  Greedy: ``top_ids[r, t, 0] == ids[r, t]``.  ``kv_cache`` "fp8" (ring path only; ValueError otherwise):
    the memory's keys / values are held as e4m3 with a power-of-two scale per (row, position, K or V, head) -- half the bytes per token
    step and per slot, results within the e4m3 rounding of the keys / values; "bf16" (default): everything is what it is without it.
    ``prompt`` may also be a ``Prefixed`` (``PrefixCache``): its rows continue cached prefixes, only the suffix is projected; ring path
    only, with the cache's own ``kv_cache`` (ValueError otherwise, before anything is launched).  ``speculative`` (a
    ``SpeculativeConfig``): every token call carries 1 + k tokens per row, k of them drafts that the call itself verifies on the device; what
    comes back follows the same rule as without the keyword, token by token, in fewer calls where the drafts are right: in exact arithmetic the
    same ids, lengths and log-probs; in fp32 the same up to the order of the GEMMs' sums; in bf16 the logits of a (1 + k)-token call differ
    from the one-token call's in their last bits (other launches, other partial sums), so where two logits are nearly tied a token, and with
    it the rest of that row, can differ -- as between graphed and eager list-form generation.  ``stats`` also receives
    ``accepted`` (int list [k + 2]: the token calls that committed 0 .. k + 1 tokens, counted on the device) and ``tokens_per_call``.  The
    drafts: an n-gram lookup over the prompt's text and the row's output, or ``draft_script`` (an int array [M, max_new_tokens]: the proposal
    for every token index; what a draft model would supply).  Not with constraints, ``top_logprobs`` or more than 64 / (k + 1) rows
    (ValueError).  None (default): every launch, graph and cached generator is what it is without the keyword."""
    cfg = config or GenerationConfig()
    if speculative is None and draft_script is not None:
        raise ValueError("generate: draft_script needs speculative= (a SpeculativeConfig)")
    if speculative is not None:
        return _generate_speculative(model, prompt, cfg, speculative, draft_script, stream_ids, graphed, stats, replay, constraints, kv_cache)
    _need_memory(model, "generate")
    M = _batch_size(prompt, prefixed_ok=True)
    _check_prompt("generate", model, prompt, kv_cache, graphed)
    V, hi = _vocab_window(model, cfg)
    if not ops.select_tokens_supported(V, V, model.compute_dtype):
        raise ValueError(f"db1_select_tokens does not support a vocabulary of {V}")
    key = _constrained("generate", model, DecodeKey(rows=M, cfg=cfg, V=V, hi=hi), constraints, cfg.max_new_tokens)
    key = _with_kv_cache("generate", model, key, kv_cache, graphed)
    return _decode(model, prompt, _State, key, graphed, replay, stats, start=(stream_ids,))


def _prompt_text(prompt, M: int) -> Optional[np.ndarray]:
    """the text tokens of an ``NLPTaskInput`` prompt batch as int64 [M, L] on the host (any other prompt: None)"""
    from .data import NLPTaskInput
    if isinstance(prompt, Prefixed) or not isinstance(prompt, NLPTaskInput):
        return None
    seq = prompt.text_seq
    arr = np.asarray(seq.cpu() if torch.is_tensor(seq) else seq).astype(np.int64)
    return arr.reshape(M, -1)


def _generate_speculative(model, prompt, cfg, spec, draft_script, stream_ids, graphed, stats, replay, constraints, kv_cache):
    """``generate`` with ``speculative=``: every refusal first (ValueError before any launch), then ``_decode`` over a ``_SpecState``"""
    who = "generate(speculative=)"
    if not isinstance(spec, SpeculativeConfig):
        raise ValueError(f"{who}: a SpeculativeConfig expected, got {type(spec).__name__}")
    if not isinstance(cfg, GenerationConfig):
        raise ValueError(f"{who}: a GenerationConfig expected, got {type(cfg).__name__} (beam search has no speculative form)")
    if constraints is not None:
        raise ValueError(f"{who}: constraints and stop sequences are not supported (their history would have to include the drafts)")
    if cfg.top_logprobs:
        raise ValueError(f"{who}: top_logprobs is not supported")
    mlen = _need_memory(model, "generate")
    M = _batch_size(prompt, prefixed_ok=True)
    Q, mx = 1 + spec.num_draft_tokens, int(cfg.max_new_tokens)
    if M * Q > 64:
        raise ValueError(f"{who}: {M} rows of {Q} tokens per call ({M * Q} > 64, where the fused decode path of a token call ends)")
    if Q > mlen:
        raise ValueError(f"{who}: {Q} tokens per call exceed the model's mem_len {mlen}")
    text = _prompt_text(prompt, M) if spec.use_prompt else None
    if mx > ops.SPEC_MAX_HIST or (text is not None and text.shape[1] + mx > ops.SPEC_MAX_HIST):
        raise ValueError(f"{who}: the prompt's text ({0 if text is None else text.shape[1]} tokens) plus max_new_tokens {mx} exceeds "
                         f"{ops.SPEC_MAX_HIST}, the history a row's draft lookup can hold")
    script = None
    if draft_script is not None:
        script = draft_script.cpu().numpy() if torch.is_tensor(draft_script) else np.asarray(draft_script)
        if script.shape != (M, mx) or script.dtype.kind not in "iu":
            raise ValueError(f"{who}: draft_script must be an integer array of shape [{M}, {mx}] (got {script.dtype} {tuple(script.shape)})")
        script = np.clip(script.astype(np.int64), -1, 2 ** 31 - 1).astype(np.int32)     # (a value outside [0, V) is no proposal)
    _check_prompt("generate", model, prompt, kv_cache, graphed)
    V, hi = _vocab_window(model, cfg)
    _with_kv_cache("generate", model, DecodeKey(rows=M, cfg=cfg, V=V, hi=hi), kv_cache, graphed)     # (its refusals; the key below names the format)
    ctx_cap = (ops.SPEC_MAX_HIST - mx) if spec.use_prompt else 0
    ring = _ring_ok(model) if graphed is None else bool(graphed)
    cap = mlen + 64 if ring else 1
    if not ops.spec_supported(V, V, model.compute_dtype, Q, ctx_cap, mx, spec.ngram_min, spec.ngram_max, cap):
        raise ValueError(f"{who}: db1_spec_pick / db1_spec_accept do not support a vocabulary of {V} with {Q} tokens per call")
    if ring and _ring_ok(model):
        ok = (ops.relattn_decode_ring_kv8_supported(M, Q, mlen + Q, model.n_head, model.d_head) if kv_cache == "fp8" else
              ops.relattn_decode_supported(M, Q, mlen + Q, model.n_head, model.d_head, model.compute_dtype))
        if not ok:
            raise ValueError(f"{who}: the ring attention does not support {Q} tokens per call over mem_len {mlen} (kv_cache={kv_cache!r})")
    key = DecodeKeySpec(rows=M, cfg=cfg, V=V, hi=hi, speculative=_SpecPlan(config=spec, scripted=script is not None, ctx_cap=ctx_cap),
                        kv_cache=kv_cache)
    return _decode(model, prompt, _SpecState, key, graphed, replay, stats, start=(stream_ids, text, script))


def _run(model, x, cfg, n=None, **kw):
    for name in ("speculative", "draft_script"):      # (None is the call without the keyword, whichever function it goes to)
        if name in kw and kw[name] is None:
            del kw[name]
    if kw.get("speculative") is not None and (isinstance(cfg, BeamSearchConfig) or n is not None):
        raise ValueError("speculative= applies to generate under a GenerationConfig (not to beam search or best-of-n sampling)")
    if kw.get("speculative") is not None and kw.get("share_prompt"):
        raise ValueError("speculative= does not take share_prompt (a grouped memory has one token per call)")
    if kw.get("speculative") is not None:
        kw.pop("share_prompt", None)
    if isinstance(cfg, BeamSearchConfig):
        if n is not None:
            raise ValueError("n= (best-of-n sampling) takes a GenerationConfig, not a BeamSearchConfig")
        return beam_search(model, x, cfg, **kw)
    return generate(model, x, cfg, **kw) if n is None else sample_best_of(model, x, cfg, n, **kw)


def generate_captions(model, ic_batch, cfg=None, **kw):
    """captions for an ``ICTaskInput`` batch: the prompt ``[prompt, image patches]`` with an empty caption (coco_token_dataset.py layout),
    tokens in the text vocabulary unless ``cfg`` says otherwise -> what ``generate`` returns (with ``cfg.logprobs`` the log-probs too); with
    a ``BeamSearchConfig``: (ids, lengths, scores) as ``beam_search``; with ``n=`` (and ``sample_best_of``'s other keywords): the best of n
    sampled captions per image, as ``sample_best_of`` returns them"""
    return _run(model, caption_prompt(ic_batch), _text_window(model, cfg or GenerationConfig()), **kw)


def caption_prompt(ic_batch):
    """the generation prompt of an ``ICTaskInput`` batch: ``[prompt, image patches]`` and an empty caption"""
    from .data import ICTaskInput
    M = _batch_size(ic_batch)
    x = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=ic_batch.prompt_seq, img_seq=ic_batch.img_seq,
                    text_seq=torch.zeros(M, 0, dtype=torch.long))
    return _carry_patch_ids(ic_batch, x)


def answer_questions(model, vqa_batch, cfg=None, **kw):
    """answers for a ``VQATaskInput`` batch: the prompt ``[prompt, image patches, question]`` without the answer (the question is the first
    ``ques_len`` text tokens when ``ques_len`` is given, else the whole ``text_seq``), tokens in the text vocabulary unless ``cfg`` says
    otherwise -> what ``generate`` returns (with ``cfg.logprobs`` the log-probs too); with a ``BeamSearchConfig``: (ids, lengths, scores) as
    ``beam_search``; with ``n=``: the best of n sampled answers per question, as ``sample_best_of`` returns them"""
    return _run(model, question_prompt(vqa_batch), _text_window(model, cfg or GenerationConfig()), **kw)


def question_prompt(vqa_batch):
    """the generation prompt of a ``VQATaskInput`` batch: ``[prompt, image patches, question]`` without the answer"""
    q, ql = _questions(vqa_batch)
    if ql is None:
        return _question_rows(vqa_batch, q, None)
    ql = np.unique(ql)
    if ql.size != 1:
        raise ValueError("answer_questions: the questions of a batch must share one length (group them by length)")
    return _question_rows(vqa_batch, q, int(ql[0]))


def question_prompts(vqa_batch) -> List[Tuple[object, np.ndarray]]:
    """the generation prompts of a ``VQATaskInput`` batch whose questions differ in length: one ``question_prompt`` per distinct ``ques_len``
    (ascending) -> [(prompt, rows)]: ``rows`` (int64, ascending) are the batch rows the prompt's rows come from.  Every row of the batch is in
    exactly one prompt.  ``ques_len`` None: one prompt, the whole ``text_seq`` as the question."""
    G = _batch_size(vqa_batch)
    q, ql = _questions(vqa_batch)
    if ql is None:
        return [(_question_rows(vqa_batch, q, None), np.arange(G, dtype=np.int64))]
    if ql.size != G:
        raise ValueError(f"question_prompts: {ql.size} question lengths for a batch of {G} rows")
    if ql.min() < 0 or ql.max() > q.shape[1]:
        raise ValueError(f"question_prompts: question lengths must lie in [0, {q.shape[1]}]")
    groups = [(int(n), np.nonzero(ql == n)[0].astype(np.int64)) for n in np.unique(ql)]
    return [(_question_rows(vqa_batch, q, n, rows), rows) for n, rows in groups]


def image_prefix(batch):
    """the shared part of a ``VQATaskInput`` (or ``ICTaskInput``) batch's prompts, ``[prompt, image patches]`` with no text: what
    ``PrefixCache.put`` caches once per image.  Text after an image is embedded exactly as NLP text, so this prefix continued by
    ``question_suffixes``' rows (``Prefixed``) is the prompt ``question_prompts`` builds."""
    if type(batch).__name__ not in ("ICTaskInput", "VQATaskInput"):
        raise TypeError(f"image_prefix: ICTaskInput or VQATaskInput expected, got {type(batch).__name__}")
    return caption_prompt(batch)


def question_suffixes(vqa_batch) -> List[Tuple[object, np.ndarray]]:
    """the questions of a ``VQATaskInput`` batch as ``NLPTaskInput`` suffix batches, one per distinct ``ques_len`` (ascending) ->
    [(suffix, rows)], the grouping of ``question_prompts``; a question without tokens has no suffix and raises ValueError"""
    from .data import NLPTaskInput
    G = _batch_size(vqa_batch)
    q, ql = _questions(vqa_batch)
    if ql is None:
        groups = [(int(q.shape[1]), np.arange(G, dtype=np.int64))]
    else:
        if ql.size != G:
            raise ValueError(f"question_suffixes: {ql.size} question lengths for a batch of {G} rows")
        if ql.min() < 0 or ql.max() > q.shape[1]:
            raise ValueError(f"question_suffixes: question lengths must lie in [0, {q.shape[1]}]")
        groups = [(int(n), np.nonzero(ql == n)[0].astype(np.int64)) for n in np.unique(ql)]
    if groups[0][0] < 1:
        raise ValueError("question_suffixes: a question without tokens cannot continue a prefix (Prefixed needs Ls >= 1)")
    mk = lambda ids: NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=ids)
    return [(mk(q.index_select(0, torch.as_tensor(rows, device=q.device))[:, :n].contiguous()), rows) for n, rows in groups]


@torch.no_grad()
def beam_search(model, prompt, config: Optional[BeamSearchConfig] = None, graphed: Optional[bool] = None, stats: Optional[dict] = None,
                replay: bool = True, constraints: Optional[DecodingConstraints] = None,
                kv_cache: str = "bf16", share_prompt: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Beam search after ``prompt`` -- ONE ``NLPTaskInput`` / ``ICTaskInput`` / ``VQATaskInput`` batch of G prompts of one shape ->
    (ids int32 [G, R, max_new_tokens], lengths int32 [G, R], scores float32 [G, R]) on the host, R = ``num_return_sequences``: each prompt's
    best hypotheses, best first.  ``ids[g, r, :lengths[g, r]]`` are the tokens before EOS (then EOS, then ``pad_id``); the score is the sum of
    the tokens' log-probabilities (EOS included) over length^``length_penalty``, length = the tokens before EOS + 1 for a hypothesis that
    ended in EOS, max_new_tokens for one that ran to the end.  The prompt runs once per group; its memory is expanded to the W beams.
    ``graphed`` None: the hipGraph ring path where the model has one (bf16, ``use_decode``, d_head 128), else the eager list-form loop; False
    forces the eager loop (the list-form memory is reordered with index_select).  ``replay`` False (ring path): the same forward and epilogue
    run eagerly over the same ring instead of as a graph replay.  ``stats`` (a dict): receives the path taken, the number of per-token calls
    and ``parent_switches``, the number of (step, row) pairs (step > 0) whose parent was another row.  ``constraints`` (a
    ``DecodingConstraints``): applied to every step's logits on the device, over each beam's own tokens so far, before the beam step.
    ``kv_cache``: as ``generate`` takes it (db1_ring_reorder copies fp8 slots as the bytes they are).  ``share_prompt`` True (graphed bf16
    ring path only; ValueError otherwise, before anything is launched): the W beams of a group read ONE copy of their prompt's keys / values
    (``GroupedRingMemory``, db1_relattn_decode_group_fwd) instead of W; the results are those of the default path up to the order of the
    attention's partial sums.  False (default): everything is what it is without the keyword.  With ``config.num_beam_groups`` D > 1
    (diverse beam search, db1_beam_step_diverse): the same paths and keywords; a prompt's results are the best R of its D sub-groups' pools
    (equal scores: the lower sub-group first), the scores stay unpenalised, and ``stats`` also receives ``result_groups`` (int32 [G, R]:
    the sub-group every result came from).  D = 1 (default): everything is what it is without the two fields."""
    cfg = config or BeamSearchConfig()
    if not isinstance(cfg, BeamSearchConfig):
        raise TypeError(f"beam_search: BeamSearchConfig expected, got {type(cfg).__name__}")
    mlen = _need_memory(model, "beam_search")
    if int(cfg.max_new_tokens) > mlen:
        raise ValueError(f"beam_search: max_new_tokens {cfg.max_new_tokens} exceeds the model's mem_len {mlen}")
    G = _batch_size(prompt, prefixed_ok=True)
    _check_prompt("beam_search", model, prompt, kv_cache, graphed)
    W = int(cfg.num_beams)
    V, hi = _vocab_window(model, cfg)
    if cfg.eos_id is not None and int(cfg.eos_id) >= V:
        raise ValueError(f"eos_id {cfg.eos_id} lies outside the model's vocabulary ({V})")
    if not ops.beam_step_supported(V, V, W, model.compute_dtype):
        raise ValueError(f"db1_beam_step does not support a vocabulary of {V} with {W} beams")
    D = int(cfg.num_beam_groups)
    if D > 1 and not ops.beam_step_diverse_supported(V, V, W // D, D, model.compute_dtype):
        raise ValueError(f"db1_beam_step_diverse does not support a vocabulary of {V} with {D} sub-groups of {W // D} beams")
    key = _constrained("beam_search", model, DecodeKey(rows=G, cfg=cfg, V=V, hi=hi), constraints, cfg.max_new_tokens)
    key = _with_share_prompt("beam_search", model, key, share_prompt, W, prompt, kv_cache, graphed)
    key = _with_kv_cache("beam_search", model, key, kv_cache, graphed)
    return _decode(model, prompt, _BeamState, key, graphed, replay, stats)


# ------------------------------------------------------------------------------------------------------------------------- best-of-n sampling
MAX_BEST_OF = 64


def best_of_scores(sum_logprob, lengths, ended, no_candidate, length_penalty: float = 1.0) -> np.ndarray:
    """float32 scores of sampled rows: ``sum_logprob / L^length_penalty``, L = ``lengths`` + 1 where the row ``ended`` with EOS (the EOS is
    part of the sum) and ``lengths`` otherwise; -inf where ``no_candidate`` (status bit 0).  The normalisation of ``beam_search``'s scores."""
    s = np.asarray(sum_logprob, np.float32)
    L = np.asarray(lengths, np.int64) + np.asarray(ended, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = (s / np.power(np.maximum(L, 1).astype(np.float32), np.float32(length_penalty))).astype(np.float32)
    return np.where(np.asarray(no_candidate, bool), np.float32("-inf"), sc).astype(np.float32)


def best_of_order(scores, R: int) -> np.ndarray:
    """[G, n] scores -> int64 [G, R]: every group's R best columns, best first, ties to the lower column (a stable sort of the negated
    scores)"""
    return np.argsort(-np.asarray(scores, np.float32), axis=1, kind="stable")[:, :int(R)]


def _check_best_of(cfg, n, num_return_sequences, length_penalty):
    if not isinstance(cfg, GenerationConfig):
        raise TypeError(f"sample_best_of: GenerationConfig expected, got {type(cfg).__name__}")
    if cfg.greedy:
        raise ValueError("sample_best_of: a sampling config is needed (greedy=True gives n copies of one sequence)")
    if cfg.top_logprobs:
        raise ValueError("sample_best_of: top_logprobs is not supported (the ranking does not use the alternatives; use generate)")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_BEST_OF:
        raise ValueError(f"sample_best_of: n {n!r} must be an integer in [1, {MAX_BEST_OF}]")
    R = num_return_sequences
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= int(R) <= int(n):
        raise ValueError(f"sample_best_of: num_return_sequences {R!r} must lie in [1, n = {n}]")
    if not abs(float(length_penalty)) < float("inf"):
        raise ValueError(f"sample_best_of: length_penalty {length_penalty} must be finite")
    return int(n), int(R)


@torch.no_grad()
def sample_best_of(model, prompt, config: Optional[GenerationConfig], n: int, length_penalty: float = 1.0, num_return_sequences: int = 1,
                   stream_ids=None, graphed: Optional[bool] = None, stats: Optional[dict] = None,
                   constraints: Optional[DecodingConstraints] = None, kv_cache: str = "bf16",
                   share_prompt: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Best-of-n sampling after ``prompt`` (G prompts of one shape): n sampled continuations of every prompt, ranked by their normalised
    log-probability -> (ids int32 [G, R, max_new_tokens], lengths int32 [G, R], scores float32 [G, R]) on the host, R =
    ``num_return_sequences``, best first: the triple ``beam_search`` returns.  ``config``: a sampling ``GenerationConfig`` (``greedy`` raises);
    its ``logprobs`` field is set here.  ``1 <= num_return_sequences <= n <= 64``.  The prompt runs ONCE per prompt; its memory and last
    logits are expanded n-fold, as ``beam_search`` expands them to its beams, and row g * n + j samples from Philox stream g * n + j
    (``stream_ids`` of shape [G, n]: the streams to use instead).  score = sum_logprob / L^``length_penalty``, L = the tokens before EOS + 1
    for a row that ended with EOS, else its length; a row that met a step without a candidate scores -inf; ties go to the lower j.  The
    ranking is NumPy on the host over [G, n].  ``graphed``, ``stats``, ``constraints`` and ``kv_cache`` as ``generate`` takes them;
    ``share_prompt`` as ``beam_search`` takes it (the n samples of a prompt read one copy of its keys / values)."""
    cfg = config or GenerationConfig(greedy=False)
    n, R = _check_best_of(cfg, n, num_return_sequences, length_penalty)
    cfg = dataclasses.replace(cfg, logprobs=True)
    _need_memory(model, "sample_best_of")
    G = _batch_size(prompt, prefixed_ok=True)
    _check_prompt("sample_best_of", model, prompt, kv_cache, graphed)
    V, hi = _vocab_window(model, cfg)
    if not ops.select_tokens_supported(V, V, model.compute_dtype):
        raise ValueError(f"db1_select_tokens does not support a vocabulary of {V}")
    if stream_ids is not None:
        stream_ids = np.asarray(stream_ids, dtype=np.int64)
        if stream_ids.shape != (G, n):
            raise ValueError(f"sample_best_of: stream_ids of shape [{G}, {n}] expected, got {tuple(stream_ids.shape)}")
        stream_ids = stream_ids.reshape(-1)
    key = _constrained("sample_best_of", model, DecodeKey(rows=G, cfg=cfg, V=V, hi=hi, n=n), constraints, cfg.max_new_tokens)
    key = _with_share_prompt("sample_best_of", model, key, share_prompt, n, prompt, kv_cache, graphed)
    key = _with_kv_cache("sample_best_of", model, key, kv_cache, graphed)
    out, lengths, _, sums, status = _decode(model, prompt, _BestOfState, key, graphed, True, stats, start=(stream_ids,))
    out, lengths = out.numpy().reshape(G, n, -1), lengths.numpy().reshape(G, n)
    mx = out.shape[2]
    # a row ended with EOS when the token after its ``lengths`` tokens is the EOS (a row cut off at max_new_tokens has none)
    at = np.take_along_axis(out, np.minimum(lengths, mx - 1)[..., None].astype(np.int64), 2)[..., 0]
    no_cand = (status.numpy().reshape(G, n) & 1) != 0
    ended = np.zeros_like(no_cand) if cfg.eos_id is None else (lengths < mx) & (at == int(cfg.eos_id)) & ~no_cand
    scores = best_of_scores(sums.numpy().reshape(G, n), lengths, ended, no_cand, length_penalty)
    order = best_of_order(scores, R)
    pick = lambda a: torch.from_numpy(np.ascontiguousarray(np.take_along_axis(a, order.reshape(order.shape + (1,) * (a.ndim - 2)), 1)))
    return pick(out), pick(lengths), pick(scores)
