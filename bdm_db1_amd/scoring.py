"""Scoring text that somebody else wrote: token log-probabilities, per-task validation and candidate ranking.

The reference's validation (``evaluate_and_print_results``, train.py:86-138) prints one mean loss and a ``sub_loss`` dictionary per task that it
never fills; its caption / VQA evaluation can only generate.  Here

  * ``score`` runs an eval-mode forward whose head ends in ``db1_lmhead_score`` (the chunked sweep of the tied head with ``db1_score_rows`` on
    every chunk: the ``[tokens, padded vocabulary]`` logits tensor never exists) and ``db1_score_segments`` (the per-sequence sums);
  * ``validation_report`` turns that into loss / perplexity / top-1 accuracy per task kind: the ``sub_loss`` breakdown;
  * ``rank_candidates`` (``rank_captions``, ``rank_answers``) orders a closed set of continuations by likelihood: the prompt runs once per group
    through the list-form memory path, as in ``beam_search``; its last logits score token 0 of every candidate, its memory is expanded K-fold and
    ONE more call feeds tokens ``0 .. Lc-2`` and scores tokens ``1 .. Lc-1``.

What a model call needs around it -- the eval-mode switch, the vocabulary checks, the prefill with its expanded memory, the check of the decode
chain -- is generation.py's: the single decode driver there and the two entry points here share one copy of each.

The rule (candidates, lse, logprob, top1, rank, ignored rows) is stated in include/db1_hip.h (db1_score_rows) and restated in NumPy in
tests/score_rule.py.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .generation import (_batch_size, _check_chain, _eval_mode, _need_memory, _prefill, _text_window, _token_input, _vocab_window, caption_prompt,
                         question_prompt)

_KINDS = {"NLPTaskInput": "nlp", "ICTaskInput": "ic", "VQATaskInput": "vqa", "RLTaskInput": "rl"}
IGNORE = -100     # a label outside the vocabulary: the row is ignored (torch's ignore_index)


@dataclass(frozen=True)
class ScoreConfig:
    """Labels are scored over the columns ``[vocab_lo, vocab_hi)`` (``vocab_hi`` None: the model's whole vocabulary, so that the loss is the
    training loss; ``rank_captions`` / ``rank_answers`` then take the text vocabulary).  ``length_penalty``: candidate scores are divided by
    length^length_penalty.  ``chunk_rows``: rows of logits alive at a time in the sweep (None: the library's 16 384).  ``return_tokens``
    False: only the per-sequence sums are copied to the host.  ``top_n`` (1 .. 16; 0 = off, and nothing without ``return_tokens``): every
    position's n most likely tokens and their log-probabilities come back too (``db1_lmhead_score_top``)."""
    vocab_lo: int = 0
    vocab_hi: Optional[int] = None
    length_penalty: float = 0.0
    chunk_rows: Optional[int] = None
    return_tokens: bool = True
    top_n: int = 0

    def __post_init__(self):
        n = self.top_n
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= ops.MAX_TOP_N:
            raise ValueError(f"top_n {n!r} must be an integer in [0, {ops.MAX_TOP_N}]")
        if int(self.vocab_lo) < 0 or (self.vocab_hi is not None and int(self.vocab_hi) <= int(self.vocab_lo)):
            raise ValueError(f"vocabulary window [{self.vocab_lo}, {self.vocab_hi}) is empty")
        lp = float(self.length_penalty)
        if not abs(lp) < float("inf"):     # (NaN fails the comparison too)
            raise ValueError(f"length_penalty {self.length_penalty} must be finite")
        if self.chunk_rows is not None and int(self.chunk_rows) < 1:
            raise ValueError(f"chunk_rows {self.chunk_rows} must be >= 1")


@dataclass
class ScoreResult:
    """Host-side results of ``score``.  Per task input i (``return_tokens``): ``logprob[i]`` float32, ``top1[i]`` / ``rank[i]`` int32, each
    ``[B_i, L_i]``.  Per sequence, in the order of the task inputs: ``sum_logprob`` (the mask-weighted sum of the log-probabilities),
    ``tokens`` (the sum of the mask), ``hits`` (the mask-weighted number of positions whose label is the arg-max or tied with it), all
    float32, and ``task`` (int64: the index of the sequence's task input).  With ``ScoreConfig.top_n`` n: ``top_ids[i]`` int32 and
    ``top_logprob[i]`` float32, each ``[B_i, L_i, n]`` -- every position's n most likely tokens over the window, the most likely first
    (ties: the lower id; -1 / -inf where the window has fewer candidates), whatever the label (ignored positions included); None when off."""
    sum_logprob: np.ndarray
    tokens: np.ndarray
    hits: np.ndarray
    task: np.ndarray
    kinds: List[str]
    logprob: Optional[List[np.ndarray]] = None
    top1: Optional[List[np.ndarray]] = None
    rank: Optional[List[np.ndarray]] = None
    top_ids: Optional[List[np.ndarray]] = None
    top_logprob: Optional[List[np.ndarray]] = None
    status: int = 0        # OR of the status bits of the rows with mask != 0 (1: the label is no candidate, 2: the row has no candidate)
    stats: Dict[str, int] = field(default_factory=dict)
    mems: Optional[list] = None     # ``score(..., mems=)`` / ``score_document``: the memory the (last) forward returned

    @property
    def loss(self) -> float:
        """-sum(sum_logprob) / sum(tokens): what ``model.forward`` returns as ``loss`` on the same input"""
        return float(-np.sum(self.sum_logprob, dtype=np.float64) / np.sum(self.tokens, dtype=np.float64))


class _ScoreSink:
    """what ``TransformerXL._finish_forward`` hands the final hidden states to while ``score`` runs"""

    def __init__(self, cfg: ScoreConfig):
        self.cfg = cfg
        self.sweeps = 0
        self.out = None
        self.top = None

    def run(self, model, x, Wout, lab, msk, shapes, V):
        cfg = self.cfg
        T, dev = x.shape[0], x.device
        lse, logprob, top1, rank, status = _score_buffers(T, dev)
        top = {}
        if cfg.top_n and cfg.return_tokens:
            n = int(cfg.top_n)
            top = dict(top_n=n, top_ids=torch.empty(T, n, dtype=torch.int32, device=dev),
                       top_logprob=torch.empty(T, n, dtype=torch.float32, device=dev))
        ops.lmhead_score(x, Wout, lab, lse, logprob, top1, rank, status, V=V, vocab_lo=cfg.vocab_lo, vocab_hi=cfg.vocab_hi,
                         chunk_rows=0 if cfg.chunk_rows is None else int(cfg.chunk_rows), **top)
        self.top = (top["top_ids"], top["top_logprob"]) if top else None
        n_seq = sum(b for b, _ in shapes)
        seg = torch.empty(n_seq, 3, dtype=torch.float32, device=dev)
        ops.score_segments(logprob, rank, lab, msk, seg, V=V)
        self.sweeps += 1
        self.out = (logprob, top1, rank, status, seg, msk, lab, list(shapes))
        tot = seg.sum(0)        # (n_seq values: the same order on every run)
        return -tot[0] / tot[1]


def _check_window(model, cfg: ScoreConfig) -> ScoreConfig:
    V, _ = _vocab_window(model, cfg)
    if not ops.score_rows_supported(V, int(model.vocab_pad), model.compute_dtype):
        raise ValueError(f"db1_score_rows does not support a padded vocabulary of {model.vocab_pad}")
    return cfg


@torch.no_grad()
def score(model, tasks_input, config: Optional[ScoreConfig] = None, mems=None) -> ScoreResult:
    """Score the labels of ``tasks_input`` (what ``model.forward`` takes: ``NLPTaskInput`` / ``ICTaskInput`` / ``VQATaskInput`` /
    ``RLTaskInput`` with ``label`` and ``loss_mask``) under the model: ONE eval-mode forward without gradients whose head is the
    ``db1_lmhead_score`` sweep.  The model's mode is restored; no gradient or optimizer state is touched.  ``mems`` (the list
    ``model.init_mem`` or an earlier call returned): the forward attends to it, and ``ScoreResult.mems`` is the memory it returns."""
    cfg = _check_window(model, config or ScoreConfig())
    tasks_input = list(tasks_input)
    if not tasks_input:
        raise ValueError("score: no task input")
    for t in tasks_input:
        if type(t).__name__ not in _KINDS:
            raise TypeError(f"score: NLPTaskInput, ICTaskInput, VQATaskInput or RLTaskInput expected, got {type(t).__name__}")
        if t.label is None or t.loss_mask is None:
            raise ValueError("score: every task input needs label and loss_mask")
    sink = _ScoreSink(cfg)
    with _eval_mode(model):
        model._score_sink = sink
        try:
            out = model(tasks_input, compute_loss=True, mems=mems)
        finally:
            model._score_sink = None
    if sink.sweeps != 1:
        raise RuntimeError("score: the forward did not end in the scoring sweep")
    logprob, top1, rank, status, seg, msk, _, shapes = sink.out
    seg = seg.cpu().numpy()
    kinds = [_KINDS[type(t).__name__] for t in tasks_input]
    res = ScoreResult(sum_logprob=seg[:, 0].copy(), tokens=seg[:, 1].copy(), hits=seg[:, 2].copy(),
                      task=np.repeat(np.arange(len(shapes), dtype=np.int64), [b for b, _ in shapes]), kinds=kinds,
                      stats=dict(sweeps=sink.sweeps), mems=out[2] if mems is not None else None)
    st = status.cpu().numpy()[msk.cpu().numpy() != 0]            # only rows that count: a masked-out label outside the window says nothing
    res.status = int(np.bitwise_or.reduce(st)) if st.size else 0
    if cfg.return_tokens:
        lp, t1, rk = logprob.cpu().numpy(), top1.cpu().numpy(), rank.cpu().numpy()
        res.logprob, res.top1, res.rank, r0 = [], [], [], 0
        for b, l in shapes:
            res.logprob.append(lp[r0:r0 + b * l].reshape(b, l))
            res.top1.append(t1[r0:r0 + b * l].reshape(b, l))
            res.rank.append(rk[r0:r0 + b * l].reshape(b, l))
            r0 += b * l
        if sink.top is not None:
            ti, tl = (x.cpu().numpy() for x in sink.top)
            res.top_ids, res.top_logprob, r0 = [], [], 0
            for b, l in shapes:
                res.top_ids.append(ti[r0:r0 + b * l].reshape(b, l, -1))
                res.top_logprob.append(tl[r0:r0 + b * l].reshape(b, l, -1))
                r0 += b * l
    return res


def document_segments(n: int, segment_len: int) -> List[Tuple[int, int]]:
    """[begin, end) of the consecutive segments ``score_document`` feeds: ``segment_len`` positions each and a remainder.  A remainder of ONE
    position takes one from the segment before it (a 1-token call raises for models without ``same_length``); where that segment would be
    left with one position itself (``segment_len`` 2) the two are joined instead.  No segment has length 1."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or isinstance(segment_len, bool) or not isinstance(segment_len, (int, np.integer)):
        raise ValueError(f"document_segments: integers expected, got {n!r} and {segment_len!r}")
    n, s = int(n), int(segment_len)
    if s < 2:
        raise ValueError(f"segment_len {s} must be at least 2")
    if n < 2:
        raise ValueError(f"a document of {n} scored positions is too short (at least 2)")
    cuts = list(range(0, n, s)) + [n]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] == 1:
        if s > 2:
            cuts[-2] -= 1
        else:
            del cuts[-2]
    return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]


def _mem_attn_servable(model, B: int, seg_max: int) -> bool:
    """can db1_relattn_mem_fwd serve this model's calls with memory?  (host arithmetic first: no library call for a plainly unfit model)"""
    if model.compute_dtype != torch.bfloat16 or int(model.d_head) != 128:
        return False
    mlen, L = int(model.mem_len), max(int(seg_max), 65)
    return ops.relattn_mem_supported(B, L, mlen + L, mlen, int(model.n_head), int(model.d_head), int(model._window(L, mlen)), model.compute_dtype)


@torch.no_grad()
def score_document(model, tokens, config: Optional[ScoreConfig] = None, segment_len: Optional[int] = None, lengths=None, mems=None,
                   fused: Optional[bool] = None) -> ScoreResult:
    """Score texts longer than one segment with segment-level recurrence.  ``tokens``: ints ``[B, T]``, T >= 3; position p of n = T - 1 feeds
    ``tokens[:, p]`` and is labelled ``tokens[:, p + 1]``; ``lengths`` (ints ``[B]`` in ``[2, T]``): row b's positions p >= lengths[b] - 1 do
    not count.  The positions go through ``score(..., mems=)`` in the segments of ``document_segments(n, segment_len)`` (default
    ``model.n_position``), the memory starting from ``mems`` or ``model.init_mem(B)`` and handed on from segment to segment.

    One ``"nlp"`` task comes back: with ``return_tokens`` ``logprob`` / ``top1`` / ``rank`` (and the top-n fields) are ``[B, n]``;
    ``sum_logprob`` / ``tokens`` / ``hits`` per row are the segments' values added in segment order in float64 and stored as float32;
    ``status`` is the OR over the segments; ``stats = dict(segments=S, sweeps=S)``; ``mems`` is the final memory (pass it back to go on).
    ``fused``: None leaves ``model.use_mem_attn`` as it is, True / False sets it for this call (True on a model the fused kernel cannot serve
    raises ValueError before anything is launched)."""
    if type(tokens).__name__ == "Prefixed":
        raise ValueError("score_document: a Prefixed prompt is not supported (scoring runs through the list-form memory; pass ``mems=``)")
    tok = np.asarray(tokens.cpu() if torch.is_tensor(tokens) else tokens)
    if tok.dtype == object or tok.dtype.kind not in "iu" or tok.ndim != 2:
        raise ValueError("score_document: tokens must be an integer [B, T] array (rows of one length)")
    B, T = tok.shape
    if B < 1 or T < 3:
        raise ValueError(f"score_document: tokens of shape {tok.shape}: at least one row and T >= 3")
    n = T - 1
    seg_len = int(model.n_position) if segment_len is None else segment_len
    segs = document_segments(n, seg_len)
    if lengths is None:
        ln = np.full(B, T, np.int64)
    else:
        ln = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths)
        if ln.dtype == object or ln.dtype.kind not in "iu" or ln.shape != (B,) or ln.min() < 2 or ln.max() > T:
            raise ValueError(f"score_document: lengths must be {B} integers in [2, {T}]")
    _need_memory(model, "score_document")
    V = int(model.total_vocab_size)
    if tok.min() < 0 or tok.max() >= V:
        raise ValueError(f"score_document: tokens must lie in [0, {V})")
    if fused is not None and not isinstance(fused, (bool, np.bool_)):
        raise ValueError(f"score_document: fused must be None, True or False, got {fused!r}")
    if fused and not _mem_attn_servable(model, B, max(e - b for b, e in segs)):
        raise ValueError("score_document: fused=True, but db1_relattn_mem_fwd cannot serve this model (bf16, d_head 128, a window of at least one key)")
    cfg = _check_window(model, config or ScoreConfig())
    from .data import NLPTaskInput
    dev = model.dev
    ids = torch.from_numpy(np.ascontiguousarray(tok[:, :n].astype(np.int64))).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(tok[:, 1:].astype(np.int64))).to(dev)
    msk = torch.from_numpy((np.arange(n)[None, :] < (ln.astype(np.int64)[:, None] - 1)).astype(np.float32)).to(dev)
    cur = mems if mems is not None else model.init_mem(B)
    was = model.use_mem_attn
    parts = []
    try:
        if fused is not None:
            model.use_mem_attn = bool(fused)
        for b0, e0 in segs:
            x = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=msk[:, b0:e0].contiguous(), label=lab[:, b0:e0].contiguous(),
                             text_seq=ids[:, b0:e0].contiguous(), text_len=None)
            r = score(model, [x], cfg, mems=cur)
            cur = r.mems
            parts.append(r)
    finally:
        model.use_mem_attn = was
    tot = [np.zeros(B, np.float64) for _ in range(3)]
    for r in parts:       # (segment order, float64)
        for acc, x in zip(tot, (r.sum_logprob, r.tokens, r.hits)):
            acc += x.astype(np.float64)
    res = ScoreResult(sum_logprob=tot[0].astype(np.float32), tokens=tot[1].astype(np.float32), hits=tot[2].astype(np.float32),
                      task=np.zeros(B, np.int64), kinds=["nlp"], stats=dict(segments=len(segs), sweeps=sum(r.stats["sweeps"] for r in parts)),
                      mems=cur)
    for r in parts:
        res.status |= int(r.status)
    if cfg.return_tokens:
        for name in ("logprob", "top1", "rank", "top_ids", "top_logprob"):
            if getattr(parts[0], name) is not None:
                setattr(res, name, [np.concatenate([getattr(r, name)[0] for r in parts], axis=1)])
    return res


def _summary(sum_logprob, tokens, hits) -> dict:
    s, n, h = (float(np.sum(x, dtype=np.float64)) for x in (sum_logprob, tokens, hits))
    loss = -s / n if n > 0 else float("nan")
    return dict(loss=loss, ppl=math.exp(loss) if loss < 700 else float("inf"), top1_acc=h / n if n > 0 else float("nan"), tokens=n,
                sequences=int(np.size(tokens)))


def validation_report(model, tasks_input, config: Optional[ScoreConfig] = None) -> dict:
    """``score`` summarised per task kind and overall: {"overall": {...}, "nlp": {...}, "ic": {...}, ...} with ``loss`` (the mask-weighted mean
    negative log-probability), ``ppl`` = exp(loss), ``top1_acc`` (for RL batches: the action-token accuracy), ``tokens`` and ``sequences``.
    The task losses, weighted by their tokens, recombine to the overall loss, which is the loss ``model.forward`` returns."""
    cfg = config or ScoreConfig()
    r = score(model, tasks_input, cfg if not cfg.return_tokens else dataclasses.replace(cfg, return_tokens=False))
    out = {"overall": _summary(r.sum_logprob, r.tokens, r.hits)}
    for kind in dict.fromkeys(r.kinds):
        sel = np.isin(r.task, [i for i, k in enumerate(r.kinds) if k == kind])
        out[kind] = _summary(r.sum_logprob[sel], r.tokens[sel], r.hits[sel])
    return out


def _padded_rows(model, logits3d: torch.Tensor) -> torch.Tensor:
    """the [B * L, vocab_pad] buffer behind the ``[B, L, V]`` logits view a forward returned (rows of a 16-byte multiple, as db1_score_rows wants)"""
    B, L, _ = logits3d.shape
    vp = int(model.vocab_pad)
    if logits3d.stride() != (L * vp, vp, 1):
        raise RuntimeError("unexpected logits layout")
    return torch.as_strided(logits3d, (B * L, vp), (vp, 1), logits3d.storage_offset())


def _score_buffers(T, dev):
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    return torch.empty(T, **f32), torch.empty(T, **f32), torch.empty(T, **i32), torch.empty(T, **i32), torch.empty(T, **i32)


@torch.no_grad()
def rank_candidates(model, prompt, candidates, cand_len=None, config: Optional[ScoreConfig] = None,
                    stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rank K candidate continuations of every prompt by likelihood.  ``prompt``: ONE ``NLPTaskInput`` / ``ICTaskInput`` / ``VQATaskInput`` batch
    of G rows of one shape, as for ``generate``; ``candidates``: ints ``[G, K, Lc]``, or ``[K, Lc]`` shared by all prompts; ``cand_len``: an int
    or an array broadcastable to ``[G, K]`` with values in ``[1, Lc]`` (default ``Lc``) -> (scores float32 [G, K], order int64 [G, K], logprob
    float32 [G, K, Lc]) on the host.  ``logprob[g, k, i]`` is the log-probability of token i of candidate k after the prompt g and the
    candidate's tokens before i, over the window of ``config`` (0 at the positions at or after ``cand_len``, which cannot influence the earlier
    ones: the attention is causal); ``scores[g, k] = sum_{i < len} logprob[g, k, i] / len^length_penalty``; ``order[g]`` sorts ``scores[g]``
    descending, the lower k first on ties.  Tokens older than ``mem_len`` fall out of the memory, as in generation.  ``stats`` (a dict) receives
    ``model_calls`` (1 when Lc == 1, else 2)."""
    if type(prompt).__name__ == "Prefixed":
        _batch_size(prompt)     # (raises: a Prefixed prompt lives on the K/V ring, the candidates run through the list-form memory)
    cfg = _check_window(model, config or ScoreConfig())
    _need_memory(model, "rank_candidates")
    G = _batch_size(prompt)
    V, dev = int(model.total_vocab_size), model.dev
    cand = torch.as_tensor(np.asarray(candidates.cpu() if torch.is_tensor(candidates) else candidates))
    if cand.dtype not in (torch.int64, torch.int32) or cand.dim() not in (2, 3):
        raise ValueError("rank_candidates: candidates must be an integer [G, K, Lc] or [K, Lc] array")
    cand = cand.long()
    if cand.dim() == 2:
        cand = cand.unsqueeze(0).expand(G, -1, -1)
    if cand.shape[0] != G or cand.shape[1] < 1 or cand.shape[2] < 1:
        raise ValueError(f"rank_candidates: candidates of shape {tuple(cand.shape)} for {G} prompts")
    K, Lc = int(cand.shape[1]), int(cand.shape[2])
    if bool(((cand < 0) | (cand >= V)).any()):
        raise ValueError(f"rank_candidates: candidate tokens must lie in [0, {V})")
    clen = np.full((G, K), Lc, np.int64) if cand_len is None else np.broadcast_to(np.asarray(cand_len, dtype=np.int64), (G, K)).copy()
    if clen.min() < 1 or clen.max() > Lc:
        raise ValueError(f"rank_candidates: cand_len must lie in [1, {Lc}]")
    M = G * K
    cand = cand.reshape(M, Lc).contiguous().to(dev)
    valid = (torch.arange(Lc).unsqueeze(0) < torch.from_numpy(clen.reshape(M, 1))).to(dev)       # [M, Lc]
    labels = torch.where(valid, cand, torch.full_like(cand, IGNORE))                              # masked-out positions: ignored rows
    logprob, rank = torch.empty(M, Lc, dtype=torch.float32, device=dev), torch.empty(M, Lc, dtype=torch.int32, device=dev)
    win = dict(V=V, vocab_lo=cfg.vocab_lo, vocab_hi=cfg.vocab_hi)
    with _eval_mode(model):
        # call 1: the prompt once per group; the logits of its last position, repeated K-fold, score token 0 of every candidate
        logits, mems = _prefill(model, prompt, G, K if Lc > 1 else None)
        L = logits.shape[1]
        last = _padded_rows(model, logits)[L - 1::L].repeat_interleave(K, 0)          # [M, vocab_pad]
        lse, lp, t1, rk, st = _score_buffers(M, dev)
        ops.score_rows(last, labels[:, 0].contiguous(), lse, lp, t1, rk, st, **win)
        logprob[:, 0], rank[:, 0] = lp, rk
        calls = 1
        del logits, last
        if Lc > 1:
            # call 2: the memory expanded K-fold, tokens 0 .. Lc-2 of every candidate in, tokens 1 .. Lc-1 scored
            logits, _, _ = model([_token_input(cand[:, :Lc - 1].contiguous())], compute_loss=False, mems=mems)
            T = M * (Lc - 1)
            lse, lp, t1, rk, st = _score_buffers(T, dev)
            ops.score_rows(_padded_rows(model, logits), labels[:, 1:].reshape(-1).contiguous(), lse, lp, t1, rk, st, **win)
            logprob[:, 1:], rank[:, 1:] = lp.view(M, Lc - 1), rk.view(M, Lc - 1)
            calls = 2
            del logits, mems
        model._dec_state = None
        _check_chain(model)
        seg = torch.empty(M, 3, dtype=torch.float32, device=dev)
        ops.score_segments(logprob.view(-1), rank.view(-1), labels.view(-1), valid.to(torch.float32).view(-1), seg, V=V)
    if stats is not None:
        stats.update(model_calls=calls)
    sums = seg[:, 0].cpu().numpy().reshape(G, K)
    scores = (sums / np.power(clen.astype(np.float32), np.float32(cfg.length_penalty))).astype(np.float32)
    order = np.argsort(-scores, axis=1, kind="stable")          # descending, the lower k first on ties
    return torch.from_numpy(scores), torch.from_numpy(order.astype(np.int64)), logprob.view(G, K, Lc).cpu()


def rank_captions(model, ic_batch, candidates, cand_len=None, config: Optional[ScoreConfig] = None, stats: Optional[dict] = None):
    """``rank_candidates`` after the prompt ``generate_captions`` builds (``[prompt, image patches]``, an empty caption), over the text
    vocabulary unless ``config`` says otherwise"""
    return rank_candidates(model, caption_prompt(ic_batch), candidates, cand_len, _text_window(model, config or ScoreConfig()), stats)


def rank_answers(model, vqa_batch, candidates, cand_len=None, config: Optional[ScoreConfig] = None, stats: Optional[dict] = None):
    """``rank_candidates`` after the prompt ``answer_questions`` builds (``[prompt, image patches, question]``), over the text vocabulary
    unless ``config`` says otherwise"""
    return rank_candidates(model, question_prompt(vqa_batch), candidates, cand_len, _text_window(model, config or ScoreConfig()), stats)
