"""Action decoding for batched RL rollouts with nothing between the tokens but the device: the call protocol of ``get_action_batched``
(evaluate_rl.py:157-266 for M environments: the observation call, one token per call, the memorising call) with the per-token torch passes,
the argmax and the host copy replaced by ONE launch behind every model call (``db1_select_actions``: the action window, the environment's
action mask, the choice, the bin, its decoded value and the next call's input id; include/db1_hip.h, restated in tests/action_rule.py).

bf16 models with the K/V ring: two ``GraphedRingStep`` s over one ``RingMemory`` -- the observation call (M, obs_length + 1) and the token
call (M, 1) -- each with that launch and a captured ``ctr[1] += 1`` as its epilogue, so one environment step is 1 + action_length graph
replays and ONE copy back to the host.  Other models (fp32), or ``graphed=False``: the same forwards and the same launches eagerly.
``get_action`` / ``get_action_batched`` are untouched; image observations, the sliding-window mode without memory and per-environment
sampling parameters stay with them (README, "Action decoding on the device")."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..data.input_specs import RLTaskInput

MAX_CALL_TOKENS = 64      # what one call over a RingMemory takes


def action_window(args, discrete_action: bool, n_actions: Optional[int] = None):
    """-> (act_lo, act_hi): the columns ``masked_logits_for_action`` leaves (evaluate_rl.py:96-124) -- the continuous bins after the text ids
    (and after the discrete ids when those do not overlap the text ids), without the separator that ends the vocabulary; or the first
    ``n_actions`` discrete ids.  A predicted id minus act_lo is what ``recover_model_predict_token_to_tokenizer_raw`` returns."""
    text = int(args.text_vocab_size)
    if not discrete_action:
        lo = text if args.overlap_with_text else text + int(args.num_discrete_values)
        return lo, lo + int(args.num_continuous_bin)
    if n_actions is None or isinstance(n_actions, bool) or int(n_actions) != n_actions or int(n_actions) < 1:
        raise ValueError(f"action_window: a discrete action space needs n_actions >= 1 (got {n_actions!r})")
    lo = 0 if args.overlap_with_text else text
    return lo, lo + int(n_actions)


def action_mask_applies(args, discrete_action: bool) -> bool:
    """whether an environment's action mask changes the choice.  The reference subtracts the mask's penalty from the columns
    [0, n_actions) (evaluate_rl.py:121-123), which are the action window only where the discrete ids overlap the text ids; otherwise they
    are text ids the window has excluded already and the mask changes nothing -- ``get_action`` / ``get_action_batched`` reproduce that,
    and so does ``ActionDecoder``, which then hands no mask to the kernel."""
    return bool(discrete_action) and bool(args.overlap_with_text)


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


@dataclass(frozen=True)
class ActionConfig:
    """What an ``ActionDecoder`` decodes: ``obs_length`` observation tokens (+ the separator) per step, ``action_length`` action tokens;
    ``discrete_action`` with the ``n_actions`` of the action space (one id, the first token's), else continuous bins decoded to values.
    ``greedy`` (the reference's argmax), or Gumbel-max sampling at ``temperature`` after ``top_k`` (0 = off) / ``top_p`` (1 = off) under
    ``seed``: the rule and the Philox layout of ``generate``'s sampling."""
    obs_length: int
    action_length: int
    discrete_action: bool
    n_actions: Optional[int] = None
    greedy: bool = True
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        from .. import ops
        if not _is_int(self.obs_length) or self.obs_length < 1:
            raise ValueError(f"ActionConfig: obs_length {self.obs_length!r} must be an integer >= 1")
        if not _is_int(self.action_length) or not 1 <= self.action_length <= ops.ACT_MAX_LEN:
            raise ValueError(f"ActionConfig: action_length {self.action_length!r} must be an integer in [1, {ops.ACT_MAX_LEN}]")
        if not isinstance(self.discrete_action, (bool, np.bool_)):
            raise ValueError(f"ActionConfig: discrete_action {self.discrete_action!r} must be a bool")
        if self.discrete_action and (not _is_int(self.n_actions) or self.n_actions < 1):
            raise ValueError(f"ActionConfig: a discrete action space needs n_actions >= 1 (got {self.n_actions!r})")
        if not self.discrete_action and self.n_actions is not None:
            raise ValueError("ActionConfig: n_actions belongs to a discrete action space")
        if not isinstance(self.greedy, (bool, np.bool_)):
            raise ValueError(f"ActionConfig: greedy {self.greedy!r} must be a bool")
        if not _is_int(self.top_k) or not _is_int(self.seed):
            raise ValueError(f"ActionConfig: top_k {self.top_k!r} and seed {self.seed!r} must be integers")
        ops._check_sampling("ActionConfig", self.greedy, self.temperature, self.top_k, self.top_p)


class ActionDecoder:
    """M = ``n_envs`` environments of one kind, decoded together.  ``args``: the reference's arguments (``text_vocab_size``,
    ``num_discrete_values``, ``num_continuous_bin``, ``overlap_with_text``); ``cfg``: an ``ActionConfig``; ``kv_cache``: the ring's format
    ("bf16" / "fp8", as ``generate`` takes it); ``graphed``: None -- replay where the model has the K/V ring, True -- insist on it, False --
    the same launches eagerly (over the ring where the model has one: the same bits as the replays; over the list-form memory otherwise);
    ``stream_ids`` (int [M] or None: the row): the Philox stream of every environment.

    ``act`` runs one environment step; ``last_bins`` (int32 [M, action_length], host) holds its bins, ``last_tokens`` (int64 [M, 1]) the last
    action token -- what ``get_action_batched`` returns as its sequence; ``memory`` is the RingMemory or the list-form memory;
    ``stats`` counts ``env_steps``, ``replays`` and ``resets``.  The tokenizer is ``ContinuousScalarTokenizer``'s default (mu 100, M 256)."""

    def __init__(self, args, model, n_envs: int, cfg: ActionConfig, kv_cache: str = "bf16", graphed: Optional[bool] = None, stream_ids=None):
        from .. import ops
        from ..decode import GraphedRingStep, RingMemory
        who = "ActionDecoder"
        if not isinstance(cfg, ActionConfig):
            raise ValueError(f"{who}: an ActionConfig expected, got {type(cfg).__name__}")
        if not _is_int(n_envs) or n_envs < 1:
            raise ValueError(f"{who}: n_envs {n_envs!r} must be an integer >= 1")
        if kv_cache not in ("bf16", "fp8"):
            raise ValueError(f"{who}: kv_cache must be 'bf16' or 'fp8' (got {kv_cache!r})")
        M, ol, al = int(n_envs), int(cfg.obs_length), int(cfg.action_length)
        if ol + 1 > MAX_CALL_TOKENS:
            raise ValueError(f"{who}: an observation call of {ol + 1} tokens (obs_length + the separator) exceeds the {MAX_CALL_TOKENS} a call over the ring takes")
        if not int(getattr(model, "mem_len", 0) or 0) > 0:
            raise ValueError(f"{who}: the model has no memory (mem_len 0): the sliding-window mode stays with get_action")
        lo, hi = action_window(args, bool(cfg.discrete_action), cfg.n_actions)
        V = int(model.total_vocab_size)
        if not (0 <= lo < hi <= V and hi - lo <= ops.ACT_MAX_WINDOW) or not ops.select_actions_supported(V, int(model.vocab_pad), model.compute_dtype, lo, hi):
            raise ValueError(f"{who}: db1_select_actions does not take the action window [{lo}, {hi}) of a vocabulary of {V} (inside it, at most {ops.ACT_MAX_WINDOW} wide)")
        ring_ok = (model.compute_dtype == torch.bfloat16 and bool(model.use_decode) and model.d_head == 128)
        if graphed and not ring_ok:
            raise ValueError(f"{who}: graphed=True needs the bf16 K/V-cached decode path (d_head 128, mem_len > 0)")
        if kv_cache == "fp8" and not ring_ok:
            raise ValueError(f"{who}: kv_cache='fp8' needs the K/V ring (a bf16 model with the decode path, d_head 128)")
        sid = None
        if stream_ids is not None:
            sid = np.asarray(stream_ids)
            if sid.shape != (M,) or not np.issubdtype(sid.dtype, np.integer):
                raise ValueError(f"{who}: stream_ids must be {M} integers")
        self.args, self.model, self.cfg, self.M, self.V = args, model, cfg, M, V
        self.window, self.num_bins = (lo, hi), int(getattr(args, "num_continuous_bin", 1024))
        self.bin_base, self.sep_id = int(args.text_vocab_size), V - 1
        self.ring_path, self.replay = ring_ok, ring_ok and graphed is not False
        dev = model.dev
        # ---- the static device state: counters {env_step, i}; bins | values | status in ONE buffer (one copy back per environment step)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=dev)
        self._pack = torch.zeros(M * (2 * al + 1), dtype=torch.int32, device=dev)
        self.bins = self._pack[:M * al].view(M, al)
        self.values = None if cfg.discrete_action else self._pack[M * al:2 * M * al].view(torch.float32).view(M, al)
        self.status = self._pack[2 * M * al:]
        self.mask = torch.ones(M, hi - lo, dtype=torch.uint8, device=dev) if action_mask_applies(args, cfg.discrete_action) else None
        self.stream_id = None if sid is None else torch.from_numpy(sid.astype(np.int32)).to(dev)
        self._obs_x = torch.zeros(M, ol, dtype=torch.float32, device=dev)
        self._pos_obs = torch.arange(1, ol + 2, dtype=torch.long, device=dev)[None, :].expand(M, -1).contiguous()
        self._pos_tok = torch.zeros(M, 1, dtype=torch.long, device=dev)
        self._sel = dict(act_lo=lo, act_hi=hi, V=V, mask=self.mask, values=self.values, num_bins=self.num_bins, greedy=bool(cfg.greedy),
                         temperature=float(cfg.temperature), top_k=int(cfg.top_k), top_p=float(cfg.top_p), seed=int(cfg.seed), stream_id=self.stream_id)
        self.stats = dict(env_steps=0, replays=0, resets=0)
        self.last_bins = np.zeros((M, al), np.int32)
        self.last_tokens = np.zeros((M, 1), np.int64)
        rl_input = lambda pos: (lambda ids: RLTaskInput(tensor_seq=ids, vision_seq=None, text_seq=None, attention_mask=None, loss_mask=None,
                                                        label=None, position_id=pos))
        # the first launch of the selection happens here, not under a capture: at i == action_length it writes nothing
        with torch.no_grad():
            self.ctr[1:2].fill_(al)
            self._pick(torch.zeros(M, V, dtype=model.compute_dtype, device=dev), torch.zeros(M, dtype=torch.long, device=dev))
            self.ctr.zero_()
        if self.replay:
            self.memory = RingMemory(model, M, kv_dtype=kv_cache)
            # (the token step first: the observation step's epilogue writes ITS input)
            self._tok_step = GraphedRingStep(model, M, 1, memory=self.memory, make_input=rl_input(self._pos_tok), epilogue=self._tok_epilogue)
            self._tok_ids, self._tok_x = self._tok_step.ids, self._tok_step.x
            self._obs_step = GraphedRingStep(model, M, ol + 1, memory=self.memory, make_input=rl_input(self._pos_obs), epilogue=self._obs_epilogue)
            self._obs_ids, self._obs_in = self._obs_step.ids, self._obs_step.x
            self.ctr.zero_()
        else:
            self.memory = RingMemory(model, M, kv_dtype=kv_cache) if ring_ok else model.init_mem(M)
            self._tok_ids = torch.zeros(M, 1, dtype=torch.long, device=dev)
            self._obs_ids = torch.zeros(M, ol + 1, dtype=torch.long, device=dev)
            self._tok_x, self._obs_in = rl_input(self._pos_tok)(self._tok_ids), rl_input(self._pos_obs)(self._obs_ids)

    # ---- the epilogues: what follows a model call, captured with it or launched behind it
    def _pick(self, logits2d, next_ids):
        from .. import ops
        ops.select_actions(logits2d, self.ctr, self.bins, next_ids, self.status, **self._sel)

    def _obs_epilogue(self, step, logits):
        self.ctr[1:2].zero_()
        self._pick(logits[:, -1], self._tok_ids[:, 0])
        self.ctr[1:2].add_(1)

    def _tok_epilogue(self, step, logits):
        self._pick(logits[:, -1], (self._tok_ids if step is None else step.ids)[:, 0])     # (its own input: the next call's token)
        self.ctr[1:2].add_(1)

    def _eager_call(self, x, epilogue):
        res = self.model([x], compute_loss=False, mems=self.memory)
        self.memory = res[-1]
        epilogue(None, res[0])

    # ---- the public surface
    def reset(self, rows=None):
        """new episodes: in every environment (None: the zero memory, the counters back to 0) or in rows ``rows`` only, the others going on"""
        if rows is None:
            if self.ring_path:
                self.memory.reset()
            else:
                self.memory = self.model.init_mem(self.M)
            self.ctr.zero_()
            self.status.zero_()
        else:
            rows = [int(r) for r in rows]
            if len(set(rows)) != len(rows) or any(not 0 <= r < self.M for r in rows):
                raise ValueError(f"ActionDecoder.reset: rows {rows} must be distinct and lie in [0, {self.M})")
            if self.ring_path:
                self.memory.reset_rows(rows)
            else:
                for m in self.memory:
                    m[rows] = 0
        self.stats["resets"] += 1

    def act(self, obs_tokens=None, obs=None, action_masks=None):
        """one environment step of all M environments: ``obs_tokens`` (int [M, obs_length + 1]: the new observation's token ids and the
        separator, what ``get_action_batched`` takes) or ``obs`` (float [M, obs_length]: tokenised on the device by db1_obs_tokens);
        ``action_masks`` ([M, n_actions], 1 = allowed; discrete action spaces only).  -> the actions on the host: int64 [M] (discrete) or
        float32 [M, action_length] (the decoded bins).
        A status bit read back (a row without an allowed, finite action logit; a token counter out of range) raises RuntimeError naming the
        rows AFTER the step has run: its tokens -- ``act_lo`` in such a row -- have entered every row's memory, ``env_step`` and
        ``stats['env_steps']`` have advanced, and ``last_bins`` / ``last_tokens`` still hold the step before.  The flag is cleared and the
        decoder can go on; a caller that wants the named rows clean starts them again with ``reset(rows=...)``."""
        from .. import ops
        who, cfg, M, ol, al = "ActionDecoder.act", self.cfg, self.M, int(self.cfg.obs_length), int(self.cfg.action_length)
        if (obs_tokens is None) == (obs is None):
            raise ValueError(f"{who}: exactly one of obs_tokens and obs is expected")
        if obs_tokens is not None:
            toks = obs_tokens.detach().cpu().numpy() if torch.is_tensor(obs_tokens) else np.asarray(obs_tokens)
            if toks.shape != (M, ol + 1) or not np.issubdtype(toks.dtype, np.integer):
                raise ValueError(f"{who}: obs_tokens must be integers of shape ({M}, {ol + 1})")
        else:
            x = obs.detach().cpu().numpy() if torch.is_tensor(obs) else np.asarray(obs)
            if x.shape != (M, ol) or not np.issubdtype(x.dtype, np.floating):
                raise ValueError(f"{who}: obs must be floats of shape ({M}, {ol})")
        if action_masks is not None:
            if not cfg.discrete_action:
                raise ValueError(f"{who}: action masks belong to a discrete action space")
            am = action_masks.detach().cpu().numpy() if torch.is_tensor(action_masks) else np.asarray(action_masks)
            if am.shape != (M, int(cfg.n_actions)):
                raise ValueError(f"{who}: action_masks must have the shape ({M}, {int(cfg.n_actions)})")
        with torch.no_grad():
            if self.mask is not None:      # (1 = allowed, as the reference's penalty |mask - 1| * 1e10 reads it)
                if action_masks is None:
                    self.mask.fill_(1)
                else:
                    self.mask.copy_(torch.from_numpy(np.ascontiguousarray(am == 1).astype(np.uint8)))
            if obs_tokens is not None:
                self._obs_ids.copy_(torch.from_numpy(np.ascontiguousarray(toks, dtype=np.int64)))
            else:
                self._obs_x.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
                ops.obs_tokens(self._obs_x, self._obs_ids, bin_base=self.bin_base, sep_id=self.sep_id, num_bins=self.num_bins)
            if self.replay:
                self._obs_step(None)
                for _ in range(al):          # (the last one is the memorising call: its selection writes nothing)
                    self._tok_step(None)
                self.stats["replays"] += 1 + al
            else:
                self._eager_call(self._obs_in, self._obs_epilogue)
                for _ in range(al):
                    self._eager_call(self._tok_x, self._tok_epilogue)
            self.ctr[0:1].add_(1)
            host = self._pack.cpu().numpy()          # (the step's one copy back; synchronises)
        if self.replay:
            self._obs_step.check()
            self._tok_step.check()
        else:
            chk = getattr(self.model, "check_decode_chain", None)
            if chk is not None:
                chk()
        self.stats["env_steps"] += 1
        status = host[2 * M * al:]
        if status.any():
            self.status.zero_()
            none = np.nonzero(status & 1)[0].tolist()
            ctr = np.nonzero(status & 2)[0].tolist()
            raise RuntimeError(f"{who}: db1_select_actions reported rows without an allowed, finite action logit {none} and rows whose token "
                               f"counter left [0, {al}] {ctr}")
        self.last_bins = host[:M * al].reshape(M, al).copy()
        self.last_tokens = (self.last_bins[:, -1:].astype(np.int64) + self.window[0])
        if cfg.discrete_action:
            return self.last_bins[:, 0].astype(np.int64)
        return host[M * al:2 * M * al].view(np.float32).reshape(M, al).copy()
