"""Launch-bound inference with memory as ONE hipGraph replay per call.

A DB1-1.3B call with a full memory (evaluate_rl.py:157-266: batch 1, 1 .. ~50 new tokens, mem_len 1024) is ~340 short
kernels; launched one by one from Python the call is host-bound (4.8 ms wall for 3.2 ms of kernels).  ``GraphedMemoryStep``
captures the model's own forward for a fixed (batch, new-token count) once and replays it: same kernels, same results,
no per-kernel launch cost.  It is opt-in because a graph works on static buffers: the memory it returns is always the SAME
list of tensors, updated in place by the replay (the reference returns fresh tensors every call); callers that only pass the
memory back in -- like evaluate_rl's loop -- see no difference.
"""
from __future__ import annotations

import contextlib
import gc
from types import SimpleNamespace
from typing import List

import torch


@contextlib.contextmanager
def graph_capture(g, **kw):
    """``torch.cuda.graph(g, **kw)`` with Python's cyclic garbage collector held off until the capture has ended.  A collection that fires
    inside a capture destroys whatever dead cycles it finds -- a dropped GraphedRingStep with its CUDAGraph and private pool among them --
    and the HIP calls of those destructors (graph destruction, hipFree of the pool) are illegal while a stream captures: the error is
    raised inside a destructor and the process aborts.  torch collected before every capture once; since that became an option
    (``torch.compiler.config.force_cudagraph_gc``, off by default) nothing keeps a collection out of a capture as long as a model forward.
    The garbage is collected as usual after the capture."""
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):
            yield
    finally:
        if was_on:
            gc.enable()


def _token_input(ids):
    """the model input that feeds the token ids ``ids`` [rows, n] after what the memory holds"""
    from .data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=ids, text_len=None)


class GraphedMemoryStep:
    def __init__(self, model, batch_size: int, n_new: int, make_input=None):
        """``make_input(ids)`` builds the task input for static token ids [batch, n_new] (default: a text input)."""
        if model.compute_dtype != torch.bfloat16 or not model.use_decode:
            raise ValueError("GraphedMemoryStep needs the bf16 K/V-cached decode path (model.use_decode)")
        self.model, self.B, self.q = model, batch_size, n_new
        dev = model.dev
        self.ids = torch.zeros(batch_size, n_new, dtype=torch.long, device=dev)
        self.x = (make_input or _token_input)(self.ids)
        self.mems: List[torch.Tensor] = model.init_mem(batch_size)
        self.graph = None
        self.logits = None
        # eager warm-up on the static buffers: allocates every workspace, builds the R table and the K/V cache of self.mems
        with torch.no_grad():
            for _ in range(2):
                _, _, m = model([self.x], compute_loss=False, mems=self.mems)
                st = model._dec_state
                for dst, src in zip(self.mems, m):
                    dst.copy_(src)
                self.kv = [k.contiguous().clone() for k in st.kv]
                model._dec_state = model._dec_pack(self.mems, self.kv)
        self._version = model._wversion
        torch.cuda.synchronize()
        self._capture()
        self.reset_memory()  # the warm-up calls advanced the memory

    def _capture(self):
        model = self.model
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), graph_capture(g):
            logits, _, m = model([self.x], compute_loss=False, mems=self.mems)
            new_kv = model._dec_state.kv
            for dst, src in zip(self.mems, m):
                dst.copy_(src)
            for dst, src in zip(self.kv, new_kv):
                dst.copy_(src)
        self.graph, self.logits = g, logits
        model._dec_state = model._dec_pack(self.mems, self.kv)

    def reset_memory(self):
        """start a new episode: zero memory (init_mem) and the matching K/V cache (rebuilt from the zero hidden states)"""
        model = self.model
        with torch.no_grad():
            for dst, src in zip(self.mems, model.init_mem(self.B)):
                dst.copy_(src)
            model._dec_state = None
            dec = model._decode_begin(self.mems, self.B, self.q, self.mems[0].shape[1])
            for dst, src in zip(self.kv, dec.kv):
                dst.copy_(src)
            model._dec_state = model._dec_pack(self.mems, self.kv)

    def __call__(self, ids: torch.Tensor):
        """ids [batch, n_new] -> (logits [batch, n_new, vocab] (static buffer, overwritten by the next call), memory list)"""
        if self.model._wversion != self._version:
            raise RuntimeError("the weights changed after the graph was captured: build a new GraphedMemoryStep")
        self.ids.copy_(ids)
        self.graph.replay()
        return self.logits, self.mems


class RingMemory:
    """Transformer-XL memory for hipGraph-replayed inference: per layer the projected keys / values of the last ``mem_len`` tokens in a
    ring [B, mem_len + 64, 2, H, D] (``kv_dtype`` "fp8": [B, mem_len + 64, 264 H] bytes), appended IN PLACE by the attention launch of
    each call (db1_relattn_decode_ring_fwd / db1_relattn_decode_ring_kv8_fwd), and a device scalar with the ring's origin.  Pass it as ``mems`` (``model(x, compute_loss=False, mems=ring)`` returns it back as the new memory).
    What it does not keep is the reference's memory CONTENT -- the hidden states (transformer_xl.py:470-504): a caller that reads or edits
    ``mems[i]`` needs the list form (``model.init_mem``); evaluate_rl's loop only hands the memory back to the model."""

    def __init__(self, model, batch_size: int, kv_dtype: str = "bf16"):
        """``kv_dtype`` "fp8": the keys / values as e4m3 payload with one power-of-two scale per (row, position, K or V, head) -- rings of
        uint8 [B, cap, 264 H], about half the bytes to stream per token and to hold (the format: include/db1_hip.h, "fp8 K/V ring")."""
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"RingMemory: kv_dtype must be 'bf16' or 'fp8' (got {kv_dtype!r})")
        if model.compute_dtype != torch.bfloat16 or not model.use_decode or model.d_head != 128 or not model.mem_len:
            raise ValueError("RingMemory needs the bf16 K/V-cached decode path (d_head 128, mem_len > 0)")
        from . import ops
        if kv_dtype == "fp8" and not ops.relattn_decode_ring_kv8_supported(batch_size, 1, int(model.mem_len) + 1, model.n_head, model.d_head):
            raise ValueError(f"RingMemory: no fp8 K/V ring for this model (d_head 128, an even number of heads and mem_len <= 2047 expected; "
                             f"got n_head {model.n_head}, d_head {model.d_head}, mem_len {model.mem_len})")
        self.model, self.B, self.kv_dtype = model, batch_size, kv_dtype
        self.cap = int(model.mem_len) + 64
        dev = model.dev
        if kv_dtype == "fp8":
            self.kv = [torch.zeros(batch_size, self.cap, ops.kv8_slot_bytes(model.n_head, model.d_head), device=dev, dtype=torch.uint8) for _ in range(model.n_layer)]
        else:
            self.kv = [torch.zeros(batch_size, self.cap, 2, model.n_head, model.d_head, device=dev, dtype=torch.bfloat16) for _ in range(model.n_layer)]
        self.state = torch.zeros(1, dtype=torch.int32, device=dev)
        self.load_status = torch.zeros(1, dtype=torch.int32, device=dev)   # (what load_rows skipped: db1_ring_load_rows' status word)
        self._ptrs = ops.ring_pointers(self.kv)   # (the layers' base pointers for reorder: made here, never under a capture)
        self.reset()

    def reset(self):
        """a new episode: the keys / values of the zero memory (init_mem), origin 0"""
        self.load(self.model.init_mem(self.B))

    def load(self, mems):
        """fill the ring from a list-form memory (``model.init_mem`` layout: per layer the hidden states [B, mem_len, d] a call with
        ``mems=`` returned, e.g. after a prompt longer than 64 tokens ran through the list-form path): the projection ``reset`` does for the
        zero memory, applied to the given states; origin 0"""
        from . import ops
        model, mlen = self.model, int(self.model.mem_len)
        if len(mems) != model.n_layer or any(tuple(m.shape) != (self.B, mlen, model.n_embed) for m in mems):
            raise ValueError(f"RingMemory.load: expected {model.n_layer} tensors of shape ({self.B}, {mlen}, {model.n_embed})")
        with torch.no_grad():
            for ring, kv in zip(self.kv, self._project(mems, self.B)):
                if self.kv_dtype == "fp8":
                    ops.kv8_quantize(kv.contiguous(), ring[:, :mlen])
                else:
                    ring[:, :mlen].copy_(kv)
            self.state.zero_()

    def _project(self, mems, n: int, mlen: int = None):
        """the projected keys / values of a list-form memory of n rows: per layer a [n, mem_len, 2, H, D] view (``mlen``: of that many
        positions instead of mem_len).  The model keeps the decode state it had, whatever the projection does (``load_rows`` runs in the
        middle of a stream)."""
        model, mlen = self.model, int(self.model.mem_len if mlen is None else mlen)
        saved, model._dec_state = model._dec_state, None
        try:
            dec = model._decode_begin(list(mems), n, 1, mlen)
        finally:
            model._dec_state = saved
        return [kv.reshape(n, mlen, 2, model.n_head, model.d_head) for kv in dec.kv]

    def load_rows(self, mems, rows: torch.Tensor):
        """continuous batching: the n requests of a list-form memory (per layer [n, mem_len, d], as ``load`` takes it for all B rows) take
        over rows ``rows`` (int32 [n] on the device, distinct) of the ring: the projection ``load`` does, then db1_ring_load_rows writes the
        keys / values relative to the CURRENT origin (read on the device, not zeroed), so the other rows go on undisturbed.  A row outside
        [0, B) is skipped and recorded in ``self.load_status`` (int32 [1], bit 0)."""
        from . import ops
        model, mlen = self.model, int(self.model.mem_len)
        n = int(rows.numel())
        if len(mems) != model.n_layer or any(tuple(m.shape) != (n, mlen, model.n_embed) for m in mems):
            raise ValueError(f"RingMemory.load_rows: expected {model.n_layer} tensors of shape ({n}, {mlen}, {model.n_embed})")
        if n > self.B:
            raise ValueError(f"RingMemory.load_rows: {n} rows for a ring of {self.B}")
        if n == 0:
            return
        with torch.no_grad():
            src = self._project(mems, n)
            if self.kv_dtype == "fp8":   # quantised into a temporary; the slots then travel as bytes like the bf16 ones
                slots = [torch.empty(n, mlen, self.kv[0].shape[2], device=model.dev, dtype=torch.uint8) for _ in src]
                for kv, sl in zip(src, slots):
                    ops.kv8_quantize(kv.contiguous(), sl)
                src = slots
            ops.ring_load_rows(self.kv, self._ptrs, src, self.state, mlen, rows, self.load_status)

    def reset_rows(self, rows):
        """new episodes in rows ``rows`` (distinct ints in [0, B), or an int32 vector of them on the device) while the others go on: those
        rows go back to the zero memory (``reset``'s keys / values) relative to the CURRENT origin through db1_ring_load_rows; no bit of
        another row changes.  The zero memory of one row is projected (and, on an fp8 ring, quantised) once per weight version and kept
        as many times as the largest reset so far had rows: a later reset of no more rows is the one launch, with no projection and no copy."""
        from . import ops
        model, mlen = self.model, int(self.model.mem_len)
        if not torch.is_tensor(rows):
            rows = [int(r) for r in rows]
            if len(set(rows)) != len(rows) or any(not 0 <= r < self.B for r in rows):
                raise ValueError(f"RingMemory.reset_rows: rows {rows} must be distinct and lie in [0, {self.B})")
            rows = torch.tensor(rows, dtype=torch.int32).to(model.dev)
        n = int(rows.numel())
        if n > self.B:
            raise ValueError(f"RingMemory.reset_rows: {n} rows for a ring of {self.B}")
        if n == 0:
            return
        z = getattr(self, "_zero_rows", None)
        if z is None or z[0] != model._wversion:
            with torch.no_grad():
                src = [kv.contiguous() for kv in self._project(model.init_mem(1), 1)]
                if self.kv_dtype == "fp8":
                    slots = [torch.empty(1, mlen, self.kv[0].shape[2], device=model.dev, dtype=torch.uint8) for _ in src]
                    for kv, sl in zip(src, slots):
                        ops.kv8_quantize(kv, sl)
                    src = slots
            z = self._zero_rows = [model._wversion, src]
        with torch.no_grad():
            # db1_ring_load_rows reads one source row per target row: the cached source holds the zero memory as many times as the largest
            # reset so far asked for (it grows, and is copied, only then); a smaller reset reads its first n rows
            if z[1][0].shape[0] < n:
                z[1] = [s[:1].expand(n, *s.shape[1:]).contiguous() for s in z[1]]
            ops.ring_load_rows(self.kv, self._ptrs, [s[:n] for s in z[1]], self.state, mlen, rows, self.load_status)

    def reorder(self, parent: torch.Tensor, t: torch.Tensor, max_t: int = None, group: int = 1, done: torch.Tensor = None):
        """beam search: after the call that appended token t - 1, give row b the keys / values of the last ``t`` tokens of row
        ``parent[b]`` in every layer (db1_ring_reorder; ``t`` a device int32 [1], read by the launch, so this can be captured).  The older
        keys -- the prompt's, loaded from one prefill -- are the same across a group's rows and are not copied.  ``parent`` int32 [B];
        ``group``: rows per group (a parent lies in its row's group); ``done`` (int32 [B / group]): groups left alone; ``max_t`` (default
        mem_len): the largest t the call will see (sizes the staging workspace)."""
        from . import ops
        mlen = int(self.model.mem_len)
        ops.ring_reorder(self.kv, self._ptrs, self.state, mlen, t, mlen if max_t is None else int(max_t), parent, W=group, done=done)


class GroupedRingMemory:
    """The memory of G groups of W rows that share their group's prompt (beam search, best-of-n sampling; the rule: include/db1_hip.h,
    "grouped K/V ring").  ``base``: a RingMemory of G rows -- ONE copy of every prompt's mem_len keys / values per layer, filled by a prefill
    (``RingPrefill(memory.base, ...)`` or ``memory.base.load``) and only read while decoding.  ``tail``: per layer a ring [G W, cap_t, 2, H, D]
    with the keys / values every row generated itself, at most ``tail_len`` of them; ``state`` (int32 [1]) is its origin and ``n_tail``
    (int32 [1]) the number of valid tail keys.  Pass it as ``mems`` of a one-token call of G W rows: every layer's attention is
    db1_relattn_decode_group_fwd, which reads the base once per group and appends the call's own keys to the tail; origin and count advance
    after the last layer.  ``status`` (int32 [1]): bit 0 when a launch met a count or an origin out of range (``check`` raises)."""
    is_group_ring = True
    kv_dtype = "bf16"

    def __init__(self, model, G: int, W: int, tail_len: int):
        from . import ops
        G, W, Lt = int(G), int(W), int(tail_len)
        if model.compute_dtype != torch.bfloat16 or not model.use_decode or model.d_head != 128 or not model.mem_len:
            raise ValueError("GroupedRingMemory needs the bf16 K/V-cached decode path (d_head 128, mem_len > 0)")
        if G < 1 or W < 1 or G * W < 2:
            raise ValueError(f"GroupedRingMemory: G = {G} groups of W = {W} rows (at least two rows in all; one row has nothing to share)")
        mlen = int(model.mem_len)
        self.cap_t = -(-(Lt + 1) // 8) * 8
        if not ops.relattn_decode_group_supported(G, W, mlen, Lt, mlen + 64, self.cap_t, model.n_head, model.d_head, model.compute_dtype):
            raise ValueError(f"GroupedRingMemory: db1_relattn_decode_group_fwd does not support W = {W}, mem_len = {mlen}, tail_len = {Lt} "
                             f"(1 <= W <= {ops.GROUP_MAX_W}, mem_len <= {ops.GROUP_MAX_KLEN - 1}, 1 <= tail_len <= {ops.GROUP_MAX_TAIL})")
        self.model, self.G, self.W, self.B, self.Lt = model, G, W, G * W, Lt
        dev = model.dev
        self.base = RingMemory(model, G)
        self.kv = [torch.zeros(self.B, self.cap_t, 2, model.n_head, model.d_head, device=dev, dtype=torch.bfloat16) for _ in range(model.n_layer)]
        self.state = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_tail = torch.zeros(1, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ptrs = ops.ring_pointers(self.kv)   # (the tail rings' base pointers for reorder: made here, never under a capture)

    def begin(self):
        """a new run: an empty tail at origin 0 (the base is the prefill's to fill; the tail's slots need no clearing)"""
        self.state.zero_()
        self.n_tail.zero_()
        self.status.zero_()

    def reset(self):
        self.base.reset()
        self.begin()

    def advance(self):
        from . import ops
        ops.group_ring_advance(self.state, self.n_tail, self.cap_t, self.Lt, int(self.model.mem_len))

    def reorder(self, parent: torch.Tensor, t: torch.Tensor, max_t: int = None, group: int = 1, done: torch.Tensor = None):
        """beam search: ``RingMemory.reorder`` on the tail alone -- the last ``t`` tail keys of row b come from row ``parent[b]``
        (db1_ring_reorder with the tail's window as its mlen); the base is the same for a group's rows and never moves"""
        from . import ops
        ops.ring_reorder(self.kv, self._ptrs, self.state, self.Lt, t, self.Lt if max_t is None else int(max_t), parent, W=group, done=done)

    def snapshot(self):
        """origin, count and tail as they are (the base is never written by a decode call)"""
        return self.state.clone(), self.n_tail.clone(), [k.clone() for k in self.kv]

    def restore(self, snap):
        state, n_tail, kv = snap
        self.state.copy_(state)
        self.n_tail.copy_(n_tail)
        for dst, src in zip(self.kv, kv):
            dst.copy_(src)

    def check(self):
        """raise if a launch over this memory met a count or an origin out of range (a host read)"""
        if int(self.status.cpu()) != 0:
            raise RuntimeError("db1_relattn_decode_group_fwd: the tail count or a ring origin left its range")


class RingPrefill:
    """A prompt prefill straight into a RingMemory: pass it as ``mems`` and the call's rows start from the zero memory (``model.init_mem``),
    project only their own tokens, attend over (the zero memory's keys / values, their own) with db1_relattn_mem_kv_fwd, and every layer's
    last ``mem_len`` keys / values are written into ring rows ``rows`` by db1_ring_prefill_rows, relative to the ring's CURRENT origin (read
    on the device, not advanced).  The call returns ``(logits, None, this object)``.
    ``rows``: int32 [n_dst] on the device, distinct rows of the ring (None: all ``ring.B`` rows, in order); ``src``: int32 [n_dst], the call
    row every destination descends from (None: destination i from call row i) -- ``arange(n_dst) // W`` expands every prompt to W rows
    without repeating or re-projecting anything.  Shapes and dtypes are checked here, on the host (ValueError before any launch); what the
    kernel skipped on the device (a row or a source out of range) is reported through ``ring.load_status`` (bits 0 / 2).
    ``base`` (a RingMemory of the same model and kv_dtype, not ``ring`` itself; generation.PrefixCache owns one): the call's rows CONTINUE
    rows of that ring instead of the zero memory -- call row b starts from the mem_len keys / values of ring row ``base_rows[b]`` (int32
    [B_call] on the device, repeats allowed; None: the identity, which needs ``base.B`` >= the call's rows) at ``base``'s origin: the
    attention is db1_relattn_mem_ring_fwd, the slot writer db1_ring_fork_rows, ``base`` is only read, and a base row or origin out of
    range sets bit 3 of ``ring.load_status``."""
    is_ring_prefill = True

    def __init__(self, ring: RingMemory, rows: torch.Tensor = None, src: torch.Tensor = None, base: RingMemory = None, base_rows: torch.Tensor = None):
        if not isinstance(ring, RingMemory):
            raise ValueError(f"RingPrefill: a RingMemory expected, got {type(ring).__name__}")
        dev = ring.state.device
        if base is None and base_rows is not None:
            raise ValueError("RingPrefill: base_rows without a base ring")
        if base is not None:
            if not isinstance(base, RingMemory) or base is ring:
                raise ValueError("RingPrefill: base must be a RingMemory other than the destination ring")
            if base.model is not ring.model or base.kv_dtype != ring.kv_dtype or base.state.device != dev:
                raise ValueError(f"RingPrefill: base must be a ring of the same model, device and kv_dtype ({ring.kv_dtype!r}; got {base.kv_dtype!r})")
        for name, x in (("rows", rows), ("src", src), ("base_rows", base_rows)):
            if x is None:
                continue
            if not torch.is_tensor(x) or x.dtype != torch.int32 or x.dim() != 1 or x.device != dev or not x.is_contiguous():
                raise ValueError(f"RingPrefill: {name} must be a contiguous int32 vector on {dev}")
        n_dst = ring.B if rows is None else int(rows.numel())
        if n_dst > ring.B:
            raise ValueError(f"RingPrefill: {n_dst} destinations for a ring of {ring.B} rows")
        if src is not None and int(src.numel()) != n_dst:
            raise ValueError(f"RingPrefill: src holds {int(src.numel())} entries for {n_dst} destinations")
        self.ring, self.src, self.n_dst = ring, src, n_dst
        self.base, self.base_rows = base, base_rows
        self.rows = rows if rows is not None else torch.arange(ring.B, dtype=torch.int32, device=dev)

    def check_batch(self, B: int):
        """the call's batch size against the destinations: without ``src`` destination i reads call row i"""
        if self.src is None and self.n_dst > int(B):
            raise ValueError(f"RingPrefill: {self.n_dst} destinations cannot be indexed by a call of {B} rows without a src map")
        if self.src is not None and int(B) < 1:
            raise ValueError("RingPrefill: an empty call")
        if self.base_rows is not None and int(self.base_rows.numel()) != int(B):
            raise ValueError(f"RingPrefill: base_rows holds {int(self.base_rows.numel())} entries for a call of {B} rows")
        if self.base is not None and self.base_rows is None and int(B) > self.base.B:
            raise ValueError(f"RingPrefill: a call of {B} rows over a base ring of {self.base.B} rows needs base_rows")

    def zero_kv(self):
        """per layer the keys / values of one position of the zero memory, [1, 1, 2, H, D]: what ``RingMemory.reset`` projects
        (``_project``, on one position of ``init_mem(1)``), once per weight version.  Passed to the kernels with strides 0; not assumed
        to be zero."""
        ring, model = self.ring, self.ring.model
        z = getattr(ring, "_zero_kv", None)
        if z is None or z[0] != model._wversion:
            with torch.no_grad():
                kv = [k.contiguous() for k in ring._project([m[:, :1] for m in model.init_mem(1)], 1, mlen=1)]
            z = ring._zero_kv = (model._wversion, kv)
        return z[1]


class GraphedRingStep:
    """One inference call with memory (batch ``batch_size``, ``n_new`` new tokens) as ONE hipGraph replay over a RingMemory: nothing is
    concatenated, copied or re-projected per call.  Several steps (e.g. the observation call and the 1-token calls of evaluate_rl) can
    share one memory: ``GraphedRingStep(model, 1, 1, memory=obs_step.memory)``.  ``epilogue(step, logits)`` (optional) is captured into the
    same graph after the forward, e.g. a token sampler that writes the next ids into ``step.ids`` (generation.py); the warm-up does not run it."""

    def __init__(self, model, batch_size: int, n_new: int, memory: RingMemory = None, make_input=None, epilogue=None):
        self.model, self.B, self.q = model, batch_size, n_new
        self.memory = memory if memory is not None else RingMemory(model, batch_size)
        assert self.memory.B == batch_size
        dev = model.dev
        self.ids = torch.zeros(batch_size, n_new, dtype=torch.long, device=dev)
        self.x = (make_input or _token_input)(self.ids)
        from . import ops
        saved_state = self.memory.state.clone()
        grouped = getattr(self.memory, "is_group_ring", False)   # (GroupedRingMemory: origin, count and tail go back through its own snapshot)
        snap = self.memory.snapshot() if grouped else None
        saved_kv = None if (memory is None or grouped) else [k.clone() for k in self.memory.kv]
        # the persistent one-token launches of THIS step hand over through a scratch of its own, with its own pinned copy of the error
        # flag -- both created here, eagerly: a scratch first touched under capture would be allocated and zero-filled by a graph node, i.e.
        # every replay would wipe the sticky flag before anyone read it (and all steps captured on torch's capture stream would share it)
        self._scratch, self._flag_host = ops.new_chain_scratch(dev)
        pending = model._chain_watch       # (the model's own watch of its eager calls stays what it was)
        with torch.no_grad():   # eager warm-up (workspaces, the R table), then the capture
            with ops.chain_scratch_scope(self._scratch, self._flag_host):
                for _ in range(2):
                    model([self.x], compute_loss=False, mems=self.memory)
                torch.cuda.synchronize()
                model._chain_watch = None
                g = torch.cuda.CUDAGraph()
                with graph_capture(g):
                    logits, _, _ = model([self.x], compute_loss=False, mems=self.memory)
                    if epilogue is not None:
                        epilogue(self, logits)
                watch = model._chain_watch
        self.graph, self.logits = g, logits
        self._watch = watch            # the captured call's copy of the persistent launches' error flag (None: per-launch path)
        model._chain_watch = pending
        self._version = model._wversion
        if grouped:
            self.memory.restore(snap)
        elif saved_kv is None:
            self.memory.reset()
        else:   # a shared memory keeps the state its owner left
            for dst, src in zip(self.memory.kv, saved_kv):
                dst.copy_(src)
            self.memory.state.copy_(saved_state)

    def reset_memory(self):
        self.memory.reset()

    def __call__(self, ids: torch.Tensor):
        """ids [batch, n_new] (or None / ``self.ids`` itself: the tokens are already in the static input buffer) ->
        (logits [batch, n_new, vocab] (static buffer, overwritten by the next call), the RingMemory)"""
        if self.model._wversion != self._version:
            raise RuntimeError("the weights changed after the graph was captured (or a persistent launch of this graph failed): build a new GraphedRingStep")
        self.check()   # the replays the stream has finished (free: a pinned host word)
        if ids is not None and ids.data_ptr() != self.ids.data_ptr():   # (a sampler that writes the next token into ``self.ids`` skips this copy)
            self.ids.copy_(ids)
        self.graph.replay()
        return self.logits, self.memory

    def check(self, synchronize: bool = False):
        """raise if a replayed persistent launch reported a failed hand-off (TransformerXL.check_decode_chain): call with
        ``synchronize=True`` before trusting logits that were not read back through a synchronising copy"""
        if self._watch is not None:
            try:
                self.model.check_decode_chain(synchronize, watch=self._watch)   # (this step's own flag copy; the model's pending watch is not touched)
            except Exception:
                # the captured graph still contains the persistent launches: this step must not be replayed again (the model has switched the
                # chain off, so a NEW GraphedRingStep captures the per-launch path)
                self._version = -1
                self._watch = None
                raise
