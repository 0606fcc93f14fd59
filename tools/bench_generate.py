#!/usr/bin/env python3
"""Caption generation at DB1-1.3B (bf16, seeded random init): a 3 x 224 x 224 image prompt, 30 new tokens, M rows at once; ms per token of

  * generate_captions on the graphed ring path (prefill excluded: the token loop, one hipGraph replay per token with db1_select_tokens
    writing the next ids on the device), greedy and top-p 0.9;
  * the bare GraphedRingStep replay at the same M (the one-token forward alone);
  * an eager loop over the same ring that picks each token with torch argmax and a host copy (.cpu()) per token -- the evaluate_rl pattern.

    python tools/bench_generate.py [M ...]   (default 1 16 64; prints one JSON line per M)
    under rocprofv3 --kernel-trace --stats: the kernel time of db1_select_tokens

With --num-beams W the arguments are group counts G (default 1 16), and per G (M = G * W rows):

  * generate_captions with a BeamSearchConfig (W beams, no EOS) on the graphed ring path, ms per token as above;
  * the bare GraphedRingStep replay at M;
  * db1_beam_step alone (bf16 logits [M, 33 025], the text window) and db1_ring_reorder alone at t = 29 (every row takes its neighbour's
    history: 2 x M x 29 x n_layer slots read and written), device time per call from events over 50 calls.

    python tools/bench_generate.py --num-beams 4 [G ...]
With --beam-groups D --diversity LAMBDA (diverse beam search: D sub-groups of W / D beams, db1_beam_step_diverse) the same lines, each with
"beam_groups" and "diversity"; beam_step_us is then the diverse step's.
    python tools/bench_generate.py --num-beams 4 --beam-groups 2 --diversity 0.5 [G ...]
With --num-beams W --diversity-report [--diversity LAMBDA] (default 0.5): one line per divisor D of W with the mean pairwise Hamming
distance between a prompt's W results, the mean number of distinct first tokens and the mean best score against D = 1.

With --stream: continuous batching (serving.caption_stream) against lockstep batches.  256 one-image requests, 64 slots, per-request token
limits drawn once from a seeded uniform 5 .. 30 (random weights never emit EOS); one JSON line with

  * the per-replay cost of the slot graph (forward + db1_select_tokens_slots, every slot live) and of generate's graph at M = 64;
  * the total time of the stream and of generate_captions over the same requests in batches of 64 in order, each run to its longest limit
    (prefills included in both), the replay counts, the occupancy, and what the admissions cost (total - replays x per-replay cost);
  * db1_ring_load_rows alone: 16 rows into a ring of 64, device time from events, bytes read + written.

    python tools/bench_generate.py --stream [requests [slots]]
    python tools/bench_generate.py --stream --mem-attn [requests [slots]]   (model.use_mem_attn = True: the admissions' prefills through
                                                                            db1_relattn_mem_fwd; the line carries "mem_attn": true)
    python tools/bench_generate.py --ring-prefill [any of the forms above]   (model.use_ring_prefill = True: the prompt prefills go straight
                                                                            into the K/V ring; every line carries "ring_prefill": true)

With --stream --shared-prefix K: 64 images x K questions of 10 tokens as 64 K requests over 64 slots, the whole VQA prompt per request
against one ``PrefixCache.put`` per image and a ``Prefixed`` question per request (generation.PrefixCache); totals, admission times, the
puts' time and the slot graph's replay time, one JSON line.

    python tools/bench_generate.py --stream --shared-prefix 4 [images [slots]]
    python tools/bench_generate.py --ring-prefill --stream --shared-prefix 4 [images [slots]]   (the unshared form through the ring prefill)

With --stream --per-request: the stream workload above with every second request greedy and the others at top-p 0.9
(``caption_stream(..., per_request=True)``, a ``SamplingParams`` on the sampled requests: the graph ends in db1_select_tokens_slots_per)
next to the shared-config (greedy) stream of the same requests; one JSON line with the totals (``*_total_ms``: the best of 3 timed passes
after a warm-up pass, as --stream reports it; ``*_runs_ms``: all three, for medians) and replay counts, and
db1_select_tokens_slots_per against db1_select_tokens_slots alone from the same process and the same events on random bf16 logits
[slots, 33 025] over the text window: all slots greedy, all at top-p 0.9, and half and half (per-slot form only); the plain
instantiations only.

    python tools/bench_generate.py --stream --per-request [requests [slots]]

With --stream --per-request-constraints: the stream workload above (greedy) in three forms: flag off, ``per_request_constraints=True``
with no request carrying constraints, and the flag with every second request under DecodingConstraints(repetition_penalty=1.2,
no_repeat_ngram_size=3) -- the graph's epilogue is db1_constrain_logits_slots_per, the selection, db1_stop_match_per --; one JSON line
with the totals (``*_total_ms`` / ``*_runs_ms`` as --per-request reports them) and replay counts, and the two per-slot kernels alone on
bf16 logits [slots, 33 025] after t = 29 tokens per slot: all records no-op, all under those constraints, half of each, next to
db1_constrain_logits with the same scalars; db1_stop_match_per over empty tables and over 16 x 16 tables next to db1_stop_match.

    python tools/bench_generate.py --stream --per-request-constraints [requests [slots]]
    python tools/bench_generate.py --slot-constrain-kernels noop|constrained|half_and_half [M]   (the two kernels alone over ONE kind of
                                                                                                  table: the run to trace)

With --constraints: the greedy caption measurement above, unconstrained and with DecodingConstraints(repetition_penalty=1.2,
no_repeat_ngram_size=3, min_new_tokens=5) -- one db1_constrain_logits launch more in every replay (no EOS, as in every run here, so
the minimum length bans nothing) --, one JSON line per M; under rocprofv3 --kernel-trace --stats: the kernel time of db1_constrain_logits.

    python tools/bench_generate.py --constraints [M ...]

--constraints takes the newer fields as flags of their own, added to the constraints above: --penalties (frequency_penalty 0.5,
presence_penalty 0.5: the launch becomes db1_constrain_logits_pen), --logit-bias N (an N-entry bias, ids spread over the text vocabulary)
and --stop-sequences (two sequences of ids outside the text window, so they never match: one db1_stop_match launch more in every replay
and no row ends early).  --constrain-kernels [M]: the kernels alone, device time per call from events in ONE process:
db1_constrain_logits (theta 1.2) and db1_constrain_logits_pen (theta 1.2, both penalties, a 16-entry bias) on bf16 logits [M, 33 025] over
histories of t = 255 / 1023 / 4095 DISTINCT tokens (the worst case of the first-occurrence and count scans), and db1_stop_match with 16
sequences of 16 tokens whose first 15 tokens every row's tail matches (every lane compares to the end, nothing is trimmed).

    python tools/bench_generate.py --constraints --penalties --logit-bias 16 --stop-sequences [M ...]
    python tools/bench_generate.py --constrain-kernels [M]

With --logprobs: the greedy and top-p 0.9 caption measurements above with ``GenerationConfig(logprobs=False)`` and ``logprobs=True`` (the
replay ends in db1_select_tokens_lp instead of db1_select_tokens), and the two kernels alone on random bf16 logits [M, 33 025] over the text
window (device time per call from events over 50 calls), one JSON line per M; under rocprofv3 --kernel-trace --stats: the kernel times of
the LP and the plain instantiation of select_tokens_kernel.

    python tools/bench_generate.py --logprobs [M ...]
    python tools/bench_generate.py --select-kernels greedy|top_p_0.9 [M]   (the two kernels alone in ONE mode: the run to trace)
    python tools/bench_generate.py --logprobs --top-logprobs N [M ...]     (also ``top_logprobs=N``: the loop, its delta over logprobs=True,
                                                                            and db1_select_tokens_top alone)

With --best-of N the arguments are group counts G (default 16): sample_best_of (N samples per image, top-p 0.9, M = G * N rows) next to
beam search with N beams over the same images, ms per token as above.

    python tools/bench_generate.py --best-of 4 [G ...]

--kv-cache fp8 (with the default mode): the same measurements over an fp8 K/V ring (``kv_cache="fp8"``, ``RingMemory(kv_dtype="fp8")``);
every line carries "kv_cache" and the ring's bytes at that M.

    python tools/bench_generate.py --kv-cache fp8 [M ...]

--share-prompt (with --num-beams or --best-of): ``share_prompt=True`` -- the rows of a group read ONE copy of their prompt's keys / values
(``GroupedRingMemory``, db1_relattn_decode_group_fwd); every line carries "share_prompt": true and the bytes of the memory.

    python tools/bench_generate.py --num-beams 4 --share-prompt [G ...]
    python tools/bench_generate.py --best-of 4 --share-prompt [G ...]

--group-kernels [G W [n_tail ...]] (default 16 4 0 29): db1_relattn_decode_group_fwd alone against db1_relattn_decode_ring_fwd at B = G W
(q = 1, mlen = 1024, 16 heads, tail window 30), in alternation in ONE process.  Each side is a captured graph of one launch over each of
n distinct memories (more bytes than the last-level cache holds); device time per launch from events over 5 replays, the median of 7
rounds with min .. max, and the key / value bytes a launch reads.

    python tools/bench_generate.py --group-kernels [G W [n_tail ...]]

--kv8-kernels [B ...] (default 1 16 64): the two attention entry points alone, db1_relattn_decode_ring_fwd and
db1_relattn_decode_ring_kv8_fwd, in alternation in ONE process: q = 1, mlen = 1024, 16 heads, the merge as a second launch (what the
model's plain path launches) and, for B <= 2, the partials form; device time per call from events over 20 calls, the median of 7 rounds
each, with the ring bytes a call reads and the rate they amount to.

    python tools/bench_generate.py --kv8-kernels [B ...]

--decode-weights fp8 (with any mode): ``model.set_decode_weights("fp8")`` first -- the decode calls stream e4m3 copies of the layers' four
linear maps, and the one-token call takes the per-layer launches instead of the persistent chain; every line carries "decode_weights".

    python tools/bench_generate.py --decode-weights fp8 [M ...]
    python tools/bench_generate.py --decode-weights fp8 --fp8-chain [M ...]   (``set_decode_weights("fp8", chain=True)``: the one-token call
                                                                               stays on the persistent chain, db1_decode_chain_w8; every
                                                                               line carries "decode_chain_w8": true)

--chain-kernels: db1_decode_chain and db1_decode_chain_w8 alone, a layer's launch with the next layer's projection at mlen = 1024, in
alternation in ONE process.  Each side is a captured graph of one launch over each of 12 distinct sets of the five weights (1 GB of bf16,
520 MB of fp8: more than the last-level cache holds); device time per launch from events over 5 replays, the median of 7 rounds with
min .. max, the bytes of W a launch streams, and workgroup 0's stage times (db1_test_decode_chain_timestamps) of the last launch of an eager
sweep, the median of 3, so the record shows which stage the bytes came out of.

    python tools/bench_generate.py --chain-kernels

--w8-kernels [M ...] (default 1 4 16 64): db1_linear_decode and db1_linear_decode_w8 alone at the model's four layer shapes (qkv_net, o_net,
CoreNet.0 through GEGLU, CoreNet.2), in alternation in ONE process.  Each side is a captured graph of one launch over each of n copies of
the weight (600 MB of bf16 copies: more bytes than the last-level cache holds, as the 24 layers of a decode step are), so a replay is device
time without the host's launch cost; device time per launch from events over 5 replays, the median of 7 rounds with min .. max, the bytes of W a launch
streams and the rate they amount to.

    python tools/bench_generate.py --w8-kernels [M ...]

--speculative K [--draft-script perfect|wrong] [--text-prompt] [M ...] (default M = 1 4): ``generate(..., speculative=SpeculativeConfig(
num_draft_tokens=K))`` against plain ``generate`` on the same prompt in ONE process, greedy, ms per generated token by the difference
method of the default mode (30 tokens minus 10); every line carries "speculative", the draft source, the accepted histogram and the
tokens per call of the 30-token run.  Drafts: the n-gram lookup (default), the tokens of a speculative run that never accepts (perfect: the
ceiling) or an id outside the window (wrong: the cost of never accepting).  The prompt: the caption prompt, or with --text-prompt 64 text tokens that repeat an
8-token pattern.

    python tools/bench_generate.py --speculative 4 [--draft-script perfect|wrong] [--text-prompt] [M ...]

--spec-replay [B:n ...] (default 1:1 1:2 1:5 1:8 4:5): the bare ``GraphedRingStep`` replay of a call of n new tokens for B rows, ms per call.
--spec-logits: the same 22 tokens through the ring one per call, five per call, and five per call behind a first call of two: the largest
and the root-mean-square distance between the three paths' text-window logits relative to the largest logit, the relative gap between a
position's two largest logits, and how many positions' arg-max agree; each path also against an fp32 model on the same parameters.
--spec-kernels [rows ...] (default 5 64): db1_spec_pick / db1_spec_accept / db1_spec_commit at V = 33 025 over that many logits rows (Q = 5 for
5 rows, 16 otherwise) and db1_select_tokens over the same number of rows, device time from events, the median of 7 rounds."""
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdm_db1_amd import BeamSearchConfig, DecodingConstraints, GenerationConfig, GraphedRingStep, TransformerXL, generate_captions, lib, ops, synth  # noqa: E402
from bdm_db1_amd.data import ICTaskInput, NLPTaskInput  # noqa: E402
lib.apply_env_knobs()

N_NEW, REPS = 30, 3
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=torch.bfloat16)
model.eval()


def batch(M):
    rng = np.random.default_rng(M)
    return ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None,
                       prompt_seq=torch.from_numpy(rng.integers(0, 32000, (M, 4))).to(dev),
                       img_seq=torch.from_numpy(rng.standard_normal((M, 3, 224, 224)).astype(np.float32)).to(dev), text_seq=None)


def gen_ms_per_token(M, cfg, short=10, **kw):
    """the token loop of generate_captions: (time of N_NEW tokens - time of `short` tokens) / (N_NEW - short) -- the prefill, the ring load
    and the first selection are the same in both and cancel; ``kw``: handed to generate_captions (constraints=)"""
    b = batch(M)

    def best(c):
        generate_captions(model, b, c, **kw)            # capture + warm-up
        t = 1e30
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_captions(model, b, c, **kw)
            t = min(t, time.perf_counter() - t0)
        return t

    full = best(cfg)
    part = best(dataclasses.replace(cfg, max_new_tokens=short))
    return (full - part) / (N_NEW - short) * 1e3


def text_batch(M, n=64, period=8):
    rng = np.random.default_rng(100 + M)
    pat = rng.integers(0, 32000, (M, period))
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None,
                        text_seq=torch.from_numpy(np.tile(pat, (1, n // period))).to(dev), text_len=None)


def spec_main(K, script_mode, Ms, text):
    from bdm_db1_amd import SpeculativeConfig, generate
    from bdm_db1_amd.generation import _text_window, caption_prompt
    sc = SpeculativeConfig(num_draft_tokens=K)
    for M in Ms:
        x = text_batch(M) if text else caption_prompt(batch(M))
        cfg = _text_window(model, GenerationConfig(max_new_tokens=N_NEW))
        short = dataclasses.replace(cfg, max_new_tokens=10)
        plain_ids = generate(model, x, cfg)[0].numpy()
        wrong = np.full((M, N_NEW), int(model.text_vocab_size), np.int32)
        # perfect: the tokens of the Q-token call itself, from a run that never accepts (on random weights the logits are near ties, and
        # the bf16 rounding of the one-row chain and of the Q-row launches can part the two paths' arg-max)
        own_ids = generate(model, x, cfg, speculative=sc, draft_script=wrong)[0].numpy() if script_mode == "perfect" else None

        def script(c):
            if script_mode is None:
                return {}
            n = c.max_new_tokens
            return dict(draft_script=own_ids[:, :n] if script_mode == "perfect" else wrong[:, :n])

        def best(c, **kw):
            generate(model, x, c, **kw)            # capture + warm-up
            t = 1e30
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                generate(model, x, c, **kw)
                t = min(t, time.perf_counter() - t0)
            return t

        rec = {"M": M, "new_tokens": N_NEW, "speculative": K, "drafts": script_mode or "lookup", "prompt": "text" if text else "caption"}
        rec["plain_ms_per_token"] = round((best(cfg) - best(short)) / (N_NEW - 10) * 1e3, 4)
        rec["speculative_ms_per_token"] = round((best(cfg, speculative=sc, **script(cfg)) - best(short, speculative=sc, **script(short))) / (N_NEW - 10) * 1e3, 4)
        st = {}
        ids = generate(model, x, cfg, speculative=sc, stats=st, **script(cfg))[0].numpy()
        rec.update(accepted=st["accepted"], tokens_per_call=round(st["tokens_per_call"], 3), token_calls=st["token_calls"],
                   same_tokens_as_plain=bool((ids == plain_ids).all()), tokens_equal_to_plain=int((ids == plain_ids).sum()),
                   **({"same_tokens_as_script": bool((ids == own_ids).all())} if own_ids is not None else {}), speculative_over_plain=round(rec["speculative_ms_per_token"] / rec["plain_ms_per_token"], 4))
        print(json.dumps(rec), flush=True)
        model._generator = model._spec_generator = None
        torch.cuda.empty_cache()


def spec_replay_main(pairs, calls=N_NEW):
    for B, n in pairs:
        step = GraphedRingStep(model, batch_size=B, n_new=n)
        for _ in range(5):
            step(step.ids)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                step(step.ids)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / calls * 1e3)
        step.check(synchronize=True)
        del step
        torch.cuda.empty_cache()
        print(json.dumps({"B": B, "n_new": n, "bare_ring_replay_ms": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}),
              flush=True)


def spec_logits_main(Q=5, n=22):
    """the same n tokens through the K/V ring cut into calls in three ways -- one token per call (the persistent chain), Q per call, and Q per
    call behind a first call of 2 (every token at another position of its call) -- and how far the text-window logits of the three lie apart,
    next to the gap between the two largest logits of a position: what decides whether the arg-max of two paths can differ"""
    from bdm_db1_amd.decode import RingMemory
    toks = torch.from_numpy(np.random.default_rng(7).integers(0, 32000, (1, n))).to(dev)
    V = int(model.text_vocab_size)

    def run(cuts):
        ring, out, at = RingMemory(model, 1), [], 0
        with torch.no_grad():
            for L in cuts:
                x = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=toks[:, at:at + L], text_len=None)
                logits, _, _ = model([x], compute_loss=False, mems=ring)
                out.append(logits[0, :, :V].float().cpu().numpy())
                at += L
        assert at == n
        return np.concatenate(out)

    wide = [Q] * (n // Q) + ([n % Q] if n % Q else [])
    a, b, c = run([1] * n), run(wide), run([2] + [Q] * ((n - 2) // Q) + ([(n - 2) % Q] if (n - 2) % Q else []))
    # the reference: an fp32 model on the same parameters, the n tokens in ONE list-form call after the zero memory (under same_length the
    # same function of the tokens, however they are cut into calls)
    ref_model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=torch.float32)
    ref_model.load_state_dict(model.state_dict(), strict=False)
    ref_model.eval()
    with torch.no_grad():
        x = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=toks, text_len=None)
        ref = ref_model([x], compute_loss=False, mems=ref_model.init_mem(1))[0][0, :, :V].float().cpu().numpy()
    del ref_model
    top = np.sort(ref, axis=1)[:, -2:]
    gap = (top[:, 1] - top[:, 0]) / np.abs(ref).max(axis=1)
    rel = lambda u, v: float((np.abs(u - v).max(axis=1) / np.abs(u).max(axis=1)).max())
    rms = lambda u, v: float(np.sqrt(((u - v) ** 2).mean()) / np.abs(u).max())
    rec = {"Q": Q, "positions": n, "mem_len": int(model.mem_len), "max_abs_logit": round(float(np.abs(ref).max()), 4)}
    for name, u in (("one", a), ("wide", b), ("shifted", c)):      # every bf16 path against the fp32 reference
        rec.update({f"{name}_vs_fp32_max_rel": rel(ref, u), f"{name}_vs_fp32_rms_rel": rms(ref, u),
                    f"argmax_equal_{name}_vs_fp32": int((ref.argmax(1) == u.argmax(1)).sum())})
    rec.update({"one_vs_wide_max_rel": rel(a, b), "one_vs_wide_rms_rel": rms(a, b), "wide_vs_shifted_max_rel": rel(b, c), "wide_vs_shifted_rms_rel": rms(b, c),
           "top2_gap_rel_median": float(np.median(gap)), "top2_gap_rel_min": float(gap.min()), "positions_with_tied_top2": int((gap == 0).sum()),
           "argmax_equal_one_vs_wide": int((a.argmax(1) == b.argmax(1)).sum()), "argmax_equal_wide_vs_shifted": int((b.argmax(1) == c.argmax(1)).sum())})
    print(json.dumps(rec), flush=True)


def spec_kernels_us(rows, rounds=7):
    V, ld, hi, mx = int(model.total_vocab_size), int(model.vocab_pad), int(model.text_vocab_size), 64
    Q = 5 if rows <= 5 else 16
    M = rows // Q
    i32 = dict(dtype=torch.int32, device=dev)
    lg = (torch.randn(M * Q, ld, device=dev) * 3).to(torch.bfloat16)
    t, fin, lens, status, n_acc, hist, ring = (torch.zeros(n, **i32) for n in (1, M, M, M, 1, Q + 1, 1))
    out, sel, hit = torch.zeros(M, mx, **i32), torch.zeros(M, Q, **i32), torch.zeros(M, Q, **i32)
    ids = torch.zeros(M, Q, dtype=torch.long, device=dev)
    ctx, ctx_len = torch.zeros(M, 4096 - mx, **i32), torch.full((M,), 64, **i32)
    nxt, t1 = torch.zeros(M * Q, dtype=torch.long, device=dev), torch.zeros(1, **i32)
    f2, l2, s2, o2 = torch.zeros(M * Q, **i32), torch.zeros(M * Q, **i32), torch.zeros(M * Q, **i32), torch.zeros(M * Q, mx, **i32)

    def reset():
        t.zero_(); fin.zero_(); f2.zero_()
    fns = dict(spec_pick=lambda: ops.spec_pick(lg, t, fin, ids, sel, hit, q_in=Q, V=V, vocab_hi=hi, max_new=mx),
               spec_accept=lambda: ops.spec_accept(t, sel, hit, fin, lens, out, status, ids, n_acc, q_in=Q, V=V, ctx=ctx, ctx_len=ctx_len),
               spec_commit=lambda: ops.spec_commit(t, n_acc, q_in=Q, Q=Q, hist=hist, ring_state=ring, cap=1088),
               select_tokens=lambda: ops.select_tokens(lg, t1, f2, l2, o2, nxt, s2, V=V, vocab_hi=hi))
    rec = {"rows": rows, "M": M, "Q": Q, "V": V}
    for name, fn in fns.items():
        us = []
        for _ in range(rounds):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            reset()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        rec[f"{name}_us"] = round(float(np.median(us)), 2)
        rec[f"{name}_min_max_us"] = [round(min(us), 2), round(max(us), 2)]
    return rec


KV_CACHE = "bf16"      # --kv-cache
SHARE_KW = {}          # --share-prompt: dict(share_prompt=True)
BEAM_KW = {}           # --beam-groups D --diversity lambda: dict(num_beam_groups=D, diversity_penalty=lambda)


def _memory_bytes(gen):
    """the bytes of a ring generator's memory: the rings of a RingMemory, or base + tail of a GroupedRingMemory"""
    mem = gen.ring
    rings = list(mem.kv) + (list(mem.base.kv) if getattr(mem, "is_group_ring", False) else [])
    return sum(k.numel() * k.element_size() for k in rings)


def group_kernels_us(G, W, n_tail, mlen=1024, Lt=N_NEW, rounds=7, replays=5, n=8):
    """the grouped attention and the per-row ring attention alone at q = 1 (the docstring above says how)"""
    H, D, M = model.n_head, model.d_head, G * W
    cap_b, cap_t = mlen + 64, -(-(Lt + 1) // 8) * 8
    slot = 2 * H * D * 2
    # n memories a side: at G = 16, W = 4 that is 8 x 570 MB of per-row rings and 8 x 143 MB of base rings, both beyond the last-level cache
    g = torch.Generator(device=dev).manual_seed(G * 100 + W)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    qkv, u, vb, R = rnd(M, 1, 3, H, D), rnd(H, D), rnd(H, D), rnd(cap_b, H * D)
    rings = [rnd(M, cap_b, 2, H, D) for _ in range(n)]
    bases = [rnd(G, cap_b, 2, H, D) for _ in range(n)]
    tails = [rnd(M, cap_t, 2, H, D) for _ in range(n)]
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    state, state_b, state_t, nt, status = i32(0), i32(0), i32(3), i32(n_tail), i32(0)
    out = torch.empty(M, 1, H, D, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / D ** 0.5
    sides = {"ring": lambda i: ops.relattn_decode_ring_fwd(qkv, u, vb, rings[i], state, R, out, M, 1, mlen, H, D, mlen + 1, scale),
             "group": lambda i: ops.relattn_decode_group_fwd(qkv, u, vb, bases[i], state_b, tails[i], state_t, nt, Lt, R, out, G, W, mlen, H, D, mlen + 1,
                                                             scale, status)}
    graphs = {}
    for name, fn in sides.items():
        fn(0)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(n):
                fn(i)
        graphs[name] = gr
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, gr in graphs.items():
            gr.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / (replays * n) * 1e3)
    assert int(status.cpu()) == 0
    rec = {"G": G, "W": W, "M": M, "mlen": mlen, "H": H, "tail_len": Lt, "n_tail": n_tail, "memories": n}
    read = {"ring": M * mlen * slot, "group": (G * (mlen - n_tail) + M * n_tail) * slot}
    for name in sides:
        t = sorted(times[name])
        rec[f"{name}_us"] = round(t[len(t) // 2], 2)
        rec[f"{name}_us_min_max"] = [round(t[0], 2), round(t[-1], 2)]
        rec[f"{name}_read_MB"] = round(read[name] / 1e6, 1)
        rec[f"{name}_TBps"] = round(read[name] / (t[len(t) // 2] * 1e-6) / 1e12, 3)
    rec["group_over_ring"] = round(rec["group_us"] / rec["ring_us"], 4)
    return rec


def kv8_kernels_us(B, mlen=1024, rounds=7, calls=20):
    """the bf16 and the fp8 ring attention alone at q = 1 (the docstring above says how)"""
    H, D, cap = model.n_head, model.d_head, mlen + 64
    g = torch.Generator(device=dev).manual_seed(B)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    qkv, u, vb, R = rnd(B, 1, 3, H, D), rnd(H, D), rnd(H, D), rnd(cap, H * D)
    ring16 = rnd(B, cap, 2, H, D)
    ring8 = torch.empty(B, cap, ops.kv8_slot_bytes(H, D), dtype=torch.uint8, device=dev)
    ops.kv8_quantize(ring16, ring8)
    state = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(B, 1, H, D, device=dev, dtype=torch.bfloat16)
    part = torch.empty(ops.relattn_decode_ring_part_numel(B, 1, mlen + 1, H), device=dev, dtype=torch.float32)
    scale = 1.0 / D ** 0.5
    fns = {"bf16": lambda o, **kw: ops.relattn_decode_ring_fwd(qkv, u, vb, ring16, state, R, o, B, 1, mlen, H, D, mlen + 1, scale, **kw),
           "fp8": lambda o, **kw: ops.relattn_decode_ring_kv8_fwd(qkv, u, vb, ring8, state, R, o, B, 1, mlen, H, D, mlen + 1, scale, **kw)}
    rec = {"B": B, "q": 1, "mlen": mlen, "H": H}
    forms = [("out", lambda f: f(out))] + ([("partials", lambda f: f(None, part=part))] if B <= 2 else [])
    for form, call in forms:
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                times[k].append(device_us(lambda: call(f), calls))
        for k, ring in (("bf16", ring16), ("fp8", ring8)):
            us = float(np.median(times[k]))
            nbytes = B * mlen * ring[0, 0].numel() * ring.element_size()
            rec[f"{k}_{form}_us"] = round(us, 2)
            rec[f"{k}_{form}_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
            rec[f"{k}_ring_MB"] = round(nbytes / 1e6, 2)
            rec[f"{k}_{form}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
        rec[f"fp8_over_bf16_{form}"] = round(rec[f"fp8_{form}_us"] / rec[f"bf16_{form}_us"], 4)
    return rec


def w8_kernels_us(M, rounds=7, replays=5):
    """db1_linear_decode and db1_linear_decode_w8 alone at the model's four layer shapes (the docstring above says how)"""
    d, dff = model.d_model, model.d_ff
    g = torch.Generator(device=dev).manual_seed(M)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(torch.bfloat16)
    rec = {"M": M}
    for name, N, K, geglu in (("qkv_net", 3 * d, d, False), ("o_net", d, d, False), ("CoreNet.0", dff, d, True), ("CoreNet.2", d, dff, False)):
        rows = 2 * N if geglu else N
        copies = -(-600_000_000 // (2 * rows * K))      # 600 MB of bf16 copies, 310 MB of fp8 ones: neither set stays in the 256 MB last-level cache
        Ws = [rnd(rows, K, sc=0.02) for _ in range(copies)]
        W8s = [ops.w8_quantize(w) for w in Ws]
        bias = rnd(rows, sc=0.1) if name.startswith("CoreNet") else None
        x, y = rnd(M, K), torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        assert ops.linear_decode_w8_supported(M, N, K, geglu)
        graphs = {}
        for k, fn, ws in (("bf16", ops.linear_decode, Ws), ("fp8", ops.linear_decode_w8, W8s)):
            fn(x, ws[0], bias, y, geglu=geglu)          # (workspace and tickets exist before the capture)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for w in ws:
                    fn(x, w, bias, y, geglu=geglu)
            graphs[k] = gr
        times = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, gr in graphs.items():
                times[k].append(device_us(gr.replay, replays) / copies)
        for k, ws in (("bf16", Ws), ("fp8", W8s)):
            us = float(np.median(times[k]))
            nbytes = ws[0].numel() * ws[0].element_size()
            rec[f"{name}_copies"] = copies
            rec[f"{name}_{k}_us"] = round(us, 2)
            rec[f"{name}_{k}_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
            rec[f"{name}_{k}_W_MB"] = round(nbytes / 1e6, 2)
            rec[f"{name}_{k}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
        rec[f"{name}_fp8_over_bf16"] = round(rec[f"{name}_fp8_us"] / rec[f"{name}_bf16_us"], 4)
        del Ws, W8s, graphs
        torch.cuda.empty_cache()
    return rec


CHAIN_STAMPS = ("start", "A0", "B0", "y_o polled", "LN1", "A1", "B1", "act polled", "act in LDS", "A2", "B2", "f polled", "LN2", "A3")


def chain_kernels_us(copies=12, rounds=7, replays=5, mlen=1024):
    """db1_decode_chain and db1_decode_chain_w8 alone: a layer's launch (with the next layer's projection) over ``copies`` distinct sets of the
    five weights, bf16 against fp8 (the docstring above says how), and workgroup 0's stage times of one launch of each"""
    import ctypes
    d, dff, H, D = model.d_model, model.d_ff, model.n_head, model.d_head
    assert ops.decode_chain_w8_supported(d, dff, H, D, mlen + 1)
    nunit = (mlen + 1 + 127) // 128
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(torch.bfloat16)
    shapes = (("o", d, d), ("w1", 2 * dff, d), ("w2", d, dff), ("qkv", 3 * d, d))
    Ws = [{k: rnd(N, K, sc=0.02) for k, N, K in shapes} for _ in range(copies)]      # 84 MB of bf16 per copy, 43 MB of fp8
    W8s = [{k: ops.w8_quantize(w) for k, w in ws.items()} for ws in Ws]
    x, b1, b2 = rnd(1, d), rnd(2 * dff, sc=0.1), rnd(d, sc=0.1)
    g1, be1, g2, be2 = 1 + rnd(d, sc=0.1), rnd(d, sc=0.1), 1 + rnd(d, sc=0.1), rnd(d, sc=0.1)
    part = torch.zeros(H, nunit, 64, D + 2, device=dev)
    part[:, :, 0, :D] = torch.randn(H, nunit, D, device=dev, generator=g)
    part[:, :, 0, D] = torch.randn(H, nunit, device=dev, generator=g)
    part[:, :, 0, D + 1] = torch.rand(H, nunit, device=dev, generator=g) + 0.5
    xn, qn = torch.empty(1, d, device=dev, dtype=torch.bfloat16), torch.empty(1, 3 * d, device=dev, dtype=torch.bfloat16)
    sides = {"bf16": (ops.decode_chain, Ws), "fp8": (ops.decode_chain_w8, W8s)}

    def sweep(k):       # one launch per copy, consecutive slots; each touches the o_net rows of the next, as a model's layers do
        fn, ws = sides[k]
        for i, w in enumerate(ws):
            fn(part, mlen + 1, H, x, w["o"], w["w1"], b1, w["w2"], b2, w["qkv"], g1, be1, g2, be2, 1.0, 1e-5, None, None, xn, qn, i, w_o_next=ws[(i + 1) % copies]["o"])
    scratch = ops.new_chain_scratch(dev)
    off = int(lib.load().db1_decode_chain_error_offset())
    rec = {"copies": copies, "mlen": mlen}
    with ops.chain_scratch_scope(*scratch):
        graphs = {}
        for k in sides:
            sweep(k)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                sweep(k)
            graphs[k] = gr
        times = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, gr in graphs.items():
                times[k].append(device_us(gr.replay, replays) / copies)
        # stage times: the last launch of an eager sweep (its weights were read a whole sweep ago), workgroup 0's service wave, us since its start
        L = lib.load()
        L.db1_test_decode_chain_timestamps.restype = None
        ts = torch.zeros(16 + 2048, dtype=torch.int64, device=dev)
        for k in sides:
            stamps = []
            for _ in range(3):
                L.db1_test_decode_chain_timestamps(ctypes.c_void_p(ts.data_ptr()), copies - 1)
                sweep(k)
                torch.cuda.synchronize()
                t = ts.cpu().numpy().astype(np.float64)
                stamps.append((t[1:len(CHAIN_STAMPS)] - t[0]) / 100)
            L.db1_test_decode_chain_timestamps(ctypes.c_void_p(0), -1)
            rec[f"{k}_stage_us"] = dict(zip(CHAIN_STAMPS[1:], np.round(np.median(stamps, axis=0), 2).tolist()))
    assert int(scratch[0][off:off + 4].view(torch.int32).item()) == 0, "a hand-off poll ran into its limit"
    for k, (_, ws) in sides.items():
        us = float(np.median(times[k]))
        nbytes = sum(w.numel() * w.element_size() for w in ws[0].values())
        rec[f"{k}_us"] = round(us, 2)
        rec[f"{k}_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
        rec[f"{k}_W_MB"] = round(nbytes / 1e6, 2)
        rec[f"{k}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
    rec["fp8_over_bf16"] = round(rec["fp8_us"] / rec["bf16_us"], 4)
    return rec


def bare_replay_ms(M, calls=N_NEW):
    from bdm_db1_amd.decode import RingMemory
    step = GraphedRingStep(model, batch_size=M, n_new=1, memory=None if KV_CACHE == "bf16" else RingMemory(model, M, kv_dtype=KV_CACHE))
    for _ in range(5):
        step(step.ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        step(step.ids)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / calls * 1e3
    step.check(synchronize=True)
    ring = step.memory
    del step
    return ms, ring


def eager_argmax_ms(M, ring, calls=N_NEW):
    ids = torch.zeros(M, 1, dtype=torch.long, device=dev)
    V = model.text_vocab_size
    with torch.no_grad():
        for k in range(3 + calls):
            if k == 3:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            x = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=ids, text_len=None)
            logits, _, ring = model([x], compute_loss=False, mems=ring)
            ids = logits[:, -1, :V].argmax(-1).cpu()[:, None].to(dev)     # (synchronises every token)
    return (time.perf_counter() - t0) / calls * 1e3


def device_us(fn, calls=50):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def beam_kernels_us(G, W, t_reorder=N_NEW - 1):
    """db1_beam_step (with --beam-groups: db1_beam_step_diverse) on random bf16 logits at step 1 (every beam live) and db1_ring_reorder at
    t = t_reorder over a ring of M rows"""
    from bdm_db1_amd.decode import RingMemory
    from bdm_db1_amd.generation import DecodeKey, _BeamState
    M, V, hi = G * W, int(model.total_vocab_size), int(model.text_vocab_size)
    st = _BeamState(model, DecodeKey(rows=G, cfg=BeamSearchConfig(num_beams=W, max_new_tokens=N_NEW, vocab_hi=hi, **BEAM_KW), V=V, hi=hi))
    logits = torch.randn(M, V, device=dev).to(torch.bfloat16)
    ids = torch.zeros(M, 1, dtype=torch.long, device=dev)
    st.start()
    st.select(logits, ids[:, 0])
    st.t.fill_(1)
    state0 = [x.clone() for x in (st.beam_score, st.parent, st.tokens, st.pool_count, st.done)]

    def step():
        for dst, src in zip((st.beam_score, st.parent, st.tokens, st.pool_count, st.done), state0):
            dst.copy_(src)
        st.select(logits, ids[:, 0])
    restore = device_us(lambda: [dst.copy_(src) for dst, src in zip((st.beam_score, st.parent, st.tokens, st.pool_count, st.done), state0)])
    step_us = device_us(step) - restore
    if SHARE_KW:     # (share_prompt: the reorder runs on the grouped memory's tail)
        from bdm_db1_amd.decode import GroupedRingMemory
        ring = GroupedRingMemory(model, G, W, N_NEW)
    else:
        ring = RingMemory(model, M)
    Wg = st.Wg             # (the rows a parent may come from: W, with --beam-groups W / D)
    parent = torch.tensor([(b // Wg) * Wg + (b + 1) % Wg for b in range(M)], dtype=torch.int32, device=dev)
    t = torch.tensor([t_reorder], dtype=torch.int32, device=dev)
    done = torch.zeros(M // Wg, dtype=torch.int32, device=dev)
    reorder_us = device_us(lambda: ring.reorder(parent, t, max_t=N_NEW, group=Wg, done=done))
    moved = (M if Wg > 1 else 0) * t_reorder * model.n_layer * ring.kv[0][0, 0].numel() * 2 * 4   # gather + write-back, read + write each
    del ring
    torch.cuda.empty_cache()
    return step_us, reorder_us, moved


def beam_main(W, Gs):
    for G in Gs:
        M = G * W
        rec = {"G": G, "num_beams": W, "M": M, "new_tokens": N_NEW}
        if BEAM_KW:
            rec.update(beam_groups=BEAM_KW["num_beam_groups"], diversity=BEAM_KW["diversity_penalty"])
        rec["beam_ms_per_token"] = round(gen_ms_per_token(G, BeamSearchConfig(num_beams=W, max_new_tokens=N_NEW, **BEAM_KW), **SHARE_KW), 4)
        rec["memory_bytes"] = _memory_bytes(model._beam_generator)
        model._beam_generator = None
        torch.cuda.empty_cache()
        bare, ring = bare_replay_ms(M)
        del ring
        torch.cuda.empty_cache()
        rec["bare_ring_replay_ms"] = round(bare, 4)
        rec["beam_over_bare"] = round(rec["beam_ms_per_token"] / bare, 4)
        step_us, reorder_us, moved = beam_kernels_us(G, W)
        rec["beam_step_us"] = round(step_us, 2)
        rec["ring_reorder_t29_us"] = round(reorder_us, 2)
        rec["ring_reorder_t29_traffic_MB"] = round(moved / 1e6, 1)
        rec["ring_reorder_t29_TBps"] = round(moved / (reorder_us * 1e-6) / 1e12, 3) if moved else 0.0
        print(json.dumps(rec), flush=True)


def diversity_report_main(W, Gs, lam):
    """what the sub-groups buy, on this model's random weights: per D in the divisors of W, over the G caption prompts with R = W results
    each, the mean pairwise Hamming distance between a prompt's results (positions that differ, of N_NEW), the mean number of distinct first
    tokens, and the mean score of the best result minus that of D = 1 (scores are unpenalised length-normalised log-probabilities)"""
    for G in Gs:
        b = batch(G)
        best1 = None
        for D in [d for d in range(1, W + 1) if W % d == 0]:
            cfg = BeamSearchConfig(num_beams=W, max_new_tokens=N_NEW, num_return_sequences=W, num_beam_groups=D,
                                   diversity_penalty=lam if D > 1 else 0.0)
            ids, _, scores = generate_captions(model, b, cfg, **SHARE_KW)
            ids = ids.numpy()
            ham = [float((ids[g, i] != ids[g, j]).sum()) for g in range(G) for i in range(W) for j in range(i + 1, W)]
            first = [len(set(ids[g, :, 0].tolist())) for g in range(G)]
            best = float(scores[:, 0].mean())
            best1 = best if D == 1 else best1
            print(json.dumps({"G": G, "num_beams": W, "beam_groups": D, "diversity": cfg.diversity_penalty, "new_tokens": N_NEW,
                              "mean_pairwise_hamming": round(float(np.mean(ham)), 3), "mean_distinct_first_tokens": round(float(np.mean(first)), 3),
                              "mean_best_score": round(best, 5), "best_score_minus_D1": round(best - best1, 5)}), flush=True)
        model._beam_generator = None
        torch.cuda.empty_cache()


def stream_main(n_req=256, slots=64):
    from bdm_db1_amd import caption_stream
    from bdm_db1_amd.decode import RingMemory
    from bdm_db1_amd.serving import _SlotState
    from bdm_db1_amd.generation import DecodeKey, _ring_generator, _text_window, _vocab_window
    limits = np.random.default_rng(2024).integers(5, N_NEW + 1, n_req)
    cfg = GenerationConfig(max_new_tokens=N_NEW)
    batches = [batch(slots + k) for k in range((n_req + slots - 1) // slots)]       # (another seed per batch)
    rows = lambda b, r: ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=b.prompt_seq[r:r + 1],
                                    img_seq=b.img_seq[r:r + 1], text_seq=None)
    reqs = [(rows(batches[i // slots], i % slots), int(limits[i])) for i in range(n_req)]
    rec = {"requests": n_req, "slots": slots, "limits": "uniform 5..30, seed 2024", "mean_limit": round(float(limits.mean()), 2),
           "mem_attn": bool(model.use_mem_attn)}

    def timed(fn):
        fn()                                   # capture + warm-up
        t = 1e30
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = min(t, time.perf_counter() - t0)
        return t * 1e3

    # lockstep: batches of ``slots`` in order, each to its longest limit.  generate keeps ONE graph per (rows, config), so a batch with another
    # longest limit re-captures it: every batch is timed after a warm-up call of its own (no capture inside a timed call) and the times add up;
    # what the captures of a real pass over these batches would cost is reported next to it
    longest = [int(limits[i:i + slots].max()) for i in range(0, n_req, slots)]
    static_ms, capture_ms, prev = 0.0, 0.0, None
    for b, n, i in zip(batches, longest, range(0, n_req, slots)):
        k = min(slots, n_req - i)
        bb = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=b.prompt_seq[:k], img_seq=b.img_seq[:k],
                         text_seq=None)
        c = dataclasses.replace(cfg, max_new_tokens=n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate_captions(model, bb, c)                  # warm-up; captures when (k, n) differs from the batch before
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        best = 1e30
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_captions(model, bb, c)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        static_ms += best
        if (k, n) != prev:
            capture_ms += first - best
        prev = (k, n)
    rec["static_longest_limits"] = longest
    rec["static_total_ms"] = round(static_ms, 2)
    rec["static_capture_ms_not_in_total"] = round(capture_ms, 2)
    rec["static_replays"] = sum(n - 1 for n in longest)
    gen = model._generator
    gen.state.start()
    for _ in range(3):
        gen.step(gen.step.ids)
    gen.state.start()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        gen.step(gen.step.ids)
    torch.cuda.synchronize()
    rec["generate_graph_replay_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    rec["generate_graph_M"] = gen.state.M
    model._generator = None
    del gen
    torch.cuda.empty_cache()

    stats = {}

    def stream():
        for _ in caption_stream(model, reqs, cfg, slots=slots, stats=stats):
            pass
    rec["stream_total_ms"] = round(timed(stream), 2)
    rec.update(stream_replays=stats["replays"], prefill_calls=stats["prefill_calls"], occupancy=round(stats["occupancy"], 4))
    tcfg = _text_window(model, cfg)
    V, hi = _vocab_window(model, tcfg)
    sg = _ring_generator(model, _SlotState, DecodeKey(rows=slots, cfg=tcfg, V=V, hi=hi))
    st = sg.state

    def live():
        st.finished.zero_()
        st.t.zero_()
        st.limit.fill_(N_NEW)
    live()
    for _ in range(3):
        sg.step(sg.step.ids)
    live()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        sg.step(sg.step.ids)
    torch.cuda.synchronize()
    rec["slot_graph_replay_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    sg.step.check(synchronize=True)
    st.start()
    rec["slot_over_generate_replay"] = round(rec["slot_graph_replay_ms"] / rec["generate_graph_replay_ms"], 4)
    rec["replay_count_ratio_static_over_stream"] = round(rec["static_replays"] / stats["replays"], 4)
    rec["time_ratio_static_over_stream"] = round(rec["static_total_ms"] / rec["stream_total_ms"], 4)
    rec["stream_admission_ms"] = round(rec["stream_total_ms"] - stats["replays"] * rec["slot_graph_replay_ms"], 2)
    rec["static_prefill_ms"] = round(rec["static_total_ms"] - rec["static_replays"] * rec["generate_graph_replay_ms"], 2)
    # db1_ring_load_rows alone
    ring, n, mlen = sg.ring, min(16, slots), int(model.mem_len)
    src = [torch.randn(n, mlen, 2, model.n_head, model.d_head, device=dev).to(torch.bfloat16) for _ in range(model.n_layer)]
    idx = torch.arange(0, n, dtype=torch.int32, device=dev) * (slots // n)
    us = device_us(lambda: ops.ring_load_rows(ring.kv, ring._ptrs, src, ring.state, mlen, idx, ring.load_status))
    moved = 2 * n * mlen * model.n_layer * src[0][0, 0].numel() * 2
    rec.update(ring_load_rows_us=round(us, 2), ring_load_rows_MB=round(moved / 1e6, 1), ring_load_rows_TBps=round(moved / (us * 1e-6) / 1e12, 3))
    print(json.dumps(rec), flush=True)


def stream_shared_prefix_main(K, n_img=64, slots=64, q_len=10):
    """n_img images x K questions of q_len tokens as n_img * K stream requests over ``slots`` slots (per-request limits as --stream draws
    them), in two forms in ONE process: every request the whole VQA prompt [prompt, patches, question] (``unshared``; with --ring-prefill
    through the ring prefill), and every image put into a PrefixCache once, every request a ``Prefixed`` question (``shared``; the time of
    the puts is reported and counted).  Admission time = total - replays * the slot graph's replay time, as --stream reports it."""
    from bdm_db1_amd import PrefixCache, Prefixed, generate_stream
    from bdm_db1_amd.data import VQATaskInput
    from bdm_db1_amd.serving import _SlotState
    from bdm_db1_amd.generation import DecodeKey, _ring_generator, _text_window, _vocab_window
    n_req = n_img * K
    limits = np.random.default_rng(2024).integers(5, N_NEW + 1, n_req)
    cfg = _text_window(model, GenerationConfig(max_new_tokens=N_NEW))
    imgs = batch(n_img)
    ques = torch.from_numpy(np.random.default_rng(7).integers(1, 32000, (n_img, K, q_len))).to(dev)
    text = lambda ids: NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=ids, text_len=None)
    prefixes = ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=imgs.prompt_seq, img_seq=imgs.img_seq,
                           text_seq=torch.zeros(n_img, 0, dtype=torch.long))
    # request r = question r % K of image r // K: the K questions of an image arrive together
    unshared = [(VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=imgs.prompt_seq[r // K:r // K + 1],
                              img_seq=imgs.img_seq[r // K:r // K + 1], text_seq=ques[r // K, r % K][None]), int(limits[r])) for r in range(n_req)]
    rec = {"images": n_img, "questions_per_image": K, "question_tokens": q_len, "requests": n_req, "slots": slots,
           "ring_prefill": bool(model.use_ring_prefill), "mem_attn": bool(model.use_mem_attn)}

    def timed(fn):
        fn()                                   # capture + warm-up
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts)

    stats = {}

    def run(reqs):
        for _ in generate_stream(model, reqs, cfg, slots=slots, stats=stats):
            pass
    rec["unshared_total_ms"] = round(timed(lambda: run(unshared)), 2)
    rec.update(unshared_replays=stats["replays"], unshared_prefill_calls=stats["prefill_calls"])
    cache = PrefixCache(model, n_img)
    put_ms = []

    def shared():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        handles = cache.put(prefixes)                                 # (all images in one batch, as the unshared admissions batch theirs)
        torch.cuda.synchronize()
        put_ms.append((time.perf_counter() - t0) * 1e3)
        run([(Prefixed(cache, [handles[r // K]], text(ques[r // K, r % K][None])), int(limits[r])) for r in range(n_req)])
        cache.release(handles)
    rec["shared_total_ms"] = round(timed(shared), 2)
    rec.update(shared_put_ms=round(min(put_ms[1:]), 2), shared_replays=stats["replays"], shared_prefill_calls=stats["prefill_calls"],
               shared_prefixed=stats["prefixed"])
    V, hi = _vocab_window(model, cfg)
    sg = _ring_generator(model, _SlotState, DecodeKey(rows=slots, cfg=cfg, V=V, hi=hi))
    st = sg.state

    def live():
        st.finished.zero_()
        st.t.zero_()
        st.limit.fill_(N_NEW)
    live()
    for _ in range(3):
        sg.step(sg.step.ids)
    live()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        sg.step(sg.step.ids)
    torch.cuda.synchronize()
    rec["slot_graph_replay_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    sg.step.check(synchronize=True)
    st.start()
    rec["unshared_admission_ms"] = round(rec["unshared_total_ms"] - rec["unshared_replays"] * rec["slot_graph_replay_ms"], 2)
    rec["shared_admission_ms"] = round(rec["shared_total_ms"] - rec["shared_replays"] * rec["slot_graph_replay_ms"], 2)
    rec["admission_ratio_shared_over_unshared"] = round(rec["shared_admission_ms"] / rec["unshared_admission_ms"], 4)
    print(json.dumps(rec), flush=True)


def slot_select_kernels_us(M, max_new=4096):
    """db1_select_tokens_slots and db1_select_tokens_slots_per alone on random bf16 logits [M, V] over the text window, every slot live (the
    counters are rewound before every measurement: a launch advances them)"""
    V, hi = int(model.total_vocab_size), int(model.text_vocab_size)
    logits = (torch.randn(M, V, device=dev) * 3).to(torch.bfloat16)
    i32 = dict(dtype=torch.int32, device=dev)
    t, fin, n, status = (torch.zeros(M, **i32) for _ in range(4))
    limit = torch.full((M,), max_new, **i32)
    out = torch.zeros(M, max_new, **i32)
    ids = torch.zeros(M, dtype=torch.long, device=dev)
    kinds = {"greedy": dict(greedy=True, temperature=1.0, top_k=0, top_p=1.0, seed=1, vocab_lo=0, vocab_hi=hi),
             "top_p_0.9": dict(greedy=False, temperature=1.0, top_k=0, top_p=0.9, seed=1, vocab_lo=0, vocab_hi=hi)}
    recs = {k: ops.pack_slot_params(**v) for k, v in kinds.items()}
    tables = {"greedy": [recs["greedy"]] * M, "top_p_0.9": [recs["top_p_0.9"]] * M,
              "half_and_half": [recs["greedy" if i % 2 == 0 else "top_p_0.9"] for i in range(M)]}
    rec = {}

    def measure(fn):
        for x in (t, fin, n, status):
            x.zero_()
        us = device_us(fn)
        assert int(status.max()) == 0 and int(t.min()) == 53
        return round(us, 2)

    for name, kw in kinds.items():
        rec[f"slots_{name}_us"] = measure(lambda: ops.select_tokens_slots(logits, t, limit, fin, n, out, ids, status, V=V, **kw))
    for name, table in tables.items():
        params = torch.from_numpy(np.stack(table)).to(dev)
        rec[f"slots_per_{name}_us"] = measure(lambda: ops.select_tokens_slots_per(logits, params, t, limit, fin, n, out, ids, status, V=V))
    return rec


def stream_per_request_main(n_req=256, slots=64):
    from bdm_db1_amd import SamplingParams, caption_stream
    limits = np.random.default_rng(2024).integers(5, N_NEW + 1, n_req)
    cfg = GenerationConfig(max_new_tokens=N_NEW)
    batches = [batch(slots + k) for k in range((n_req + slots - 1) // slots)]
    rows = lambda b, r: ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=b.prompt_seq[r:r + 1],
                                    img_seq=b.img_seq[r:r + 1], text_seq=None)
    shared = [(rows(batches[i // slots], i % slots), int(limits[i])) for i in range(n_req)]
    sampled = SamplingParams(greedy=False, top_p=0.9, seed=1)
    mixed = [r if i % 2 == 0 else r + (sampled,) for i, r in enumerate(shared)]
    rec = {"requests": n_req, "slots": slots, "limits": "uniform 5..30, seed 2024", "mix": "even requests greedy, odd requests top-p 0.9"}

    def total(reqs, **kw):
        stats = {}

        def run():
            for _ in caption_stream(model, reqs, cfg, slots=slots, stats=stats, **kw):
                pass
        run()                                  # capture + warm-up
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 2), [round(x, 2) for x in ts], stats["replays"]

    rec["shared_total_ms"], rec["shared_runs_ms"], rec["shared_replays"] = total(shared)
    rec["flag_only_total_ms"], rec["flag_only_runs_ms"], rec["flag_only_replays"] = total(shared, per_request=True)
    rec["per_request_total_ms"], rec["per_request_runs_ms"], rec["per_request_replays"] = total(mixed, per_request=True)
    model._slot_generator = None
    torch.cuda.empty_cache()
    rec.update(slot_select_kernels_us(slots))
    print(json.dumps(rec), flush=True)


def slot_constrain_kernels_us(M, t=N_NEW - 1, bad_cap=64, bias_cap=64, only=None):
    """db1_constrain_logits_slots_per and db1_stop_match_per alone (the docstring above says on what)"""
    V, hi = int(model.total_vocab_size), int(model.text_vocab_size)
    logits = (torch.randn(M, V, device=dev) * 3).to(torch.bfloat16)
    i32 = dict(dtype=torch.int32, device=dev)
    hist = ((torch.arange(N_NEW, device=dev)[None, :] * 7 + torch.arange(M, device=dev)[:, None] * 13) % hi).to(torch.int32).contiguous()
    tt, fin, status = torch.full((M,), t, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
    cons = DecodingConstraints(repetition_penalty=1.2, no_repeat_ngram_size=3)
    rows = {"noop": ops.pack_slot_constraints(None, None, bad_cap, bias_cap), "constrained": ops.pack_slot_constraints(cons, None, bad_cap, bias_cap)}
    tables = {"noop": [rows["noop"]] * M, "constrained": [rows["constrained"]] * M,
              "half_and_half": [rows["noop" if i % 2 == 0 else "constrained"] for i in range(M)]}
    rec = {}
    for name, table in tables.items():
        if only not in (None, name):
            continue
        c, bad, bi, bv = (torch.from_numpy(np.stack([r[k] for r in table])).to(dev) for k in range(4))
        rec[f"constrain_slots_per_{name}_us"] = round(device_us(lambda: ops.constrain_logits_slots_per(
            logits, c, tt, hist, fin, status, V=V, bad=bad, bias_ids=bi, bias_val=bv)), 2)
    assert int(status.max()) == 0 and int(fin.max()) == 0
    rec["constrain_scalar_us"] = round(device_us(lambda: ops.constrain_logits(logits, tt, hist, V=V, finished=fin, repetition_penalty=1.2,
                                                                               no_repeat_ngram_size=3)), 2)
    # the stop kernels: every row holds 20 tokens whose last 15 are the first 15 of every sequence; ``checked`` is rewound before every launch
    seqs = [list(range(100, 115)) + [200 + k] for k in range(16)]
    full = ops.pack_slot_constraints(DecodingConstraints(stop_sequences=seqs), None, 0, 0)
    lengths, checked, hit = torch.full((M,), 20, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
    out = torch.zeros(M, N_NEW, **i32)
    out[:, 4:19] = torch.arange(100, 115, **i32)
    out[:, 19] = 114
    ids = torch.zeros(M, dtype=torch.long, device=dev)
    rewind = device_us(lambda: checked.zero_())

    def timed(fn):
        def go():
            checked.zero_()
            fn()
        return round(device_us(go) - rewind, 2)

    for name, row in (("empty", rows["noop"]), ("16x16", full)):
        if only not in (None, "noop" if name == "empty" else "constrained"):
            continue
        tok, n = (torch.from_numpy(np.tile(row[k], (M,) + (1,) * row[k].ndim)).to(dev) for k in (4, 5))
        rec[f"stop_match_per_{name}_us"] = timed(lambda: ops.stop_match_per(tok, n, lengths, checked, fin, hit, out, ids))
    tok, n = torch.from_numpy(full[4]).to(dev), torch.from_numpy(full[5]).to(dev)
    rec["stop_match_16x16_us"] = timed(lambda: ops.stop_match(tok, n, lengths, checked, fin, hit, out, ids))
    assert int(hit.max()) == 0 and int(checked.min()) == 20
    return rec


def stream_per_request_constraints_main(n_req=256, slots=64):
    from bdm_db1_amd import caption_stream
    limits = np.random.default_rng(2024).integers(5, N_NEW + 1, n_req)
    cfg = GenerationConfig(max_new_tokens=N_NEW)
    batches = [batch(slots + k) for k in range((n_req + slots - 1) // slots)]
    rows = lambda b, r: ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=b.prompt_seq[r:r + 1],
                                    img_seq=b.img_seq[r:r + 1], text_seq=None)
    shared = [(rows(batches[i // slots], i % slots), int(limits[i])) for i in range(n_req)]
    cons = DecodingConstraints(repetition_penalty=1.2, no_repeat_ngram_size=3)
    mixed = [r if i % 2 == 0 else r + (None, cons) for i, r in enumerate(shared)]
    rec = {"requests": n_req, "slots": slots, "limits": "uniform 5..30, seed 2024",
           "mix": "even requests unconstrained, odd requests repetition_penalty 1.2 + no_repeat_ngram_size 3"}

    def total(reqs, **kw):
        stats = {}

        def run():
            for _ in caption_stream(model, reqs, cfg, slots=slots, stats=stats, **kw):
                pass
        run()                                  # capture + warm-up
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 2), [round(x, 2) for x in ts], stats["replays"]

    rec["flag_off_total_ms"], rec["flag_off_runs_ms"], rec["flag_off_replays"] = total(shared)
    rec["flag_only_total_ms"], rec["flag_only_runs_ms"], rec["flag_only_replays"] = total(shared, per_request_constraints=True)
    rec["mixed_total_ms"], rec["mixed_runs_ms"], rec["mixed_replays"] = total(mixed, per_request_constraints=True)
    model._slot_generator = None
    torch.cuda.empty_cache()
    rec.update(slot_constrain_kernels_us(slots))
    print(json.dumps(rec), flush=True)


def constrain_kernels_us(M=64, max_new=4096, ts=(255, 1023, 4095)):
    """db1_constrain_logits, db1_constrain_logits_pen and db1_stop_match alone (the docstring above says on what)"""
    V, hi = int(model.total_vocab_size), int(model.text_vocab_size)
    logits = (torch.randn(M, V, device=dev) * 3).to(torch.bfloat16)
    i32 = dict(dtype=torch.int32, device=dev)
    hist = ((torch.arange(max_new, device=dev)[None, :] * 7 + torch.arange(M, device=dev)[:, None] * 13) % hi).to(torch.int32).contiguous()
    assert all(len(set(r.tolist())) == max_new for r in hist[:2].cpu())
    bias_ids = (torch.arange(16, device=dev) * 2001).to(torch.int32)
    bias_val = torch.linspace(-2, 2, 16, device=dev)
    rec = {"M": M}
    for t in ts:
        tt = torch.tensor([t], **i32)
        rec[f"constrain_t{t}_us"] = round(device_us(lambda: ops.constrain_logits(logits, tt, hist, V=V, repetition_penalty=1.2)), 2)
        rec[f"constrain_pen_t{t}_us"] = round(device_us(lambda: ops.constrain_logits(
            logits, tt, hist, V=V, repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5, bias_ids=bias_ids, bias_val=bias_val)), 2)
        rec[f"count_scan_t{t}_us"] = round(rec[f"constrain_pen_t{t}_us"] - rec[f"constrain_t{t}_us"], 2)
    # db1_stop_match: every row holds 20 tokens whose last 15 are the first 15 of every sequence; ``checked`` is rewound before every launch
    seqs = [list(range(100, 115)) + [200 + k] for k in range(16)]
    tok, n = ops.pack_stop_sequences(seqs)
    tok, n = torch.from_numpy(tok).to(dev), torch.from_numpy(n).to(dev)
    lengths, checked, fin, hit = torch.full((M,), 20, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
    out = torch.zeros(M, N_NEW, **i32)
    out[:, 4:19] = torch.arange(100, 115, **i32)
    out[:, 19] = 114
    ids = torch.zeros(M, dtype=torch.long, device=dev)

    def stop():
        checked.zero_()
        ops.stop_match(tok, n, lengths, checked, fin, hit, out, ids)
    rewind = device_us(lambda: checked.zero_())
    rec["stop_match_16x16_us"] = round(device_us(stop) - rewind, 2)
    assert int(hit.max()) == 0 and int(checked.min()) == 20
    return rec


SELECT_MODES = {"greedy": dict(), "top_p_0.9": dict(greedy=False, top_p=0.9, seed=1)}


def select_kernels_us(M, modes=tuple(SELECT_MODES)):
    """db1_select_tokens and db1_select_tokens_lp alone on random bf16 logits [M, V] over the text window, greedy and top-p 0.9"""
    V, hi = int(model.total_vocab_size), int(model.text_vocab_size)
    logits = (torch.randn(M, V, device=dev) * 3).to(torch.bfloat16)
    i32 = dict(dtype=torch.int32, device=dev)
    t, fin, n, status = torch.zeros(1, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
    out = torch.zeros(M, N_NEW, **i32)
    ids = torch.zeros(M, dtype=torch.long, device=dev)
    lp, sums = torch.zeros(M, N_NEW, device=dev), torch.zeros(M, device=dev)
    rec = {}
    for name in modes:
        kw = SELECT_MODES[name]
        run = lambda **more: ops.select_tokens(logits, t, fin, n, out, ids, status, V=V, vocab_hi=hi, **kw, **more)
        rec[f"select_{name}_us"] = round(device_us(run), 2)
        rec[f"select_lp_{name}_us"] = round(device_us(lambda: run(logprob=lp, sum_logprob=sums)), 2)
        if TOP_N:
            ti, tl = torch.zeros(M, N_NEW, TOP_N, **i32), torch.zeros(M, N_NEW, TOP_N, device=dev)
            rec[f"select_top{TOP_N}_{name}_us"] = round(device_us(lambda: run(logprob=lp, sum_logprob=sums, top_n=TOP_N, top_ids=ti,
                                                                               top_logprob=tl)), 2)
    return rec


def logprobs_main(Ms):
    for M in Ms:
        rec = {"M": M, "new_tokens": N_NEW}
        for name, cfg in (("greedy", GenerationConfig(max_new_tokens=N_NEW)),
                          ("top_p_0.9", GenerationConfig(max_new_tokens=N_NEW, greedy=False, top_p=0.9, seed=1))):
            rec[f"{name}_ms_per_token"] = round(gen_ms_per_token(M, cfg), 4)
            rec[f"{name}_logprobs_ms_per_token"] = round(gen_ms_per_token(M, dataclasses.replace(cfg, logprobs=True)), 4)
            rec[f"{name}_logprobs_minus_plain_us"] = round((rec[f"{name}_logprobs_ms_per_token"] - rec[f"{name}_ms_per_token"]) * 1e3, 2)
            if TOP_N:
                key = f"{name}_top{TOP_N}_ms_per_token"
                rec[key] = round(gen_ms_per_token(M, dataclasses.replace(cfg, logprobs=True, top_logprobs=TOP_N)), 4)
                rec[f"{name}_top{TOP_N}_minus_logprobs_us"] = round((rec[key] - rec[f"{name}_logprobs_ms_per_token"]) * 1e3, 2)
        model._generator = None
        torch.cuda.empty_cache()
        rec.update(select_kernels_us(M))
        print(json.dumps(rec), flush=True)


def best_of_main(N, Gs):
    for G in Gs:
        rec = {"G": G, "n": N, "M": G * N, "new_tokens": N_NEW}
        cfg = GenerationConfig(max_new_tokens=N_NEW, greedy=False, top_p=0.9, seed=1)
        rec["best_of_ms_per_token"] = round(gen_ms_per_token(G, cfg, n=N, **SHARE_KW), 4)
        rec["memory_bytes"] = _memory_bytes(model._best_of_generator)
        model._best_of_generator = None
        torch.cuda.empty_cache()
        rec["beam_ms_per_token"] = round(gen_ms_per_token(G, BeamSearchConfig(num_beams=N, max_new_tokens=N_NEW), **SHARE_KW), 4)
        model._beam_generator = None
        torch.cuda.empty_cache()
        rec["best_of_over_beam"] = round(rec["best_of_ms_per_token"] / rec["beam_ms_per_token"], 4)
        print(json.dumps(rec), flush=True)


args = sys.argv[1:]
if "--mem-attn" in args:       # calls with memory and more than 64 new tokens (the prompt prefills) take the fused attention over memory
    model.use_mem_attn = True
    args = [a for a in args if a != "--mem-attn"]
if "--ring-prefill" in args:   # the prompt prefills project only their own tokens and write their keys / values straight into the K/V ring
    model.use_ring_prefill = True
    args = [a for a in args if a != "--ring-prefill"]
    _dumps = json.dumps
    json.dumps = lambda rec, **kw: _dumps(dict(rec, ring_prefill=True) if isinstance(rec, dict) else rec, **kw)   # every line of this run says so
if "--share-prompt" in args:   # beam search and best-of-n read one copy of a group's prompt keys / values (share_prompt=True)
    if "--num-beams" not in args and "--best-of" not in args:
        sys.exit("--share-prompt goes with --num-beams or --best-of")
    SHARE_KW = dict(share_prompt=True)
    args = [a for a in args if a != "--share-prompt"]
    _dumps_sp = json.dumps
    json.dumps = lambda rec, **kw: _dumps_sp(dict(rec, share_prompt=True) if isinstance(rec, dict) else rec, **kw)   # every line of this run says so
if "--speculative" in args:
    i = args.index("--speculative")
    K_, rest = int(args[i + 1]), args[:i] + args[i + 2:]
    mode_ = None
    if "--draft-script" in rest:
        j = rest.index("--draft-script")
        mode_, rest = rest[j + 1], rest[:j] + rest[j + 2:]
        if mode_ not in ("perfect", "wrong"):
            sys.exit("--draft-script perfect|wrong")
    spec_main(K_, mode_, [int(a) for a in rest if a != "--text-prompt"] or [1, 4], "--text-prompt" in rest)
    sys.exit(0)
if "--spec-replay" in args:
    spec_replay_main([tuple(int(v) for v in a.split(":")) for a in args if a != "--spec-replay"] or [(1, 1), (1, 2), (1, 5), (1, 8), (4, 5)])
    sys.exit(0)
if "--spec-logits" in args:
    spec_logits_main()
    sys.exit(0)
if "--spec-kernels" in args:
    for rows_ in [int(a) for a in args if a != "--spec-kernels"] or [5, 64]:
        print(json.dumps(spec_kernels_us(rows_)), flush=True)
    sys.exit(0)
if "--group-kernels" in args:
    rest = [int(a) for a in args if a != "--group-kernels"]
    G_, W_ = (rest + [16, 4])[:2] if len(rest) >= 2 else (16, 4)
    for n_tail in rest[2:] or [0, 29]:
        print(json.dumps(group_kernels_us(G_, W_, n_tail)), flush=True)
    sys.exit(0)
if "--w8-kernels" in args:
    for M in [int(a) for a in args if a != "--w8-kernels"] or [1, 4, 16, 64]:
        print(json.dumps(w8_kernels_us(M)), flush=True)
    sys.exit(0)
if "--chain-kernels" in args:
    print(json.dumps(chain_kernels_us()), flush=True)
    sys.exit(0)
if "--decode-weights" in args:   # the decode calls stream fp8 copies of the layers' four linear maps (model.set_decode_weights)
    i = args.index("--decode-weights")
    fp8_chain = "--fp8-chain" in args       # ... and the one-token call stays on the persistent chain (db1_decode_chain_w8)
    model.set_decode_weights(args[i + 1], chain=fp8_chain)
    args = [a for a in args[:i] + args[i + 2:] if a != "--fp8-chain"]
    _dumps_dw = json.dumps
    _dw_fields = lambda: dict(decode_weights=model.decode_weights, **({"decode_chain_w8": True} if model.decode_chain_w8 else {}))
    json.dumps = lambda rec, **kw: _dumps_dw(dict(rec, **_dw_fields()) if isinstance(rec, dict) else rec, **kw)   # every line of this run says so
TOP_N = None
if "--top-logprobs" in args:
    i = args.index("--top-logprobs")
    TOP_N = int(args[i + 1])
    args = args[:i] + args[i + 2:]
if "--select-kernels" in args:
    i = args.index("--select-kernels")
    M = int((args[:i] + args[i + 2:] or [64])[0])
    print(json.dumps({"M": M, **select_kernels_us(M, (args[i + 1],))}), flush=True)
    sys.exit(0)
if "--logprobs" in args:
    logprobs_main([int(a) for a in args if a != "--logprobs"] or [1, 16, 64])
    sys.exit(0)
if "--best-of" in args:
    i = args.index("--best-of")
    best_of_main(int(args[i + 1]), [int(a) for a in args[:i] + args[i + 2:]] or [16])
    sys.exit(0)
if "--stream" in args and "--shared-prefix" in args:
    i = args.index("--shared-prefix")
    stream_shared_prefix_main(int(args[i + 1]), *[int(a) for a in args[:i] + args[i + 2:] if a != "--stream"][:2])
    sys.exit(0)
if "--stream" in args:
    rest = [int(a) for a in args if a not in ("--stream", "--per-request", "--per-request-constraints")]
    (stream_per_request_constraints_main if "--per-request-constraints" in args else
     stream_per_request_main if "--per-request" in args else stream_main)(*rest[:2])
    sys.exit(0)
if "--diversity-report" in args:   # --num-beams W --diversity-report [--diversity LAMBDA] [G ...]: what the sub-groups buy, per divisor D of W
    rest = [a for a in args if a != "--diversity-report"]
    lam = 0.5
    if "--diversity" in rest:
        i = rest.index("--diversity")
        lam, rest = float(rest[i + 1]), rest[:i] + rest[i + 2:]
    i = rest.index("--num-beams")
    diversity_report_main(int(rest[i + 1]), [int(a) for a in rest[:i] + rest[i + 2:]] or [16], lam)
    sys.exit(0)
if "--beam-groups" in args or "--diversity" in args:      # diverse beam search: D sub-groups, a Hamming penalty between them
    if "--num-beams" not in args:
        sys.exit("--beam-groups / --diversity go with --num-beams")
    for flag, name, conv in (("--beam-groups", "num_beam_groups", int), ("--diversity", "diversity_penalty", float)):
        if flag in args:
            i = args.index(flag)
            BEAM_KW[name] = conv(args[i + 1])
            args = args[:i] + args[i + 2:]
    BEAM_KW.setdefault("num_beam_groups", 1)
    BEAM_KW.setdefault("diversity_penalty", 0.0)
if "--num-beams" in args:
    i = args.index("--num-beams")
    W = int(args[i + 1])
    beam_main(W, [int(a) for a in args[:i] + args[i + 2:]] or [1, 16])
    sys.exit(0)
if "--slot-constrain-kernels" in args:
    i = args.index("--slot-constrain-kernels")
    M = int(args[i + 2]) if len(args) > i + 2 else 64
    print(json.dumps({"M": M, **slot_constrain_kernels_us(M, only=args[i + 1])}), flush=True)
    sys.exit(0)
if "--constrain-kernels" in args:
    print(json.dumps(constrain_kernels_us(*[int(a) for a in args if a != "--constrain-kernels"][:1])), flush=True)
    sys.exit(0)
if "--constraints" in args:
    cons = DecodingConstraints(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=5)
    if "--penalties" in args:
        cons = dataclasses.replace(cons, frequency_penalty=0.5, presence_penalty=0.5)
    if "--logit-bias" in args:
        i = args.index("--logit-bias")
        nb = int(args[i + 1])
        args = args[:i] + args[i + 2:]
        cons = dataclasses.replace(cons, logit_bias={(k * int(model.text_vocab_size)) // nb: (k % 5 - 2) * 0.5 for k in range(nb)})
    if "--stop-sequences" in args:      # (ids past the text window are never generated: the sequences never match)
        tv = int(model.text_vocab_size)
        cons = dataclasses.replace(cons, stop_sequences=[(tv, tv + 1), (tv + 2, tv + 3, tv + 4)])
    args = [a for a in args if a not in ("--penalties", "--stop-sequences")]
    for M in [int(a) for a in args if a != "--constraints"] or [1, 16, 64]:
        rec = {"M": M, "new_tokens": N_NEW, "constraints": dataclasses.asdict(cons)}
        rec["greedy_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW)), 4)
        rec["constrained_greedy_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW), constraints=cons), 4)
        rec["constrained_minus_plain_us"] = round((rec["constrained_greedy_ms_per_token"] - rec["greedy_ms_per_token"]) * 1e3, 2)
        if cons.edits_more or cons.stop_sequences:      # the kernels' own time at this M, mid-caption (t = 15), from events in this process
            model._generator = None
            torch.cuda.empty_cache()
            rec.update({k: v for k, v in constrain_kernels_us(M, N_NEW, (15,)).items() if k != "M"})
        print(json.dumps(rec), flush=True)
    sys.exit(0)
if "--kv8-kernels" in args:
    for B in [int(a) for a in args if a != "--kv8-kernels"] or [1, 16, 64]:
        print(json.dumps(kv8_kernels_us(B)), flush=True)
    sys.exit(0)
if "--kv-cache" in args:
    i = args.index("--kv-cache")
    KV_CACHE = args[i + 1]
    args = args[:i] + args[i + 2:]
kv_kw = {} if KV_CACHE == "bf16" else dict(kv_cache=KV_CACHE)      # (the default run makes the call it always made)
Ms = [int(a) for a in args] or [1, 16, 64]
for M in Ms:
    rec = {"M": M, "new_tokens": N_NEW, "kv_cache": KV_CACHE}
    rec["greedy_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW), **kv_kw), 4)
    rec["top_p_0.9_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW, greedy=False, top_p=0.9, seed=1), **kv_kw), 4)
    rec["ring_bytes"] = sum(k.numel() * k.element_size() for k in model._generator.ring.kv)
    model._generator = None
    torch.cuda.empty_cache()
    bare, ring = bare_replay_ms(M)
    rec["bare_ring_replay_ms"] = round(bare, 4)
    rec["eager_argmax_cpu_ms_per_token"] = round(eager_argmax_ms(M, ring), 4)
    del ring
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
