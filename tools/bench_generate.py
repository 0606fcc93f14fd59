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

    python tools/bench_generate.py --num-beams 4 [G ...]"""
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdm_db1_amd import BeamSearchConfig, GenerationConfig, GraphedRingStep, TransformerXL, generate_captions, lib, ops, synth  # noqa: E402
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


def gen_ms_per_token(M, cfg, short=10):
    """the token loop of generate_captions: (time of N_NEW tokens - time of `short` tokens) / (N_NEW - short) -- the prefill, the ring load
    and the first selection are the same in both and cancel"""
    b = batch(M)

    def best(c):
        generate_captions(model, b, c)                  # capture + warm-up
        t = 1e30
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_captions(model, b, c)
            t = min(t, time.perf_counter() - t0)
        return t

    full = best(cfg)
    part = best(dataclasses.replace(cfg, max_new_tokens=short))
    return (full - part) / (N_NEW - short) * 1e3


def bare_replay_ms(M, calls=N_NEW):
    step = GraphedRingStep(model, batch_size=M, n_new=1)
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
    """db1_beam_step on random bf16 logits at step 1 (every beam live) and db1_ring_reorder at t = t_reorder over a ring of M rows"""
    from bdm_db1_amd.decode import RingMemory
    from bdm_db1_amd.generation import _BeamState
    M, V, hi = G * W, int(model.total_vocab_size), int(model.text_vocab_size)
    st = _BeamState(model, G, BeamSearchConfig(num_beams=W, max_new_tokens=N_NEW, vocab_hi=hi), V, hi)
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
    ring = RingMemory(model, M)
    parent = torch.tensor([(b // W) * W + (b + 1) % W for b in range(M)], dtype=torch.int32, device=dev)
    t = torch.tensor([t_reorder], dtype=torch.int32, device=dev)
    done = torch.zeros(G, dtype=torch.int32, device=dev)
    reorder_us = device_us(lambda: ring.reorder(parent, t, max_t=N_NEW, group=W, done=done))
    moved = (M if W > 1 else 0) * t_reorder * model.n_layer * ring.kv[0][0, 0].numel() * 2 * 4   # gather + write-back, read + write each
    del ring
    torch.cuda.empty_cache()
    return step_us, reorder_us, moved


def beam_main(W, Gs):
    for G in Gs:
        M = G * W
        rec = {"G": G, "num_beams": W, "M": M, "new_tokens": N_NEW}
        rec["beam_ms_per_token"] = round(gen_ms_per_token(G, BeamSearchConfig(num_beams=W, max_new_tokens=N_NEW)), 4)
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


args = sys.argv[1:]
if "--num-beams" in args:
    i = args.index("--num-beams")
    W = int(args[i + 1])
    beam_main(W, [int(a) for a in args[:i] + args[i + 2:]] or [1, 16])
    sys.exit(0)
Ms = [int(a) for a in args] or [1, 16, 64]
for M in Ms:
    rec = {"M": M, "new_tokens": N_NEW}
    rec["greedy_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW)), 4)
    rec["top_p_0.9_ms_per_token"] = round(gen_ms_per_token(M, GenerationConfig(max_new_tokens=N_NEW, greedy=False, top_p=0.9, seed=1)), 4)
    model._generator = None
    torch.cuda.empty_cache()
    bare, ring = bare_replay_ms(M)
    rec["bare_ring_replay_ms"] = round(bare, 4)
    rec["eager_argmax_cpu_ms_per_token"] = round(eager_argmax_ms(M, ring), 4)
    del ring
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
