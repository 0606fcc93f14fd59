#!/usr/bin/env python3
"""Fused attention over memory (db1_relattn_mem_fwd) at the DB1-1.3B geometry (bf16, seeded random data / init), three measurements:

  * the kernel against the materialised sequence it replaces in ``_attention_fwd`` -- two ``gemm_batched`` launches into fp32 [H, B, Lq, Lk]
    buffers, ``relattn_softmax_fwd``, a third batched GEMM -- with ``relattn_add_head_bias`` excluded on both sides, alternated in ONE
    process, device events around synchronised work, at B = 64, H = 16, q = 200, mlen = 1024, shift = 0 (the caption prompt over
    ``init_mem``) and B = 16, q = 1024, mlen = 1024, shift = 0 (a long-text segment); the two outputs are compared on the way;
  * ``score_document`` on B = 16, T = 4097, segment_len = 1024 with ``fused=True`` against ``fused=False``: tokens/s and peak memory;
  * ``tools/bench_generate.py --stream`` with and without ``--mem-attn`` (a process each, three runs each in alternation):
    ``stream_admission_ms`` and ``stream_total_ms``, medians and spreads.  ``--no-stream`` leaves this part out.

    python tools/bench_mem_attn.py [--out profiles/mem_attn_1p3b.txt] [--reps 7] [--no-stream]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdm_db1_amd import TransformerXL, lib, ops, score_document, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_attn_1p3b.txt"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-stream", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed_pair(fa, fb, reps):
    """ms of fa and fb, alternated: [reps] each"""
    for f in (fa, fb, fa, fb):
        f()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for f, dst in ((fa, out[0]), (fb, out[1])):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            dst.append(e0.elapsed_time(e1))
    return out


def stat(x):
    x = sorted(x)
    return dict(median=round(x[len(x) // 2], 4), min=round(x[0], 4), max=round(x[-1], 4))


def kernel_pair(B, H, q, mlen, shift, reps):
    D, klen = 128, mlen + q
    nd, scale = klen, 1.0 / math.sqrt(D)
    g = torch.Generator(device=dev).manual_seed(q * 7 + B)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    qkv, R = rnd(B, klen, 3, H, D), rnd(nd, H * D)
    qu, qv = rnd(B, q, H, D), rnd(B, q, H, D)
    out_f, out_m = torch.empty(B, q, H, D, device=dev, dtype=torch.bfloat16), torch.empty(B, q, H, D, device=dev, dtype=torch.bfloat16)
    AC = torch.empty(H, B, q, klen, device=dev, dtype=torch.float32)
    T = torch.empty(H, B, q, nd, device=dev, dtype=torch.float32)
    assert ops.relattn_mem_supported(B, q, klen, mlen, H, D, shift, torch.bfloat16, qkv.stride(1), qkv.stride(0))

    def fused():
        ops.relattn_mem_fwd(qu, qv, qkv[:, :, 1], qkv[:, :, 2], R, out_f, None, B, q, klen, mlen, H, D, shift, scale)

    def materialised():     # what _attn_probs and _attention_fwd launch after relattn_add_head_bias
        ops.gemm_batched(qu.permute(2, 0, 1, 3), qkv[:, :, 1].permute(2, 0, 3, 1), AC)
        ops.gemm_batched(qv.permute(2, 0, 1, 3), R.view(nd, H, D).permute(1, 2, 0).unsqueeze(1).expand(H, B, D, nd), T)
        ops.relattn_softmax_fwd(AC, T, None, H, B, q, klen, nd, mlen, shift, scale)
        ops.gemm_batched(AC, qkv[:, :, 2].permute(2, 0, 1, 3), out_m.permute(2, 0, 1, 3))

    tf, tm = timed_pair(fused, materialised, reps)
    diff = float((out_f.float() - out_m.float()).abs().max() / out_m.float().abs().max())
    # operations of the fused kernel: per 32-key step and 16-query tile 8 + 12 + 8 MFMA of 16 x 16 x 32 (S, the 48 distances, P.V)
    steps = sum(((min(i0 + 63, q - 1) + mlen) >> 5) - (max(0, i0 - shift + 1) >> 5) + 1 for i0 in range(0, q, 64))
    flop = 2.0 * 16 * 16 * 32 * 28 * 4 * steps * B * H
    useful = 2.0 * B * H * D * 3 * sum(min(shift + mlen, i + mlen + 1) for i in range(q))
    rec = dict(B=B, H=H, q=q, mlen=mlen, shift=shift, fused_ms=stat(tf), materialised_ms=stat(tm),
               speedup_median=round(stat(tm)["median"] / stat(tf)["median"], 2), fused_issued_TFLOP=round(flop / 1e12, 3),
               fused_issued_TFLOPs_per_s=round(flop / 1e12 / (stat(tf)["median"] * 1e-3), 1), visible_pairs_TFLOP=round(useful / 1e12, 3),
               fp32_score_bytes_GB=round(2 * AC.numel() * 4 / 1e9, 2), max_diff_over_max=round(diff, 5))
    say(json.dumps(rec))
    return rec


# ---- 3 runs first: its processes are started before this one touches the device (every process has the GPU to itself)
stream_lines = []
if not args.no_stream:
    stream_lines.append("## 3. tools/bench_generate.py --stream (256 requests, 64 slots), --mem-attn against the default, three processes each in alternation")
    runs = {"mem_attn": [], "default": []}
    for k in range(3):
        for name, extra in (("mem_attn", ["--mem-attn"]), ("default", [])):
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_generate.py"), "--stream"] + extra, capture_output=True, text=True,
                               timeout=900)
            if p.returncode != 0:
                print(f"bench_generate.py --stream {' '.join(extra)} failed with status {p.returncode}: {p.stderr[-2000:]}", flush=True)
                sys.exit(1)      # (nothing more is started on the device after a failed run)
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            print(f"stream run {k} {name}: admission {rec['stream_admission_ms']} ms, total {rec['stream_total_ms']} ms", flush=True)
            runs[name].append(rec)
    for name, recs in runs.items():
        stream_lines.append(json.dumps(dict(form=name, stream_admission_ms=stat([r["stream_admission_ms"] for r in recs]),
                                            stream_total_ms=stat([r["stream_total_ms"] for r in recs]),
                                            static_total_ms=stat([r["static_total_ms"] for r in recs]),
                                            static_prefill_ms=stat([r["static_prefill_ms"] for r in recs]),
                                            slot_graph_replay_ms=stat([r["slot_graph_replay_ms"] for r in recs]),
                                            runs=dict(stream_admission_ms=[r["stream_admission_ms"] for r in recs],
                                                      stream_total_ms=[r["stream_total_ms"] for r in recs]))))

lib.apply_env_knobs()
say("# fused attention over memory, DB1-1.3B geometry (H = 16, D = 128), bf16; ms from device events, alternated in one process")
say("## 1. db1_relattn_mem_fwd against gemm_batched x 2 + relattn_softmax_fwd + gemm_batched (relattn_add_head_bias on neither side)")
kernel_pair(64, 16, 200, 1024, 0, args.reps)
kernel_pair(16, 16, 1024, 1024, 0, args.reps)
torch.cuda.empty_cache()

say("## 2. score_document, B = 16, T = 4097, segment_len = 1024 (four segments over init_mem), fused=True against fused=False")
torch.manual_seed(0)
model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=torch.bfloat16)
model.eval()
tok = np.random.default_rng(4097).integers(0, 32000, (16, 4097))
from bdm_db1_amd import ScoreConfig  # noqa: E402
scfg = ScoreConfig(return_tokens=False)
res = {}
for name, flag in (("fused", True), ("materialised", False), ("fused", True), ("materialised", False), ("fused", True), ("materialised", False)):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    r = score_document(model, tok, scfg, segment_len=1024, fused=flag)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.setdefault(name, []).append((dt, torch.cuda.max_memory_allocated() / 2 ** 30, r.loss))
for name, runs in res.items():
    runs = runs[1:]                        # (the first run of each form is its warm-up)
    ts = sorted(x[0] for x in runs)
    say(json.dumps(dict(path=name, seconds=[round(t, 4) for t in ts], tokens_per_s=round(16 * 4096 / ts[len(ts) // 2], 1),
                        peak_GiB=round(max(x[1] for x in runs), 2), loss=round(runs[-1][2], 5))))
del model
torch.cuda.empty_cache()

for l in stream_lines:
    say(l)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
