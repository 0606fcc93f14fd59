#!/usr/bin/env python3
"""The prefill straight into the K/V ring at the DB1-1.3B geometry (bf16, H = 16, D = 128, seeded random data / init), three measurements:

  * db1_relattn_mem_kv_fwd (the memory broadcast with strides 0, and a real [B, mlen] memory) against db1_relattn_mem_fwd on the concatenated
    K/V, alternated in ONE process, device events, at B = 64, q = 200, mlen = 1024, shift = 0 and B = 16, q = 1024, mlen = 1024, shift = 0;
    the outputs are compared bit for bit on the way;
  * db1_ring_prefill_rows (all layers: one launch each) against the chain it replaces -- ``RingMemory._project``'s GEMMs over n * mlen rows,
    ``kv8_quantize`` on an fp8 ring, ``ring_load_rows`` -- at n = 16 and 64 rows, q = 200, mlen = 1024, bf16 and fp8 rings;
  * ``tools/bench_generate.py --stream`` (256 requests, 64 slots) with ``--ring-prefill``, with ``--mem-attn`` and with neither, a process
    each, ``--stream-runs`` runs each in alternation (0 leaves this part out); ``--lockstep`` adds ``bench_generate.py 1 16 64`` and
    ``--num-beams 4`` with and without the flag.

    python tools/bench_ring_prefill.py [--out profiles/ring_prefill_1p3b.txt] [--reps 7] [--stream-runs 3] [--lockstep] [--no-kernels]
                                       [--parent-root DIR]   (a built checkout of the parent commit: its default stream joins part 3)"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bdm_db1_amd import TransformerXL, lib, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_prefill_1p3b.txt"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--stream-runs", type=int, default=3)
ap.add_argument("--lockstep", action="store_true")
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its default stream joins the alternation")
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []
BF = torch.bfloat16


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps):
    """ms of every function of ``fns``, alternated: [reps] each"""
    for f in fns + fns:
        f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for f, dst in zip(fns, out):
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


def bench_child(extra, timeout=1100, root=ROOT):
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_generate.py")] + extra, capture_output=True, text=True, timeout=timeout,
                       cwd=root)
    if p.returncode != 0:
        print(f"bench_generate.py {' '.join(extra)} failed with status {p.returncode}: {p.stderr[-2000:]}", flush=True)
        sys.exit(1)      # (nothing more is started on the device after a failed run)
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


# ---- the child processes first: they are started before this one touches the device (every process has the GPU to itself)
child_lines = []
if args.stream_runs:
    child_lines.append(f"## 3. tools/bench_generate.py --stream (256 requests, 64 slots): --ring-prefill, --mem-attn, neither; {args.stream_runs} processes each in alternation")
    forms = (("ring_prefill", ["--ring-prefill"], ROOT), ("mem_attn", ["--mem-attn"], ROOT), ("default", [], ROOT))
    if args.parent_root:         # (the flag off must cost what the parent commit costs)
        forms += (("parent_default", [], os.path.abspath(args.parent_root)),)
    runs = {name: [] for name, _, _ in forms}
    for k in range(args.stream_runs):
        for name, extra, root in forms:
            rec = bench_child(["--stream"] + extra, root=root)[-1]
            print(f"stream run {k} {name}: admission {rec['stream_admission_ms']} ms, total {rec['stream_total_ms']} ms", flush=True)
            runs[name].append(rec)
    keys = ("stream_admission_ms", "stream_total_ms", "static_total_ms", "static_prefill_ms", "slot_graph_replay_ms", "generate_graph_replay_ms")
    for name, recs in runs.items():
        child_lines.append(json.dumps(dict(form=name, **{k: stat([r[k] for r in recs]) for k in keys}, runs={k: [r[k] for r in recs] for k in keys[:2]})))
if args.lockstep:
    child_lines.append("## 4. tools/bench_generate.py 1 16 64 and --num-beams 4 1 16, with and without --ring-prefill (one process each)")
    for extra in (["1", "16", "64"], ["--ring-prefill", "1", "16", "64"], ["--num-beams", "4", "1", "16"], ["--ring-prefill", "--num-beams", "4", "1", "16"]):
        for rec in bench_child(extra):
            child_lines.append(json.dumps(dict(args=" ".join(extra), **rec)))
            print(child_lines[-1], flush=True)

lib.apply_env_knobs()
H, D = 16, 128


def kernel_a(B, q, mlen, shift, reps):
    klen, scale = mlen + q, 1.0 / math.sqrt(D)
    g = torch.Generator(device=dev).manual_seed(q * 7 + B)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(BF)
    new, mem, row = rnd(B, q, 3, H, D), rnd(B, mlen, 2, H, D), rnd(1, 1, 2, H, D)
    qu, qv, R = rnd(B, q, H, D), rnd(B, q, H, D), rnd(klen, H * D)
    cat = torch.cat([mem, new[:, :, 1:3]], 1).contiguous()
    cat_row = torch.cat([row.expand(B, mlen, 2, H, D), new[:, :, 1:3]], 1).contiguous()
    o = [torch.empty(B, q, H, D, device=dev, dtype=BF) for _ in range(4)]
    fns = [lambda: ops.relattn_mem_fwd(qu, qv, cat[:, :, 0], cat[:, :, 1], R, o[0], None, B, q, klen, mlen, H, D, shift, scale),
           lambda: ops.relattn_mem_kv_fwd(qu, qv, new[:, :, 1], new[:, :, 2], mem[:, :, 0], mem[:, :, 1], R, o[1], None, B, q, mlen, H, D, shift, scale),
           lambda: ops.relattn_mem_kv_fwd(qu, qv, new[:, :, 1], new[:, :, 2], row[:, :, 0], row[:, :, 1], R, o[2], None, B, q, mlen, H, D, shift, scale)]
    t = timed(fns, reps)
    ops.relattn_mem_fwd(qu, qv, cat_row[:, :, 0], cat_row[:, :, 1], R, o[3], None, B, q, klen, mlen, H, D, shift, scale)
    torch.cuda.synchronize()
    say(json.dumps(dict(B=B, q=q, mlen=mlen, shift=shift, relattn_mem_fwd_concatenated_ms=stat(t[0]), relattn_mem_kv_fwd_real_memory_ms=stat(t[1]),
                        relattn_mem_kv_fwd_broadcast_row_ms=stat(t[2]), bit_equal_real=bool(torch.equal(o[0].view(torch.int16), o[1].view(torch.int16))),
                        bit_equal_broadcast=bool(torch.equal(o[3].view(torch.int16), o[2].view(torch.int16))))))


def kernel_b(model, n, q, mlen, fp8, reps):
    from bdm_db1_amd.decode import RingMemory, RingPrefill
    M, nl, d = 64, model.n_layer, model.d_model
    ring = RingMemory(model, M, kv_dtype="fp8" if fp8 else "bf16")
    zkv = RingPrefill(ring).zero_kv()
    g = torch.Generator(device=dev).manual_seed(n + q)
    new = [torch.randn(n, q, 3, H, D, device=dev, generator=g).to(BF) for _ in range(nl)]
    mems = [torch.randn(n, mlen, d, device=dev, generator=g).to(BF) for _ in range(nl)]
    rows = torch.arange(n, dtype=torch.int32, device=dev) * (M // n)

    def direct():
        for i in range(nl):
            ops.ring_prefill_rows(ring.kv[i], new[i][:, :, 1], new[i][:, :, 2], zkv[i][:, :, 0], zkv[i][:, :, 1], ring.state, mlen, rows, None, ring.load_status)

    def chain():
        ring.load_rows(mems, rows)

    def copy_only():
        src = chain.src
        ops.ring_load_rows(ring.kv, ring._ptrs, src, ring.state, mlen, rows, ring.load_status)
    with torch.no_grad():
        chain.src = [torch.empty(n, mlen, *ring.kv[0].shape[2:], device=dev, dtype=ring.kv[0].dtype) for _ in range(nl)]
        t = timed([direct, chain, copy_only], reps)
    written = n * mlen * nl * ring.kv[0][0, 0].numel() * ring.kv[0].element_size()
    md = stat(t[0])["median"]
    say(json.dumps(dict(n=n, q=q, mlen=mlen, ring="fp8" if fp8 else "bf16", layers=nl, ring_prefill_rows_all_layers_ms=stat(t[0]),
                        project_quantize_load_rows_ms=stat(t[1]), ring_load_rows_alone_ms=stat(t[2]), written_MB=round(written / 1e6, 1),
                        ring_prefill_rows_written_TBps=round(written / (md * 1e-3) / 1e12, 3), chain_over_direct=round(stat(t[1])["median"] / md, 1))))
    del ring
    torch.cuda.empty_cache()


if not args.no_kernels:
    say("# prefill straight into the K/V ring, DB1-1.3B geometry (H = 16, D = 128), bf16; ms from device events, alternated in one process")
    say("## 1. db1_relattn_mem_kv_fwd (a real [B, mlen] memory; one memory row, strides 0) against db1_relattn_mem_fwd on the concatenated K/V")
    kernel_a(64, 200, 1024, 0, args.reps)
    kernel_a(16, 1024, 1024, 0, args.reps)
    torch.cuda.empty_cache()
    say("## 2. db1_ring_prefill_rows, one launch per layer, against _project's GEMMs + (kv8_quantize) + ring_load_rows, all 24 layers, a ring of 64 rows")
    torch.manual_seed(0)
    model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=BF)
    model.eval()
    for fp8 in (False, True):
        for n in (16, 64):
            kernel_b(model, n, 200, int(model.mem_len), fp8, args.reps)
    del model
    torch.cuda.empty_cache()

for l in child_lines:
    say(l)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.no_kernels and os.path.exists(args.out) else "w") as f:
    f.write("\n".join(lines) + "\n")
