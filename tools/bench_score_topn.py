"""db1_score_rows_top (n = 1, 5, 16) against db1_score_rows on the chunk tools/bench_score.py uses (16 384 x 33 280 bf16), and score() at
64 x 1024 on DB1-1.3B with and without top_n=5; every set of calls in alternation, one JSON line each (profiles/score_topn_1p3b.txt).

    python tools/bench_score_topn.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bdm_db1_amd import ScoreConfig, TransformerXL, ops, score, synth
dev = torch.device("cuda", 0)

def timed(fs, reps):
    for f in fs * 2:
        f()
    torch.cuda.synchronize()
    out = [[] for _ in fs]
    for _ in range(reps):
        for f, dst in zip(fs, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); f(); e1.record(); torch.cuda.synchronize()
            dst.append(e0.elapsed_time(e1))
    return out

def stat(x):
    x = sorted(x)
    return dict(median=round(x[len(x) // 2], 4), min=round(x[0], 4), max=round(x[-1], 4))

T, V, ld = 16384, 33025, 33280
g = torch.Generator(device=dev).manual_seed(0)
logits = (torch.randn(T, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
labels = torch.randint(0, V, (T,), device=dev, generator=g)
lse, lp = torch.empty(T, device=dev), torch.empty(T, device=dev)
t1, rk, st = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
tops = {n: (torch.empty(T, n, dtype=torch.int32, device=dev), torch.empty(T, n, device=dev)) for n in (1, 5, 16)}
fs = [lambda: ops.score_rows(logits, labels, lse, lp, t1, rk, st, V=V)] + \
     [lambda n=n: ops.score_rows(logits, labels, lse, lp, t1, rk, st, V=V, top_n=n, top_ids=tops[n][0], top_logprob=tops[n][1]) for n in (1, 5, 16)]
r = timed(fs, 15)
rec = dict(what="score_rows_top_vs_score_rows", rows=T, ld=ld, dtype="bf16", score_rows_us={k: round(v * 1e3, 1) for k, v in stat(r[0]).items()})
for n, x in zip((1, 5, 16), r[1:]):
    rec[f"score_rows_top{n}_us"] = {k: round(v * 1e3, 1) for k, v in stat(x).items()}
print(json.dumps(rec), flush=True)
del logits
torch.manual_seed(0)
model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=torch.bfloat16)
model.eval()
B, L = 64, 1024
batch = synth.text_batch(B, L, 1, dev)
r = timed([lambda: score(model, [batch], ScoreConfig()), lambda: score(model, [batch], ScoreConfig(top_n=5))], 5)
print(json.dumps(dict(what="score_64x1024", score_ms=stat(r[0]), score_top5_ms=stat(r[1]))), flush=True)
