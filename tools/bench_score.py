#!/usr/bin/env python3
"""Scoring at the DB1-1.3B geometry (bf16, seeded random init), three comparisons, the two sides of each alternated in one process, every shape
warmed up, device events around synchronised work:

  * db1_score_rows against db1_masked_ce_fwd on one 16 384 x 33 280 chunk of bf16 logits (V = 33 025);
  * score() on a 64 x 1024 text batch against the eval-mode forward(compute_loss=True) of the same batch (time and peak memory);
  * rank_answers for G = 16 prompts (4 prompt tokens + 196 patches + 8 question tokens), K = 8 candidates of Lc = 4 tokens against the
    teacher-forced single call over the G * K full sequences (prompt (+) candidate over the zero memory).

    python tools/bench_score.py [--out profiles/score_1p3b.txt] [--reps 7]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdm_db1_amd import ScoreConfig, TransformerXL, lib, ops, rank_answers, score, synth  # noqa: E402
from bdm_db1_amd.data import ICTaskInput, VQATaskInput  # noqa: E402
lib.apply_env_knobs()

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_1p3b.txt"))
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
dev = torch.device("cuda", 0)


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


lines, records = [], []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


# ---- 1. the row kernel against the CE forward on one chunk
T, V, ld = 16384, 33025, 33280
g = torch.Generator(device=dev).manual_seed(0)
logits = (torch.randn(T, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
labels = torch.randint(0, V, (T,), device=dev, generator=g)
mask = torch.ones(T, device=dev)
lse, lp = torch.empty(T, device=dev), torch.empty(T, device=dev)
t1, rk, st = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
sums = torch.zeros(2, device=dev)
a, b = timed_pair(lambda: ops.score_rows(logits, labels, lse, lp, t1, rk, st, V=V),
                  lambda: ops.masked_ce_fwd(logits, labels, mask, lse, sums, V), max(args.reps, 15))
sa, sb = stat(a), stat(b)
gb = T * ld * 2 / 1e9
rec = dict(what="score_rows_vs_masked_ce_fwd", rows=T, ld=ld, score_rows_us={k: round(v * 1e3, 1) for k, v in sa.items()},
           masked_ce_fwd_us={k: round(v * 1e3, 1) for k, v in sb.items()}, ratio_of_medians=round(sa["median"] / sb["median"], 3),
           score_rows_TBps=round(gb / sa["median"], 2), masked_ce_fwd_TBps=round(gb / sb["median"], 2))
records.append(rec)
say(f"db1_score_rows      {rec['score_rows_us']} us   ({rec['score_rows_TBps']} TB/s of logits read)")
say(f"db1_masked_ce_fwd   {rec['masked_ce_fwd_us']} us   ({rec['masked_ce_fwd_TBps']} TB/s; includes its 1-block loss sum)")
say(f"ratio of medians    {rec['ratio_of_medians']}")
del logits

# ---- 2. score() against the eval-mode forward at 64 x 1024
torch.manual_seed(0)
model = TransformerXL(synth.db1_config("1.3B"), device=dev, compute_dtype=torch.bfloat16)
model.eval()
B, L = 64, 1024
batch = synth.text_batch(B, L, 1, dev)
cfg = ScoreConfig(return_tokens=False)


def fwd():
    with torch.no_grad():
        return model([batch], compute_loss=True)[1]


def peak(f):
    f()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 30


a, b = timed_pair(lambda: score(model, [batch], cfg), fwd, args.reps)
sa, sb = stat(a), stat(b)
rec = dict(what="score_vs_eval_forward", B=B, L=L, score_ms=sa, forward_ms=sb, ratio_of_medians=round(sa["median"] / sb["median"], 4),
           forward_spread=round((sb["max"] - sb["min"]) / sb["median"], 4), score_peak_GiB=round(peak(lambda: score(model, [batch], cfg)), 2),
           forward_peak_GiB=round(peak(fwd), 2), loss_score=round(score(model, [batch], cfg).loss, 6), loss_forward=round(float(fwd()), 6))
records.append(rec)
say()
say(f"score()                         {sa} ms   peak {rec['score_peak_GiB']} GiB   loss {rec['loss_score']}")
say(f"eval forward(compute_loss=True) {sb} ms   peak {rec['forward_peak_GiB']} GiB   loss {rec['loss_forward']}")
say(f"ratio of medians {rec['ratio_of_medians']}; spread of the forward itself (max - min) / median = {rec['forward_spread']}")

# ---- 3. rank_answers against the single call over the G * K full sequences
G, K, Lc = 16, 8, 4
rng = np.random.default_rng(2)
prompt = torch.from_numpy(rng.integers(0, 32000, (G, 4))).to(dev)
img = torch.from_numpy(rng.standard_normal((G, 3, 224, 224)).astype(np.float32)).to(dev)
ques = torch.from_numpy(rng.integers(1, 32000, (G, 8))).to(dev)
cand = rng.integers(1, 32000, (G, K, Lc))
base = dict(position_id=None, attention_mask=None, loss_mask=None, label=None)
vqa = VQATaskInput(prompt_seq=prompt, img_seq=img, text_seq=ques, img_id_seq=None, ques_id_seq=None, ques_len=None, **base)
full = ICTaskInput(prompt_seq=prompt.repeat_interleave(K, 0), img_seq=img.repeat_interleave(K, 0),
                   text_seq=torch.cat([ques.repeat_interleave(K, 0), torch.from_numpy(cand.reshape(G * K, Lc)).to(dev)], 1), **base)
flat = torch.from_numpy(cand.reshape(-1)).to(dev)


def single_call(want_scale=False):
    """-> logprob [G, K, Lc] (and, outside the timed calls, max|logits| of the call)"""
    V = model.total_vocab_size
    with torch.no_grad():
        model._dec_state = None
        lg, _, _ = model([full], compute_loss=False, mems=model.init_mem(G * K))
        Lf = lg.shape[1]
        rows = torch.zeros(G * K * Lc, (V + 7) // 8 * 8, dtype=lg.dtype, device=dev)       # rows of a 16-byte multiple
        rows[:, :V] = lg[:, Lf - Lc - 1:Lf - 1].reshape(G * K * Lc, V)
        f = lambda dt: torch.empty(G * K * Lc, dtype=dt, device=dev)
        out = [f(torch.float32), f(torch.float32), f(torch.int32), f(torch.int32), f(torch.int32)]
        ops.score_rows(rows, flat, *out, V=V, vocab_hi=32000)
        model._dec_state = None
        return (out[1].view(G, K, Lc), float(lg.abs().max())) if want_scale else out[1].view(G, K, Lc)


a, b = timed_pair(lambda: rank_answers(model, vqa, cand), single_call, args.reps)
sa, sb = stat(a), stat(b)
ref_lp, scale = single_call(want_scale=True)
d = (rank_answers(model, vqa, cand)[2] - ref_lp.cpu()).abs()
per_pos = [round(float(d[:, :, i].max()), 4) for i in range(Lc)]
rec = dict(what="rank_answers_vs_single_call", G=G, K=K, Lc=Lc, rank_answers_ms=sa, single_call_ms=sb, ratio_of_medians=round(sa["median"] / sb["median"], 4),
           max_abs_logprob_difference=round(float(d.max()), 4), mean_abs_logprob_difference=round(float(d.mean()), 4),
           max_abs_difference_per_position=per_pos, max_abs_logits=round(scale, 3), derived_bound_6e_2_of_max_logits=round(6e-2 * scale, 4))
records.append(rec)
say()
say(f"rank_answers (prefill of {G} rows + one {G * K}-row call of {Lc - 1} tokens) {sa} ms")
say(f"single call over {G * K} full sequences of {full.text_seq.shape[1] + 4 + 196} tokens           {sb} ms")
say(f"ratio of medians {rec['ratio_of_medians']}; |logprob difference| between the two: max {rec['max_abs_logprob_difference']}, mean "
    f"{rec['mean_abs_logprob_difference']}, max per candidate position {per_pos}; max|logits| {rec['max_abs_logits']}, so the bound 6e-2 x "
    f"max|logits| the tests derive is {rec['derived_bound_6e_2_of_max_logits']}")
say()
for r in records:
    say(json.dumps(r))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("Scoring at DB1-1.3B (bf16, seeded random init).  MI355X, one run; times from device events around synchronised work, the two sides of\n"
            "each comparison alternated in one process after warm-up; {median, min, max} over the repetitions.\n\n"
            f"  python tools/bench_score.py --reps {args.reps}\n\n" + "\n".join(lines) + "\n")
