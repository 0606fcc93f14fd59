"""Action decoding for RL rollouts on DB1-1.3B (random weights): milliseconds per environment step, obs_length 17, action_length 6,
continuous actions, M environments.

  (a) ``get_action_batched`` over a ``RingMemory``: per token one eager model call, the torch passes over the logits, argmax, a host copy;
  (b) ``ActionDecoder``: 1 + 6 graph replays with db1_select_actions behind each, one copy back per environment step;
  (c) the bare replays of the two ``GraphedRingStep`` s (the observation call and six token calls) without an epilogue: what (b) cannot go below.

``python tools/bench_actions.py`` drives everything: for (a) and (b) three processes a side, started in alternation (a, b, a, b, a, b), each
measuring every M; the medians with min .. max over the three are reported; then one process for (c) and for the kernels alone
(db1_select_actions against db1_select_tokens over the same window on the same rows, greedy and top-p 0.9, device time from events).  Every
child's record and the summary are appended to ``profiles/actions_1p3b.txt``.  A child that fails ends the run: nothing more is started on
the GPU after it.

  --child a|b|rest     one measuring process (what the driver starts); prints one JSON line per M
  --rows M [M ...]     default 1 4 16 64
  --steps N            timed environment steps per measurement (default 20)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OBS, ACT = 17, 6
OUT = os.path.join(ROOT, "profiles", "actions_1p3b.txt")


def child(kind, rows, steps):
    import numpy as np
    import torch
    from bdm_db1_amd import GraphedRingStep, TransformerXL, ops, synth
    from bdm_db1_amd.data import RLTaskInput
    from bdm_db1_amd.decode import RingMemory
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder, action_window, get_action_batched
    from bdm_db1_amd.tokenizer import ContinuousScalarTokenizer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = synth.db1_config("1.3B")
    model = TransformerXL(cfg, device=dev, compute_dtype=torch.bfloat16)
    model.eval()
    args = SimpleNamespace(overlap_with_text=cfg.overlap_with_text, text_vocab_size=cfg.text_vocab_size, num_discrete_values=cfg.num_discrete_values,
                           num_continuous_bin=cfg.num_continuous_bin, n_position=cfg.n_position, use_prompt=False)
    lo, hi = action_window(args, False)

    def observations(M, n):
        rng = np.random.default_rng(M)
        return [np.concatenate([lo + rng.integers(0, hi - lo, (M, OBS)), np.full((M, 1), hi)], axis=1).astype(np.int64) for _ in range(n)]

    def timed(step_fn, obs):
        for o in obs[:3]:
            step_fn(o)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for o in obs[3:]:
            step_fn(o)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (len(obs) - 3) * 1e3

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

    for M in rows:
        rec = {"case": kind, "M": M, "obs_length": OBS, "action_length": ACT, "steps": steps}
        obs = observations(M, steps + 3)
        with torch.no_grad():
            if kind == "a":
                tok, state = ContinuousScalarTokenizer(cfg.num_continuous_bin), {"mem": RingMemory(model, M)}

                def step_a(o):
                    _, _, state["mem"] = get_action_batched(args, model, torch.from_numpy(o), tok, OBS, ACT, False, None, state["mem"])
                rec["ms_per_env_step"] = round(timed(step_a, obs), 4)
            elif kind == "b":
                dec = ActionDecoder(args, model, M, ActionConfig(OBS, ACT, False))
                rec["ms_per_env_step"] = round(timed(lambda o: dec.act(obs_tokens=o), obs), 4)
                rec["replays_per_env_step"] = dec.stats["replays"] // dec.stats["env_steps"]
            else:
                ring = RingMemory(model, M)
                pos_o = torch.arange(1, OBS + 2, device=dev)[None, :].expand(M, -1).contiguous()
                pos_t = torch.zeros(M, 1, dtype=torch.long, device=dev)
                rl = lambda pos: (lambda ids: RLTaskInput(tensor_seq=ids, vision_seq=None, text_seq=None, attention_mask=None, loss_mask=None, label=None,
                                                          position_id=pos))
                s_tok = GraphedRingStep(model, M, 1, memory=ring, make_input=rl(pos_t))
                s_obs = GraphedRingStep(model, M, OBS + 1, memory=ring, make_input=rl(pos_o))
                s_tok.ids.fill_(lo)

                def step_c(o):
                    s_obs.ids.copy_(torch.from_numpy(o))
                    s_obs(None)
                    for _ in range(ACT):
                        s_tok(None)
                rec["ms_per_env_step"] = round(timed(step_c, obs), 4)
                s_obs.check(synchronize=True)
                s_tok.check(synchronize=True)
                # the kernels alone: the same rows, the same window
                V = int(model.total_vocab_size)
                logits = (torch.randn(M, V, device=dev) * 3).to(torch.bfloat16)
                i32 = dict(dtype=torch.int32, device=dev)
                t, fin, n, status = torch.zeros(1, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
                out, ids = torch.zeros(M, ACT, **i32), torch.zeros(M, dtype=torch.long, device=dev)
                ctr, bins, vals = torch.zeros(2, **i32), torch.zeros(M, ACT, **i32), torch.zeros(M, ACT, device=dev)
                for name, kw in (("greedy", dict(greedy=True)), ("top_p_0.9", dict(greedy=False, top_p=0.9, seed=1))):
                    rec[f"select_tokens_{name}_us"] = round(device_us(lambda: ops.select_tokens(logits, t, fin, n, out, ids, status, V=V, vocab_lo=lo,
                                                                                                  vocab_hi=hi, **kw)), 2)
                    rec[f"select_actions_{name}_us"] = round(device_us(lambda: ops.select_actions(logits, ctr, bins, ids, status, V=V, act_lo=lo,
                                                                                                    act_hi=hi, values=vals, **kw)), 2)
                del s_obs, s_tok
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["a", "b", "rest"])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rows, a.steps)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lines, per = [], {}
    for kind in ["a", "b"] * 3 + ["rest"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps), "--rows"] + [str(m) for m in a.rows]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout + r.stderr[-4000:], file=sys.stderr)
            print(f"child {kind} ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            sys.exit(1)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                rec = json.loads(ln)
                lines.append(ln)
                per.setdefault((rec["case"], rec["M"]), []).append(rec)
                print(ln, flush=True)
    for M in a.rows:
        s = {"summary": True, "M": M}
        for kind in ("a", "b"):
            v = [r["ms_per_env_step"] for r in per[(kind, M)]]
            s[f"{kind}_ms_median"], s[f"{kind}_ms_min"], s[f"{kind}_ms_max"] = statistics.median(v), min(v), max(v)
        rest = per[("rest", M)][0]
        s["c_ms"] = rest["ms_per_env_step"]
        s.update({k: v for k, v in rest.items() if k.endswith("_us")})
        lines.append(json.dumps(s))
        print(lines[-1], flush=True)
    with open(OUT, "a") as f:
        f.write(f"# tools/bench_actions.py --rows {' '.join(map(str, a.rows))} --steps {a.steps}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
