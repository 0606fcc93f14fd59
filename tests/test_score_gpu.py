"""Scoring end to end (bdm_db1_amd.scoring): token log-probs against the NumPy oracle's logits, the loss against the eval-mode forward,
mixtures and the validation report, the memory the sweep saves, candidate ranking against a teacher-forced single call, agreement with
generation, and training after scoring."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

import gpu_common  # noqa: E402
import score_rule as R  # noqa: E402
from gpu_common import _model, _need_gpu, _prompt, _tdev  # noqa: E402,F401


def _inputs(tasks):
    from bdm_db1_amd.data import ICTaskInput, NLPTaskInput, RLTaskInput, VQATaskInput
    T = lambda a: None if a is None else _tdev(a)
    out = []
    for t in tasks:
        base = dict(position_id=T(t.get("position_id")), attention_mask=None, loss_mask=T(t.get("loss_mask")), label=T(t.get("label")))
        if t["kind"] == "nlp":
            out.append(NLPTaskInput(text_seq=T(t["text_seq"]), text_len=None, **base))
        elif t["kind"] == "rl":
            out.append(RLTaskInput(text_seq=None, vision_seq=T(t["vision_seq"]), tensor_seq=T(t["tensor_seq"]), **base))
        elif t["kind"] == "vqa":
            out.append(VQATaskInput(prompt_seq=T(t["prompt_seq"]), img_seq=T(t["img_seq"]), text_seq=T(t["text_seq"]), img_id_seq=None,
                                    ques_id_seq=None, ques_len=T(t["ques_len"]), **base))
        else:
            out.append(ICTaskInput(prompt_seq=T(t["prompt_seq"]), img_seq=T(t["img_seq"]), text_seq=T(t["text_seq"]), img_id_seq=None, **base))
    return out


def _batch(name, cfg):
    from golden_util import make_batch
    return make_batch(name, cfg, 7)


def _check_rows_against_logits(lp, top1, rank, ref_logits, labels, lo, hi, tol):
    """every row: logprob within tol of the float64 log-softmax of ``ref_logits`` over [lo, hi); top1 an arg-max up to tol; rank inside the
    interval the tolerance allows"""
    worst = 0.0
    for r in range(ref_logits.shape[0]):
        l = ref_logits[r, lo:hi].astype(np.float64)
        y = int(labels[r])
        lse = np.logaddexp.reduce(l)
        assert lo <= y < hi
        ly = ref_logits[r, y]
        worst = max(worst, abs(float(lp[r]) - (ly - lse)))
        assert lo <= top1[r] < hi and ref_logits[r, top1[r]] >= l.max() - tol, r
        assert np.sum(l > ly + tol) <= rank[r] <= np.sum(l >= ly - tol) - 1, r
    return worst


@pytest.mark.parametrize("name", ["small_mixed", "small_vqa"])     # rl + nlp + ic, vqa + nlp
def test_fp32_token_scores_follow_the_oracle(name):
    from oracle import db1_oracle as O
    from bdm_db1_amd import ScoreConfig, score
    cfg, model, oracle = _model(name)
    tasks = _batch(name, cfg)
    V = model.total_vocab_size
    ref_logits, ref_loss, _ = oracle.forward([O.TaskBatch(**t) for t in tasks])
    # 2e-4 of max|logits|: twice the 1e-4-of-max gate test_model_gpu.py puts on the logits themselves (a log-prob is a difference of two such quantities)
    tol = 2e-4 * np.abs(ref_logits).max()
    for scfg in (ScoreConfig(), ScoreConfig(chunk_rows=40)):
        res = score(model, _inputs(tasks), scfg)
        assert res.stats["sweeps"] == 1 and res.status == 0 and res.kinds == [t["kind"] for t in tasks]
        r0 = 0
        for i, t in enumerate(tasks):
            B, L = t["label"].shape
            lab = t["label"].copy()
            if t["kind"] == "rl":
                lab[lab == -1] = 0                    # transformer_xl.py:644-645
            assert res.logprob[i].shape == res.top1[i].shape == res.rank[i].shape == (B, L)
            worst = _check_rows_against_logits(res.logprob[i].reshape(-1), res.top1[i].reshape(-1), res.rank[i].reshape(-1),
                                               ref_logits[r0:r0 + B].reshape(B * L, -1), lab.reshape(-1), 0, V, tol)
            print(f"{name}/{t['kind']}: max |logprob - oracle| {worst:.2e} (tol {tol:.2e})")
            assert worst <= tol
            # the per-sequence sums are the masked sums of the per-token results
            seq = slice(int(np.sum(res.task < i)), int(np.sum(res.task <= i)))
            assert np.allclose(res.sum_logprob[seq], (res.logprob[i].astype(np.float64) * t["loss_mask"]).sum(1), rtol=1e-6, atol=0)
            assert (res.tokens[seq] == t["loss_mask"].sum(1)).all()
            assert (res.hits[seq] == ((res.rank[i] == 0) * t["loss_mask"]).sum(1)).all()
            r0 += B
        assert abs(res.loss - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))


def test_text_window_scores_follow_the_oracle():
    from oracle import db1_oracle as O
    from bdm_db1_amd import ScoreConfig, score
    cfg, model, oracle = _model("small_window")
    tasks = _batch("small_window", cfg)
    hi = cfg["text_vocab_size"]
    ref_logits, _, _ = oracle.forward([O.TaskBatch(**t) for t in tasks])
    tol = 2e-4 * np.abs(ref_logits).max()
    res = score(model, _inputs(tasks), ScoreConfig(vocab_lo=1, vocab_hi=hi))
    B, L = tasks[0]["label"].shape
    lab = tasks[0]["label"].reshape(-1)
    keep = lab >= 1                           # label 0 lies outside the window: -inf, rank -1, status bit 0
    lp = res.logprob[0].reshape(-1)
    assert (lp[~keep] == -np.inf).all() and (res.rank[0].reshape(-1)[~keep] == -1).all() and \
        res.status == (1 if (~keep & (tasks[0]["loss_mask"].reshape(-1) != 0)).any() else 0)      # (status: the rows that count only)
    worst = _check_rows_against_logits(lp[keep], res.top1[0].reshape(-1)[keep], res.rank[0].reshape(-1)[keep],
                                       ref_logits.reshape(B * L, -1)[keep], lab[keep], 1, hi, tol)
    assert worst <= tol


@pytest.mark.parametrize("chunk_rows", [None, 64, 100])      # T = 288: one chunk; 4.5 chunks; 2.88 chunks
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loss_equals_the_eval_mode_forward(dtype, chunk_rows):
    from bdm_db1_amd import ScoreConfig, score
    cfg, model, _ = _model("small_mixed", dtype)
    tasks = _batch("small_mixed", cfg)
    with torch.no_grad():
        _, loss = model(_inputs(tasks), compute_loss=True)
    res = score(model, _inputs(tasks), ScoreConfig(chunk_rows=chunk_rows))
    # bf16: both read bf16 logits of the same operands; the bound is the issue's 1e-5 also where the sweep takes several chunks, the last one short
    rel = abs(res.loss - float(loss)) / abs(float(loss))
    print(f"{dtype} chunk_rows {chunk_rows}: loss {float(loss):.7f} score {res.loss:.7f} rel {rel:.2e}")
    assert rel <= 1e-5
    assert not model.training and model._score_sink is None
    model.train()
    score(model, _inputs(tasks))
    assert model.training                       # the mode is restored


def test_mixture_equals_separate_calls_and_report_recombines():
    from bdm_db1_amd import score, validation_report
    cfg, model, _ = _model("small_mixed")
    tasks = _batch("small_mixed", cfg)
    order = [1, 2, 0]                           # [nlp, ic, rl]
    tasks = [tasks[i] for i in order]
    assert [t["kind"] for t in tasks] == ["nlp", "ic", "rl"]
    mix = score(model, _inputs(tasks))
    assert mix.task.tolist() == [0, 0, 1, 1, 2, 2]
    # a sequence's rows go through the same kernels whatever else is in the batch (measured difference: 0), so the results are EQUAL
    n0 = 0
    for i, t in enumerate(tasks):
        one = score(model, _inputs([t]))
        n = one.tokens.size
        sl = slice(n0, n0 + n)
        assert (one.tokens == mix.tokens[sl]).all() and (one.hits == mix.hits[sl]).all()
        assert (one.top1[0] == mix.top1[i]).all() and (one.rank[0] == mix.rank[i]).all()
        assert (one.logprob[0].view(np.int32) == mix.logprob[i].view(np.int32)).all()
        assert (one.sum_logprob.view(np.int32) == mix.sum_logprob[sl].view(np.int32)).all()
        n0 += n
    rep = validation_report(model, _inputs(tasks))
    assert set(rep) == {"overall", "nlp", "ic", "rl"}
    tok = sum(rep[k]["tokens"] for k in ("nlp", "ic", "rl"))
    assert tok == rep["overall"]["tokens"] == float(mix.tokens.sum()) and rep["overall"]["sequences"] == 6
    recombined = sum(rep[k]["loss"] * rep[k]["tokens"] for k in ("nlp", "ic", "rl")) / tok
    assert abs(recombined - rep["overall"]["loss"]) <= 1e-9 * abs(recombined)
    assert abs(rep["overall"]["loss"] - mix.loss) <= 1e-9 * abs(mix.loss)
    for k in rep:
        assert abs(rep[k]["ppl"] - np.exp(rep[k]["loss"])) <= 1e-9 * rep[k]["ppl"] and 0.0 <= rep[k]["top1_acc"] <= 1.0


def test_sweep_saves_the_logits_tensor(monkeypatch):
    from bdm_db1_amd import ScoreConfig, TransformerXL, ops, score, synth
    cfg = synth.db1_config("tiny", n_embed=256, n_head=2, n_layer=2, n_position=1024, mem_len=1024, fp16=True)
    torch.manual_seed(3)
    model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)
    model.eval()
    B, L = 8, 1024
    batch = synth.text_batch(B, L, 1, DEV)
    calls = {"ce": 0}
    real = ops.masked_ce_fwd
    monkeypatch.setattr(ops, "masked_ce_fwd", lambda *a, **k: (calls.__setitem__("ce", calls["ce"] + 1), real(*a, **k))[1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    res = score(model, [batch], ScoreConfig(chunk_rows=2048, return_tokens=False))
    torch.cuda.synchronize()
    peak_score = torch.cuda.max_memory_allocated()
    assert res.stats["sweeps"] == 1 and calls["ce"] == 0          # the hook was taken
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        _, loss = model([batch], compute_loss=True)
    torch.cuda.synchronize()
    peak_fwd = torch.cuda.max_memory_allocated()
    assert calls["ce"] == 1
    logits_bytes = B * L * model.vocab_pad * 2
    print(f"peak: score {peak_score / 2**20:.0f} MiB, forward {peak_fwd / 2**20:.0f} MiB, logits tensor {logits_bytes / 2**20:.0f} MiB")
    # the chunk is a quarter of T: three quarters of the logits tensor are saved; at least half of it is required
    assert peak_score <= peak_fwd - logits_bytes // 2
    # four chunks of 2048 rows against the forward's one GEMM over 8192 rows: the same 1e-5 relative as the one-chunk case
    print(f"loss: forward {float(loss):.7f} score {res.loss:.7f}")
    assert abs(res.loss - float(loss)) <= 1e-5 * abs(float(loss))


# ------------------------------------------------------------------------------------------------------------- candidate ranking
def _full_sequences(kind, fields, cand):
    """the G * K sequences prompt (+) candidate as oracle / model fields (rows g * K + k)"""
    G, K, Lc = cand.shape
    rep = {k: np.repeat(v, K, axis=0) for k, v in fields.items()}
    rep["text_seq"] = np.concatenate([rep["text_seq"], cand.reshape(G * K, Lc)], axis=1)
    return rep


def _single_call_oracle(oracle, cfg, kind, fields, cand):
    """float64 logits [G * K, Lc, V] of the positions that predict the candidate's tokens, from ONE oracle forward over the zero memory"""
    from oracle import db1_oracle as O
    G, K, Lc = cand.shape
    full = _full_sequences(kind, fields, cand)
    mems = [np.zeros((G * K, cfg["mem_len"], cfg["n_embed"])) for _ in range(cfg["n_layer"])]
    logits, _, _ = oracle.forward([O.TaskBatch(kind="ic" if kind == "vqa" else kind, **full)], compute_loss=False, mems=mems)
    L = logits.shape[1]
    return logits[:, L - Lc - 1:L - 1]


def _score_rows_of(logits3d, labels, V, lo, hi):
    """db1_score_rows on the rows of a [N, L, V] logits slice, copied into a buffer whose rows are a multiple of 16 bytes -> logprob [N * L]"""
    from bdm_db1_amd import ops
    N, L, _ = logits3d.shape
    buf = torch.zeros(N * L, (V + 7) // 8 * 8, dtype=logits3d.dtype, device=logits3d.device)
    buf[:, :V] = logits3d.reshape(N * L, V)
    f = lambda dt: torch.empty(N * L, dtype=dt, device=buf.device)
    lse, lp, t1, rk, st = f(torch.float32), f(torch.float32), f(torch.int32), f(torch.int32), f(torch.int32)
    ops.score_rows(buf, labels, lse, lp, t1, rk, st, V=V, vocab_lo=lo, vocab_hi=hi)
    return lp


def _single_call_model(model, kind, fields, cand, lo, hi):
    """logprob [G, K, Lc] of the candidates from ONE model forward of the G * K full sequences over the zero memory + db1_score_rows"""
    from bdm_db1_amd.data import ICTaskInput, NLPTaskInput
    G, K, Lc = cand.shape
    full = _full_sequences(kind, fields, cand)
    base = dict(position_id=None, attention_mask=None, loss_mask=None, label=None)
    x = NLPTaskInput(text_seq=_tdev(full["text_seq"]), text_len=None, **base) if kind == "nlp" else \
        ICTaskInput(prompt_seq=_tdev(full["prompt_seq"]), img_seq=_tdev(full["img_seq"]), text_seq=_tdev(full["text_seq"]), **base)
    with torch.no_grad():
        model._dec_state = None
        logits, _, _ = model([x], compute_loss=False, mems=model.init_mem(G * K))
    L = logits.shape[1]
    lp = _score_rows_of(logits[:, L - Lc - 1:L - 1], _tdev(cand.reshape(-1)), model.total_vocab_size, lo, hi)
    return lp.view(G, K, Lc).cpu().numpy(), float(logits.float().abs().max())


@pytest.mark.parametrize("kind", ["nlp", "ic", "vqa"])
def test_fp32_rank_candidates_follows_the_oracles_single_call(kind):
    from bdm_db1_amd import ScoreConfig, rank_candidates
    cfg, model, oracle = _model("small_vqa")
    hi = cfg["text_vocab_size"]
    rng = np.random.default_rng(5)
    G, K, Lc = 3, 4, 4                                  # mem_len 40 >= prompt (<= 12) + Lc
    x, fields = _prompt(rng, kind, G, hi)
    cand = rng.integers(1, hi, (G, K, Lc))
    cand[1, 2] = cand[1, 0]                             # two equal candidates: equal scores, the lower k first
    clen = np.full((G, K), Lc)
    clen[0, 1], clen[2, 3] = 2, 1
    scfg = ScoreConfig(vocab_hi=hi, length_penalty=0.7)
    stats = {}
    scores, order, lp = rank_candidates(model, x, cand, clen, scfg, stats=stats)
    assert stats["model_calls"] == 2 and scores.shape == (G, K) and order.shape == (G, K) and lp.shape == (G, K, Lc)
    assert scores.dtype == torch.float32 and order.dtype == torch.int64 and lp.dtype == torch.float32
    ref = _single_call_oracle(oracle, cfg, kind, fields, cand)[:, :, :hi]
    tol = 2e-4 * np.abs(ref).max()
    ref_lp = (np.take_along_axis(ref, cand.reshape(G * K, Lc, 1), 2)[..., 0] - np.logaddexp.reduce(ref, axis=2)).reshape(G, K, Lc)
    lp = lp.numpy()
    keep = np.arange(Lc)[None, None] < clen[:, :, None]
    err = np.abs(lp - ref_lp)[keep].max()
    print(f"{kind}: max |logprob - oracle single call| {err:.2e} (tol {tol:.2e})")
    assert err <= tol and (lp[~keep] == 0).all()
    # scores and order: exactly the rule applied to the returned log-probs
    s_ref, o_ref = R.candidate_scores(lp, clen, 0.7)
    assert np.abs(scores.numpy() - s_ref).max() <= 1e-6 * np.abs(s_ref).max()
    assert (order.numpy() == np.argsort(-scores.numpy(), axis=1, kind="stable")).all()
    assert scores[1, 0] == scores[1, 2] and list(order[1].numpy()).index(0) < list(order[1].numpy()).index(2)
    # shortening a candidate leaves its earlier entries bit-equal
    _, _, lp_full = rank_candidates(model, x, cand, None, scfg)
    assert (lp_full.numpy()[keep].view(np.int32) == lp[keep].view(np.int32)).all()


def test_rank_candidates_shared_candidates_and_single_token():
    from bdm_db1_amd import ScoreConfig, rank_candidates
    cfg, model, _ = _model("small_vqa")
    hi = cfg["text_vocab_size"]
    rng = np.random.default_rng(6)
    G, K = 3, 5
    x, _ = _prompt(rng, "nlp", G, hi)
    shared = rng.integers(1, hi, (K, 3))
    a = rank_candidates(model, x, shared, config=ScoreConfig(vocab_hi=hi))
    b = rank_candidates(model, x, np.broadcast_to(shared, (G, K, 3)).copy(), config=ScoreConfig(vocab_hi=hi))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    stats = {}
    s1, o1, lp1 = rank_candidates(model, x, shared[:, :1], config=ScoreConfig(vocab_hi=hi), stats=stats)
    assert stats["model_calls"] == 1 and lp1.shape == (G, K, 1)
    assert (lp1[:, :, 0].numpy().view(np.int32) == a[2][:, :, 0].numpy().view(np.int32)).all() and torch.equal(s1, lp1[:, :, 0])
    for bad in (dict(cand_len=0), dict(cand_len=4)):
        with pytest.raises(ValueError):
            rank_candidates(model, x, shared, **bad)
    with pytest.raises(ValueError):
        rank_candidates(model, x, np.full((K, 3), 10 ** 6))


def _bf16_model(seed=5):
    return gpu_common._bf16_model(seed)[1]


@pytest.mark.parametrize("kind", ["nlp", "ic", "vqa"])
def test_bf16_rank_candidates_matches_the_single_call(kind):
    from bdm_db1_amd import ScoreConfig, rank_candidates
    model = _bf16_model()
    hi = 32000
    rng = np.random.default_rng(8)
    G, K, Lc = 3, 4, 4
    x, fields = _prompt(rng, kind, G, hi)
    cand = rng.integers(1, hi, (G, K, Lc))
    _, _, lp = rank_candidates(model, x, cand, config=ScoreConfig(vocab_hi=hi))
    ref, scale = _single_call_model(model, kind, fields, cand, 0, hi)
    # The long single call and the prefill + short call take different attention kernels.  test_decode_gpu.py accepts 3e-2 relative error on the
    # logits between "two bf16 pipelines, different rounding points"; a log-prob is a difference of two such quantities: 6e-2 of max|logits|.
    # Measured on this model: 2.0e-3 (nlp), 0 (ic), 5.2e-4 (vqa) against a bound of 0.33 (max|logits| 5.5 .. 5.6) -- far below it; the derived
    # bound is kept.
    tol = 6e-2 * scale
    err = np.abs(lp.numpy() - ref).max()
    print(f"bf16 {kind}: max |logprob - single call| {err:.3e} (derived bound {tol:.3e}, max|logits| {scale:.3f})")
    assert err <= tol


def test_rank_answers_agrees_with_greedy_generation():
    from bdm_db1_amd import GenerationConfig, ScoreConfig, answer_questions, rank_answers
    cfg, model, oracle = _model("small_vqa")
    hi = cfg["text_vocab_size"]
    rng = np.random.default_rng(12)
    G, K, Lc = 4, 6, 3
    x, fields = _prompt(rng, "vqa", G, hi)
    ids, _ = answer_questions(model, x, GenerationConfig(max_new_tokens=Lc, vocab_hi=hi))
    a = ids.numpy().astype(np.int64)                                   # [G, Lc]: the greedy answers
    cand = np.repeat(a[:, None, :], K, axis=1)
    for g in range(G):
        others = [t for t in rng.permutation(hi) if t != a[g, -1]][:K - 1]
        cand[g, 1:, -1] = others
    scores, order, lp = rank_answers(model, x, cand, config=ScoreConfig(length_penalty=0.0))
    # the oracle's logits of the last step, teacher-forced on the greedy answer: candidate 0 must win where its top-2 gap is clear
    ref = _single_call_oracle(oracle, cfg, "vqa", fields, a[:, None, :])[:, -1, :hi]
    tol = 2e-4 * np.abs(ref).max()
    srt = np.sort(ref, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > tol
    assert clear.sum() >= 3, clear
    for g in np.nonzero(clear)[0]:
        assert int(np.argmax(ref[g])) == a[g, -1], g
        assert int(order[g, 0]) == 0, (g, scores[g])
        assert (lp[g, :, :-1].numpy().view(np.int32) == lp[g, 0, :-1].numpy().view(np.int32)).all()    # the common prefix: the same bits


def _bf16_answer_case(model_seed, prompt_seed, G=4, K=6, Lc=3, hi=32000):
    """greedy bf16 answers, K candidates that differ in the last token, rank_answers, and the eager loop's logits of the last step"""
    from bdm_db1_amd import GenerationConfig, ScoreConfig, answer_questions, rank_answers
    from bdm_db1_amd.data import NLPTaskInput
    model = _bf16_model(model_seed)
    rng = np.random.default_rng(prompt_seed)
    x, _ = _prompt(rng, "vqa", G, hi)
    ids, _ = answer_questions(model, x, GenerationConfig(max_new_tokens=Lc, vocab_hi=hi))
    a = ids.numpy().astype(np.int64)
    cand = np.repeat(a[:, None, :], K, axis=1)
    for g in range(G):
        cand[g, 1:, -1] = [t for t in rng.permutation(hi) if t != a[g, -1]][:K - 1]
    scores, order, lp = rank_answers(model, x, cand, config=ScoreConfig(length_penalty=0.0))
    # the eager loop: the prompt, then the answer's tokens one per call over the list-form memory; the logits that choose the last token
    with torch.no_grad():
        model._dec_state = None
        logits, _, mems = model([x], compute_loss=False, mems=model.init_mem(G))
        for t in range(Lc - 1):
            y = NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(a[:, t:t + 1]), text_len=None)
            logits, _, mems = model([y], compute_loss=False, mems=mems)
        model._dec_state = None
    last = logits[:, -1, :hi].double().cpu().numpy()
    return a, order.numpy(), scores.numpy(), lp.numpy(), last


def test_bf16_rank_answers_agrees_with_greedy_generation():
    a, order, scores, lp, last = _bf16_answer_case(model_seed=5, prompt_seed=12)
    # the candidates share every term but the last, so their order is the order of the last step's logits; between two bf16 pipelines the
    # project accepts 3e-2 of max|logits| on a logit (test_decode_gpu.py), on a difference of two logits twice that
    tol = 6e-2 * np.abs(last).max()
    srt = np.sort(last, axis=1)
    gap = srt[:, -1] - srt[:, -2]
    print(f"bf16: top-2 gaps of the eager loop {gap} against tol {tol:.3f}")
    clear = gap > tol
    assert clear.sum() >= 3, (gap, tol)
    for g in np.nonzero(clear)[0]:
        assert int(np.argmax(last[g])) == a[g, -1], g
        assert int(order[g, 0]) == 0, (g, scores[g])
        assert (lp[g, :, :-1].view(np.int32) == lp[g, 0, :-1].view(np.int32)).all()      # the common prefix: the same bits


def test_training_after_scoring_is_bit_equal():
    """the bit-reproducible optimizer step of test_model_gpu.py (bf16 mixture batch, dropout, global-norm clip, AdamW, fused head + loss: no
    float atomics on this path), twice from the same state, once with a score() call between the two steps"""
    from bdm_db1_amd import TransformerXL, initialize, score, synth
    cfg = synth.db1_config("1.3B", n_layer=2, n_embed=512, n_head=4, drop=0.1, embd_pdrop=0.1)

    def run(with_score):
        torch.manual_seed(7)
        model = TransformerXL(cfg, compute_dtype=torch.bfloat16)
        eargs = SimpleNamespace(lr=1e-3, weight_decay=0.01, clip_grad=1.0, optimizer="adamw", keep_logits=False, fuse_head_loss=True)
        engine, _, _, _ = initialize(eargs, model)
        engine.train()
        batch = synth.mixture_batch(4, cfg.n_position, 3, DEV, cfg)
        losses = []
        for step in range(2):
            _, loss = engine(batch)
            engine.backward(loss)
            grads = model.arena.grad.clone()
            engine.step()
            losses.append(float(loss))
            if step == 0 and with_score:
                res = score(model, batch)
                assert model.training and res.stats["sweeps"] == 1 and res.kinds == ["rl", "nlp", "ic"] and np.isfinite(res.loss)
        return model, losses, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}

    model, l0, g0, p0 = run(False)
    _, l1, g1, p1 = run(True)
    assert l0 == l1, (l0, l1)
    bad = [n for n in model.arena.offsets if not torch.equal(model.arena.view(g0, n), model.arena.view(g1, n))]
    assert not bad, bad
    badp = [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert not badp, badp
