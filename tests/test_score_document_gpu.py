"""score_document (long-text scoring with segment-level recurrence) and the fused attention over memory in the model: fp32 against the NumPy
oracle chained over the same segments and bit-equal to a hand-written loop over score(..., mems=); bf16 through the new branch of
_attention_fwd (counted launches, logits against an fp32 model of the same parameters); and a prompt prefill with the flag on."""
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

from gpu_common import DEV, _model, _need_gpu, _tdev  # noqa: E402,F401


def _text(ids, label=None, mask=None):
    from bdm_db1_amd.data import NLPTaskInput
    T = lambda a: None if a is None else _tdev(a)
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=T(mask), label=T(label), text_seq=T(ids), text_len=None)


def test_fp32_document_scores_follow_the_oracle_and_the_hand_written_loop():
    from oracle import db1_oracle as O
    from bdm_db1_amd import ScoreConfig, document_segments, score, score_document
    cfg, model, oracle = _model("small_mems")
    Bn, T, seg_len = 2, 60, 24
    n = T - 1
    rng = np.random.default_rng(60)
    tok = rng.integers(0, cfg["text_vocab_size"], (Bn, T))
    lengths = np.array([T, 41])
    mask = (np.arange(n)[None, :] < lengths[:, None] - 1).astype(np.float32)
    segs = document_segments(n, seg_len)
    assert segs == [(0, 24), (24, 48), (48, 59)]
    res = score_document(model, tok, ScoreConfig(top_n=3), segment_len=seg_len, lengths=lengths)
    assert res.kinds == ["nlp"] and res.stats == dict(segments=3, sweeps=3) and res.status == 0
    assert res.logprob[0].shape == res.top1[0].shape == res.rank[0].shape == (Bn, n) and res.top_ids[0].shape == res.top_logprob[0].shape == (Bn, n, 3)
    assert len(res.mems) == cfg["n_layer"] and tuple(res.mems[0].shape) == (Bn, cfg["mem_len"], cfg["n_embed"])
    # ---- the oracle chained over the same segments
    omems = [np.zeros((Bn, cfg["mem_len"], cfg["n_embed"])) for _ in range(cfg["n_layer"])]
    ref = []
    for b0, e0 in segs:
        lg, _, omems = oracle.forward([O.TaskBatch(kind="nlp", text_seq=tok[:, b0:e0].astype(np.int64))], compute_loss=False, mems=omems)
        ref.append(lg)
    ref = np.concatenate(ref, axis=1).astype(np.float64)                      # [B, n, V]
    tol = 2e-4 * np.abs(ref).max()       # (tests/test_score_gpu.py: twice the 1e-4-of-max gate on the logits themselves)
    ref_lp = np.take_along_axis(ref, tok[:, 1:, None], 2)[..., 0] - np.logaddexp.reduce(ref, axis=2)
    worst = float(np.abs(res.logprob[0] - ref_lp).max())
    ref_loss = float(-(ref_lp * mask).sum() / mask.sum())
    print(f"score_document fp32: max |logprob - oracle| {worst:.2e} (tol {tol:.2e}), loss {res.loss:.6f} vs oracle {ref_loss:.6f}")
    assert worst <= tol
    assert abs(res.loss - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    assert (res.tokens == mask.sum(1)).all()
    assert np.allclose(res.sum_logprob, (res.logprob[0].astype(np.float64) * mask).sum(1), rtol=1e-6, atol=0)
    assert (res.top_ids[0][..., 0] == res.top1[0]).all()
    # ---- a hand-written loop over score(..., mems=): the same bits, the same last memory
    mems = model.init_mem(Bn)
    lps = []
    for b0, e0 in segs:
        r = score(model, [_text(tok[:, b0:e0], tok[:, b0 + 1:e0 + 1], mask[:, b0:e0])], ScoreConfig(), mems=mems)
        assert r.mems is not None and r.stats["sweeps"] == 1
        mems = r.mems
        lps.append(r.logprob[0])
    assert np.array_equal(np.concatenate(lps, axis=1).view(np.int32), res.logprob[0].view(np.int32))
    assert all(torch.equal(a, b) for a, b in zip(mems, res.mems))
    # ---- the returned memory continues the document: two halves give the bits of the whole
    half = score_document(model, tok[:, :49], segment_len=seg_len)
    rest = score_document(model, tok[:, 48:], segment_len=seg_len, mems=half.mems)
    whole = score_document(model, tok, segment_len=seg_len)
    assert np.array_equal(np.concatenate([half.logprob[0], rest.logprob[0]], axis=1).view(np.int32), whole.logprob[0].view(np.int32))
    # ---- score without mems returns none, as before
    assert score(model, [_text(tok[:, :24], tok[:, 1:25], mask[:, :24])]).mems is None
    with pytest.raises(ValueError):
        score_document(model, tok, fused=True)                                # fp32: the fused kernel cannot serve it
    assert model.use_mem_attn is False


@pytest.fixture(scope="module")
def d128():
    """the mems_d128 configuration widened to n_position = 128, mem_len = 96: a bf16 model and an fp32 model on the same parameters"""
    from golden_util import case_cfg, make_params
    from bdm_db1_amd import TransformerXL
    cfg = case_cfg("mems_d128")
    cfg.update(n_position=128, mem_len=96)
    params = make_params(cfg, 128)
    models = []
    for dt in (torch.bfloat16, torch.float32):
        m = TransformerXL(SimpleNamespace(**cfg), device=DEV, compute_dtype=dt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        m.eval()
        models.append(m)
    return cfg, models[0], models[1]


class _Count:
    def __init__(self, monkeypatch):
        from bdm_db1_amd import ops
        self.n, self.q = 0, []
        real = ops.relattn_mem_fwd

        def counted(*a, **k):
            self.n += 1
            self.q.append(a[8])
            return real(*a, **k)
        monkeypatch.setattr(ops, "relattn_mem_fwd", counted)


def _chain_logits(model, tok, segs, flag):
    """last-segment logits of the list-form memory path over the segments, with model.use_mem_attn = flag"""
    was = model.use_mem_attn
    model.use_mem_attn = flag
    try:
        with torch.no_grad():
            mems = model.init_mem(tok.shape[0])
            for b0, e0 in segs:
                logits, _, mems = model([_text(tok[:, b0:e0])], compute_loss=False, mems=mems)
    finally:
        model.use_mem_attn = was
    return logits.float().cpu().numpy().astype(np.float64)


def test_bf16_document_takes_the_fused_branch(d128, monkeypatch):
    from bdm_db1_amd import document_segments, score_document
    cfg, model, model32 = d128
    assert model.d_head == 128 and model.use_mem_attn is False
    Bn, seg_len = 2, 80
    rng = np.random.default_rng(231)
    tok = rng.integers(0, cfg["text_vocab_size"], (Bn, 231))                   # n = 230: segments of 80, 80, 70 positions
    cnt = _Count(monkeypatch)
    on = score_document(model, tok, segment_len=seg_len, fused=True)
    assert on.stats == dict(segments=3, sweeps=3) and cnt.n == 3 * cfg["n_layer"] and cnt.q == [80] * 2 * cfg["n_layer"] + [70] * cfg["n_layer"]
    assert model.use_mem_attn is False                                        # restored
    cnt.n = 0
    short = score_document(model, tok[:, :191], segment_len=seg_len, fused=True)      # 80, 80, 30: the last goes the K/V-cached way (<= 64 tokens)
    assert short.stats["segments"] == 3 and cnt.n == 2 * cfg["n_layer"]
    cnt.n = 0
    off = score_document(model, tok, segment_len=seg_len, fused=False)
    assert cnt.n == 0
    cnt.n = 0
    score_document(model, tok, segment_len=seg_len)                           # None: the model's own setting (off)
    assert cnt.n == 0
    model.use_mem_attn = True
    try:
        score_document(model, tok, segment_len=seg_len, fused=False)
        assert cnt.n == 0 and model.use_mem_attn is True
        score_document(model, tok, segment_len=seg_len)
        assert cnt.n == 3 * cfg["n_layer"]
    finally:
        model.use_mem_attn = False
    assert np.isfinite(on.logprob[0]).all() and np.isfinite(off.logprob[0]).all()
    # ---- logits of the last segment against the fp32 model on the same parameters: the bf16 logits gate of tests/test_geometry_gpu.py
    segs = document_segments(230, seg_len)
    ref = _chain_logits(model32, tok, segs, False)
    e = {}
    for name, flag in (("fused", True), ("materialised", False)):
        e[name] = float(np.abs(_chain_logits(model, tok, segs, flag) - ref).max() / np.abs(ref).max())
        print(f"bf16 logits of the last segment vs fp32, {name} path: max-norm rel err {e[name]:.3e}")
    assert e["fused"] < 3e-2
    d = float(np.abs(on.logprob[0].astype(np.float64) - off.logprob[0]).max())
    print(f"max |logprob fused - logprob materialised| = {d:.3e}; loss fused {on.loss:.5f}, materialised {off.loss:.5f}")


def test_prefill_with_the_flag_takes_the_fused_branch(d128, monkeypatch):
    from bdm_db1_amd import generation
    cfg, model, _ = d128
    rng = np.random.default_rng(70)
    prompt = _text(rng.integers(0, cfg["text_vocab_size"], (2, 70)))
    cnt = _Count(monkeypatch)
    with torch.no_grad():
        off, _ = generation._prefill(model, prompt, 2)
        assert cnt.n == 0
        model.use_mem_attn = True
        try:
            on, mems = generation._prefill(model, prompt, 2)
        finally:
            model.use_mem_attn = False
    assert cnt.n == cfg["n_layer"] and cnt.q == [70] * cfg["n_layer"]
    assert len(mems) == cfg["n_layer"] and tuple(mems[0].shape) == (2, cfg["mem_len"], cfg["n_embed"])
    a, b = on[:, -1].float().cpu().numpy().astype(np.float64), off[:, -1].float().cpu().numpy().astype(np.float64)
    e = float(np.abs(a - b).max() / np.abs(b).max())
    print(f"prefill, last-position logits, flag on vs off: max-norm rel err {e:.3e}")
    assert e < 3e-2
