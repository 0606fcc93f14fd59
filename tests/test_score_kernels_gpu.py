"""db1_score_rows / db1_lmhead_score / db1_score_segments against the NumPy rule (tests/score_rule.py) on the same stored values (bf16 inputs
are made by rounding first, so both sides see identical numbers)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

import score_rule as R  # noqa: E402
from gpu_common import _need_gpu  # noqa: E402,F401

# Both sides sum at most 2^16 positive fp32 terms after subtracting the same maximum, in different orders: a pairwise or blocked fp32 sum of
# that many terms is good to about 16 ulp relative, 2e-6 absolute after the log.  The gate is 1e-5 absolute.
TOL = 1e-5


def _outs(T, nan=True):
    f = torch.full((T,), float("nan"), device=DEV) if nan else torch.empty(T, device=DEV)
    return [f.clone(), f.clone()] + [torch.full((T,), -12345, dtype=torch.int32, device=DEV) for _ in range(3)]


def _rows(rng, T, V, ld, dtype):
    """logits [T, ld] (device, `dtype`) with constructed ties and non-finite entries, labels, and the float32 values as stored"""
    l = (rng.standard_normal((T, ld)) * 3).astype(np.float32)
    labels = rng.integers(0, V, T)
    hi_col = V - 1
    l[0, 5] = l[0, hi_col] = 50.0                   # two equal maxima: top1 = 5
    labels[0] = hi_col                              #   ... and the label ties with them: rank 0
    l[1, 3] = l[1, 2 if V < 200 else 150] = 7.0     # the label (column 3) ties with a larger column (below the maximum or not)
    labels[1] = 3
    l[2, 0:4] = [np.nan, np.inf, -np.inf, 60.0]     # non-finite entries are no candidates
    labels[2] = 1                                   #   ... a label on +inf: logprob -inf, status 1
    l[3, 1] = np.nan
    labels[3] = 1
    labels[4] = -100                                # ignored
    labels[5] = V + 3 if T > 5 else labels[4]       # ignored (beyond the vocabulary)
    l[6, :] = np.nan                                # no candidate at all
    l[7, :] = -np.inf
    labels[7] = -1
    l[:, V:] = 1e9                                  # the padding columns must never be read as candidates
    t = torch.from_numpy(l).to(DEV).to(dtype)
    return t, torch.from_numpy(labels).to(DEV), t.float().cpu().numpy()


def _compare(got, ref, exact_only=False):
    lse, lp, t1, rk, st = [g.cpu().numpy() for g in got]
    assert (t1 == ref[2]).all(), np.nonzero(t1 != ref[2])
    assert (rk == ref[3]).all(), np.nonzero(rk != ref[3])
    assert (st == ref[4]).all(), np.nonzero(st != ref[4])
    for g, r, name in ((lse, ref[0], "lse"), (lp, ref[1], "logprob")):
        assert not np.isnan(g).any(), name
        inf = np.isinf(r)
        assert (g[inf] == r[inf]).all(), name
        err = np.abs(g[~inf].astype(np.float64) - r[~inf]).max() if (~inf).any() else 0.0
        print(f"{name}: max abs err {err:.2e}")
        assert err <= TOL, (name, err)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V,ld,text_hi", [(33025, 33280, 32000), (365, 512, 300)])
def test_score_rows_matches_the_rule(dtype, V, ld, text_hi):
    from bdm_db1_amd import ops
    assert ops.score_rows_supported(V, ld, dtype)
    rng = np.random.default_rng(V)
    T = 24
    logits, labels, stored = _rows(rng, T, V, ld, dtype)
    before = logits.clone()
    for lo, hi in ((0, V), (0, text_hi), (17, 18)):
        got = _outs(T)
        ops.score_rows(logits, labels, *got, V=V, vocab_lo=lo, vocab_hi=hi)
        torch.cuda.synchronize()
        _compare(got, R.score_rows(stored[:, :V], labels.cpu().numpy(), lo, hi))
        again = _outs(T)
        ops.score_rows(logits, labels, *again, V=V, vocab_lo=lo, vocab_hi=hi)
        for a, b in zip(got, again):                     # fixed-order reductions: the same bits
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(logits.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_lse_matches_masked_ce_fwd_on_finite_logits(dtype):
    from bdm_db1_amd import ops
    V, ld, T = 33025, 33280, 40
    rng = np.random.default_rng(3)
    logits = torch.from_numpy((rng.standard_normal((T, ld)) * 3).astype(np.float32)).to(DEV).to(dtype)
    labels = torch.from_numpy(rng.integers(0, V, T)).to(DEV)
    got = _outs(T)
    ops.score_rows(logits, labels, *got, V=V)
    lse = torch.empty(T, device=DEV)
    sums = torch.zeros(2, device=DEV)
    mask = torch.ones(T, device=DEV)
    ops.masked_ce_fwd(logits, labels, mask, lse, sums, V)
    err = float((got[0].double() - lse.double()).abs().max())
    print(f"lse vs masked_ce_fwd: {err:.2e}")
    assert err <= TOL


def test_bad_arguments_are_refused_before_launch():
    from bdm_db1_amd import lib, ops
    V, T = 100, 4
    logits = torch.zeros(T, 104, device=DEV)
    labels = torch.zeros(T, dtype=torch.int64, device=DEV)
    o = _outs(T)
    with pytest.raises(ValueError):
        ops.score_rows(logits, labels, *o, V=V, vocab_lo=50, vocab_hi=50)
    with pytest.raises(ValueError):
        ops.score_rows(logits, labels, *o, V=V, vocab_hi=101)
    with pytest.raises(ValueError):
        ops.score_rows(logits[:, :101], labels, *o[:3], o[3].long(), o[4])
    with pytest.raises(ValueError):
        ops.score_rows(torch.zeros(T, 102, device=DEV)[:, :101], labels, *o, V=100)        # rows that are no 16-byte multiple
    with pytest.raises(ValueError):
        ops.score_rows(torch.zeros(T, 40000, device=DEV), labels, *o)                     # longer than a workgroup's registers
    assert not ops.score_rows_supported(40000, 40000, torch.float32) and ops.score_rows_supported(33025, 33280, torch.float32)
    with pytest.raises(ValueError):
        ops.score_segments(o[1], o[3], labels, torch.ones(T, device=DEV), torch.empty(3, 3, device=DEV), V=V)
    L = lib.load()
    assert L.db1_score_rows(0, 0, 0, 0, 0, 0, 0, 4, 100, 104, 0, 0, 100, 0) == -1
    assert L.db1_score_segments(0, 0, 0, 0, 0, 0, 4, 100, 0) == -1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("chunk", [96, 4096])
def test_lmhead_score_equals_gemm_then_score_rows(dtype, chunk):
    from bdm_db1_amd import ops
    V, rows, d, T = 1000, 1024, 256, 200          # T is no multiple of 96; 4096 > T
    rng = np.random.default_rng(7)
    h = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32)).to(DEV).to(dtype)
    W = torch.from_numpy((rng.standard_normal((rows, d)) * 0.3).astype(np.float32)).to(DEV).to(dtype)
    labels = torch.from_numpy(rng.integers(0, V, T)).to(DEV)
    labels[3], labels[100] = -100, 999
    logits = torch.empty(T, rows, device=DEV, dtype=dtype)
    ops.gemm(h, W.t(), logits)
    before = logits.clone()
    for lo, hi in ((0, V), (10, 900)):
        ref = _outs(T)
        ops.score_rows(logits, labels, *ref, V=V, vocab_lo=lo, vocab_hi=hi)
        ops.reserve_workspace(64 << 20)
        for buf in ops._workspace.bufs.values():     # NaN-prefilled workspace (all-ones bytes: a NaN in bf16 and in fp32)
            buf.fill_(0xFF)
        got = _outs(T)
        ops.lmhead_score(h, W, labels, *got, V=V, vocab_lo=lo, vocab_hi=hi, chunk_rows=chunk)
        torch.cuda.synchronize()
        for g, r in zip(got[2:], ref[2:]):
            assert torch.equal(g, r)
        for g, r in zip(got[:2], ref[:2]):
            assert not torch.isnan(g).any()
            inf = torch.isinf(r)
            assert torch.equal(g[inf], r[inf])
            err = float((g[~inf].double() - r[~inf].double()).abs().max())
            print(f"sweep vs materialised: {err:.2e}")
            assert err <= TOL
    assert torch.equal(logits.view(torch.uint8), before.view(torch.uint8))
    _compare(ref, R.score_rows(logits.float().cpu().numpy()[:, :V], labels.cpu().numpy(), 10, 900))


def test_score_segments_against_float64_sums():
    from bdm_db1_amd import ops
    rng = np.random.default_rng(11)
    V = 500
    for n_seg, seg_len in ((5, 1024), (7, 37), (3, 1)):
        n = n_seg * seg_len
        lp = (-rng.random(n) * 12).astype(np.float32)
        rank = rng.integers(-1, 3, n).astype(np.int32)
        labels = rng.integers(0, V, n)
        mask = (rng.random(n) > 0.3).astype(np.float32)
        labels[rng.random(n) < 0.1] = -100
        if seg_len > 1:
            m2, l2 = mask.reshape(n_seg, seg_len), lp.reshape(n_seg, seg_len)
            m2[1, :] = 0.0                                   # a fully masked segment
            l2[1, 0] = -np.inf                               #   ... whose -inf does not count
            m2[2, 3], l2[2, 3] = 1.0, -np.inf                # a counted -inf
            labels.reshape(n_seg, seg_len)[2, 3] = 4
            l2[0, 1], m2[0, 1] = -np.inf, 0.0                # a masked-out -inf: no NaN
        ref = R.score_segments(lp, rank, labels, mask, n_seg, V)
        dev = [torch.from_numpy(a).to(DEV) for a in (lp, rank, labels, mask)]
        out = torch.full((n_seg, 3), float("nan"), device=DEV)
        ops.score_segments(*dev, out, V=V)
        out2 = torch.full((n_seg, 3), float("nan"), device=DEV)
        ops.score_segments(*dev, out2, V=V)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
        got = out.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any()
        inf = np.isinf(ref)
        assert (got[inf] == ref[inf]).all()
        if seg_len > 1:
            assert got[2, 0] == -np.inf and (got[1] == 0).all()
        assert (np.abs(got[~inf] - ref[~inf]) <= 1e-6 * np.abs(ref[~inf])).all()


def test_score_rows_and_sweep_replay_from_a_graph():
    from bdm_db1_amd.decode import graph_capture
    from bdm_db1_amd import ops
    V, rows, d, T = 1000, 1024, 256, 160
    rng = np.random.default_rng(13)
    h = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    W = torch.from_numpy((rng.standard_normal((rows, d)) * 0.3).astype(np.float32)).to(DEV).to(torch.bfloat16)
    labels = torch.from_numpy(rng.integers(0, V, T)).to(DEV)
    logits = torch.empty(T, rows, device=DEV, dtype=torch.bfloat16)
    ops.gemm(h, W.t(), logits)
    eager_rows, eager_sweep = _outs(T), _outs(T)
    ops.score_rows(logits, labels, *eager_rows, V=V, vocab_hi=900)
    ops.lmhead_score(h, W, labels, *eager_sweep, V=V, vocab_hi=900, chunk_rows=64)
    g_rows, g_sweep = _outs(T), _outs(T)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.lmhead_score(h, W, labels, *g_sweep, V=V, vocab_hi=900, chunk_rows=64)      # (warm-up on the side stream: its workspace)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):      # (the cyclic collector held off: bdm_db1_amd.decode.graph_capture)
        ops.score_rows(logits, labels, *g_rows, V=V, vocab_hi=900)
        ops.lmhead_score(h, W, labels, *g_sweep, V=V, vocab_hi=900, chunk_rows=64)
    for o in g_rows + g_sweep:
        o.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager_rows + eager_sweep, g_rows + g_sweep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
