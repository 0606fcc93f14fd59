"""db1_select_tokens (on-device next-token selection) against the NumPy restatement of its rule in tests/select_rule.py: greedy bit for bit,
sampling token for token up to near ties, the sampled distribution against the filtered softmax, and the EOS / finished / lengths state."""
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

import select_rule as R  # noqa: E402
from gpu_common import _need_gpu  # noqa: E402,F401


class State:
    def __init__(self, M, max_new=8, q=1):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.t = torch.zeros(1, **i32)
        self.finished = torch.zeros(M, **i32)
        self.lengths = torch.zeros(M, **i32)
        self.status = torch.zeros(M, **i32)
        self.out = torch.full((M, max_new), -7, **i32)
        self.ids = torch.full((M, q), -9, dtype=torch.long, device=DEV)

    def call(self, logits, **kw):
        from bdm_db1_amd import ops
        ops.select_tokens(logits, self.t, self.finished, self.lengths, self.out, self.ids[:, 0], self.status, **kw)
        return self.ids[:, 0].cpu().numpy()


def _logits(rng, M, V, ld, dtype, scale=3.0):
    x = np.full((M, ld), 1e4, np.float32)          # padding columns: huge, so picking one is caught
    x[:, :V] = rng.standard_normal((M, V)).astype(np.float32) * scale
    t = torch.from_numpy(x).to(DEV).to(dtype)
    return t, t.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,V", [(1, 7), (5, 1000), (64, 33025), (5, 33025)])
def test_greedy_matches_the_rule(dtype, M, V):
    rng = np.random.default_rng(V + M)
    ld = V + (64 - V % 64) + 64
    lg, x = _logits(rng, M, V, ld, dtype)
    x = x[:, :V]
    # planted ties of the maximum (lowest column must win), -inf and NaN entries
    for r in range(M):
        c = rng.choice(V, size=min(3, V), replace=False)
        top = x[r].max() + 1.0
        x[r, c] = top
        lg[r, c] = top
        if V > 4:
            lg[r, int(c.min()) - 1 if c.min() > 0 else V - 1] = float("nan")
            lg[r, (int(c.max()) + 2) % V] = float("-inf")
    x = lg.float().cpu().numpy().astype(np.float64)[:, :V]
    for lo, hi in [(0, V), (0, max(1, V // 2)), (V // 3, V - V // 5 if V > 5 else V)]:
        s = State(M)
        got = s.call(lg, V=V, vocab_lo=lo, vocab_hi=hi)
        ref = R.select(x, lo, hi)
        assert (got == ref).all(), (lo, hi, np.nonzero(got != ref))
        assert (s.out[:, 0].cpu().numpy() == ref).all() and (s.status.cpu().numpy() == 0).all()
        assert (s.lengths.cpu().numpy() == 1).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_with_nothing_finite_sets_the_status_bit(dtype):
    lg = torch.randn(3, 100, device=DEV).to(dtype)
    lg[1, 10:20] = float("-inf")
    lg[1, 15] = float("nan")
    s = State(3)
    got = s.call(lg, vocab_lo=10, vocab_hi=20, pad_id=5, greedy=False, top_p=0.5)
    st, fin = s.status.cpu().numpy(), s.finished.cpu().numpy()
    assert got[1] == 5 and st[1] & 1 and fin[1] == 1 and s.lengths[1].item() == 0
    assert st[0] == 0 and st[2] == 0 and fin[0] == 0 and fin[2] == 0 and 10 <= got[0] < 20 and 10 <= got[2] < 20


GRID = [(1.0, 0, 1.0), (0.7, 0, 0.9), (1.3, 50, 1.0), (1.0, 40, 0.8), (0.5, 0, 0.5), (2.0, 1000, 0.95), (1.0, 3, 1.0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [1000, 33025])
def test_sampling_matches_the_rule(dtype, V):
    rng = np.random.default_rng(7)
    M, draws, mism = 64, 0, 0
    lg, x = _logits(rng, M, V, V + 63, dtype)
    x = x[:, :V]
    sids = torch.from_numpy(rng.integers(0, 2 ** 31, M).astype(np.int32)).to(DEV)
    sid_h = sids.cpu().numpy()
    for T, k, p in GRID:
        for step in range(3):
            s = State(M)
            seed = 0x1234_5678_9ABC + step
            got = s.call(lg, V=V, vocab_lo=2, vocab_hi=V - 1, greedy=False, temperature=T, top_k=k, top_p=p, seed=seed, step_base=step * 11,
                         stream_id=sids)
            for r in range(M):
                tok, sc = R.select_row(x[r], 2, V - 1, False, T, k, p, seed, int(sid_h[r]), step * 11)
                draws += 1
                kept, cum, above = R.kept_set(x[r], 2, V - 1, T, k, p)
                g = int(got[r])
                assert 2 <= g < V - 1 and np.isfinite(x[r, g])
                if not kept[g]:   # only a token at the top-p boundary (the mass above it within 1e-5 of top_p) may slip in
                    assert k == 0 or x[r, g] >= np.sort(x[r, 2:V - 1])[::-1][k - 1], (T, k, p, r)
                    assert abs(above[g] - p) < 1e-5, (T, k, p, r, above[g])
                if g != tok:
                    mism += 1
                    u = R.uniforms(V, int(sid_h[r]), step * 11, seed)
                    sg = x[r, g] / T - np.log(-np.log(u[g]))
                    scale = np.abs(x[r, 2:V - 1]).max() / T + 20.0
                    assert not kept[g] or sc[tok] - sg < 1e-5 * scale, (T, k, p, r, g, tok, sc[tok] - sg)
    assert mism <= 0.001 * draws, (mism, draws)


def test_sampled_distribution_matches_the_filtered_softmax():
    from scipy.stats import chisquare
    V, M = 500, 1000
    base = np.full(V, -4.0)
    base[[3, 17, 100, 101, 250, 499]] = [2.0, 1.5, 1.0, 1.0, 0.2, -0.5]
    T, k, p = 0.8, 5, 0.97
    kept = R.kept_set(base, 0, V, T, k, p)[0]
    e = np.where(kept, np.exp((base - base.max()) / T), 0.0)
    prob = e / e.sum()
    lg = torch.from_numpy(np.tile(base, (M, 1)).astype(np.float32)).to(DEV)
    sids = torch.arange(M, dtype=torch.int32, device=DEV)
    counts = np.zeros(V)
    for step in range(20):
        s = State(M)
        got = s.call(lg, greedy=False, temperature=T, top_k=k, top_p=p, seed=99, step_base=step, stream_id=sids)
        counts += np.bincount(got, minlength=V)
    assert counts[~kept].sum() == 0
    idx = np.nonzero(kept)[0]
    _, pv = chisquare(counts[idx], prob[idx] * counts.sum())
    assert pv > 1e-3, (pv, counts[idx], prob[idx] * counts.sum())


def test_top_k_1_is_greedy_and_calls_are_deterministic():
    rng = np.random.default_rng(3)
    lg, x = _logits(rng, 16, 33025, 33088, torch.bfloat16)
    g = State(16).call(lg, V=33025)
    assert (State(16).call(lg, V=33025, greedy=False, top_k=1, temperature=0.7, seed=4) == g).all()
    a = State(16).call(lg, V=33025, greedy=False, top_p=0.9, seed=4)
    b = State(16).call(lg, V=33025, greedy=False, top_p=0.9, seed=4)
    c = State(16).call(lg, V=33025, greedy=False, top_p=0.9, seed=5)
    assert (a == b).all() and (a != c).any()


def test_rows_are_independent_of_the_batch():
    rng = np.random.default_rng(4)
    lg, _ = _logits(rng, 8, 5000, 5000, torch.float32, scale=1.0)
    sids = torch.arange(100, 108, dtype=torch.int32, device=DEV)
    full = State(8).call(lg, greedy=False, top_p=0.95, seed=11, stream_id=sids)
    for r in (0, 3, 7):
        one = State(1).call(lg[r:r + 1], greedy=False, top_p=0.95, seed=11, stream_id=sids[r:r + 1].contiguous())
        assert one[0] == full[r]


def test_eos_finished_pad_lengths_and_next_ids():
    """a scripted logits sequence: row 0 picks EOS at t = 2, row 1 at t = 0, row 2 never; tokens go to out[:, t] and to a column of [M, q]"""
    M, V, eos, pad, n = 3, 50, 7, 1, 5
    s = State(M, max_new=n, q=3)
    script = [[10, eos, 12], [11, 3, 13], [eos, 4, 14], [12, 5, 15], [13, 6, 16]]
    from bdm_db1_amd import ops
    for t in range(n):
        lg = torch.zeros(M, V, device=DEV)
        for r in range(M):
            lg[r, script[t][r]] = 5.0
        ops.select_tokens(lg, s.t, s.finished, s.lengths, s.out, s.ids[:, 2], s.status, eos_id=eos, pad_id=pad)
        assert s.ids[:, 2].tolist() == [script[t][0] if t <= 2 else pad, script[t][1] if t == 0 else pad, script[t][2]]
        s.t.add_(1)
    assert s.out.cpu().numpy().tolist() == [[10, 11, eos, pad, pad], [eos, pad, pad, pad, pad], [12, 13, 14, 15, 16]]
    assert s.lengths.tolist() == [2, 0, 5] and s.finished.tolist() == [1, 1, 0] and s.status.tolist() == [0, 0, 0]
    assert (s.ids[:, :2] == -9).all()


def test_graph_captured_call_equals_the_eager_call():
    from bdm_db1_amd.decode import graph_capture
    rng = np.random.default_rng(5)
    lg, _ = _logits(rng, 64, 33025, 33088, torch.bfloat16)
    eager = State(64, max_new=4)
    ref = []
    for _ in range(4):
        ref.append(eager.call(lg, V=33025, greedy=False, top_p=0.9, top_k=200, seed=8))
        eager.t.add_(1)
    gs = State(64, max_new=4)
    from bdm_db1_amd import ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the capture
        ops.select_tokens(lg, gs.t, gs.finished, gs.lengths, gs.out, gs.ids[:, 0], gs.status, V=33025, greedy=False, top_p=0.9, top_k=200, seed=8)
    torch.cuda.current_stream().wait_stream(side)
    gs.lengths.zero_()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):      # (the cyclic collector held off: bdm_db1_amd.decode.graph_capture)
        ops.select_tokens(lg, gs.t, gs.finished, gs.lengths, gs.out, gs.ids[:, 0], gs.status, V=33025, greedy=False, top_p=0.9, top_k=200, seed=8)
        gs.t.add_(1)
    for i in range(4):
        graph.replay()
        assert (gs.ids[:, 0].cpu().numpy() == ref[i]).all()
    assert torch.equal(gs.out, eager.out) and torch.equal(gs.lengths, eager.lengths)


def test_invalid_arguments():
    from bdm_db1_amd import lib, ops
    s = State(2)
    lg = torch.randn(2, 100, device=DEV)
    for kw in (dict(vocab_lo=50, vocab_hi=50), dict(vocab_lo=0, vocab_hi=101), dict(greedy=False, temperature=0.0),
               dict(greedy=False, top_p=0.0), dict(greedy=False, top_p=1.5), dict(greedy=False, top_k=-1)):
        with pytest.raises(ValueError):
            s.call(lg, **kw)
    with pytest.raises(ValueError):
        s.call(lg.half())
    with pytest.raises(ValueError):
        s.call(torch.randn(2, 40000, device=DEV))
    L = lib.load()
    P = lambda x: x.data_ptr()
    args = lambda V, lo, hi, T, dt: (P(lg), 2, V, 100, dt, lo, hi, T, 0, 1.0, 0, 0, 0, -1, 0, 0, P(s.t), None, P(s.finished), P(s.lengths),
                                     P(s.out), s.out.shape[1], P(s.ids), 1, P(s.status), None, 0, None)
    assert L.db1_select_tokens(*args(100, 10, 5, 1.0, 0)) == ops.DB1_ERR_BAD_SHAPE
    assert L.db1_select_tokens(*args(100, 0, 100, 0.0, 0)) == ops.DB1_ERR_BAD_SHAPE
    assert L.db1_select_tokens(*args(100, 0, 100, 1.0, 7)) == ops.DB1_ERR_UNSUPPORTED_DTYPE
    assert L.db1_select_tokens(*args(40000, 0, 100, 1.0, 0)) in (ops.DB1_ERR_BAD_SHAPE, ops.DB1_ERR_UNSUPPORTED)
    assert L.db1_select_tokens_workspace_bytes(64, 33025, 1) == 0
    assert L.db1_select_tokens_supported(33025, 33088, 1) and not L.db1_select_tokens_supported(40000, 40000, 1)
    torch.cuda.synchronize()
