"""db1_beam_step against the NumPy rule (tests/beam_rule.py) step by step, and db1_ring_reorder against a torch gather, bit for bit."""
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

import beam_rule as B  # noqa: E402
from beam_kernel_common import _bits_equal, _compare, _launch, _upload  # noqa: E402
from gpu_common import _need_gpu  # noqa: E402,F401


def _logits(rng, M, V, W, t, eos, case):
    l = rng.standard_normal((M, V)).astype(np.float32) * 3.0
    l[:, 7] = l[:, 8]                                     # planted ties (same row, same logit)
    l[:, 11] = np.nan
    l[:, 12] = np.inf
    l[:, 13] = -np.inf
    l[0, 20:40] = l[0, 20]
    if M >= 2:
        l[1] = l[0] if t == 0 else l[1]
    G = M // W
    for g in range(G):
        r = slice(g * W, (g + 1) * W)
        if g % 3 == 0:
            l[r, eos] = l[r].max(axis=1) + 1.0            # EOS at rank 0 of its rows
        elif g % 3 == 1:
            srt = np.sort(np.where(np.isfinite(l[r]), l[r], -np.inf), axis=1)
            l[r, eos] = srt[:, -(W + 2)] - 1e-3            # EOS a little below the row's top W + 1
    if case == "norow" and M > 1:
        l[M - 1, :] = np.nan                              # a row without a candidate
    return l


@pytest.mark.parametrize("V", [200, 33025])
@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("W", [1, 2, 4, 16])
def test_beam_step_follows_the_rule(W, G, V):
    M = G * W
    dt = torch.bfloat16 if (W + G) % 2 else torch.float32
    lo, hi = (3, 190) if V == 200 else (0, 32000)
    eos, pad, alpha, mx = 5, hi - 1, 0.8, 5
    rng = np.random.default_rng(W * 1000 + G * 10 + (V > 1000))
    S = B.new_state(G, W, mx, pad)
    n_amb = n_groups = 0
    for t in range(mx):
        if t == 2 and G >= 3:
            S["done"][1] = 1                               # an already-done group
        l = _logits(rng, M, V, W, t, eos, "norow" if t == 3 else "")
        lt = torch.from_numpy(l).to(DEV).to(dt)
        lw = lt.float().cpu().numpy()                      # (bf16: the widened values the kernel sees)
        want, amb = B.step(S, lw, t, W, lo, hi, eos, pad, alpha)
        got = _launch(S, lt, t, W, 1, 0.0, lo, hi, eos, pad, alpha, V, plain=True)
        _compare(got, want, amb, W, 1, t)
        if t == 1:      # the same inputs give the same bits
            _bits_equal(got, _launch(S, lt, t, W, 1, 0.0, lo, hi, eos, pad, alpha, V, plain=True))
        n_amb += int(amb.sum())
        n_groups += G
        S = got                                            # the next step starts from the device's state
    assert n_amb <= n_groups // 4


def test_beam_step_counter_out_of_range_and_bad_arguments():
    from bdm_db1_amd import ops
    W, G, V, mx = 2, 2, 300, 4
    S = B.new_state(G, W, mx, 0)
    l = torch.randn(G * W, V, device=DEV)
    got = _launch(S, l, mx, W, 1, 0.0, 0, V, -1, 7, 1.0, V, plain=True)
    assert (got["status"] & 2).all() and (got["next_ids"] == 7).all() and (got["pool_count"] == 0).all()
    D = _upload(S)
    ids = torch.zeros(G * W, dtype=torch.long, device=DEV)
    tt = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = [tt, D["beam_score"], D["parent"], D["tokens"], D["pool_tokens"], D["pool_len"], D["pool_score"], D["pool_slot"], D["pool_count"],
            D["done"], D["switches"], ids, D["status"]]
    for bad in (dict(W=3), dict(W=17), dict(W=2, vocab_lo=5, vocab_hi=5), dict(W=2, vocab_hi=V + 1), dict(W=2, length_penalty=float("inf"))):
        with pytest.raises(ValueError):
            ops.beam_step(l, *args, **bad)
    wrong = list(args)
    wrong[4] = D["pool_tokens"][:, :, :2]
    with pytest.raises(ValueError):
        ops.beam_step(l, *wrong, W=W)
    with pytest.raises(ValueError):
        ops.beam_step(l.double(), *args, W=W)


def _reorder_case(M, W, cap, mlen, s0, t, max_t, parent, done, L=3, H=2, D=128):
    from bdm_db1_amd import ops
    g = torch.Generator().manual_seed(M * 7 + t)
    rings = [torch.randint(-32768, 32767, (M, cap, 2, H, D), generator=g, dtype=torch.int16).to(DEV).view(torch.bfloat16) for _ in range(L)]
    ref = [r.view(torch.int16).clone() for r in rings]
    par = torch.tensor(parent, dtype=torch.int32)
    dn = None if done is None else torch.tensor(done, dtype=torch.int32)
    if 1 <= t <= max_t:      # (the expected rows are read from the ORIGINAL rings, never from rows already rewritten)
        slots = torch.tensor([(s0 + mlen - t + i) % cap for i in range(t)], device=DEV)
        for b in range(M):
            if int(par[b]) != b and (dn is None or not int(dn[b // W])):
                for x, r in zip(ref, rings):
                    x[b, slots] = r.view(torch.int16)[int(par[b])][slots]
    ptrs = ops.ring_pointers(rings)
    state = torch.tensor([s0], dtype=torch.int32, device=DEV)
    tt = torch.tensor([t], dtype=torch.int32, device=DEV)
    ops.ring_reorder(rings, ptrs, state, mlen, tt, max_t, par.to(DEV), W=W, done=None if dn is None else dn.to(DEV))
    torch.cuda.synchronize()
    for x, r in zip(ref, rings):
        assert torch.equal(x, r.view(torch.int16))


@pytest.mark.parametrize("name,W,parent_fn,t,s0,done", [
    ("t0_noop", 4, lambda M, W: [(b // W) * W for b in range(M)], 0, 3, None),
    ("identity", 4, lambda M, W: list(range(M)), 7, 3, None),
    ("swaps", 4, lambda M, W: [b ^ 1 for b in range(M)], 7, 3, None),
    ("all_from_one", 4, lambda M, W: [(b // W) * W + 2 for b in range(M)], 9, 3, None),
    ("wrap", 4, lambda M, W: [(b // W) * W + (b + 1) % W for b in range(M)], 12, 80, None),
    ("done_groups", 4, lambda M, W: [(b // W) * W + (b + 3) % W for b in range(M)], 5, 50, [1, 0, 1]),
    ("w16", 16, lambda M, W: [(b * 5) % W for b in range(M)], 10, 83, None),
])
def test_ring_reorder_matches_a_gather(name, W, parent_fn, t, s0, done):
    G = 3 if W < 16 else 1
    M, mlen = G * W, 20
    _reorder_case(M, W, mlen + 64, mlen, s0, t, 12, parent_fn(M, W), done)


def test_ring_reorder_bad_arguments():
    from bdm_db1_amd import ops
    rings = [torch.zeros(4, 30, 2, 2, 128, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    ptrs = ops.ring_pointers(rings)
    i1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    par = torch.arange(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.ring_reorder(rings, ptrs, i1, 20, i1, 21, par, W=2)          # max_t > mlen
    with pytest.raises(ValueError):
        ops.ring_reorder(rings, ptrs, i1, 30, i1, 5, par, W=2)           # mlen >= cap
    with pytest.raises(ValueError):
        ops.ring_reorder(rings, ptrs, i1, 20, i1, 5, par, W=3)           # W does not divide M
    with pytest.raises(ValueError):
        ops.ring_reorder(rings, ptrs[:1], i1, 20, i1, 5, par, W=2)
    with pytest.raises(ValueError):
        ops.ring_reorder(rings, ptrs, i1, 20, i1, 5, par[:3], W=2)
