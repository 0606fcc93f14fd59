"""What the GPU tests of db1_beam_step and db1_beam_step_diverse share: the state's way to the device and back, one launch of either step, and
the comparison with the NumPy rule (tests/beam_rule.py).  A plain module, imported like gpu_common."""
import numpy as np
import torch

DEV = "cuda"
DEV_KEYS = ("beam_score", "parent", "tokens", "pool_tokens", "pool_len", "pool_score", "pool_slot", "pool_count", "done", "switches", "status")
ALL_KEYS = DEV_KEYS + ("next_ids",)


def _upload(S):
    return {k: torch.from_numpy(np.ascontiguousarray(S[k])).to(DEV) for k in DEV_KEYS}


def _download(Dv, ids):
    S = {k: v.cpu().numpy() for k, v in Dv.items()}
    S["next_ids"] = ids[:, 0].cpu().numpy().astype(np.int64)
    return S


def _launch(S, logits, t, Wp, D, lam, lo, hi, eos, pad, alpha, V, plain=False):
    """one launch from the state ``S``: db1_beam_step_diverse, or (``plain``) db1_beam_step over the G * D sub-groups as groups"""
    from bdm_db1_amd import ops
    Dv = _upload(S)
    ids = torch.full((logits.shape[0], 2), -5, dtype=torch.long, device=DEV)     # (column 0 of [M, 2]: the row stride is 2)
    tt = torch.tensor([t], dtype=torch.int32, device=DEV)
    args = (logits, tt, Dv["beam_score"], Dv["parent"], Dv["tokens"], Dv["pool_tokens"], Dv["pool_len"], Dv["pool_score"], Dv["pool_slot"],
            Dv["pool_count"], Dv["done"], Dv["switches"], ids[:, 0], Dv["status"])
    kw = dict(W=Wp, V=V, vocab_lo=lo, vocab_hi=hi, eos_id=eos, pad_id=pad, length_penalty=alpha)
    if plain:
        ops.beam_step(*args, **kw)
    else:
        ops.beam_step_diverse(*args, D=D, diversity_penalty=lam, **kw)
    torch.cuda.synchronize()
    assert (ids[:, 1] == -5).all()
    return _download(Dv, ids)


def _close(a, b, rtol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same_inf = (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b)))
    return bool(np.all(same_inf | (np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))))


def _compare(got, want, amb, Wp, D, t):
    """(sub-)group by (sub-)group; the status always.  An ambiguous sub-group may have fed other tokens to the later sub-groups of its
    prompt, so those are compared by status alone as well (D = 1, the plain step: the ambiguous group alone)"""
    Q = len(want["done"])
    for q in range(Q):
        rows = slice(q * Wp, (q + 1) * Wp)
        assert got["status"][q] == want["status"][q], q
        if amb[(q // D) * D:q + 1].any():
            continue
        assert got["done"][q] == want["done"][q], (q, t)
        assert (got["parent"][rows] == want["parent"][rows]).all(), (q, t)
        assert (got["next_ids"][rows] == want["next_ids"][rows]).all(), (q, t)
        assert (got["tokens"][rows, :t + 1] == want["tokens"][rows, :t + 1]).all(), (q, t)
        assert _close(got["beam_score"][rows], want["beam_score"][rows]), (q, t)
        assert got["switches"][q] == want["switches"][q], (q, t)
        n = int(want["pool_count"][q])
        assert got["pool_count"][q] == n, (q, t)
        assert (got["pool_len"][q, :n] == want["pool_len"][q, :n]).all(), (q, t)
        assert _close(got["pool_score"][q, :n], want["pool_score"][q, :n]), (q, t)
        gt = got["pool_tokens"][q, got["pool_slot"][q, :n]]
        wt = want["pool_tokens"][q, want["pool_slot"][q, :n]]
        assert (gt == wt).all(), (q, t)


def _bits_equal(a, b):
    for k in ALL_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
