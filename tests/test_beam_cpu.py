"""Beam search without a GPU: the NumPy rule (tests/beam_rule.py) against exhaustive search and against greedy selection, and the
BeamSearchConfig checks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_rule as B  # noqa: E402
import select_rule as S  # noqa: E402


def _table(V, seed):
    """a deterministic next-token table: logits of the token after a prefix (the same prefix always gives the same row)"""
    cache = {}

    def row(prefix):
        key = tuple(int(x) for x in prefix)
        if key not in cache:
            h = np.random.default_rng([seed] + [x + 1 for x in key] + [len(key)])
            cache[key] = (h.standard_normal(V) * 2.0).astype(np.float32)
        return cache[key]
    return row


def _exhaustive(row, V, max_new, eos, alpha):
    """every hypothesis: the sequences that end in EOS before max_new, and the ones that run max_new tokens -> sorted (score, tokens)"""
    hyps = []

    def lp(prefix):
        l = row(prefix).astype(np.float64)
        return l - (l.max() + np.log(np.exp(l - l.max()).sum()))

    def walk(prefix, total):
        n = len(prefix)
        if n == max_new:
            hyps.append((total / max_new ** alpha, tuple(prefix)))
            return
        p = lp(prefix)
        for c in range(V):
            if c == eos:
                hyps.append(((total + p[c]) / (n + 1) ** alpha, tuple(prefix) + (eos,)))
            else:
                walk(prefix + [c], total + p[c])
    walk([], 0.0)
    return sorted(hyps, key=lambda h: -h[0])


@pytest.mark.parametrize("V,max_new,eos,alpha,seed", [(3, 3, 1, 1.0, 0), (4, 2, 0, 0.7, 1), (5, 2, -1, 1.0, 2), (3, 3, 2, 1.5, 3), (2, 3, -1, 1.0, 4)])
def test_rule_equals_exhaustive_search(V, max_new, eos, alpha, seed):
    W = 16
    row = _table(V, seed)
    best = _exhaustive(row, V, max_new, eos, alpha)
    G = 2           # (two identical groups: the groups must not see each other)
    ids, lengths, scores, st = B.search(lambda hist: np.stack([row(h) for h in hist]), G, W, max_new, 0, V, eos=eos, pad=V + 7, alpha=alpha, R=W)
    R = min(W, len(best))
    for g in range(G):
        for r in range(R):
            sc, toks = best[r]
            n = len(toks) - (1 if toks and toks[-1] == eos else 0)
            assert abs(float(scores[g, r]) - sc) < 1e-5 * max(1.0, abs(sc)), (g, r)
            assert int(lengths[g, r]) == n, (g, r)
            assert tuple(ids[g, r, :len(toks)]) == toks and (ids[g, r, len(toks):] == V + 7).all(), (g, r)
        assert (scores[g, :int(st["pool_count"][g])] == np.sort(scores[g, :int(st["pool_count"][g])])[::-1]).all()


@pytest.mark.parametrize("seed", range(4))
def test_one_beam_is_greedy(seed):
    V, max_new = 50, 6
    row = _table(V, seed + 10)
    ids, lengths, scores, _ = B.search(lambda hist: np.stack([row(h) for h in hist]), 1, 1, max_new, 3, 40)
    prefix = []
    for _ in range(max_new):
        prefix.append(int(S.select(row(prefix)[None], 3, 40)[0]))
    assert ids[0, 0].tolist() == prefix and int(lengths[0, 0]) == max_new


def test_rule_details():
    """EOS at rank >= W is dropped, unfilled beams die, a done group writes pad, t outside [0, max_new) sets status bit 1"""
    W, V, pad = 2, 6, 9
    st = B.new_state(1, W, 4, pad)
    l = np.full((W, V), -np.inf, np.float32)
    l[0, :4] = [3.0, 2.0, 1.0, 0.0]              # row 0 only (t = 0): ranks 0..3 = columns 0..3
    s1, _ = B.step(st, l, 0, W, 0, V, eos=2, pad=pad)
    assert s1["next_ids"].tolist() == [0, 1] and s1["pool_count"][0] == 0       # EOS (column 2) at rank 2 >= W: dropped
    s2, _ = B.step(st, l, 0, W, 0, V, eos=0, pad=pad)
    assert s2["pool_count"][0] == 1 and s2["pool_len"][0, 0] == 0 and s2["next_ids"].tolist() == [1, 2]
    assert s2["pool_tokens"][0, 0].tolist() == [0, pad, pad, pad]
    # a row without candidates at t > 0 while the other row lives
    l2 = np.full((W, V), np.nan, np.float32)
    l2[1, 5] = 1.0
    s3, _ = B.step(s1, l2, 1, W, 0, V, pad=pad)
    assert s3["status"][0] & 1 and s3["next_ids"].tolist() == [5, pad] and s3["beam_score"][1] == -np.inf and s3["parent"].tolist() == [1, 1]
    assert s3["tokens"][0, :2].tolist() == [1, 5]
    s4, _ = B.step(s1, l2, 7, W, 0, V, pad=pad)
    assert s4["status"][0] & 2
    s1["done"][0] = 1
    s5, _ = B.step(s1, l, 1, W, 0, V, pad=pad)
    assert s5["next_ids"].tolist() == [pad, pad] and (s5["tokens"] == s1["tokens"]).all()


def test_beam_config_rejects_bad_values():
    from bdm_db1_amd.generation import BeamSearchConfig
    BeamSearchConfig()
    for kw in (dict(num_beams=0), dict(num_beams=17), dict(max_new_tokens=0), dict(length_penalty=float("nan")),
               dict(length_penalty=float("inf")), dict(num_return_sequences=0), dict(num_beams=2, num_return_sequences=3),
               dict(vocab_lo=-1), dict(vocab_lo=5, vocab_hi=5), dict(sync_every=0), dict(eos_id=-2)):
        with pytest.raises(ValueError):
            BeamSearchConfig(**kw)
    assert BeamSearchConfig(num_beams=16, num_return_sequences=16, length_penalty=-0.5).num_beams == 16
