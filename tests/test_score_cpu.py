"""Scoring without a GPU: ScoreConfig's argument checks, the NumPy rule (tests/score_rule.py) against a float64 restatement written a second
way, and the new C prototypes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_rule as R  # noqa: E402


@pytest.mark.parametrize("kw", [dict(vocab_lo=-1), dict(vocab_lo=5, vocab_hi=5), dict(vocab_lo=9, vocab_hi=3), dict(length_penalty=float("nan")),
                                dict(length_penalty=float("inf")), dict(chunk_rows=0), dict(chunk_rows=-4)])
def test_score_config_rejects_bad_values(kw):
    from bdm_db1_amd import ScoreConfig
    with pytest.raises(ValueError):
        ScoreConfig(**kw)


def test_score_config_defaults_and_exports():
    import bdm_db1_amd as pkg
    c = pkg.ScoreConfig()
    assert (c.vocab_lo, c.vocab_hi, c.length_penalty, c.chunk_rows, c.return_tokens) == (0, None, 0.0, None, True)
    assert pkg.ScoreConfig(vocab_lo=3, vocab_hi=9, length_penalty=-0.5, chunk_rows=1).chunk_rows == 1
    for name in ("score", "validation_report", "rank_candidates", "rank_captions", "rank_answers", "ScoreResult"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None


def _second_way(l, y, lo, hi):
    """float64, sort-based rank, np.logaddexp.reduce"""
    l64 = np.asarray(l, np.float64)
    V = l64.size
    idx = [c for c in range(lo, hi) if np.isfinite(l64[c])]
    if idx:
        vals = l64[idx]
        lse = np.logaddexp.reduce(vals)
        order = sorted(idx, key=lambda c: (-l64[c], c))
        top1 = order[0]
    else:
        lse, top1 = -np.inf, -1
    st = 0 if idx else 2
    if not 0 <= y < V:
        return lse, 0.0, top1, -1, st
    if y not in idx:
        return lse, -np.inf, top1, -1, st | 1
    srt = np.sort(l64[idx])
    rank = len(srt) - int(np.searchsorted(srt, l64[y], side="right"))
    return lse, l64[y] - lse, top1, rank, st


def _check(l, y, lo, hi):
    a, b = R.score_row(l, y, lo, hi), _second_way(l, y, lo, hi)
    assert a[2:] == b[2:], (a, b)
    for u, v in zip(a[:2], b[:2]):
        assert (u == v) or abs(float(u) - v) <= 1e-5, (a, b)
    assert not np.isnan(a[0]) and not np.isnan(a[1])


def test_rule_matches_the_float64_restatement():
    rng = np.random.default_rng(0)
    V = 777
    for i in range(40):
        l = (rng.standard_normal(V) * 4).astype(np.float32)
        lo, hi = [(0, V), (100, 300), (5, 6)][i % 3]
        _check(l, int(rng.integers(0, V)), lo, hi)
        _check(l, int(rng.integers(lo, hi)), lo, hi)
    # ties at the top; a label that ties with a larger column
    l = (rng.standard_normal(V)).astype(np.float32)
    l[40] = l[600] = 9.0
    for y in (40, 600, 3):
        _check(l, y, 0, V)
    assert R.score_row(l, 600, 0, V)[2:4] == (40, 0)
    assert R.score_row(l, 600, 41, V)[2:4] == (600, 0)
    # NaN / +-inf are never candidates, also as labels
    l[7], l[8], l[9] = np.nan, np.inf, -np.inf
    for y in (7, 8, 9, 40, 10):
        _check(l, y, 0, V)
    assert R.score_row(l, 8, 0, V)[1] == -np.inf and R.score_row(l, 8, 0, V)[3:] == (-1, 1)
    # labels outside the window; ignored labels
    _check(l, 3, 100, 200)
    assert R.score_row(l, 3, 100, 200)[3:] == (-1, 1)
    for y in (-100, -1, V, V + 5):
        _check(l, y, 0, V)
        assert R.score_row(l, y, 0, V)[1] == 0.0 and R.score_row(l, y, 0, V)[3:] == (-1, 0)
    # an empty candidate set
    e = np.full(V, np.nan, np.float32)
    e[0] = 1.0
    _check(e, 5, 1, V)
    assert R.score_row(e, 5, 1, V) == (-np.inf, -np.inf, -1, -1, 3)
    assert R.score_row(e, -100, 1, V) == (-np.inf, 0.0, -1, -1, 2)


def test_segment_rule():
    lp = np.array([-1.0, -2.0, -np.inf, -3.0, -np.inf, -4.0], np.float32)
    rank = np.array([0, 3, -1, 0, -1, 0], np.int32)
    labels = np.array([1, 2, 3, -100, 4, 5])
    mask = np.array([1, 1, 0, 1, 1, 1], np.float32)
    out = R.score_segments(lp, rank, labels, mask, 2, 10)
    assert out[0].tolist() == [-3.0, 2.0, 1.0]
    assert out[1, 0] == -np.inf and out[1, 1:].tolist() == [2.0, 1.0] and not np.isnan(out).any()
    s, order = R.candidate_scores(np.array([[[-1.0, -1.0], [-1.0, -3.0], [-2.0, 0.0]]]), np.array([[2, 1, 1]]), 0.0)
    assert s.tolist() == [[-2.0, -1.0, -2.0]] and order.tolist() == [[1, 0, 2]]


def test_prototypes_are_declared():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for n in ("db1_score_rows_supported", "db1_score_rows", "db1_lmhead_score_workspace_bytes", "db1_lmhead_score", "db1_score_segments"):
        assert n in names
    protos = lib.parse_header()
    assert len(protos["db1_score_rows"][1]) == 14 and len(protos["db1_lmhead_score"][1]) == 19 and len(protos["db1_score_segments"][1]) == 9

