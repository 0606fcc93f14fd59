"""The log-prob rule (tests/logprob_rule.py) against a second formulation, the best-of-n ranking, the ``logprobs`` field of the config, the
prototypes of the two ``_lp`` entry points and ``sample_best_of``'s argument checks.  No GPU."""
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logprob_rule as L  # noqa: E402


def test_the_rule_agrees_with_logaddexp():
    rng = np.random.default_rng(0)
    V, lo, hi = 300, 7, 280
    for trial in range(20):
        l = rng.standard_normal(V) * 3
        l[rng.integers(0, V, 12)] = rng.choice([np.nan, np.inf, -np.inf], 12)
        l[:lo] = 50.0                                       # (outside the window: must not count)
        l[hi:] = 50.0
        w = l[lo:hi]
        want = np.logaddexp.reduce(w[np.isfinite(w)])
        assert abs(L.lse(l, lo, hi) - want) < 1e-12
        tok = lo + int(np.nanargmax(np.where(np.isfinite(w), w, np.nan)))
        assert abs(L.logprob(l, tok, lo, hi) - (l[tok] - want)) < 1e-12
    # the probabilities of the candidates sum to one; a two-candidate row by hand
    l = np.array([9.0, 0.0, np.log(3.0), np.nan, 9.0])
    assert abs(L.logprob(l, 1, 1, 4) - np.log(0.25)) < 1e-12 and abs(L.logprob(l, 2, 1, 4) - np.log(0.75)) < 1e-12
    assert L.lse(np.array([np.nan, -np.inf, 1.0]), 0, 2) == -np.inf


def test_bookkeeping_of_a_launch():
    V, mx = 6, 3
    lg = np.array([[0.0, 1.0, 2.0, 0.0, 0.0, 0.0],       # picks 2
                   [5.0, 0.0, 0.0, 0.0, 0.0, 0.0],       # finished on entry
                   [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan],   # no candidate
                   [0.0, 0.0, 0.0, 0.0, 0.0, 3.0]])      # picks 5
    fin = np.array([False, True, False, False])
    lps = np.full((4, mx), np.nan)
    sums = np.full(4, 10.0)
    toks = L.step(lg, 1, mx, fin, lps, sums, 0, V)
    assert toks.tolist() == [2, -2, -1, 5]
    assert lps[0, 1] == L.logprob(lg[0], 2, 0, V) and sums[0] == 10.0 + lps[0, 1]
    assert lps[1, 1] == 0.0 and sums[1] == 10.0                       # finished: wrote 0, sum untouched
    assert lps[2, 1] == 0.0 and sums[2] == 10.0 and fin[2]            # no candidate: wrote 0, sum untouched
    assert np.isnan(lps[:, [0, 2]]).all()                             # the other columns are not the launch's
    # t out of range: nothing is written
    lps2, sums2 = np.full((4, mx), np.nan), np.full(4, 10.0)
    L.step(lg, mx, mx, np.array([False, True, False, False]), lps2, sums2, 0, V)
    assert np.isnan(lps2).all() and (sums2 == 10.0).all()
    # a given token is scored instead of the rule's own choice
    lps3, sums3 = np.zeros((4, mx)), np.zeros(4)
    L.step(lg, 0, mx, np.zeros(4, bool), lps3, sums3, 0, V, tokens=[1, 0, 0, 0])
    assert lps3[0, 0] == L.logprob(lg[0], 1, 0, V)


def test_best_of_ranking_ties_eos_and_no_candidate_rows():
    sums = np.array([[-6.0, -4.0, -4.0, -1.0], [-3.0, -3.0, -8.0, -2.0]])
    lengths = np.array([[3, 2, 1, 5], [3, 2, 4, 1]])
    ended = np.array([[False, False, True, False], [False, True, False, False]])
    nocand = np.array([[False, False, False, True], [False, False, False, False]])
    sc = L.best_of_scores(sums, lengths, ended, nocand, 1.0)
    assert sc[0].tolist() == [-2.0, -2.0, -2.0, -np.inf]              # EOS counts: -4 / (1 + 1); the no-candidate row is last
    assert sc[1].tolist() == [-1.0, -1.0, -2.0, -2.0]                 # -3 / (2 + 1)
    assert L.best_of_order(sc, 4) == [[0, 1, 2, 3], [0, 1, 2, 3]]     # ties: the lower j first
    assert L.best_of_order(sc, 2) == [[0, 1], [0, 1]]
    sc0 = L.best_of_scores(sums, lengths, ended, nocand, 0.0)         # no normalisation: the sums themselves
    assert sc0[1].tolist() == [-3.0, -3.0, -8.0, -2.0] and L.best_of_order(sc0, 2)[1] == [3, 0]
    # the package's ranking is the rule's
    from bdm_db1_amd import generation as G
    for pen in (0.0, 0.7, 1.0, 2.0):
        want = L.best_of_scores(sums, lengths, ended, nocand, pen)
        got = G.best_of_scores(sums, lengths, ended, nocand, pen)
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-6, atol=0) and (np.isinf(got) == np.isinf(want)).all()
        assert G.best_of_order(got, 3).tolist() == L.best_of_order(got, 3)


def test_logprobs_is_part_of_the_config_key():
    from bdm_db1_amd import GenerationConfig
    a, b = GenerationConfig(), GenerationConfig(logprobs=True)
    assert a.logprobs is False and a != b and hash(a) != hash(b)
    assert dataclasses.fields(GenerationConfig)[-1].name == "logprobs"
    assert (2, a, 100, 90) != (2, b, 100, 90)                         # (the generator's cache key holds the config)
    assert dataclasses.replace(b, logprobs=False) == a


def test_lp_prototypes_extend_their_parents_by_two_pointers():
    import ctypes
    from bdm_db1_amd import lib
    protos = lib.parse_header()
    for name in ("db1_select_tokens", "db1_select_tokens_slots"):
        ret, args = protos[name]
        ret_lp, args_lp = protos[name + "_lp"]
        assert ret_lp is ret and len(args_lp) == len(args) + 2
        assert args_lp[:-5] == args[:-3] and args_lp[-3:] == args[-3:]              # (the tail: ws, ws_bytes, stream)
        assert args_lp[-5:-3] == [ctypes.c_void_p, ctypes.c_void_p]
    assert "db1_select_tokens_lp_supported" not in protos and "db1_select_tokens_lp_workspace_bytes" not in protos


def test_sample_best_of_refuses_bad_arguments_before_touching_the_model():
    import bdm_db1_amd as pkg
    from bdm_db1_amd import BeamSearchConfig, GenerationConfig, sample_best_of
    assert "sample_best_of" in pkg.__all__
    cfg = GenerationConfig(greedy=False, top_p=0.9)
    with pytest.raises(ValueError):
        sample_best_of(None, None, GenerationConfig(), 4)                           # greedy
    for n, R in ((0, 1), (65, 1), (4, 5), (4, 0), (True, 1)):
        with pytest.raises(ValueError):
            sample_best_of(None, None, cfg, n, num_return_sequences=R)
    with pytest.raises(ValueError):
        sample_best_of(None, None, cfg, 4, length_penalty=float("inf"))
    with pytest.raises(TypeError):
        sample_best_of(None, None, BeamSearchConfig(), 4)


def test_ops_wrappers_take_both_logprob_buffers_or_neither():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd import ops
    dev = torch.device("cpu")
    lp, s = torch.zeros(3, 8), torch.zeros(3)
    assert ops._check_logprobs("w", None, None, 3, 8, dev) is False
    assert ops._check_logprobs("w", lp, s, 3, 8, dev) is True
    for a, b in ((lp, None), (None, s), (lp.double(), s), (lp, torch.zeros(4)), (torch.zeros(3, 7), s), (lp.t().contiguous().t(), s)):
        with pytest.raises(ValueError):
            ops._check_logprobs("w", a, b, 3, 8, dev)
