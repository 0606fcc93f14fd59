"""The top-n rule (tests/topn_rule.py) against a second formulation, the config fields that switch the alternatives on, the prototypes and
exports of the ``_top`` entry points and the argument checks that come before any launch.  No GPU."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import topn_rule as T  # noqa: E402

NEW = ("db1_select_tokens_top", "db1_select_tokens_slots_top", "db1_score_rows_top", "db1_lmhead_score_top")


def _second(l, lo, hi, n):
    """a stable float64 argsort of the negated window plus np.logaddexp.reduce: the rule without its helpers"""
    w = np.asarray(l, np.float64)[lo:hi]
    order = np.argsort(-np.where(np.isfinite(w), w, -np.inf), kind="stable")
    order = [int(i) for i in order if np.isfinite(w[i])][:n]
    ids, lps = np.full(n, -1, np.int64), np.full(n, -np.inf)
    if order:
        lse = np.logaddexp.reduce(w[np.isfinite(w)])
        ids[:len(order)] = np.asarray(order) + lo
        lps[:len(order)] = w[order] - lse
    return ids, lps


def _rows():
    rng = np.random.default_rng(5)
    V = 203
    rows = []
    for _ in range(12):
        l = rng.integers(-3, 4, V).astype(np.float64) * 0.5            # 7 distinct values: ties everywhere
        l[rng.integers(0, V, 15)] = rng.choice([np.nan, np.inf, -np.inf], 15)
        rows.append(l)
    rows.append(rng.standard_normal(V) * 3)
    return rows, V


@pytest.mark.parametrize("n", [1, 5, 16])
def test_the_rule_agrees_with_a_stable_argsort_and_logaddexp(n):
    rows, V = _rows()
    for l in rows:
        for lo, hi in ((0, V), (5, V - 3), (17, 20)):                # whole row, a window not aligned to 4, a 3-column window
            ids, lps = T.top_row(l, lo, hi, n)
            want_ids, want_lps = _second(l, lo, hi, n)
            assert np.array_equal(ids, want_ids)
            k = int((ids >= 0).sum())
            assert np.abs(lps[:k] - want_lps[:k]).max(initial=0.0) < 1e-12 and np.isneginf(lps[k:]).all()
            assert (np.diff(lps[:k]) <= 0).all()
            assert ((ids[:k] >= lo) & (ids[:k] < hi)).all() and np.isfinite(l[ids[:k]]).all()
            # probabilities: the n best never sum to more than one, all candidates to one
            assert np.exp(lps[:k]).sum() <= 1 + 1e-12


def test_fewer_candidates_than_n_and_no_candidate():
    l = np.array([9.0, 1.0, np.nan, 1.0, 9.0])
    ids, lps = T.top_row(l, 1, 4, 5)                                   # a 3-column window with one NaN: 2 candidates, tied
    assert ids.tolist() == [1, 3, -1, -1, -1] and np.allclose(lps[:2], np.log(0.5)) and np.isneginf(lps[2:]).all()
    ids, lps = T.top_row(np.array([np.nan, -np.inf, np.inf, 1.0]), 0, 3, 4)
    assert (ids == -1).all() and np.isneginf(lps).all()
    ids, lps = T.top_row(np.full(8, -np.inf), 0, 8, 16)
    assert (ids == -1).all() and np.isneginf(lps).all()
    for n in (0, 17):
        with pytest.raises(ValueError):
            T.top_row(l, 0, 5, n)


def test_signed_zeros_are_one_value_unless_the_keys_order_them():
    l = np.array([-0.0, 0.0, -1.0, 0.0, -0.0])
    assert T.top_row(l, 0, 5, 5)[0].tolist() == [0, 1, 3, 4, 2]       # scoring: by column among the zeros
    assert T.top_row(l, 0, 5, 5, signed_zero=True)[0].tolist() == [1, 3, 0, 4, 2]     # generation: +0.0 first, as the arg-max's keys have it
    assert np.array_equal(T.top_row(l, 0, 5, 5)[1], T.top_row(l, 0, 5, 5, signed_zero=True)[1])


def test_bookkeeping_of_a_lockstep_and_a_slot_launch():
    lg = np.array([[0.0, 1.0, 2.0, 0.0], [5.0, 0.0, 0.0, 0.0], [np.nan, np.inf, -np.inf, np.nan]])
    ids, lps = np.full((3, 2, 2), 7, np.int64), np.full((3, 2, 2), 7.0)
    T.step(lg, 1, 2, np.array([False, True, False]), ids, lps, 0, 4)
    assert ids[0, 1].tolist() == [2, 1] and (ids[1:, 1] == -1).all() and np.isneginf(lps[1:, 1]).all()
    assert (ids[:, 0] == 7).all() and (lps[:, 0] == 7.0).all()        # the other column is not the launch's
    T.step(lg, 2, 2, np.zeros(3, bool), ids, lps, 0, 4)               # t out of range: nothing
    assert (ids[:, 0] == 7).all() and ids[0, 1].tolist() == [2, 1]
    ids, lps = np.full((4, 3, 2), 7, np.int64), np.full((4, 3, 2), 7.0)
    #                     slot 1 live at t = 2, slot 9 does not exist, slot 0 vacant;  then slot 3 at its limit, slot 2 live at t = 0
    T.step_slots(lg, [1, 9, 0], np.array([0, 2, 0, 2]), np.array([3, 3, 3, 2]), np.array([1, 0, 0, 0]), ids, lps, 0, 4)
    assert ids[1, 2].tolist() == [2, 1] and (np.delete(ids.reshape(-1, 2), 1 * 3 + 2, 0) == 7).all()
    T.step_slots(lg, [3, 2, 9], np.array([0, 2, 0, 2]), np.array([3, 3, 3, 2]), np.array([1, 0, 0, 0]), ids, lps, 0, 4)
    assert (ids[3] == 7).all() and ids[2, 0].tolist() == [0, 1]


def test_configs_refuse_bad_values_before_a_model_is_touched():
    from bdm_db1_amd import GenerationConfig, sample_best_of
    from bdm_db1_amd.scoring import ScoreConfig
    assert GenerationConfig(logprobs=True, top_logprobs=16).top_logprobs == 16
    for kw in (dict(top_logprobs=3), dict(logprobs=True, top_logprobs=17), dict(logprobs=True, top_logprobs=-1),
               dict(logprobs=True, top_logprobs=True), dict(logprobs=True, top_logprobs=2.0)):
        with pytest.raises(ValueError):
            GenerationConfig(**kw)
    assert ScoreConfig(top_n=16).top_n == 16
    for n in (17, -1, True, 1.5):
        with pytest.raises(ValueError):
            ScoreConfig(top_n=n)
    with pytest.raises(ValueError, match="top_logprobs"):
        sample_best_of(None, None, GenerationConfig(greedy=False, top_p=0.9, logprobs=True, top_logprobs=4), 4)


def test_default_configs_are_what_they_were_without_the_field():
    from bdm_db1_amd import GenerationConfig
    from bdm_db1_amd.scoring import ScoreConfig, ScoreResult
    import inspect
    g = [f.name for f in dataclasses.fields(GenerationConfig)]
    assert "top_logprobs" in g and g[-1] == "logprobs"                 # (what dataclasses.fields ends with is what it was)
    params = list(inspect.signature(GenerationConfig).parameters.values())
    assert params[-1].name == "top_logprobs" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY      # the constructor's new last argument
    assert [p.name for p in params[:-1]] == [n for n in g if n != "top_logprobs"]
    old = (30, False, 0.7, 40, 0.9, 3, 5, 0, 1, 90, 8, True)           # every field a caller could set before, positionally
    a, b = GenerationConfig(*old), GenerationConfig(*old, top_logprobs=0)
    assert a == b and hash(a) == hash(b) and a.top_logprobs == 0 and (2, a, 100, 90) == (2, b, 100, 90)
    assert GenerationConfig() == GenerationConfig(top_logprobs=0) and hash(GenerationConfig()) == hash(GenerationConfig(top_logprobs=0))
    c = dataclasses.replace(a, top_logprobs=5)
    assert c != a and (2, a, 100, 90) != (2, c, 100, 90)               # (the generator's cache key holds the config: non-zero, another key)
    s = [f.name for f in dataclasses.fields(ScoreConfig)]
    assert s[-1] == "top_n" and ScoreConfig(3, 50, 0.5, 7, False) == ScoreConfig(3, 50, 0.5, 7, False, top_n=0)
    assert hash(ScoreConfig()) == hash(ScoreConfig(top_n=0)) and ScoreConfig(top_n=4) != ScoreConfig()
    r = ScoreResult(sum_logprob=np.zeros(1), tokens=np.ones(1), hits=np.zeros(1), task=np.zeros(1, np.int64), kinds=["nlp"])
    assert r.top_ids is None and r.top_logprob is None


def test_top_prototypes_extend_their_parents_by_a_count_and_two_pointers():
    from bdm_db1_amd import lib
    protos = lib.parse_header()
    added = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for parent, name in (("db1_select_tokens_lp", "db1_select_tokens_top"), ("db1_select_tokens_slots_lp", "db1_select_tokens_slots_top"),
                         ("db1_score_rows", "db1_score_rows_top"), ("db1_lmhead_score", "db1_lmhead_score_top")):
        ret, args = protos[parent]
        ret_t, args_t = protos[name]
        assert ret_t is ret and len(args_t) == len(args) + 3, name
        assert args_t[:-6] == args[:-3] and args_t[-6:-3] == added and args_t[-3:] == args[-3:], name
    assert not [n for n in protos if "_top_supported" in n or "_top_workspace_bytes" in n]


def test_the_built_library_exports_the_new_symbols():
    from bdm_db1_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert getattr(so, name) is not None and name in lib.declared_symbols()


def test_ops_wrappers_take_all_three_top_arguments_or_none():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd import ops
    dev = torch.device("cpu")
    ids, lp = torch.zeros(3, 8, 5, dtype=torch.int32), torch.zeros(3, 8, 5)
    assert ops._check_top("w", None, None, None, (3, 8), dev) == 0
    assert ops._check_top("w", 5, ids, lp, (3, 8), dev) == 5
    assert ops._check_top("w", 2, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), (4,), dev) == 2
    for n, a, b in ((5, ids, None), (None, ids, lp), (5, None, lp), (0, ids, lp), (17, ids, lp), (True, ids, lp), (4, ids, lp),
                    (5, ids.long(), lp), (5, ids, lp.double()), (5, ids[:2], lp), (5, ids, torch.zeros(3, 5, 8).transpose(1, 2))):
        with pytest.raises(ValueError):
            ops._check_top("w", n, a, b, (3, 8), dev)
