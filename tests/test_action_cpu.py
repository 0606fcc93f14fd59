"""Action decoding without a GPU: the rule of tests/action_rule.py against the product's own torch passes (masked_logits_for_action, argmax,
recover_model_predict_token_to_tokenizer_raw) for every vocabulary layout; action_window; the refusals of the config and of the ops wrappers
with the library neither loaded nor called; the prototypes; the memorising call; and the ambiguity cap of the GPU kernel test's rows."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import action_cases as C  # noqa: E402
import action_rule as A  # noqa: E402

TEXT, NDV, NB, N_ACT = 50, 20, 32, 6


def _args(overlap):
    return SimpleNamespace(overlap_with_text=overlap, text_vocab_size=TEXT, num_discrete_values=NDV, num_continuous_bin=NB)


def _vocab(overlap):
    return TEXT + NB + (0 if overlap else NDV) + 1


@pytest.mark.parametrize("overlap,discrete,masked", [(o, d, m) for o in (True, False) for d in (True, False) for m in ((False, True) if d else (False,))])
def test_greedy_rule_is_the_products_masked_argmax(overlap, discrete, masked):
    """masks exist for discrete action spaces only (evaluate_rl.py:121-123); where the discrete ids do not overlap the text ids the
    reference's penalty lands on text columns outside the window and changes nothing: action_mask_applies says so, and the rule gets no mask"""
    from bdm_db1_amd.evaluation import (action_mask_applies, action_window, masked_logits_for_action,
                                        recover_model_predict_token_to_tokenizer_raw)
    args, V, M = _args(overlap), _vocab(overlap), 7
    rng = np.random.default_rng(17 + 2 * overlap + discrete)
    space = SimpleNamespace(n=N_ACT) if discrete else None
    lo, hi = action_window(args, discrete, N_ACT if discrete else None)
    for trial in range(4):
        x = (rng.standard_normal((M, V)) * 3).astype(np.float32)
        x[:, :lo] += 9.0           # (the best logits lie outside the window)
        x[:, hi:] += 9.0
        for r in range(M):
            c = lo + rng.choice(hi - lo, 2, replace=False)
            x[r, c] = x[r, lo:hi].max() + 0.5      # a tie: the lowest column wins
        mask = (rng.random(N_ACT) < 0.5).astype(np.float64) if masked else None
        if masked:
            mask[rng.integers(N_ACT)] = 1.0
        ref = masked_logits_for_action(args, torch.from_numpy(x.copy())[:, None, :], discrete, space, env_action_mask=mask)
        ref_tok = ref[:, -1, :].argmax(-1).numpy()
        ref_bin = recover_model_predict_token_to_tokenizer_raw(args, torch.from_numpy(ref_tok.copy()), discrete).numpy()
        bins, ids, status = np.full((M, 2), -7, np.int32), np.full((M, 1), -9, np.int64), np.zeros(M, np.int32)
        rule_mask = np.tile(mask[None, :] == 1, (M, 1)).astype(np.uint8) if masked and action_mask_applies(args, discrete) else None
        tok = A.select_actions(x, (3, 1), bins, None, ids, status, act_lo=lo, act_hi=hi, mask=rule_mask)
        assert (tok == ref_tok).all() and (ids[:, 0] == ref_tok).all() and (bins[:, 1] == ref_bin).all(), (overlap, discrete, masked, trial)
        assert (bins[:, 0] == -7).all() and (status == 0).all()
    assert action_mask_applies(args, discrete) == (discrete and overlap)


def test_action_window():
    from bdm_db1_amd.evaluation import action_window
    db1 = SimpleNamespace(overlap_with_text=True, text_vocab_size=32000, num_discrete_values=1024, num_continuous_bin=1024)
    assert action_window(db1, False) == (32000, 33024) and action_window(db1, True, 6) == (0, 6)
    sep = SimpleNamespace(overlap_with_text=False, text_vocab_size=32000, num_discrete_values=1024, num_continuous_bin=1024)
    assert action_window(sep, False) == (33024, 34048) and action_window(sep, True, 18) == (32000, 32018)
    for bad in (None, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_actions"):
            action_window(db1, True, bad)


def test_config_refusals():
    from bdm_db1_amd.evaluation import ActionConfig
    ok = ActionConfig(obs_length=17, action_length=6, discrete_action=False)
    assert ok.greedy and ok.top_k == 0 and ok.top_p == 1.0 and ok.temperature == 1.0 and ok.seed == 0 and ok.n_actions is None
    with pytest.raises(Exception):
        ok.seed = 3                 # frozen
    ActionConfig(3, 1, True, n_actions=6, greedy=False, temperature=0.7, top_k=5, top_p=0.9, seed=11)
    for kw in (dict(obs_length=0), dict(obs_length=2.0), dict(obs_length=True), dict(action_length=0), dict(action_length=65), dict(discrete_action=1),
               dict(discrete_action=True), dict(discrete_action=True, n_actions=0), dict(discrete_action=True, n_actions=2.0), dict(n_actions=6),
               dict(greedy=0), dict(greedy=False, temperature=0.0), dict(greedy=False, temperature=float("inf")), dict(greedy=False, top_p=0.0),
               dict(greedy=False, top_p=1.5), dict(greedy=False, top_k=-1), dict(top_k=1.5), dict(seed="x")):
        with pytest.raises(ValueError, match="ActionConfig"):
            ActionConfig(**{**dict(obs_length=4, action_length=3, discrete_action=False), **kw})


def test_ops_refuse_on_the_host_before_the_library_is_loaded(monkeypatch):
    from bdm_db1_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    i32, f32, i64, u8 = torch.int32, torch.float32, torch.int64, torch.uint8
    z = lambda *s, dt=i32: torch.zeros(*s, dtype=dt)
    M, V = 3, 200
    good = dict(logits2d=z(M, V, dt=f32), ctr=z(2), bins=z(M, 3), next_ids=z(M, dt=i64), status=z(M), act_lo=150, act_hi=199)
    for kw in (dict(act_lo=150, act_hi=150), dict(act_hi=201), dict(act_lo=-1), dict(logits2d=z(M, 6000, dt=f32), act_lo=0, act_hi=4097),
               dict(logits2d=z(M, V, dt=torch.float16)), dict(logits2d=z(M, 2 * V, dt=f32)[:, ::2]), dict(logits2d=z(V, dt=f32)), dict(V=201),
               dict(ctr=z(1)), dict(ctr=z(2, dt=i64)), dict(bins=z(M, 0)), dict(bins=z(M, 65)), dict(bins=z(M + 1, 3)), dict(bins=z(M, 3, dt=i64)),
               dict(bins=z(M * 3)), dict(values=z(M, 2, dt=f32)), dict(values=z(M, 3)), dict(next_ids=z(M)), dict(next_ids=z(M + 1, dt=i64)),
               dict(status=z(M - 1)), dict(stream_id=z(M, dt=i64)), dict(mask=z(M, 50, dt=u8)), dict(mask=z(M, 0, dt=u8)), dict(mask=z(M, 6)),
               dict(mask=z(M + 1, 6, dt=u8)), dict(mask=z(6, dt=u8)), dict(num_bins=0), dict(greedy=False, temperature=0.0),
               dict(greedy=False, top_p=0.0), dict(greedy=False, top_p=1.5), dict(greedy=False, top_k=-1)):
        a = {**good, **kw}
        pos = [a.pop(k) for k in ("logits2d", "ctr", "bins", "next_ids", "status")]
        with pytest.raises(ValueError, match="select_actions"):
            ops.select_actions(*pos, **a)
    x, ids = z(M, 4, dt=f32), z(M, 5, dt=i64)
    for a, kw in (((z(M, 4), ids), {}), ((z(4, dt=f32), ids), {}), ((z(M, 8, dt=f32)[:, ::2], ids), {}), ((z(0, 4, dt=f32), z(0, 5, dt=i64)), {}),
                  ((x, z(M, 4, dt=i64)), {}), ((x, z(M, 5)), {}), ((x, z(M + 1, 5, dt=i64)), {}), ((x, z(M, 10, dt=i64)[:, ::2]), {}),
                  ((x, ids), dict(num_bins=0)), ((x, ids), dict(bin_base=-1)), ((x, ids), dict(sep_id=-1))):
        with pytest.raises(ValueError, match="obs_tokens"):
            ops.obs_tokens(*a, **{**dict(bin_base=100, sep_id=199), **kw})


def test_prototypes_are_in_the_header():
    from bdm_db1_amd import lib
    protos = lib.parse_header()
    assert len(protos["db1_select_actions"][1]) == 26 and len(protos["db1_obs_tokens"][1]) == 11
    assert len(protos["db1_select_actions_supported"][1]) == 5 and len(protos["db1_select_actions_workspace_bytes"][1]) == 3
    src = open(lib.HEADER).read()
    for word in ("db1_select_actions", "db1_obs_tokens", "i == act_len", "step_base + ctr[0] * act_len + ctr[1]", "tests/action_rule.py"):
        assert word in src, word


def test_the_memorising_call_and_a_counter_out_of_range_write_nothing_in_the_rule():
    rng = np.random.default_rng(2)
    M, V, L = 4, 60, 3
    x = rng.standard_normal((M, V))
    fresh = lambda: (np.full((M, L), -7, np.int32), np.full((M, L), -5.0, np.float32), np.full((M, 2), -9, np.int64), np.zeros(M, np.int32))
    bins, vals, ids, st = fresh()
    assert A.select_actions(x, (5, L), bins, vals, ids, st, act_lo=10, act_hi=40) is None
    assert (bins == -7).all() and (vals == -5.0).all() and (ids == -9).all() and (st == 0).all()
    for i in (-1, L + 1):
        bins, vals, ids, st = fresh()
        assert A.select_actions(x, (5, i), bins, vals, ids, st, act_lo=10, act_hi=40) is None
        assert (bins == -7).all() and (vals == -5.0).all() and (ids == -9).all() and (st == 2).all()
    bins, vals, ids, st = fresh()
    x[2, 10:40] = -np.inf
    tok = A.select_actions(x, (5, 1), bins, vals, ids, st, act_lo=10, act_hi=40, ids_col=1, num_bins=32)
    assert tok[2] == 10 and bins[2, 1] == 0 and st.tolist() == [0, 0, 1, 0] and (ids[:, 1] == tok).all() and (ids[:, 0] == -9).all()
    assert (bins[:, [0, 2]] == -7).all() and (vals[:, 1] == A.decode_action(tok - 10, 32)).all() and vals[2, 1] == -1.0
    assert A.step_of(11, 2, 3, 1) == 18


def test_ambiguity_cap_of_the_kernel_tests_rows():
    """the GPU kernel test compares with the float64 rule outside the rows whose top-p cut the kernel's fp32 masses may place elsewhere
    (a cumulative mass within 1e-5 of top_p, the select test's slack): at most 5 % of its rows may be such rows"""
    s = C.SAMPLING
    total = amb = 0
    for V, lo, hi in C.WINDOWS:
        for M in C.ROWS:
            for dt in C.DTYPES:
                x, mask, _ = C.make(V, lo, hi, M, dt)
                for mk in (None, mask):
                    for r in range(M):
                        total += 1
                        amb += A.ambiguous(x[r, :V], lo, hi, None if mk is None else mk[r], s["temperature"], s["top_k"], s["top_p"])
    assert total == 4 * (1 + 3 + 64) * 2 * 2 and amb <= 0.05 * total, (amb, total)
