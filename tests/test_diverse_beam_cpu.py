"""Diverse beam search without a GPU: the rule of tests/diverse_beam_rule.py against beam_rule at lambda = 0, the candidates a row must
keep (W' + W, not W' + W - 1: a planted case whose stored state differs), the merge of the pools, the refusals of the config and of the
wrapper, the prototypes, and the conditions the cases of test_diverse_beam_kernels_gpu.py must meet so that they test the penalty -- on the seeds that test uses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_rule as B  # noqa: E402
import diverse_beam_cases as C  # noqa: E402
import diverse_beam_rule as DR  # noqa: E402


def _same(a, b):
    for k in DR.STATE_KEYS:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


def _bf16(l):
    return torch.from_numpy(l).to(torch.bfloat16).float().numpy()


# ------------------------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("D,Wp", C.SHAPES)
def test_lambda_zero_is_the_plain_rule_over_the_sub_groups(D, Wp):
    G, V, lam = 3, 200, 0.0
    lo, hi = C.window(V)
    seen = 0
    for t, S, l, nxt, amb in C.run(D, Wp, G, V, lam, lambda S, l, t: DR.step(S, l, t, D * Wp, D, 0.0, lo, hi, C.EOS, hi - 1, C.ALPHA)):
        want, wamb = B.step(S, l, t, Wp, lo, hi, C.EOS, hi - 1, C.ALPHA)
        _same(nxt, want)
        assert np.array_equal(amb, wamb)
        seen += 1
    out = DR.step(S, l, C.STEPS, D * Wp, D, 0.0, lo, hi, C.EOS, hi - 1, C.ALPHA)[0]        # the counter out of range, too
    _same(out, B.step(S, l, C.STEPS, Wp, lo, hi, C.EOS, hi - 1, C.ALPHA)[0])
    assert seen == C.STEPS


@pytest.mark.parametrize("D,Wp", [s for s in C.SHAPES if s[0] > 1])
@pytest.mark.parametrize("lam", C.LAMS + [1e4])
def test_rows_cut_to_their_top_w_plus_wprime_give_the_uncut_rule(D, Wp, lam):
    G, V, W = 3, 200, D * Wp
    lo, hi = C.window(V)
    for t, S, l, nxt, amb in C.run(D, Wp, G, V, lam, lambda S, l, t: DR.step(S, l, t, W, D, lam, lo, hi, C.EOS, hi - 1, C.ALPHA)):
        wu, wc = {}, {}
        _same(DR.step(S, l, t, W, D, lam, lo, hi, C.EOS, hi - 1, C.ALPHA, walked=wu)[0], nxt)
        cut = DR.step(S, l, t, W, D, lam, lo, hi, C.EOS, hi - 1, C.ALPHA, k_row=Wp + W, walked=wc)[0]
        _same(cut, nxt)
        assert wc == wu                                   # the same 2W' candidates walked, in the same order


def _closed_form_case(D=4, Wp=4, V=64, lam=1e4):
    """t = 0, no EOS, a penalty larger than any score difference: sub-group d must take its row's raw ranks d W' .. d W' + W' - 1"""
    W = D * Wp
    rng = np.random.default_rng(5)
    l = np.tile(rng.permutation(V).astype(np.float32)[None], (W, 1))
    S = DR.new_state(1, W, D, 3, 0)
    return S, l, W, np.argsort(-l[0], kind="stable")


def test_closed_form_at_t0_and_one_candidate_too_few():
    D, Wp, lam = 4, 4, 1e4
    S, l, W, order = _closed_form_case(D, Wp, lam=lam)
    V = l.shape[1]
    full = DR.step(S, l, 0, W, D, lam, 0, V)[0]
    for d in range(D):
        assert list(full["next_ids"][d * Wp:(d + 1) * Wp]) == list(order[d * Wp:(d + 1) * Wp]), d
    # the stored scores are the unpenalised log-probabilities
    lse = B._lse32(l[0])
    assert np.allclose(full["beam_score"], (l[0][full["next_ids"]] - lse).astype(np.float32), rtol=0, atol=1e-5)
    wu, wc, ws = {}, {}, {}
    DR.step(S, l, 0, W, D, lam, 0, V, walked=wu)
    _same(DR.step(S, l, 0, W, D, lam, 0, V, k_row=Wp + W, walked=wc)[0], full)
    assert wc == wu and [c for _, c in wu[D - 1]] == list(order[W - Wp:W + Wp])
    # one candidate fewer per row: the last sub-group's walk loses its last candidate (raw rank W + W' - 1) to a penalised one.  Here
    # (W' = 4, no EOS) the stored state does not show it; test_the_last_candidate_of_a_row_reaches_the_state plants the case that does
    DR.step(S, l, 0, W, D, lam, 0, V, k_row=Wp + W - 1, walked=ws)
    assert ws[D - 1][:-1] == wu[D - 1][:-1] and ws[D - 1][-1] != wu[D - 1][-1] and ws[D - 1][-1][1] in order[:W - Wp]
    assert all(ws[d] == wu[d] for d in range(D - 1))


@pytest.mark.parametrize("D", [2, 3, 4, 16])
def test_the_last_candidate_of_a_row_reaches_the_state(D):
    """W' = 1: the last sub-group's new beam is its row's raw rank W' + W - 1 (cases.k_row_case).  With the row lists cut to W' + W the
    state is the uncut rule's; cut to W' + W - 1 the stored token and beam score differ"""
    S, l, eos, lam = C.k_row_case(D)
    V, pad, W = l.shape[1], l.shape[1] - 1, D
    full = DR.step(S, l, 0, W, D, lam, 0, V, eos, pad)[0]
    assert list(full["tokens"][:, 0]) == list(range(1, D + 1))
    assert list(full["pool_count"]) == [0] * (D - 1) + [1] and list(full["pool_tokens"][D - 1, 0, :1]) == [eos]
    lse = B._lse32(l[D - 1])
    assert abs(float(full["beam_score"][D - 1]) - float(l[D - 1, D] - lse)) < 1e-5      # the unpenalised score of token D
    _same(DR.step(S, l, 0, W, D, lam, 0, V, eos, pad, k_row=1 + W)[0], full)
    short = DR.step(S, l, 0, W, D, lam, 0, V, eos, pad, k_row=W)[0]
    assert list(short["tokens"][:, 0]) == list(range(1, D)) + [1]                      # a penalised token in the place of token D
    assert abs(float(short["beam_score"][D - 1]) - float(l[D - 1, 1] - lse)) < 1e-5
    assert not np.array_equal(short["beam_score"], full["beam_score"])


def test_a_done_sub_group_feeds_nothing_and_eos_is_never_counted():
    D, Wp, V, lam = 3, 1, 32, 1e4
    l = np.tile(np.arange(V, 0, -1).astype(np.float32)[None], (3, 1))       # token 0 is every row's best, then 1, 2, ...
    S = DR.new_state(1, 3, D, 4, 0)
    assert list(DR.step(S, l, 0, 3, D, lam, 0, V)[0]["next_ids"]) == [0, 1, 2]
    S["done"][0] = 1
    out = DR.step(S, l, 0, 3, D, lam, 0, V, pad=31)[0]
    assert list(out["next_ids"]) == [31, 0, 1]                              # sub-group 1 is the first to choose
    S["done"][0] = 0
    out = DR.step(S, l, 0, 3, D, lam, 0, V, eos=0)[0]                       # EOS on top: a hypothesis in every pool, never penalised
    assert list(out["pool_count"]) == [1, 1, 1] and list(out["next_ids"]) == [0, 0, 0] and out["done"].all()


# ------------------------------------------------------------------------------------------------------------------------------ the merge
def test_merge_of_the_pools():
    inf = np.inf
    scores = np.array([[-1.0, -2.0, -inf], [-1.0, -1.5, -2.0], [-0.5, -inf, -inf]], np.float32)
    counts = [2, 3, 1]
    assert DR.merge_order(scores, counts) == [(2, 0), (0, 0), (1, 0), (1, 1), (0, 1), (1, 2)]
    D, Wp, mx = 3, 3, 2
    S = DR.new_state(2, D * Wp, D, mx, 9)
    S["pool_score"][:3] = scores
    S["pool_count"][:3] = counts
    S["pool_len"][:3] = np.arange(9).reshape(3, 3)
    S["pool_slot"][:3] = [[2, 0, 1], [0, 1, 2], [1, 0, 2]]
    S["pool_tokens"][:3] = np.arange(18).reshape(3, 3, 2)
    ids, lengths, sc, groups = DR.results(S, D * Wp, D, 4, 9)
    assert list(groups[0]) == [2, 0, 1, 1] and list(lengths[0]) == [6, 0, 3, 4] and list(sc[0]) == [-0.5, -1.0, -1.0, -1.5]
    assert ids[0].tolist() == [[14, 15], [4, 5], [6, 7], [8, 9]]
    assert list(groups[1]) == [-1] * 4 and (ids[1] == 9).all() and np.isneginf(sc[1]).all()      # a prompt without a hypothesis


def test_beam_state_merges_as_the_rule_does():
    from types import SimpleNamespace
    from bdm_db1_amd import generation as gen
    D, Wp, G, R, mx = 3, 2, 2, 5, 3
    rng = np.random.default_rng(3)
    S = DR.new_state(G, D * Wp, D, mx, 0)
    S["pool_count"][:] = [2, 1, 2, 0, 2, 1]
    sc = np.sort(rng.integers(-4, 0, (G * D, Wp)).astype(np.float32), axis=1)[:, ::-1]      # small integers: equal scores across pools
    S["pool_score"][:] = np.where(np.arange(Wp)[None] < S["pool_count"][:, None], sc, -np.inf)
    S["pool_len"][:] = rng.integers(1, 4, (G * D, Wp))
    S["pool_slot"][:] = [rng.permutation(Wp) for _ in range(G * D)]
    S["pool_tokens"][:] = rng.integers(0, 50, (G * D, Wp, mx))
    st = object.__new__(gen._BeamState)
    st.G, st.D, st.Q, st.Wg, st.W = G, D, G * D, Wp, D * Wp
    st.cfg = SimpleNamespace(num_return_sequences=R, max_new_tokens=mx, pad_id=0)
    for k in ("pool_tokens", "pool_slot", "pool_len", "pool_score", "pool_count", "status", "switches"):
        setattr(st, k, torch.from_numpy(S[k]))
    ids, lengths, scores = st.result()
    wi, wl, ws, wg = DR.results(S, D * Wp, D, R, 0)
    assert np.array_equal(ids.numpy(), wi) and np.array_equal(lengths.numpy(), wl) and np.array_equal(scores.numpy(), ws)
    stats = st.stats()
    assert np.array_equal(stats["result_groups"].numpy(), wg) and stats["parent_switches"] == 0


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_config_refusals_and_defaults():
    import dataclasses
    from bdm_db1_amd import generation as gen
    cfg = gen.BeamSearchConfig()
    assert (cfg.num_beam_groups, cfg.diversity_penalty) == (1, 0.0)
    assert [f.name for f in dataclasses.fields(cfg)][-2:] == ["num_beam_groups", "diversity_penalty"]
    assert cfg == gen.BeamSearchConfig(num_beam_groups=1, diversity_penalty=0.0)
    for ok in (dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5), dict(num_beams=4, num_beam_groups=4, diversity_penalty=0.0),
               dict(num_beams=15, num_beam_groups=5, diversity_penalty=1e4), dict(num_beams=16, num_beam_groups=16, diversity_penalty=1)):
        gen.BeamSearchConfig(**ok)
    for bad in (dict(num_beams=4, num_beam_groups=3), dict(num_beams=4, num_beam_groups=0), dict(num_beams=4, num_beam_groups=8),
                dict(num_beams=4, num_beam_groups=-2), dict(num_beams=4, num_beam_groups=2.0), dict(num_beams=4, num_beam_groups=True),
                dict(num_beams=4, num_beam_groups=2, diversity_penalty=-0.1), dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("inf")),
                dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("nan")), dict(num_beams=4, num_beam_groups=2, diversity_penalty=None),
                dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.5), dict(num_beams=4, diversity_penalty=1.0)):
        with pytest.raises(ValueError, match="num_beam_groups|diversity_penalty"):
            gen.BeamSearchConfig(**bad)


def _operands(G=2, D=2, Wp=2, V=40, mx=3):
    Q, M = G * D, G * D * Wp
    i32, f32 = torch.int32, torch.float32
    z = lambda *s, dt=i32: torch.zeros(*s, dtype=dt)
    return [torch.zeros(M, V), z(1), z(M, dt=f32), z(M), z(M, mx), z(Q, Wp, mx), z(Q, Wp), z(Q, Wp, dt=f32), z(Q, Wp), z(Q), z(Q), z(Q),
            z(M, dt=torch.int64), z(Q)]


def test_the_wrapper_refuses_before_the_library_is_called(monkeypatch):
    from bdm_db1_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    good = dict(W=2, D=2, diversity_penalty=0.5)
    for kw in (dict(D=0), dict(D=-1), dict(W=0), dict(W=4, D=5), dict(W=1, D=17), dict(W=3), dict(diversity_penalty=-1.0),
               dict(diversity_penalty=float("inf")), dict(diversity_penalty=float("nan")), dict(vocab_lo=5, vocab_hi=5), dict(vocab_hi=41),
               dict(length_penalty=float("inf")), dict(V=41)):
        with pytest.raises(ValueError, match="beam_step_diverse"):
            ops.beam_step_diverse(*_operands(), **dict(good, **kw))
    args = _operands()
    for i, wrong in ((0, args[0].double()), (0, args[0][:, ::2]), (0, args[0][:7]), (1, args[1].long()), (2, args[2][:7]), (4, args[4].long()),
                     (5, args[5][:, :, :2]), (5, torch.zeros(2, 4, 3, dtype=torch.int32)), (6, args[6][:3]), (7, args[7].int()), (9, args[9][:2]),
                     (10, torch.zeros(8, dtype=torch.int32)), (12, args[12].int()), (12, args[12][:7]), (13, args[13].float())):
        a = list(args)
        a[i] = wrong
        with pytest.raises(ValueError, match="beam_step_diverse"):
            ops.beam_step_diverse(*a, **good)
    with pytest.raises(AssertionError, match="the library was called"):      # good arguments reach it
        ops.beam_step_diverse(*args, **good)


def test_prototypes():
    import ctypes
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    protos = lib.parse_header()
    for n in ("db1_beam_step_diverse", "db1_beam_step_diverse_supported", "db1_beam_step_diverse_workspace_bytes"):
        assert n in names
    restype, argtypes = protos["db1_beam_step_diverse"]
    plain = protos["db1_beam_step"][1]
    assert restype is ctypes.c_int and len(argtypes) == len(plain) + 2
    assert argtypes[:5] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float] and argtypes[5:] == plain[3:]
    assert protos["db1_beam_step_diverse_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 6)
    assert protos["db1_beam_step_diverse_supported"][1] == [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]


# ------------------------------------------------------------------------------------------- the GPU test's cases, on the GPU test's seeds
@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("lam", C.LAMS)
@pytest.mark.parametrize("V", C.VS)
@pytest.mark.parametrize("G", C.GS)
@pytest.mark.parametrize("D,Wp", C.SHAPES)
def test_the_gpu_cases_exercise_the_penalty_and_stay_unambiguous(D, Wp, G, V, lam, dt):
    W = D * Wp
    lo, hi = C.window(V)
    widen = _bf16 if dt == "bfloat16" else (lambda l: l)
    n_amb = differ = 0
    for t, S, l, nxt, amb in C.run(D, Wp, G, V, lam, lambda S, l, t: DR.step(S, l, t, W, D, lam, lo, hi, C.EOS, hi - 1, C.ALPHA), widen):
        n_amb += int(amb.sum())
        plain = DR.step(S, l, t, W, D, 0.0, lo, hi, C.EOS, hi - 1, C.ALPHA)[0]
        differ += t >= 1 and not np.array_equal(plain["next_ids"], nxt["next_ids"])
        if t == 2:
            q = C.done_subgroup(G, D)
            assert S["done"][q] == 1 and (nxt["next_ids"][q * Wp:(q + 1) * Wp] == hi - 1).all()
    kinds = [C.eos_kind(g, G) for g in range(G)]
    assert any(k != 0 for k in kinds)                         # a prompt without EOS on top
    assert n_amb <= (G * D * C.STEPS) // 4
    if D > 1 and G == 3:
        assert differ >= 2, differ

