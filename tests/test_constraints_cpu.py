"""The decoding-constraint rule (tests/constraint_rule.py, the NumPy restatement of db1_constrain_logits) on hand-worked rows, the
``DecodingConstraints`` validation, and the rule composed with the selection and beam rules.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_rule as B  # noqa: E402
import constraint_rule as C  # noqa: E402
import select_rule as R  # noqa: E402

NINF = np.float32(-np.inf)


def _row(*v):
    return np.array([v], np.float32)


def _hist(*h, mx=8):
    return np.array([list(h) + [0] * (mx - len(h))], np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint32 if a.dtype == np.float32 else np.uint16) ==
                                                          b.view(np.uint32 if b.dtype == np.float32 else np.uint16)).all()


def test_repetition_penalty_by_hand():
    l = _row(2.0, -2.0, 0.0, 3.0, np.inf, -np.inf, np.nan, 1.0)
    h = _hist(0, 1, 0, 0, 2, 4, 5, 6)                       # token 0 three times: penalised ONCE; 4, 5, 6 hit non-finite logits
    out = C.apply(l, h, 7, V=8, theta=2.0)
    want = _row(1.0, -4.0, 0.0, 3.0, np.inf, -np.inf, np.nan, 1.0)
    assert _same_bits(out, want)
    assert _same_bits(C.apply(l, h, 2, V=8, theta=2.0), _row(1.0, -4.0, 0.0, 3.0, np.inf, -np.inf, np.nan, 1.0))
    assert _same_bits(C.apply(l, h, 1, V=8, theta=2.0), _row(1.0, -2.0, 0.0, 3.0, np.inf, -np.inf, np.nan, 1.0))
    assert _same_bits(C.apply(l, h, 0, V=8, theta=2.0), l)                       # no history yet
    assert _same_bits(C.apply(l, h, 7, V=8, theta=1.0), l)                       # off
    # theta < 1 rewards repetition; the two products are single fp32 multiplications by theta and by fp32(1 / theta)
    th = np.float32(0.7)
    inv = np.float32(1.0 / float(th))
    out = C.apply(l, h, 2, V=8, theta=0.7)
    assert out[0, 0] == np.float32(np.float32(2.0) * inv) and out[0, 1] == np.float32(np.float32(-2.0) * th)
    # history entries outside [0, V) are skipped (a pad_id beyond the window, a negative id); V < ld: the padding keeps its bits
    out = C.apply(l, _hist(-1, 9, 7, 3), 4, V=7, theta=2.0)
    assert _same_bits(out, _row(2.0, -2.0, 0.0, 1.5, np.inf, -np.inf, np.nan, 1.0))


def test_bans_override_the_penalty_and_the_guard_leaves_rows_alone():
    l = _row(2.0, -2.0, 0.5, 3.0)
    h = _hist(3, 1)
    out = C.apply(l, h, 2, V=4, theta=2.0, bad=(3, 4, 99), eos_id=2, min_new=3)
    assert _same_bits(out, _row(2.0, -4.0, -np.inf, -np.inf))          # 3: penalised AND banned -> -inf; 2: EOS held back; 4, 99: outside
    assert _same_bits(C.apply(l, h, 2, V=4, eos_id=2, min_new=2), l)   # t == min_new: EOS is free again
    assert _same_bits(C.apply(l, h, 2, V=4, eos_id=-1, min_new=5), l)  # no EOS: the minimum length is a no-op
    assert _same_bits(C.apply(l, h, 2, V=2, bad=(2, 3)), l)            # bans outside [0, V) are ignored
    # the guard: t outside [0, max_new), a finished row, a row_map entry outside the slots
    for t in (-1, 8, 100):
        assert _same_bits(C.apply(l, h, t, V=4, theta=2.0, bad=(0,)), l)
    assert _same_bits(C.apply(l, h, 2, V=4, theta=2.0, bad=(0,), finished=[1]), l)
    assert _same_bits(C.apply(l, h, 2, V=4, theta=2.0, bad=(0,), row_map=[1]), l)
    assert _same_bits(C.apply(l, h, 2, V=4, theta=2.0, bad=(0,), row_map=[-1]), l)
    # two rows, per-slot counters, rows mapped to swapped slots: row 0 reads slot 1's history and counter
    l2 = np.concatenate([l, l])
    h2 = np.concatenate([_hist(3, 1), _hist(0, 0)])
    out = C.apply(l2, h2, np.array([2, 1]), V=4, theta=2.0, row_map=[1, 0])
    assert _same_bits(out, np.concatenate([_row(1.0, -2.0, 0.5, 3.0), _row(2.0, -4.0, 0.5, 1.5)]))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_ngram_edges(n):
    V = 6
    l = _row(*np.arange(1, V + 1, dtype=np.float32))
    H = [1, 2, 1, 2, 1, 3, 1, 2]
    h = _hist(*H, mx=9)
    for t in (n - 2, n - 1, n, 5, 8):
        if t < 0:
            continue
        out = C.apply(l, h, t, V=V, ngram=n)
        n1 = n - 1
        ban = {H[i] for i in range(n1, t) if H[i - n1:i] == H[t - n1:t]}         # the definition, spelled out
        if t <= n - 1:
            assert not ban                                                        # nothing while t < n; at t = n - 1 the range [n - 1, t) is empty
        want = l.copy()
        want[0, sorted(ban)] = NINF
        assert _same_bits(out, want), (n, t)
    if n == 1:
        assert C.banned_columns(H, 5, 1, (), -1, 0) == {1, 2}
        assert C.banned_columns(H, 1, 1, (), -1, 0) == {1}
        assert C.banned_columns(H, 0, 1, (), -1, 0) == set()
    if n == 2:
        assert C.banned_columns(H, 1, 2, (), -1, 0) == set()                      # t = n - 1
        assert C.banned_columns(H, 2, 2, (), -1, 0) == set()                      # t = n: the suffix [2] has no earlier copy
        assert C.banned_columns(H, 3, 2, (), -1, 0) == {2}                        # suffix [1] occurred at 0, followed by 2
        assert C.banned_columns(H, 7, 2, (), -1, 0) == {2, 3}                     # suffix [1]: followed by 2 (twice) and by 3
    if n == 3:
        assert C.banned_columns(H, 2, 3, (), -1, 0) == set()                      # t = n - 1
        assert C.banned_columns(H, 3, 3, (), -1, 0) == set()                      # t = n
        assert C.banned_columns(H, 4, 3, (), -1, 0) == {1}                        # suffix [1, 2] -> 1
        assert C.banned_columns(H, 8, 3, (), -1, 0) == {1}                        # suffix [1, 2] occurred twice, both followed by 1
        assert C.banned_columns([1, 2, 3, 1, 2, 4, 1, 2], 8, 3, (), -1, 0) == {3, 4}     # ... twice, with DIFFERENT continuations


def test_bf16_rounding_at_a_tie():
    # x = -1.0078125 (bf16 0xBF81), theta = 1.5: the fp32 product -1.51171875 = 0xBFC18000 lies exactly half way between the bf16 values
    # 0xBFC1 and 0xBFC2 -> ties to EVEN: 0xBFC2
    x = np.array([[0xBF81]], np.uint16)
    assert C.bf16_widen(x)[0, 0] == np.float32(-1.0078125)
    prod = np.float32(np.float32(-1.0078125) * np.float32(1.5))
    assert prod.view(np.uint32) == 0xBFC18000
    out = C.apply(x, _hist(0), 1, V=1, dtype=C.BF16, theta=1.5)
    assert out.dtype == np.uint16 and out[0, 0] == 0xBFC2
    # the neighbouring tie rounds DOWN to the even 0xBFC4: -1.0234375 (0xBF83) * 1.5 = -1.53515625 = 0xBFC48000
    y = np.array([[0xBF83]], np.uint16)
    assert np.float32(np.float32(-1.0234375) * np.float32(1.5)).view(np.uint32) == 0xBFC48000
    assert C.apply(y, _hist(0), 1, V=1, dtype=C.BF16, theta=1.5)[0, 0] == 0xBFC4
    # not a tie: plain rounding; a ban is the bf16 -inf; bf16_bits is the inverse of the widening on representable values
    assert C.apply(np.array([[0x4000, 0x4000]], np.uint16), _hist(0), 1, V=2, dtype=C.BF16, theta=1.3, bad=(1,)).tolist() == \
        [[int(C.bf16_bits(np.array([np.float32(2.0) * np.float32(1.0 / float(np.float32(1.3)))]))[0]), 0xFF80]]
    allbits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    fin = np.isfinite(C.bf16_widen(allbits))
    assert (C.bf16_bits(C.bf16_widen(allbits))[fin] == allbits[fin]).all()


def test_decoding_constraints_validation():
    from bdm_db1_amd import DecodingConstraints
    d = DecodingConstraints()
    assert d.is_noop and d == DecodingConstraints(1.0, 0, 0, ()) and hash(d) == hash(DecodingConstraints())
    c = DecodingConstraints(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=5, bad_token_ids=[7, np.int64(9)])
    assert not c.is_noop and c.bad_token_ids == (7, 9) and {c: 1}[DecodingConstraints(1.2, 3, 5, (7, 9))] == 1
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=1), dict(min_new_tokens=1), dict(bad_token_ids=(0,))):
        assert not DecodingConstraints(**kw).is_noop
    with pytest.raises(Exception):
        c.min_new_tokens = 3                                      # frozen
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(min_new_tokens=-1),
               dict(bad_token_ids=(-1,)), dict(bad_token_ids=(1.0,)), dict(bad_token_ids=(True,)), dict(bad_token_ids=tuple(range(1025)))):
        with pytest.raises(ValueError):
            DecodingConstraints(**kw)
    assert len(DecodingConstraints(bad_token_ids=tuple(range(1024))).bad_token_ids) == 1024


def test_generation_entry_points_take_the_keyword():
    import inspect
    import bdm_db1_amd as pkg
    for name in ("generate", "beam_search", "generate_stream"):
        assert "constraints" in inspect.signature(getattr(pkg, name)).parameters, name
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for n in ("db1_constrain_logits_supported", "db1_constrain_logits_workspace_bytes", "db1_constrain_logits"):
        assert n in names


def test_a_banned_argmax_yields_the_runner_up():
    rng = np.random.default_rng(0)
    V = 50
    l = rng.standard_normal((1, V)).astype(np.float32)
    order = np.argsort(-l[0])
    top, second, third = int(order[0]), int(order[1]), int(order[2])
    assert R.select_row(l[0], 0, V)[0] == top
    h = _hist(second)
    # the arg-max is banned outright; the runner-up is in the history of a 1-gram ban; the third wins
    assert R.select_row(C.apply(l, h, 1, V=V, bad=(top,))[0], 0, V)[0] == second
    assert R.select_row(C.apply(l, h, 1, V=V, bad=(top,), ngram=1)[0], 0, V)[0] == third
    # a penalty large enough to push the (positive) arg-max under the runner-up
    lp = np.abs(l) + np.float32(0.1)
    o = np.argsort(-lp[0])
    assert R.select_row(C.apply(lp, _hist(int(o[0])), 1, V=V, theta=100.0)[0], 0, V)[0] == int(o[1])
    # sampling never draws a banned column
    for seed in range(20):
        assert R.select_row(C.apply(l, h, 1, V=V, bad=(top,))[0], 0, V, greedy=False, seed=seed)[0] != top
    # beams: one group of two beams at step 0 (only beam 0 is live): the beams take the two best NON-banned columns, and the banned
    # column is outside the log-sum-exp their scores are measured against
    S0 = B.new_state(1, 2, 4)
    l2 = np.concatenate([l, l])
    S, _ = B.step(S0, l2, 0, 2, 0, V)
    assert S["tokens"][:, 0].tolist() == [top, second]
    e = C.apply(l2, np.zeros((2, 4), np.int32), 0, V=V, bad=(top,))
    S, _ = B.step(S0, e, 0, 2, 0, V)
    assert S["tokens"][:, 0].tolist() == [second, third]
    rest = np.delete(l[0].astype(np.float64), top)
    lse = rest.max() + np.log(np.exp(rest - rest.max()).sum())
    assert abs(float(S["beam_score"][0]) - (float(l[0, second]) - lse)) < 1e-5
    # EOS held back by the minimum length: the beam that wanted EOS takes the next token instead of ending
    S, _ = B.step(S0, l2, 0, 2, 0, V, eos=top)
    assert S["pool_count"][0] == 1
    S, _ = B.step(S0, C.apply(l2, np.zeros((2, 4), np.int32), 0, V=V, eos_id=top, min_new=1), 0, 2, 0, V, eos=top)
    assert S["pool_count"][0] == 0 and S["tokens"][:, 0].tolist() == [second, third]
