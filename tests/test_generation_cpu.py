"""Generation without a GPU: GenerationConfig's argument checks, clip_at_eos against the reference decoder's clipping rule, and sanity
checks of the NumPy restatement of the selection rule (tests/select_rule.py) that the GPU tests compare db1_select_tokens with."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import select_rule as R  # noqa: E402


@pytest.mark.parametrize("kw", [dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(greedy=False, temperature=0.0),
                                dict(greedy=False, temperature=-1.0), dict(vocab_lo=5, vocab_hi=5), dict(vocab_lo=7, vocab_hi=3),
                                dict(vocab_lo=-1), dict(max_new_tokens=0), dict(top_k=-2), dict(sync_every=0), dict(seed=-1)])
def test_generation_config_rejects_bad_arguments(kw):
    from bdm_db1_amd import GenerationConfig
    with pytest.raises(ValueError):
        GenerationConfig(**kw)


def test_generation_config_accepts_good_arguments():
    from bdm_db1_amd import GenerationConfig
    GenerationConfig()
    GenerationConfig(greedy=True, temperature=0.0)    # (the temperature is unused when greedy)
    GenerationConfig(greedy=False, temperature=0.7, top_k=40, top_p=0.9, seed=2 ** 63, vocab_lo=0, vocab_hi=32000, eos_id=2)


def _reference_decode(data, eos, max_length=30):
    """text_decoder.py:53-58 (Decoder.decode, clip_at_eos=True) on the id level: the ids it hands to the tokenizer"""
    data = data[:max_length]
    for i, d in enumerate(data):
        if d == eos:
            data = data[:i]
            break
    return list(data)


def test_clip_at_eos_matches_the_reference_decoder():
    from bdm_db1_amd import clip_at_eos
    eos, pad = 2, 0
    rows = [[5, 6, 7, 2, 0, 0], [2, 0, 0, 0, 0, 0], [9, 9, 9, 9, 9, 9], [3, 2, 0, 0, 0, 0]]
    lengths = [3, 0, 6, 1]   # what db1_select_tokens counts: the tokens before EOS
    got = clip_at_eos(np.array(rows, np.int32), np.array(lengths, np.int32))
    assert got == [_reference_decode(r, eos, max_length=6) for r in rows]
    assert got == [[5, 6, 7], [], [9, 9, 9, 9, 9, 9], [3]]


def test_restated_top_k_1_is_argmax_and_full_window_keeps_everything():
    rng = np.random.default_rng(0)
    for V in (7, 300, 5000):
        l = rng.standard_normal(V) * 2
        l[rng.integers(0, V)] = -np.inf
        lo, hi = 1, V - 1
        kept = R.kept_set(l, lo, hi, 0.7, 0, 1.0)[0]
        assert kept.sum() == np.isfinite(l[lo:hi]).sum() and not kept[0] and not kept[V - 1]
        tok, _ = R.select_row(l, lo, hi, greedy=False, temperature=0.7, top_k=1, seed=3)
        assert tok == lo + int(np.argmax(np.where(np.isfinite(l[lo:hi]), l[lo:hi], -np.inf)))
        kept1 = R.kept_set(l, lo, hi, 1.0, 1, 1.0)[0]
        assert kept1.sum() == 1 and kept1[tok]


def test_restated_top_p_keeps_the_smallest_head_with_enough_mass():
    l = np.log(np.array([0.5, 0.2, 0.2, 0.05, 0.05]))
    assert R.kept_set(l, 0, 5, 1.0, 0, 0.5)[0].tolist() == [True, False, False, False, False]
    assert R.kept_set(l, 0, 5, 1.0, 0, 0.6)[0].tolist() == [True, True, True, False, False]   # the tie at 0.2 is kept whole
    assert R.kept_set(l, 0, 5, 1.0, 0, 0.95)[0].tolist() == [True] * 5
    assert R.kept_set(l, 0, 5, 1.0, 2, 1.0)[0].tolist() == [True, True, True, False, False]   # k-th largest tied: both kept


def test_restated_uniforms_are_the_documented_philox_words():
    from oracle import db1_oracle as O
    u = R.uniforms(10, stream_id=5, step=7, seed=(11 << 32) | 3)
    o = O.philox4x32_10(np.uint64(2), np.uint64(5), np.uint64(7), np.uint64(R.SITE_SAMPLE), 3, 11)
    assert u[9] == ((int(o[1]) >> 8) + 0.5) * 2.0 ** -24
    assert np.all((u > 0) & (u < 1))


def test_restated_thresholds_match_a_sort_based_statement():
    """kept_set against the definition read literally: the k-th largest value, then the largest kept value tau with mass{l >= tau} >= top_p"""
    rng = np.random.default_rng(1)
    for it in range(40):
        V = int(rng.integers(5, 400))
        l = np.round(rng.standard_normal(V) * 2, 1)      # (rounded: many ties)
        T, k, p = float(rng.uniform(0.3, 2)), int(rng.integers(0, V)), float(rng.uniform(0.05, 1.0))
        lo, hi = int(rng.integers(0, 3)), V - int(rng.integers(0, 3))
        cand = np.zeros(V, bool)
        cand[lo:hi] = True
        keep = cand.copy()
        if k > 0:
            keep &= l >= sorted(l[cand], reverse=True)[min(k, cand.sum()) - 1]
        e = np.where(keep, np.exp((l - l[keep].max()) / T), 0.0)
        if p < 1:
            tau = max(v for v in set(l[keep]) if e[keep & (l >= v)].sum() >= p * e.sum() * (1 - 1e-12))
            keep &= l >= tau
        assert (R.kept_set(l, lo, hi, T, k, p)[0] == keep).all(), it
