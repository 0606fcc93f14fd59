"""db1_beam_step_diverse against the NumPy rule (tests/diverse_beam_rule.py) step by step from the device's own state, against
db1_beam_step bit for bit where the penalty is off, the closed form at t = 0, and every refusal.  The cases are those of
tests/diverse_beam_cases.py; test_diverse_beam_cpu.py asserts on the same seeds that they exercise the penalty."""
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
import diverse_beam_cases as C  # noqa: E402
import diverse_beam_rule as DR  # noqa: E402
from beam_kernel_common import DEV_KEYS, _bits_equal, _close, _compare, _launch, _upload  # noqa: E402
from gpu_common import _need_gpu  # noqa: E402,F401

@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("lam", C.LAMS)
@pytest.mark.parametrize("V", C.VS)
@pytest.mark.parametrize("G", C.GS)
@pytest.mark.parametrize("D,Wp", C.SHAPES)
def test_diverse_step_follows_the_rule(D, Wp, G, V, lam, dt):
    W = D * Wp
    lo, hi = C.window(V)
    pad, tdt = hi - 1, getattr(torch, dt)
    n_amb = 0
    dev = {}

    def widen(l):                                          # (bf16: the widened values the kernel sees)
        dev["l"] = torch.from_numpy(l).to(DEV).to(tdt)
        return dev["l"].float().cpu().numpy()

    def step(S, lw, t):
        want, amb = DR.step(S, lw, t, W, D, lam, lo, hi, C.EOS, pad, C.ALPHA)
        got = _launch(S, dev["l"], t, Wp, D, lam, lo, hi, C.EOS, pad, C.ALPHA, V)
        _compare(got, want, amb, Wp, D, t)
        if t == 1:      # the same inputs give the same bits
            _bits_equal(got, _launch(S, dev["l"], t, Wp, D, lam, lo, hi, C.EOS, pad, C.ALPHA, V))
        if t == 2:      # the planted done sub-group: pad to its rows, nothing else of it touched
            q = C.done_subgroup(G, D)
            assert (got["next_ids"][q * Wp:(q + 1) * Wp] == pad).all()
            for k in ("beam_score", "parent", "tokens"):
                assert np.array_equal(got[k][q * Wp:(q + 1) * Wp], S[k][q * Wp:(q + 1) * Wp]), k
        return got, amb                                    # the next step starts from the device's state

    for t, S, l, nxt, amb in C.run(D, Wp, G, V, lam, step, widen):
        n_amb += int(amb.sum())
    assert n_amb <= (G * D * C.STEPS) // 4


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("D,Wp", C.SHAPES)
def test_without_a_penalty_the_bits_of_the_plain_step(D, Wp, dt):
    """D = 1: db1_beam_step itself; D > 1: db1_beam_step over G * D groups of W'"""
    G, V, lam = 3, 33025, 0.0
    lo, hi = C.window(V)
    pad, tdt = hi - 1, getattr(torch, dt)
    dev = {}

    def widen(l):
        dev["l"] = torch.from_numpy(l).to(DEV).to(tdt)
        return l

    def step(S, l, t):
        got = _launch(S, dev["l"], t, Wp, D, lam, lo, hi, C.EOS, pad, C.ALPHA, V)
        _bits_equal(got, _launch(S, dev["l"], t, Wp, D, lam, lo, hi, C.EOS, pad, C.ALPHA, V, plain=True))
        return got, None

    assert sum(1 for _ in C.run(D, Wp, G, V, lam, step, widen)) == C.STEPS


@pytest.mark.parametrize("D,Wp", [(4, 4), (16, 1), (2, 8), (8, 2), (3, 5)])
def test_closed_form_at_t0(D, Wp):
    """no EOS, a penalty above every score difference: sub-group d takes its row's raw ranks d W' .. d W' + W' - 1, scores unpenalised"""
    W, V, G, lam = D * Wp, 3000, 2, 1e4
    rng = np.random.default_rng(D * 100 + Wp)
    l = np.stack([np.tile(rng.permutation(V).astype(np.float32)[None] * 0.01, (W, 1)) for _ in range(G)]).reshape(G * W, V)
    S = DR.new_state(G, W, D, 3, 0)
    got = _launch(S, torch.from_numpy(l).to(DEV), 0, Wp, D, lam, 0, V, -1, 0, 1.0, V)
    for g in range(G):
        order = np.argsort(-l[g * W], kind="stable")
        assert list(got["next_ids"][g * W:(g + 1) * W]) == list(order[:W]), g
        lse = B._lse32(l[g * W])
        assert _close(got["beam_score"][g * W:(g + 1) * W], l[g * W][order[:W]] - lse)
    assert not got["done"].any() and not got["status"].any() and (got["pool_count"] == 0).all()


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("D", [2, 3, 4, 16])
def test_the_last_candidate_of_a_row_reaches_the_state(D, dt):
    """W' = 1 (cases.k_row_case): the last sub-group's new beam is its row's raw rank W' + W - 1, so a kernel that kept one candidate
    fewer per row would store a penalised token and its score.  Against the UNCUT rule; the rule cut to W' + W - 1 must differ from it"""
    S, l, eos, lam = C.k_row_case(D)
    V, pad, W = l.shape[1], l.shape[1] - 1, D
    lt = torch.from_numpy(l).to(DEV).to(getattr(torch, dt))          # (integers up to 64 and -50: exact in bf16)
    assert np.array_equal(lt.float().cpu().numpy(), l)
    want, amb = DR.step(S, l, 0, W, D, lam, 0, V, eos, pad)
    short = DR.step(S, l, 0, W, D, lam, 0, V, eos, pad, k_row=W)[0]
    assert not amb.any() and short["tokens"][D - 1, 0] == 1 and want["tokens"][D - 1, 0] == D
    got = _launch(S, lt, 0, 1, D, lam, 0, V, eos, pad, 1.0, V)
    _compare(got, want, amb, 1, D, 0)
    assert list(got["tokens"][:, 0]) == list(range(1, D + 1)) and list(got["pool_count"]) == [0] * (D - 1) + [1]
    assert _close(got["beam_score"][D - 1], l[D - 1, D] - B._lse32(l[D - 1]))


def test_counter_out_of_range():
    D, Wp, G, V, mx = 2, 2, 2, 300, 4
    S = DR.new_state(G, D * Wp, D, mx, 0)
    S["done"][1] = 1
    l = torch.randn(G * D * Wp, V, device=DEV)
    for t in (mx, -1):
        got = _launch(S, l, t, Wp, D, 0.5, 0, V, -1, 7, 1.0, V)
        assert list(got["status"]) == [2, 0, 2, 2] and (got["next_ids"] == 7).all() and (got["pool_count"] == 0).all()
        for k in ("beam_score", "parent", "tokens", "pool_score", "done"):
            assert np.array_equal(got[k], S[k]), k


def test_refusals_of_the_wrapper():
    from bdm_db1_amd import ops
    D, Wp, G, V, mx = 2, 2, 2, 300, 4
    S = DR.new_state(G, D * Wp, D, mx, 0)
    l = torch.randn(G * D * Wp, V, device=DEV)
    Dv = _upload(S)
    ids = torch.zeros(G * D * Wp, dtype=torch.long, device=DEV)
    tt = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = [tt, Dv["beam_score"], Dv["parent"], Dv["tokens"], Dv["pool_tokens"], Dv["pool_len"], Dv["pool_score"], Dv["pool_slot"],
            Dv["pool_count"], Dv["done"], Dv["switches"], ids, Dv["status"]]
    good = dict(W=Wp, D=D, diversity_penalty=0.5)
    for bad in (dict(D=0), dict(W=3), dict(W=4, D=5), dict(vocab_lo=5, vocab_hi=5), dict(vocab_hi=V + 1), dict(length_penalty=float("inf")),
                dict(diversity_penalty=-1.0), dict(diversity_penalty=float("nan")), dict(diversity_penalty=float("inf"))):
        with pytest.raises(ValueError):
            ops.beam_step_diverse(l, *args, **dict(good, **bad))
    wrong = list(args)
    wrong[4] = Dv["pool_tokens"][:, :, :2]
    with pytest.raises(ValueError):
        ops.beam_step_diverse(l, *wrong, **good)
    with pytest.raises(ValueError):
        ops.beam_step_diverse(l.double(), *args, **good)
    torch.cuda.synchronize()
    for k in DEV_KEYS:
        assert np.array_equal(Dv[k].cpu().numpy(), S[k]), k      # nothing was launched


def test_refusals_of_the_library_with_their_codes():
    """past the wrapper: every refusal of db1_beam_step_diverse itself, with db1_beam_step's codes, and nothing launched"""
    from bdm_db1_amd import lib, ops
    L = lib.load()
    D, Wp, G, V, mx = 2, 2, 2, 300, 4
    M = G * D * Wp
    S = DR.new_state(G, D * Wp, D, mx, 0)
    l = torch.randn(M, V, device=DEV)
    Dv = _upload(S)
    ids = torch.full((M,), -5, dtype=torch.long, device=DEV)
    tt = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = int(L.db1_beam_step_diverse_workspace_bytes(M, V, Wp, D, mx, 0))
    assert need > int(L.db1_beam_step_workspace_bytes(M, V, Wp, mx, 0)) > 0           # (K_row = W' + W > 2W')
    assert int(L.db1_beam_step_diverse_workspace_bytes(M, V, Wp, 1, mx, 0)) == int(L.db1_beam_step_workspace_bytes(M, V, Wp, mx, 0))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    P = lambda x: x.data_ptr()
    base = dict(logits=P(l), G=G, D=D, W=Wp, lam=0.5, V=V, ld=V, dt=0, lo=0, hi=V, eos=-1, pad=0, lp=1.0, t=P(tt), mx=mx,
                beam_score=P(Dv["beam_score"]), parent=P(Dv["parent"]), tokens=P(Dv["tokens"]), pool_tokens=P(Dv["pool_tokens"]),
                pool_len=P(Dv["pool_len"]), pool_score=P(Dv["pool_score"]), pool_slot=P(Dv["pool_slot"]), pool_count=P(Dv["pool_count"]),
                done=P(Dv["done"]), switches=P(Dv["switches"]), next_ids=P(ids), stride=1, status=P(Dv["status"]), ws=P(ws), wsn=need,
                stream=ops.stream())
    WS_SMALL = -4                                          # (DB1_ERR_WORKSPACE_TOO_SMALL)
    cases = [(dict(D=0), ops.DB1_ERR_UNSUPPORTED), (dict(D=-1), ops.DB1_ERR_UNSUPPORTED), (dict(D=9), ops.DB1_ERR_UNSUPPORTED),
             (dict(W=0), ops.DB1_ERR_UNSUPPORTED), (dict(W=9), ops.DB1_ERR_UNSUPPORTED), (dict(dt=7), ops.DB1_ERR_UNSUPPORTED),
             (dict(V=70000, ld=70000, hi=70000), ops.DB1_ERR_UNSUPPORTED), (dict(ld=V - 1), ops.DB1_ERR_UNSUPPORTED),
             (dict(G=0), ops.DB1_ERR_BAD_SHAPE), (dict(G=16384), ops.DB1_ERR_BAD_SHAPE), (dict(mx=0), ops.DB1_ERR_BAD_SHAPE),
             (dict(lo=5, hi=5), ops.DB1_ERR_BAD_SHAPE), (dict(hi=V + 1), ops.DB1_ERR_BAD_SHAPE), (dict(lo=-1), ops.DB1_ERR_BAD_SHAPE),
             (dict(lam=-0.5), ops.DB1_ERR_BAD_SHAPE), (dict(lam=float("inf")), ops.DB1_ERR_BAD_SHAPE), (dict(lam=float("nan")), ops.DB1_ERR_BAD_SHAPE),
             (dict(lp=float("inf")), ops.DB1_ERR_BAD_SHAPE), (dict(wsn=need - 1), WS_SMALL), (dict(ws=None), WS_SMALL)]
    cases += [({k: None}, ops.DB1_ERR_BAD_SHAPE) for k in ("logits", "t", "beam_score", "parent", "tokens", "pool_tokens", "pool_len", "pool_score",
                                                          "pool_slot", "pool_count", "done", "switches", "next_ids", "status")]
    for kw, code in cases:
        a = dict(base, **kw)
        assert L.db1_beam_step_diverse(*a.values()) == code, kw
    torch.cuda.synchronize()
    assert (ids == -5).all()
    for k in DEV_KEYS:
        assert np.array_equal(Dv[k].cpu().numpy(), S[k]), k
    assert L.db1_beam_step_diverse(*base.values()) == 0
    torch.cuda.synchronize()
    assert (ids != -5).all()
