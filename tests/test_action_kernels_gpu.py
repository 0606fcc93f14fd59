"""db1_select_actions and db1_obs_tokens (include/db1_hip.h, "action decoding") on the GPU: the tokens bit-equal to db1_select_tokens on a
copy of the logits with -inf at the masked columns, and equal to the NumPy rule of tests/action_rule.py outside the rows whose top-p cut is
ambiguous in fp32 (tests/test_action_cpu.py caps those at 5 %); the values bit-equal to db1_mulaw_decode's action branch; the memorising
call and a counter out of range; determinism; the library's refusals; the observation ids against db1_mulaw_discretize."""
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

import action_cases as C  # noqa: E402
import action_rule as A  # noqa: E402
from gpu_common import Guarded, _need_gpu  # noqa: E402,F401

G = os.path.join(ROOT, "tests", "golden")
ISENT = -7680             # gpu_common's sentinel, as an integer


class IntGuard:
    """an integer tensor of ``shape`` in the middle of an allocation filled with the sentinel (64 elements before and after)"""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 128,), ISENT, dtype=dtype, device=DEV)
        self.t = self.buf[64:64 + self.n].view(*shape)

    def np(self):
        return self.t.cpu().numpy().copy()

    def intact(self, name):
        assert (self.buf[:64] == ISENT).all() and (self.buf[64 + self.n:] == ISENT).all(), f"{name}: a guard element changed"


class Out:
    """the outputs of one launch, all at the sentinel: bins / values [M, act_len], the next ids as column 2 of [M, 3], status 0"""

    def __init__(self, M, act_len, env_step, i):
        self.bins, self.ids = IntGuard((M, act_len), torch.int32), IntGuard((M, 3), torch.int64)
        self.values = Guarded(M, act_len, "f32")
        self.status = IntGuard((M,), torch.int32)
        self.status.t.zero_()
        self.ctr = torch.tensor([env_step, i], dtype=torch.int32, device=DEV)

    def call(self, logits, with_values=True, **kw):
        from bdm_db1_amd import ops
        ops.select_actions(logits, self.ctr, self.bins.t, self.ids.t[:, 2], self.status.t, values=self.values.t if with_values else None, **kw)
        return self

    def intact(self):
        for name in ("bins", "ids", "values", "status"):
            getattr(self, name).intact(name)

    def bits(self):
        return (self.bins.np(), self.ids.np(), self.values.buf.view(torch.int32).cpu().numpy().copy(), self.status.np())


def _select_tokens_ref(lg, x_masked_dev, lo, hi, V, step, sids, kw):
    """db1_select_tokens on the masked copy at Philox step ``step`` -> (tokens, status)"""
    from bdm_db1_amd import ops
    M = lg.shape[0]
    i32 = dict(dtype=torch.int32, device=DEV)
    t, fin, ln, st = torch.zeros(1, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32), torch.zeros(M, **i32)
    out, ids = torch.zeros(M, 1, **i32), torch.zeros(M, dtype=torch.long, device=DEV)
    ops.select_tokens(x_masked_dev, t, fin, ln, out, ids, st, V=V, vocab_lo=lo, vocab_hi=hi, pad_id=lo, step_base=step, stream_id=sids,
                      seed=C.SEED, **kw)
    return ids.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("M", C.ROWS)
@pytest.mark.parametrize("V,lo,hi", C.WINDOWS)
def test_tokens_are_select_tokens_on_the_masked_row_and_the_rule(V, lo, hi, M, dt):
    from bdm_db1_amd import ops
    x, mask, sid_h = C.make(V, lo, hi, M, dt)
    lg = torch.from_numpy(x).to(DEV).to(C.TD[dt])
    sids = torch.from_numpy(sid_h).to(DEV)
    all_vals = torch.empty(1024, dtype=torch.float32, device=DEV)
    ops.mulaw_decode(torch.arange(1024, dtype=torch.int64, device=DEV), all_vals, True, 1024)
    all_vals = all_vals.cpu().numpy()
    checked = skipped = 0
    for mk in (None, mask):
        xm = x.copy()
        if mk is not None:
            xm[:, lo:lo + mk.shape[1]][mk == 0] = -np.inf
        lgm = torch.from_numpy(xm).to(DEV).to(C.TD[dt])
        mk_dev = None if mk is None else torch.from_numpy(mk).to(DEV)
        for kw in (dict(greedy=True), C.SAMPLING):
            amb = [False] * M if kw["greedy"] else [A.ambiguous(x[r, :V], lo, hi, None if mk is None else mk[r], kw["temperature"], kw["top_k"],
                                                                kw["top_p"]) for r in range(M)]
            for act_len, i in C.STEPS:
                o = Out(M, act_len, C.ENV_STEP, i).call(lg, V=V, act_lo=lo, act_hi=hi, mask=mk_dev, num_bins=1024, seed=C.SEED,
                                                        step_base=C.STEP_BASE, stream_id=sids, **kw)
                bins, ids, vals, status = o.bins.np(), o.ids.np(), o.values.np(), o.status.np()
                o.intact()
                step = A.step_of(C.STEP_BASE, C.ENV_STEP, act_len, i)
                ref_tok, ref_st = _select_tokens_ref(lg, lgm, lo, hi, V, step, sids, kw)
                tok = ids[:, 2]
                assert (tok == ref_tok).all(), (mk is not None, kw["greedy"], act_len, i, np.nonzero(tok != ref_tok))
                assert ((status & 1) == (ref_st & 1)).all() and ((status & ~1) == 0).all()
                assert (ids[:, :2] == ISENT).all()                                  # (the strided column only)
                assert (bins[:, i] == tok - lo).all() and ((tok >= lo) & (tok < hi)).all()
                assert (np.delete(bins, i, axis=1) == ISENT).all() and (np.delete(vals, i, axis=1) == -7680.0).all()
                assert np.array_equal(vals[:, i].view(np.int32), all_vals[np.clip(bins[:, i], 0, 1023)].view(np.int32))
                # the rule
                rb, rv = np.full((M, act_len), ISENT, np.int32), np.full((M, act_len), -7680.0, np.float32)
                ri, rs = np.full((M, 3), ISENT, np.int64), np.zeros(M, np.int32)
                rule_tok = A.select_actions(x[:, :V], (C.ENV_STEP, i), rb, rv, ri, rs, act_lo=lo, act_hi=hi, mask=mk, num_bins=1024, seed=C.SEED,
                                            step_base=C.STEP_BASE, stream_ids=sid_h, ids_col=2, **kw)
                for r in range(M):
                    if amb[r]:
                        skipped += 1
                        continue
                    checked += 1
                    assert tok[r] == rule_tok[r] and status[r] == rs[r], (r, mk is not None, kw["greedy"], act_len, i)
                    assert np.array_equal(vals[r].view(np.int32), rv[r].view(np.int32)) and (bins[r] == rb[r]).all()
                if M >= 3 and mk is not None:
                    assert status[1] == 1 and tok[1] == lo and bins[1, i] == 0          # the row without a candidate
                # determinism: a second launch gives the same bits
                again = Out(M, act_len, C.ENV_STEP, i).call(lg, V=V, act_lo=lo, act_hi=hi, mask=mk_dev, num_bins=1024, seed=C.SEED,
                                                            step_base=C.STEP_BASE, stream_id=sids, **kw)
                for a, b in zip(o.bits(), again.bits()):
                    assert np.array_equal(a, b)
    assert skipped <= 0.05 * (checked + skipped)


def test_values_of_all_1024_bins_are_mulaw_decodes():
    from bdm_db1_amd import ops
    nb, lo = 1024, 50
    lg = torch.zeros(nb, 1100, device=DEV)
    lg[torch.arange(nb), lo + torch.arange(nb)] = 5.0
    o = Out(nb, 1, 0, 0).call(lg, act_lo=lo, act_hi=lo + nb, num_bins=nb)
    ref = torch.empty(nb, dtype=torch.float32, device=DEV)
    ops.mulaw_decode(torch.arange(nb, dtype=torch.int64, device=DEV), ref, True, nb)
    assert (o.bins.np()[:, 0] == np.arange(nb)).all() and (o.status.np() == 0).all()
    assert np.array_equal(o.values.np()[:, 0].view(np.int32), ref.cpu().numpy().view(np.int32))
    o.intact()
    # no values buffer: the rest is the same
    p = Out(nb, 1, 0, 0).call(lg, with_values=False, act_lo=lo, act_hi=lo + nb, num_bins=nb)
    assert np.array_equal(p.bins.np(), o.bins.np()) and np.array_equal(p.ids.np(), o.ids.np()) and (p.values.np() == -7680.0).all()


@pytest.mark.parametrize("dt", C.DTYPES)
def test_memorising_call_and_a_counter_out_of_range_write_nothing(dt):
    V, lo, hi = C.WINDOWS[1]
    x, mask, sid_h = C.make(V, lo, hi, 3, dt)
    lg = torch.from_numpy(x).to(DEV).to(C.TD[dt])
    for kw in (dict(greedy=True), C.SAMPLING):
        o = Out(3, 3, 5, 3).call(lg, V=V, act_lo=lo, act_hi=hi, **kw)
        assert (o.bins.np() == ISENT).all() and (o.ids.np() == ISENT).all() and (o.values.np() == -7680.0).all() and (o.status.np() == 0).all()
        o.intact()
        for i in (-1, 4, 1 << 20):
            o = Out(3, 3, 5, i).call(lg, V=V, act_lo=lo, act_hi=hi, **kw)
            assert (o.bins.np() == ISENT).all() and (o.ids.np() == ISENT).all() and (o.values.np() == -7680.0).all() and (o.status.np() == 2).all()
            o.intact()


def test_the_library_refuses_before_any_launch():
    from bdm_db1_amd import lib, ops
    L = lib.load()
    M, V = 2, 200
    lg = torch.randn(M, V, device=DEV)
    o = Out(M, 3, 0, 0)
    mask = torch.ones(M, 6, dtype=torch.uint8, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()

    def call(**kw):
        a = dict(logits=P(lg), M=M, V=V, ld=V, dt=0, lo=150, hi=199, mask=None, n_mask=0, T=1.0, top_k=0, top_p=1.0, greedy=1, ctr=P(o.ctr), act_len=3,
                 nb=1024, bins=P(o.bins.t), values=P(o.values.t), ids=P(o.ids.t), stride=3, status=P(o.status.t))
        a.update(kw)
        return L.db1_select_actions(a["logits"], a["M"], a["V"], a["ld"], a["dt"], a["lo"], a["hi"], a["mask"], a["n_mask"], a["T"], a["top_k"], a["top_p"],
                                    a["greedy"], 0, 0, 0, a["ctr"], None, a["act_len"], a["nb"], a["bins"], a["values"], a["ids"], a["stride"], a["status"], None)
    bad = ops.DB1_ERR_BAD_SHAPE
    for kw, code in ((dict(dt=7), ops.DB1_ERR_UNSUPPORTED_DTYPE), (dict(logits=None), bad), (dict(ctr=None), bad), (dict(bins=None), bad),
                     (dict(ids=None), bad), (dict(status=None), bad), (dict(lo=150, hi=150), bad), (dict(hi=201), bad), (dict(lo=-1), bad),
                     (dict(V=6000, ld=6000, lo=0, hi=4097), ops.DB1_ERR_UNSUPPORTED), (dict(mask=P(mask), n_mask=50), bad),
                     (dict(mask=P(mask), n_mask=0), bad), (dict(n_mask=6), bad), (dict(n_mask=-1), bad), (dict(act_len=0), bad), (dict(act_len=65), bad),
                     (dict(nb=0), bad), (dict(M=0), bad), (dict(ld=V - 1), bad), (dict(greedy=0, T=0.0), bad), (dict(greedy=0, T=float("inf")), bad),
                     (dict(greedy=0, top_k=-1), bad), (dict(greedy=0, top_p=0.0), bad), (dict(greedy=0, top_p=1.5), bad)):
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert (o.bins.np() == ISENT).all() and (o.ids.np() == ISENT).all() and (o.values.np() == -7680.0).all() and (o.status.np() == 0).all()
    assert call() == 0 and call(values=None) == 0 and call(mask=P(mask), n_mask=6) == 0
    assert L.db1_select_actions_workspace_bytes(64, 33025, 1) == 0
    assert L.db1_select_actions_supported(33025, 33280, 1, 32000, 33024) and L.db1_select_actions_supported(40000, 40000, 0, 0, 4096)
    assert not L.db1_select_actions_supported(40000, 40000, 0, 0, 4097) and not L.db1_select_actions_supported(200, 200, 0, 5, 5)
    assert not L.db1_select_actions_supported(200, 200, 0, 150, 201) and not L.db1_select_actions_supported(200, 200, 7, 150, 199)
    x, ids = torch.zeros(M, 4, device=DEV), IntGuard((M, 5), torch.int64)
    for args in ((None, M, 4, P(ids.t), 5), (P(x), M, 4, None, 5), (P(x), 0, 4, P(ids.t), 5), (P(x), M, 0, P(ids.t), 5), (P(x), M, 4, P(ids.t), 4)):
        assert L.db1_obs_tokens(*args, 100, 199, 1024, 100.0, 256.0, None) == bad, args
    for tail in ((100, 199, 0), (-1, 199, 1024), (100, -1, 1024)):
        assert L.db1_obs_tokens(P(x), M, 4, P(ids.t), 5, *tail, 100.0, 256.0, None) == bad, tail
    torch.cuda.synchronize()
    assert (ids.np() == ISENT).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("obs_dim", [1, 4, 17])
def test_obs_tokens_are_mulaw_discretize_plus_the_offset(obs_dim):
    from bdm_db1_amd import ops
    gold = np.load(os.path.join(G, "scalar_tokenizer.npz"))
    flat = np.concatenate([gold["known_obs"], gold["obs"]]).astype(np.float32)
    M = flat.shape[0] // obs_dim
    x = torch.from_numpy(flat[:M * obs_dim].reshape(M, obs_dim)).to(DEV)
    ref = torch.empty(M, obs_dim, dtype=torch.int32, device=DEV)
    ops.mulaw_discretize(x, ref, False, 1024)
    gold_ids = np.concatenate([gold["known_obs_ids"], gold["obs_ids"]])[:M * obs_dim].reshape(M, obs_dim)
    assert np.array_equal(ref.cpu().numpy(), gold_ids)
    base, sep, q = 32000, 33024, obs_dim + 3           # (a row stride above obs_dim + 1: the columns behind the separator stay)
    ids = IntGuard((M, q), torch.int64)
    ops.obs_tokens(x, ids.t, bin_base=base, sep_id=sep, num_bins=1024)
    got = ids.np()
    assert np.array_equal(got[:, :obs_dim], base + gold_ids.astype(np.int64)) and (got[:, obs_dim] == sep).all() and (got[:, obs_dim + 1:] == ISENT).all()
    ids.intact("ids")


# windows that touch 5 and 4 of the row's 1024-column blocks (select_actions_kernel<T, 5>: the groups of blocks b and b + 4 fold into one
# partial sum and the slot index 4 ((jb + v) & 3) wraps), and the two 1024-wide windows of DB1's vocabularies
WIDE = [(6000, 1000, 5096), (6000, 2000, 4500), (33025, 32000, 33024), (34049, 33024, 34048)]
# top-p alone at T = 1 over flattened logits keeps hundreds of tokens: the fp32 sums of the kept mass have hundreds of terms, in every
# virtual wave, so another order of summation than db1_select_tokens' moves a threshold in some row
MODES = [dict(greedy=True), dict(greedy=False, temperature=1.0, top_k=0, top_p=0.9), dict(greedy=False, temperature=1.3, top_k=700, top_p=0.5), C.SAMPLING]


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("V,lo,hi", WIDE)
def test_wide_windows_and_long_top_p_sums_are_select_tokens(V, lo, hi, dt):
    M = 64
    x, mask, sid_h = C.make(V, lo, hi, M, dt)
    x[:, lo:hi] /= 3.0                                   # (unit variance: a flat distribution)
    x = torch.from_numpy(x).to(C.TD[dt]).float().numpy()
    lg = torch.from_numpy(x).to(DEV).to(C.TD[dt])
    sids = torch.from_numpy(sid_h).to(DEV)
    for mk in (None, mask):
        xm = x.copy()
        if mk is not None:
            xm[:, lo:lo + mk.shape[1]][mk == 0] = -np.inf
        lgm = torch.from_numpy(xm).to(DEV).to(C.TD[dt])
        mk_dev = None if mk is None else torch.from_numpy(mk).to(DEV)
        for kw in MODES:
            for env_step, i in ((0, 0), (7, 2)):
                o = Out(M, 3, env_step, i).call(lg, V=V, act_lo=lo, act_hi=hi, mask=mk_dev, num_bins=hi - lo, seed=C.SEED, step_base=C.STEP_BASE,
                                                stream_id=sids, **kw)
                ref_tok, ref_st = _select_tokens_ref(lg, lgm, lo, hi, V, A.step_of(C.STEP_BASE, env_step, 3, i), sids, kw)
                tok, status = o.ids.np()[:, 2], o.status.np()
                assert (tok == ref_tok).all(), (mk is not None, kw, env_step, i, np.nonzero(tok != ref_tok))
                assert np.array_equal(status, ref_st & 1) and (o.bins.np()[:, i] == tok - lo).all() and ((tok >= lo) & (tok < hi)).all()
                o.intact()
                if not kw["greedy"] and kw["top_k"] != 5 and mk is None:       # (the kept sets are wide: the draws spread over the window)
                    assert len(np.unique(tok)) > M // 2
