"""ActionDecoder (bdm_db1_amd.evaluation) on the GPU: the reference's golden episode on the fp32 model; on the bf16 ring, bit for bit what
get_action_batched gives over a RingMemory of the same format (origin round the ring, a masked discrete space, the fp8 ring); eager against
replay; float observations; row resets; sampling; the existing path's bits afterwards; the refusals with the model never called."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

from gpu_common import _bf16_model, _need_gpu  # noqa: E402,F401

G = os.path.join(ROOT, "tests", "golden")
M = 3


def _args(cfg):
    g = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    return SimpleNamespace(overlap_with_text=g("overlap_with_text"), text_vocab_size=g("text_vocab_size"), num_discrete_values=g("num_discrete_values"),
                           num_continuous_bin=g("num_continuous_bin"), n_position=g("n_position"), use_prompt=False)


def _obs_tokens(rng, steps, ol, text=32000, nb=1024):
    """per step int64 [M, ol + 1]: distinct observation bins per row, then the separator"""
    return [np.concatenate([text + rng.integers(0, nb, (M, ol)), np.full((M, 1), text + nb)], axis=1).astype(np.int64) for _ in range(steps)]


def _masks(rng, steps, n):
    out = []
    for _ in range(steps):
        m = (rng.random((M, n)) < 0.5).astype(np.float64)
        m[np.arange(M), rng.integers(0, n, M)] = 1.0
        out.append(m)
    return out


def _batched_episode(args, model, obs, ol, al, disc, n_actions, masks, kv_dtype):
    """get_action_batched over a RingMemory -> per step (actions, the last tokens)"""
    from bdm_db1_amd.decode import RingMemory
    from bdm_db1_amd.evaluation import get_action_batched
    from bdm_db1_amd.tokenizer import ContinuousScalarTokenizer
    tok = ContinuousScalarTokenizer(args.num_continuous_bin)
    memory = RingMemory(model, M, kv_dtype=kv_dtype)
    space = SimpleNamespace(n=n_actions) if disc else None
    res = []
    with torch.no_grad():
        for st, o in enumerate(obs):
            acts, last, memory = get_action_batched(args, model, torch.from_numpy(o), tok, ol, al, disc, space, memory,
                                                    action_masks=None if masks is None else masks[st])
            res.append((np.array(acts), last.numpy().copy()))
    return res


@pytest.fixture(scope="module")
def bf16():
    """the bf16 ring model, and -- before any ActionDecoder exists -- what get_action_batched gives on the continuous case"""
    cfg, model = _bf16_model(mem_len=40)
    args = _args(cfg)
    obs = _obs_tokens(np.random.default_rng(31), 20, 4)
    base = {kv: _batched_episode(args, model, obs, 4, 3, False, None, None, kv) for kv in ("bf16", "fp8")}
    return SimpleNamespace(cfg=cfg, model=model, args=args, obs=obs, base=base)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_fp32_golden_episode_in_every_row():
    """the memory cases of the REFERENCE's get_action episode (tests/golden/get_action.npz) on the small_mems model, M = 3 rows: every row's
    actions and last tokens equal the reference's, the last layer's memory within 1e-4 (test_model_gpu's gate for get_action_batched)"""
    from golden_util import CASES, GET_ACTION_CASES, case_cfg, get_action_inputs, make_params
    from bdm_db1_amd import TransformerXL
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    name = "small_mems"
    cfg = case_cfg(name)
    params = make_params(cfg, 100 + list(CASES).index(name))
    params["pos_emb.inv_freq"] = np.load(os.path.join(G, f"model_{name}.npz"))["inv_freq"]
    model = TransformerXL(SimpleNamespace(**cfg), compute_dtype=torch.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    model.eval()
    gold = dict(np.load(os.path.join(G, "get_action.npz")))
    for case in ("mem_continuous", "mem_discrete_masked"):
        mem, disc, ol, al, steps, strat, use_prompt, lfp = GET_ACTION_CASES[case]
        obs, _, masks = get_action_inputs(case, cfg)
        dec = ActionDecoder(_args(cfg), model, M, ActionConfig(ol, al, disc, n_actions=6 if disc else None))
        assert not dec.replay and isinstance(dec.memory, list)
        for st in range(steps):
            am = None if masks[st] is None else np.tile(masks[st][None, :], (M, 1))
            acts = dec.act(obs_tokens=np.tile(obs[st][None, :], (M, 1)), action_masks=am)
            assert acts.dtype == (np.int64 if disc else np.float32) and acts.shape == ((M,) if disc else (M, al))
            for row in range(M):
                assert np.array_equal(np.asarray(acts[row], np.float64).reshape(-1), np.asarray(gold[f"{case}/{st}/act"], np.float64).reshape(-1)), (case, st, row)
                assert np.array_equal(dec.last_tokens[row], gold[f"{case}/{st}/seq"]), (case, st, row)
                got, ref = dec.memory[-1][row:row + 1].double().cpu().numpy(), gold[f"{case}/{st}/mem_last"].astype(np.float64)
                assert np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30) < 1e-4, (case, st, row)
        assert dec.stats == dict(env_steps=steps, replays=0, resets=0)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_continuous_actions_equal_get_action_batched_round_the_ring(bf16, kv):
    """obs_length 4, action_length 3, 20 environment steps = 160 tokens: the origin goes round the 104-slot ring"""
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(4, 3, False), kv_cache=kv)
    assert dec.replay and dec.memory.kv_dtype == kv and dec.memory.cap == 104 and dec.window == (32000, 33024)
    for st, o in enumerate(bf16.obs):
        acts = dec.act(obs_tokens=o)
        ref_acts, ref_last = bf16.base[kv][st]
        assert _same_bits(acts, ref_acts.astype(np.float32)) and ref_acts.dtype == np.float32, (kv, st)
        assert np.array_equal(dec.last_tokens, ref_last) and dec.last_bins.dtype == np.int32 and dec.last_bins.shape == (M, 3)
        assert _same_bits(acts, (dec.last_bins.astype(np.float32) / np.float32(1024) * np.float32(2) - np.float32(1)))
    assert dec.stats == dict(env_steps=20, replays=80, resets=0)
    assert int(dec.memory.state.cpu()) == 160 % 104 and dec.ctr.cpu().tolist()[0] == 20


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_masked_discrete_actions_equal_get_action_batched(bf16, kv):
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    rng = np.random.default_rng(41)
    obs, masks = _obs_tokens(rng, 6, 3), _masks(rng, 6, 6)
    masks[2] = None                     # (a step without a mask in between)
    ref = _batched_episode(bf16.args, bf16.model, obs, 3, 1, True, 6, masks, kv)
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(3, 1, True, n_actions=6), kv_cache=kv)
    seen_masked = False
    for st, o in enumerate(obs):
        acts = dec.act(obs_tokens=o, action_masks=masks[st])
        assert acts.dtype == np.int64 and np.array_equal(acts, ref[st][0]) and np.array_equal(dec.last_tokens, ref[st][1]), (kv, st)
        assert np.array_equal(dec.last_bins[:, 0], acts)
        if masks[st] is not None:
            assert (masks[st][np.arange(M), acts] == 1).all()
            seen_masked = True
    assert seen_masked
    # the mask matters: without it some step picks a forbidden action
    free = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(3, 1, True, n_actions=6), kv_cache=kv)
    hits = 0
    for st, o in enumerate(obs):
        a = free.act(obs_tokens=o)
        if masks[st] is not None:
            hits += int((masks[st][np.arange(M), a] == 0).sum())
    assert hits > 0


def test_eager_launches_give_the_replays_bits(bf16):
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(4, 3, False), graphed=False)
    assert not dec.replay and dec.ring_path
    for st, o in enumerate(bf16.obs[:14]):          # (112 tokens: once round the ring)
        acts = dec.act(obs_tokens=o)
        assert _same_bits(acts, bf16.base["bf16"][st][0].astype(np.float32)), st
    assert dec.stats == dict(env_steps=14, replays=0, resets=0)


def test_float_observations_are_tokenised_on_the_device(bf16):
    from bdm_db1_amd import ops
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    rng = np.random.default_rng(51)
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(4, 3, False))
    xs = [(rng.standard_normal((M, 4)) * np.array([0.01, 1.0, 30.0, 300.0])).astype(np.float32) for _ in range(5)]
    got = [dec.act(obs=x) for x in xs]
    dec.reset()
    for x, g in zip(xs, got):
        ids = torch.empty(M, 4, dtype=torch.int32, device=DEV)
        ops.mulaw_discretize(torch.from_numpy(x).to(DEV), ids, False, 1024)
        toks = np.concatenate([32000 + ids.cpu().numpy().astype(np.int64), np.full((M, 1), 33024)], axis=1)
        assert len(np.unique(toks[:, :4])) > 4
        assert _same_bits(dec.act(obs_tokens=toks), g)
    assert dec.stats["resets"] == 1 and dec.stats["env_steps"] == 10


def test_row_reset_leaves_the_other_rows_alone(bf16):
    """reset(rows=[1]) after step 3: from there row 1 follows a fresh decoder fed the same observations, rows 0 and 2 an undisturbed run; the
    zero memory is projected by the first row reset only"""
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    cfg, obs = ActionConfig(4, 3, False), bf16.obs[:9]
    plain = [b[0].astype(np.float32) for b in bf16.base["bf16"][:9]]          # (the undisturbed run: the continuous test pins it to the decoder)
    dec = ActionDecoder(bf16.args, bf16.model, M, cfg)
    calls = []
    project = dec.memory._project
    dec.memory._project = lambda *a, **k: (calls.append(1), project(*a, **k))[1]
    got = [dec.act(obs_tokens=o) for o in obs[:3]]
    before = [k.clone() for k in dec.memory.kv]
    dec.reset(rows=[1])
    assert len(calls) == 1
    # the ring itself: row 1's window (mem_len slots from the origin, which stays where it was) holds the zero memory's keys / values, as a
    # new RingMemory holds them from slot 0; it held something else before; every slot of rows 0 and 2 keeps its bits
    from bdm_db1_amd.decode import RingMemory
    origin, zero = int(dec.memory.state.cpu()), RingMemory(bf16.model, M)
    assert origin == 24 and int(zero.state.cpu()) == 0
    slots = (origin + torch.arange(40, device=DEV)) % dec.memory.cap
    for k, b, z in zip(dec.memory.kv, before, zero.kv):
        assert torch.equal(k[[0, 2]].view(torch.int16), b[[0, 2]].view(torch.int16))
        assert torch.equal(k[1, slots].view(torch.int16), z[1, :40].view(torch.int16)) and not torch.equal(b[1, slots], z[1, :40])
    got += [dec.act(obs_tokens=o) for o in obs[3:6]]
    dec.reset(rows=[1])                  # a second episode in the same row: no projection
    assert len(calls) == 1
    got += [dec.act(obs_tokens=o) for o in obs[6:]]
    assert dec.stats["resets"] == 2 and int(dec.memory.load_status.cpu()) == 0
    fresh = ActionDecoder(bf16.args, bf16.model, M, cfg)
    ep1 = [fresh.act(obs_tokens=o) for o in obs[3:6]]
    fresh.reset()
    ep2 = [fresh.act(obs_tokens=o) for o in obs[6:]]
    for st in range(9):
        assert _same_bits(got[st][[0, 2]], plain[st][[0, 2]]), st
        want = plain[st][1] if st < 3 else (ep1[st - 3][1] if st < 6 else ep2[st - 6][1])
        assert _same_bits(got[st][1], want), st
    with pytest.raises(ValueError, match="rows"):
        dec.reset(rows=[0, 0])
    with pytest.raises(ValueError, match="rows"):
        dec.reset(rows=[3])


def test_list_form_row_reset_zeroes_the_row():
    """graphed=False on a model without the ring (fp32): a row reset zeroes that row of the list-form memory and no other"""
    from golden_util import case_cfg, make_params
    from bdm_db1_amd import TransformerXL
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    cfg = case_cfg("small_mems")
    model = TransformerXL(SimpleNamespace(**cfg), compute_dtype=torch.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(cfg, 3).items()}, strict=False)
    model.eval()
    dec = ActionDecoder(_args(cfg), model, M, ActionConfig(4, 2, False), graphed=False)
    obs = _obs_tokens(np.random.default_rng(5), 2, 4, text=300, nb=64)
    dec.act(obs_tokens=obs[0])
    before = [m.clone() for m in dec.memory]
    dec.reset(rows=[1])
    for m, b in zip(dec.memory, before):
        assert (m[1] == 0).all() and torch.equal(m[[0, 2]], b[[0, 2]]) and b[1].abs().max() > 0
    dec.act(obs_tokens=obs[1])
    with pytest.raises(ValueError, match="graphed=True"):
        ActionDecoder(_args(cfg), model, M, ActionConfig(4, 2, False), graphed=True)
    with pytest.raises(ValueError, match="fp8"):
        ActionDecoder(_args(cfg), model, M, ActionConfig(4, 2, False), kv_cache="fp8")


def test_sampling_is_reproducible_seeded_and_inside_the_mask(bf16):
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    sample = dict(greedy=False, temperature=1.5, top_k=50, top_p=0.95)
    obs = bf16.obs[:6]
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(4, 3, False, seed=7, **sample), stream_ids=[5, 6, 7])
    a = [dec.act(obs_tokens=o) for o in obs]
    dec.reset()
    b = [dec.act(obs_tokens=o) for o in obs]
    other = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(4, 3, False, seed=8, **sample), stream_ids=[5, 6, 7])
    c = [other.act(obs_tokens=o) for o in obs]
    assert all(_same_bits(x, y) for x, y in zip(a, b)) and any(not _same_bits(x, y) for x, y in zip(a, c))
    greedy = [x[0].astype(np.float32) for x in bf16.base["bf16"][:6]]
    assert any(not _same_bits(x, y) for x, y in zip(a, greedy))
    rng = np.random.default_rng(61)
    obs3, masks = _obs_tokens(rng, 8, 3), _masks(rng, 8, 6)
    disc = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(3, 1, True, n_actions=6, greedy=False, temperature=4.0, seed=3))
    picks = []
    for o, m in zip(obs3, masks):
        acts = disc.act(obs_tokens=o, action_masks=m)
        assert (m[np.arange(M), acts] == 1).all()
        picks.append(acts)
    assert len(np.unique(np.stack(picks))) > 1


def test_refusals_come_before_the_model_is_called(bf16, monkeypatch):
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    model, args = bf16.model, bf16.args
    dec = ActionDecoder(args, model, M, ActionConfig(3, 1, True, n_actions=6))
    cont = ActionDecoder(args, model, M, ActionConfig(4, 3, False))

    def no_call(*a, **k):
        raise AssertionError("the model was called")
    monkeypatch.setattr(model, "_forward", no_call)
    ok = ActionConfig(4, 3, False)
    wide = SimpleNamespace(**{**vars(args), "num_continuous_bin": 5000})
    for kw, what in ((dict(cfg=ActionConfig(64, 3, False)), "64"), (dict(args=wide), "window"), (dict(n_envs=0), "n_envs"), (dict(n_envs=2.0), "n_envs"),
                     (dict(cfg=dict(obs_length=4)), "ActionConfig expected"), (dict(kv_cache="int8"), "kv_cache"),
                     (dict(stream_ids=[1, 2]), "stream_ids"), (dict(cfg=ActionConfig(3, 1, True, n_actions=40000)), "window")):
        a = dict(args=args, model=model, n_envs=M, cfg=ok)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            ActionDecoder(a.pop("args"), a.pop("model"), a.pop("n_envs"), a.pop("cfg"), **a)
    toks, m = np.zeros((M, 4), np.int64), np.ones((M, 6))
    for d, kw, what in ((dec, dict(), "exactly one"), (dec, dict(obs_tokens=toks, obs=np.zeros((M, 3), np.float32)), "exactly one"),
                        (dec, dict(obs_tokens=toks[:, :3]), "obs_tokens"), (dec, dict(obs_tokens=toks.astype(np.float32)), "obs_tokens"),
                        (dec, dict(obs=np.zeros((M, 4), np.float32)), "obs must"), (dec, dict(obs=np.zeros((M, 3), np.int64)), "obs must"),
                        (dec, dict(obs_tokens=toks, action_masks=m[:, :5]), "action_masks"), (dec, dict(obs_tokens=toks, action_masks=m[:2]), "action_masks"),
                        (cont, dict(obs_tokens=np.zeros((M, 5), np.int64), action_masks=m), "discrete")):
        with pytest.raises(ValueError, match=what):
            d.act(**kw)
    assert dec.stats["env_steps"] == 0 and cont.stats["env_steps"] == 0


def test_a_status_bit_raises_and_names_the_rows(bf16):
    from bdm_db1_amd.evaluation import ActionConfig, ActionDecoder
    dec = ActionDecoder(bf16.args, bf16.model, M, ActionConfig(3, 1, True, n_actions=6))
    m = np.ones((M, 6))
    m[2] = 0                              # no action allowed in row 2
    with pytest.raises(RuntimeError, match=r"\[2\]"):
        dec.act(obs_tokens=_obs_tokens(np.random.default_rng(1), 1, 3)[0], action_masks=m)
    acts = dec.act(obs_tokens=_obs_tokens(np.random.default_rng(2), 1, 3)[0])        # (the flag was cleared: the decoder goes on)
    assert acts.shape == (M,)


def test_get_action_batched_keeps_its_bits_after_all_of_this(bf16):
    again = _batched_episode(bf16.args, bf16.model, bf16.obs, 4, 3, False, None, None, "bf16")
    for (a, la), (b, lb) in zip(again, bf16.base["bf16"]):
        assert _same_bits(a, b) and np.array_equal(la, lb)
