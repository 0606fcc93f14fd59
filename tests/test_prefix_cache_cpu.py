"""The prefix cache without a device: the fork rule (tests/ring_fork_rule.py) against a second formulation -- bf16: unpack the base window,
concatenate, keep the last mlen rows, roll them to the origin; fp8: byte moves of the base slots plus ``pack`` of the call's rows -- on
q <, ==, > mlen, wrapping origins on both rings, cap_base != cap_dst, repeated sources and every status bit; the ring-memory rule of the
attention; the host refusals of RingPrefill(base=...), Prefixed, PrefixCache's free list; the VQA helpers; the prototypes.  No GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kv8_rule as K8  # noqa: E402
import ring_fork_rule as RF  # noqa: E402

H, D = 2, 128
MLEN, CAP, M, CAP_BASE, M_BASE = 12, 20, 5, 17, 3


def _bf16_values(rng, *shape):
    """random bf16 values as float32 (the low 16 bits cleared)"""
    a = rng.standard_normal(shape).astype(np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _rings(rng, fp8):
    """(a destination ring holding a pattern, a base ring whose every slot holds data)"""
    kv = _bf16_values(rng, M_BASE, CAP_BASE, 2, H, D)
    if fp8:
        return np.full((M, CAP, K8.slot_bytes(H)), 0x5A, np.uint8), K8.pack(kv * np.float32(0.25))
    return np.full((M, CAP, 2, H, D), np.float32(-7.5), np.float32), kv


def _second_way(ring, base, new_kv, mlen, origin, origin_base, rows, src, base_rows, fp8):
    """the same result from whole-array operations: the base row's window, cat, the last mlen rows, one roll"""
    out = np.array(ring, copy=True)
    M_, cap = ring.shape[:2]
    Mb, capb = base.shape[:2]
    n_src, q = new_kv.shape[:2]
    status = 0
    for i, row in enumerate(rows):
        s = i if src is None else src[i]
        bad = (0 if 0 <= row < M_ else 1) | (0 if 0 <= origin < cap else 2) | (0 if 0 <= s < n_src else 4)
        r = None if bad & 4 else (s if base_rows is None else base_rows[s])
        bad |= 8 if (r is not None and not 0 <= r < Mb) or not 0 <= origin_base < capb else 0
        status |= bad
        if bad:
            continue
        window = np.roll(base[r], -origin_base, 0)[:mlen]                 # the memory, linear: slots origin_base .. + mlen - 1 (mod cap_base)
        enc = K8.pack(new_kv[s]) if fp8 else new_kv[s]                    # fp8: the call's rows packed, the memory's slots moved as bytes
        last = np.concatenate([window, enc], 0)[-mlen:]
        out[row, (origin + np.arange(mlen)) % cap] = last
    return out, status


CASES = [
    # (q, origin, origin_base, rows, src, base_rows, the status expected)
    (5, 0, 0, [3, 1], None, [2, 0], 0),                         # q < mlen
    (MLEN, 0, 3, [0, 4], None, [1, 1], 0),                      # q == mlen: everything from the call
    (17, 3, 16, [2, 0], None, None, 0),                         # q > mlen; base_rows None: the identity
    (5, 15, 11, [3, 1], None, [0, 2], 0),                       # both windows wrap: 15 + 12 > 20, 11 + 12 > 17
    (1, 19, 16, [4, 2], None, [1, 1], 0),                       # one new row, both wrapping, one base row shared
    (7, 9, 9, [0, 1, 2, 3], [0, 0, 1, 1], [2, 2], 0),           # repeated sources over a repeated base row
    (7, 9, 9, [0, 9, 2, -1], [1, 0, 1, 0], [0, 1], 1),          # rows outside [0, M): bit 0
    (7, CAP, 9, [0, 1], None, [0, 1], 2),                       # the origin outside [0, cap): bit 1, nothing written
    (7, 9, 9, [0, 1, 2], [1, 2, -1], [0, 1], 4),                # sources outside [0, n_src): bit 2
    (7, 9, 9, [0, 1], None, [M_BASE, 1], 8),                    # a base row outside [0, M_base): bit 3, that destination skipped
    (7, 9, 9, [0, 1], None, [-1, -1], 8),
    (7, 9, CAP_BASE, [0, 1], None, [0, 1], 8),                  # the base origin outside [0, cap_base): bit 3, nothing written
    (7, -1, -1, [M, 1], [0, 5], [0, 7], 15),
]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("q,origin,origin_base,rows,src,base_rows,expect", CASES)
def test_fork_rule_against_the_second_formulation(q, origin, origin_base, rows, src, base_rows, expect, fp8):
    rng = np.random.default_rng([q, origin % 97, origin_base % 97, len(rows)])
    new_kv = _bf16_values(rng, 2, q, 2, H, D) * np.float32(8.0)
    ring, base = _rings(rng, fp8)
    base0 = base.copy()
    got, st = RF.fork_rows(ring, base, new_kv, MLEN, origin, origin_base, rows, src, base_rows, fp8=fp8)
    want, st2 = _second_way(ring, base, new_kv, MLEN, origin, origin_base, rows, src, base_rows, fp8)
    assert st == st2 == expect and np.array_equal(got, want)
    assert np.array_equal(base, base0)
    written = [(i, r) for i, r in enumerate(rows) if expect == 0 or (0 <= r < M and 0 <= origin < CAP and 0 <= origin_base < CAP_BASE and
                                                                      0 <= (i if src is None else src[i]) < 2 and
                                                                      0 <= base_rows[i if src is None else src[i]] < M_BASE)]
    keep = np.ones((M, CAP), bool)
    for _, r in written:
        keep[r, (origin + np.arange(MLEN)) % CAP] = False
    assert np.array_equal(got[keep], ring[keep])
    assert bool(written) == (not np.array_equal(got, ring))
    if fp8 and q < MLEN:      # the memory's slots stay byte-identical: nothing is requantised
        for i, r in written:
            s = i if src is None else src[i]
            b = s if base_rows is None else base_rows[s]
            assert np.array_equal(got[r, (origin + np.arange(MLEN - q)) % CAP], base[b, (origin_base + q + np.arange(MLEN - q)) % CAP_BASE])


def test_fork_keeps_fp8_slots_that_requantising_would_change():
    """a base slot whose scale is not the canonical one (a crafted, larger power of two) dequantises to values a fresh ``pack`` would give
    another scale: the fork must move its bytes"""
    rng = np.random.default_rng(4)
    kv = _bf16_values(rng, M_BASE, CAP_BASE, 2, H, D)
    scales = np.exp2(K8.scale_exponent(np.abs(kv).max(-1)) + 2.0)
    base = K8.pack(kv, scales)
    assert not np.array_equal(base, K8.pack(K8.dequantize(*K8.unpack(base, H))))
    ring = np.full((M, CAP, K8.slot_bytes(H)), 0x5A, np.uint8)
    got, st = RF.fork_rows(ring, base, _bf16_values(rng, 1, 4, 2, H, D), MLEN, 18, 13, [2], None, [1], fp8=True)
    assert st == 0 and np.array_equal(got[2, (18 + np.arange(MLEN - 4)) % CAP], base[1, (13 + 4 + np.arange(MLEN - 4)) % CAP_BASE])


def test_the_forked_window_is_the_last_mlen_rows():
    q, origin, origin_base = 5, 15, 11
    base = np.full((M_BASE, CAP_BASE, 2, H, D), -1.0, np.float32)
    base[1, (origin_base + np.arange(MLEN)) % CAP_BASE] = np.arange(MLEN, dtype=np.float32).reshape(MLEN, 1, 1, 1)
    new = (100 + np.arange(q, dtype=np.float32)).reshape(1, q, 1, 1, 1) * np.ones((1, 1, 2, H, D), np.float32)
    got, st = RF.fork_rows(np.full((1, CAP, 2, H, D), -2.0, np.float32), base, new, MLEN, origin, origin_base, [0], None, [1])
    assert st == 0
    assert [got[0, (origin + j) % CAP, 0, 0, 0] for j in range(MLEN)] == [float(v) for v in range(q, MLEN)] + [100.0 + v for v in range(q)]


@pytest.mark.parametrize("fp8", [False, True])
def test_ring_memory_rule(fp8):
    rng = np.random.default_rng(9)
    _, base = _rings(rng, fp8)
    val = K8.dequantize(*K8.unpack(base, H)) if fp8 else base
    mem, st = RF.ring_memory(base, MLEN, 11, [2, 2, 0], fp8=fp8, H=H)
    assert st == 0 and mem.shape == (3, MLEN, 2, H, D)
    for b, r in enumerate([2, 2, 0]):
        for j in (0, 5, 6, MLEN - 1):                       # (11 + 6 = 17 wraps to slot 0)
            assert np.array_equal(mem[b, j], val[r, (11 + j) % CAP_BASE])
    ident, st = RF.ring_memory(base, MLEN, 0, None, B=2, fp8=fp8, H=H)
    assert st == 0 and np.array_equal(ident, val[:2, :MLEN])
    # the guard: clamped to row 0 / origin 0, bit 3
    g, st = RF.ring_memory(base, MLEN, 11, [1, M_BASE], fp8=fp8, H=H)
    assert st == 8 and np.array_equal(g[1], mem[2]) and np.array_equal(g[0, 0], val[1, 11])          # (mem[2] is row 0's window)
    g, st = RF.ring_memory(base, MLEN, CAP_BASE, [1], fp8=fp8, H=H)
    assert st == 8 and np.array_equal(g[0], val[1, :MLEN])


# ------------------------------------------------------------------------------------------------------------------ host refusals
def _fake_ring(model, B=4, kv_dtype="bf16"):
    torch = pytest.importorskip("torch")
    from bdm_db1_amd.decode import RingMemory
    ring = object.__new__(RingMemory)           # (no device: the attributes RingPrefill's host checks read)
    ring.B, ring.model, ring.state, ring.kv_dtype = B, model, torch.zeros(1, dtype=torch.int32), kv_dtype
    return ring


def test_ring_prefill_base_refusals():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd.decode import RingPrefill
    model = SimpleNamespace(dev=torch.device("cpu"))
    ring, base, base8, other = _fake_ring(model), _fake_ring(model, 3), _fake_ring(model, 3, "fp8"), _fake_ring(SimpleNamespace(dev=torch.device("cpu")), 3)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    ok = RingPrefill(ring, i32(3, 1), None, base, i32(2, 2))
    assert ok.base is base and ok.base_rows.tolist() == [2, 2] and ok.n_dst == 2
    plain = RingPrefill(ring, i32(3, 1))
    assert plain.base is None and plain.base_rows is None          # (with base=None nothing changes)
    for bad in (dict(base=ring), dict(base="ring"), dict(base=base8), dict(base=other), dict(base_rows=i32(0, 1)), dict(base=base, base_rows=[0, 1]),
                dict(base=base, base_rows=torch.tensor([0, 1])), dict(base=base, base_rows=i32(0, 1).view(1, 2)), dict(base=base, base_rows=i32(0, 1, 2, 3)[::2])):
        with pytest.raises(ValueError):
            RingPrefill(ring, i32(3, 1), None, **bad)
    ok.check_batch(2)
    with pytest.raises(ValueError):
        ok.check_batch(3)                       # base_rows holds two entries
    ident = RingPrefill(ring, None, i32(0, 0, 1, 2), base)
    ident.check_batch(3)
    with pytest.raises(ValueError):
        ident.check_batch(4)                    # the identity needs base.B >= the call's rows


def _fake_model(**kw):
    return SimpleNamespace(**dict(dict(ring_prefill_supported=True, _wversion=0, total_vocab_size=100), **kw))


def _nlp(G, L):
    torch = pytest.importorskip("torch")
    from bdm_db1_amd.data import NLPTaskInput
    return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=torch.zeros(G, L, dtype=torch.long))


def test_prefix_cache_free_list():
    pytest.importorskip("torch")
    from bdm_db1_amd.generation import PrefixCache, PrefixHandle
    model = _fake_model()
    cache = PrefixCache(model, 4, kv_cache="fp8")
    assert cache.free == 4 and cache.rows == 4 and cache.kv_cache == "fp8"
    a = cache._take(3)
    assert [h.row for h in a] == [0, 1, 2] and cache.free == 1 and cache.rows_of([a[1], a[1], a[0]]) == [1, 1, 0]
    with pytest.raises(RuntimeError):
        cache._take(2)                          # fewer than G rows are free ...
    assert cache.free == 1                      # ... and nothing was taken
    cache.release([a[1]])
    assert cache.free == 2
    with pytest.raises(RuntimeError):
        cache.rows_of([a[1]])                   # a released handle
    with pytest.raises(RuntimeError):
        cache.release([a[1]])
    with pytest.raises(RuntimeError):
        cache.release([a[0], a[0]])
    b = cache._take(2)
    assert [h.row for h in b] == [1, 3] and b[0] != a[1]
    with pytest.raises(RuntimeError):
        cache.rows_of([a[1]])                   # the row's earlier tenant
    with pytest.raises(ValueError):
        cache.rows_of([1])
    with pytest.raises(RuntimeError):
        PrefixCache(model, 4).release([a[0]])   # another cache's handle
    model._wversion = 1
    with pytest.raises(RuntimeError):
        cache.rows_of([a[0]])                   # a handle from before a weight change
    cache.release(a[:1] + a[2:] + b)
    assert cache.free == 4 and cache.rows_of([]) == []
    assert isinstance(cache._take(1)[0], PrefixHandle) and cache.rows_of(cache._take(1)) == [1]
    for bad in (dict(rows=0), dict(rows=True), dict(rows=2.0), dict(kv_cache="fp16")):
        with pytest.raises(ValueError):
            PrefixCache(model, **dict(dict(rows=2), **bad))
    with pytest.raises(ValueError):
        PrefixCache(_fake_model(ring_prefill_supported=False), 2)     # (an fp32 model, no use_decode, pre-LN, no memory)


def test_prefixed_refusals():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd import generation as G
    from bdm_db1_amd import scoring, serving
    model = _fake_model(compute_dtype=torch.bfloat16, use_decode=True, mem_len=40, d_head=128, ring_prefill_ok=lambda L: L <= 100)
    cache = G.PrefixCache(model, 4)
    h = cache._take(2)
    p = G.Prefixed(cache, [h[0], h[0], h[1]], _nlp(3, 7))
    assert p.suffix_len == 7 and G._batch_size(p, prefixed_ok=True) == 3
    for bad in (dict(cache="cache"), dict(handles=h), dict(suffix=_nlp(3, 0)), dict(suffix=torch.zeros(3, 7)), dict(handles=[0, 1, 2])):
        with pytest.raises(ValueError):
            G.Prefixed(**dict(dict(cache=cache, handles=[h[0], h[0], h[1]], suffix=_nlp(3, 7)), **bad))
    with pytest.raises(ValueError):
        G._batch_size(p)                                        # rank_candidates' and PrefixCache.put's own first step
    with pytest.raises(ValueError):
        scoring.rank_candidates(model, p, [[1, 2]])
    with pytest.raises(ValueError):
        scoring.score_document(model, p)
    G._check_prompt("generate", model, p, "bf16", None)
    G._check_prompt("generate", model, _nlp(3, 7), "fp8", False)       # (a plain prompt is not looked at)
    for bad in (dict(kv_cache="fp8"), dict(graphed=False), dict(model=_fake_model()),
                dict(model=_fake_model(compute_dtype=torch.float32, use_decode=True, mem_len=40, d_head=128))):
        args = dict(dict(model=model, kv_cache="bf16", graphed=None), **bad)
        with pytest.raises(ValueError):
            G._check_prompt("generate", args["model"], p, args["kv_cache"], args["graphed"])
    with pytest.raises(ValueError):
        G._check_prompt("generate", model, G.Prefixed(cache, h, _nlp(2, 101)), "bf16", None)      # a suffix the ring prefill does not take
    cache.release(h[1:])
    with pytest.raises(RuntimeError):
        G._check_prompt("generate", model, p, "bf16", None)
    # the stream's request list: a shape key per (cache, suffix length), the check applied per Prefixed prompt
    cfg = G.GenerationConfig(max_new_tokens=4)
    q = G.Prefixed(cache, [h[0]], _nlp(1, 7))
    q2, other = G.Prefixed(cache, [h[0]] * 2, _nlp(2, 9)), G.Prefixed(G.PrefixCache(model, 2), [], _nlp(0, 7))
    assert serving._shape_key(q) == serving._shape_key(G.Prefixed(cache, [h[0]] * 2, _nlp(2, 7))) != serving._shape_key(q2)
    assert serving._shape_key(q)[:1] == serving._shape_key(other)[:1] and serving._shape_key(q) != serving._shape_key(other)
    seen = []
    reqs = list(serving._requests([q, _nlp(2, 7), (q2, 3)], cfg, check_prefixed=seen.append))
    assert [r.index for r in reqs] == [0, 1, 2, 3, 4] and seen == [q, q2] and reqs[0].key == serving._shape_key(q) != reqs[1].key
    g = serving._gather([reqs[4], reqs[3]])
    assert isinstance(g, G.Prefixed) and g.handles == [h[0], h[0]] and tuple(g.suffix.text_seq.shape) == (2, 9)


def test_vqa_helpers():
    torch = pytest.importorskip("torch")
    from bdm_db1_amd import generation as G
    from bdm_db1_amd.data import VQATaskInput
    text = torch.arange(4 * 6).view(4, 6)
    vqa = VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=torch.ones(4, 2, dtype=torch.long),
                       img_seq=torch.zeros(4, 3, 32, 32), text_seq=text, ques_len=torch.tensor([3, 5, 3, 1]))
    pre = G.image_prefix(vqa)
    assert type(pre).__name__ == "ICTaskInput" and tuple(pre.text_seq.shape) == (4, 0) and pre.prompt_seq is vqa.prompt_seq and pre.img_seq is vqa.img_seq
    suf = G.question_suffixes(vqa)
    prompts = G.question_prompts(vqa)
    assert [tuple(s.text_seq.shape) for s, _ in suf] == [(1, 1), (2, 3), (1, 5)]
    for (s, rows), (p, prows) in zip(suf, prompts):          # the grouping, and the question tokens, of question_prompts
        assert type(s).__name__ == "NLPTaskInput" and np.array_equal(rows, prows) and torch.equal(s.text_seq, p.text_seq)
    vqa.ques_len = torch.tensor([3, 0, 3, 1])
    with pytest.raises(ValueError):
        G.question_suffixes(vqa)
    with pytest.raises(TypeError):
        G.image_prefix(_nlp(2, 3))


def test_exports_and_prototypes():
    import bdm_db1_amd as pkg
    from bdm_db1_amd import generation, lib
    for n in ("PrefixCache", "Prefixed", "image_prefix", "question_suffixes"):
        assert n in pkg.__all__ and getattr(pkg, n) is getattr(generation, n)
    names = lib.declared_symbols()
    for n in ("db1_relattn_mem_ring_supported", "db1_relattn_mem_ring_workspace_bytes", "db1_relattn_mem_ring_fwd", "db1_ring_fork_rows_supported",
              "db1_ring_fork_rows"):
        assert n in names
    protos = lib.parse_header()
    # the ring attention: db1_relattn_mem_kv_fwd's arguments with (k_mem, v_mem, 2 strides) replaced by the seven of the issue's list
    assert len(protos["db1_relattn_mem_ring_fwd"][1]) == len(protos["db1_relattn_mem_kv_fwd"][1]) - 4 + 7
    assert len(protos["db1_ring_fork_rows"][1]) == 24 and len(protos["db1_ring_fork_rows_supported"][1]) == 7
    assert len(protos["db1_relattn_mem_ring_supported"][1]) == 9
