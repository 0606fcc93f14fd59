"""score_document on the host: the segmentation (a pure function) and every refusal, all of which happen before anything is launched --
the model here is a plain namespace without a device."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch = pytest.importorskip("torch")

from bdm_db1_amd import document_segments, score_document  # noqa: E402


def _covers(segs, n):
    assert segs[0][0] == 0 and segs[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
    assert all(e - b >= 2 for b, e in segs)                      # a 1-token call raises for models without same_length


def test_document_segments():
    assert document_segments(48, 24) == [(0, 24), (24, 48)]                              # remainder 0
    assert document_segments(49, 24) == [(0, 24), (24, 47), (47, 49)]                    # remainder 1: one position from the segment before
    assert document_segments(59, 24) == [(0, 24), (24, 48), (48, 59)]                    # remainder > 1
    assert document_segments(10, 24) == [(0, 10)]                                        # n < segment_len
    assert document_segments(24, 24) == [(0, 24)]
    assert document_segments(25, 24) == [(0, 23), (23, 25)]                              # n == segment_len + 1
    assert document_segments(4096, 1024) == [(i, i + 1024) for i in range(0, 4096, 1024)]
    assert document_segments(5, 2) == [(0, 2), (2, 5)] and document_segments(3, 2) == [(0, 3)]   # nothing to take from a 2-position segment: joined
    for n in range(2, 80):
        for s in range(2, 12):
            segs = document_segments(n, s)
            _covers(segs, n)
            assert all(e - b <= s + (1 if s == 2 else 0) for b, e in segs)
            assert len(segs) in (n // s, -(-n // s)) or n < s
    for bad in ((10, 1), (10, 0), (10, -3), (1, 4), (0, 4), (10.0, 4), (10, 2.5), (True, 4)):
        with pytest.raises(ValueError):
            document_segments(*bad)


def _fake(mem_len=8, dtype=torch.float32, d_head=64):
    return SimpleNamespace(mem_len=mem_len, n_position=8, compute_dtype=dtype, d_head=d_head, n_head=2, total_vocab_size=50, use_mem_attn=False,
                           training=False)


TOK = np.arange(40).reshape(2, 20) % 50


@pytest.mark.parametrize("what,kw", [
    ("ragged", dict(tokens=[[1, 2, 3, 4], [1, 2, 3]])),
    ("float tokens", dict(tokens=TOK.astype(np.float32))),
    ("one row of tokens, no batch axis", dict(tokens=TOK[0])),
    ("T < 3", dict(tokens=TOK[:, :2])),
    ("segment_len < 2", dict(tokens=TOK, segment_len=1)),
    ("lengths below 2", dict(tokens=TOK, lengths=[1, 20])),
    ("lengths above T", dict(tokens=TOK, lengths=[20, 21])),
    ("lengths of another batch", dict(tokens=TOK, lengths=[20])),
    ("float lengths", dict(tokens=TOK, lengths=[20.0, 19.0])),
    ("token outside the vocabulary", dict(tokens=TOK + 40)),
    ("fused on an fp32 model", dict(tokens=TOK, fused=True)),
    ("fused neither bool nor None", dict(tokens=TOK, fused=1)),
])
def test_refusals_before_any_launch(what, kw):
    model = _fake()
    with pytest.raises(ValueError):
        score_document(model, **kw)
    assert model.use_mem_attn is False


def test_refuses_a_model_without_memory_and_a_head_size_the_kernel_lacks():
    with pytest.raises(ValueError, match="memory"):
        score_document(_fake(mem_len=0), TOK)
    with pytest.raises(ValueError, match="fused"):
        score_document(_fake(dtype=torch.bfloat16, d_head=64), TOK, fused=True)


def test_score_result_carries_the_memory():
    import dataclasses
    from bdm_db1_amd import ScoreResult
    f = {x.name: x for x in dataclasses.fields(ScoreResult)}
    assert f["mems"].default is None
