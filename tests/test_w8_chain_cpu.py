"""fp8 weights in the persistent one-token chain (include/db1_hip.h, "fp8 weights in the persistent chain") without a GPU: the prototypes, the
host wrapper's refusals before the library is touched, and the lane / piece / scale-block map the header states (tests/w8_chain_rule.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")

import w8_chain_rule as C8  # noqa: E402
import w8_rule as W8  # noqa: E402

NEW_PROTOTYPES = ("db1_decode_chain_w8_supported", "db1_decode_chain_w8")


def test_prototypes_are_declared_and_resolve():
    from bdm_db1_amd import lib
    names = lib.declared_symbols()
    for n in NEW_PROTOTYPES:
        assert n in names, n
    Lb = lib.load()
    for n in NEW_PROTOTYPES:
        assert hasattr(Lb, n), n
    # the fp8 entry point takes the bf16 entry point's argument list
    protos = lib._protos if getattr(lib, "_protos", None) else None
    if protos:
        assert protos["db1_decode_chain_w8"] == protos["db1_decode_chain"]
        assert protos["db1_decode_chain_w8_supported"] == protos["db1_decode_chain_supported"]


class _Touched(Exception):
    pass


def test_wrapper_refuses_wrong_buffers_before_the_library(monkeypatch):
    """a buffer of the wrong size, dtype or device is a ValueError and the library is not called; a well-formed call passes these checks (and, on
    host tensors, stops at the wrapper's device check of the operands -- still before the library)"""
    from bdm_db1_amd import lib, ops

    def touched(*a, **k):
        raise _Touched()
    monkeypatch.setattr(lib, "call", touched)
    monkeypatch.setattr(ops, "decode_chain_scratch", touched)
    d, dff, H = 256, 384, 2
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    buf = lambda N, K: torch.zeros(W8.nbytes(N, K), dtype=torch.uint8)
    good = dict(w_o8=buf(d, d), w1_8=buf(2 * dff, d), w2_8=buf(d, dff), w_qkv_next8=buf(3 * d, d), w_o_next=buf(d, d))
    part = torch.zeros(H, 1, 64, 130)

    def call(**over):
        a = {**good, **over}
        ops.decode_chain_w8(part, 128, H, bf(1, d), a["w_o8"], a["w1_8"], bf(2 * dff), a["w2_8"], bf(d), a["w_qkv_next8"], bf(d), bf(d), bf(d), bf(d), 1.0, 1e-5,
                            None, None, bf(1, d), bf(1, 3 * d), 0, w_o_next=a["w_o_next"])
    with pytest.raises(lib.Db1Error, match="device tensors"):
        call()
    with pytest.raises(lib.Db1Error, match="device tensors"):
        call(w_qkv_next8=None, w_o_next=None)                                   # (both are optional)
    for name, (N, K) in dict(w_o8=(d, d), w1_8=(2 * dff, d), w2_8=(d, dff), w_qkv_next8=(3 * d, d), w_o_next=(d, d)).items():
        ok = good[name]
        bad = [ok[:-4], torch.cat([ok, ok[:4]]), torch.zeros(N * K, dtype=torch.uint8),          # size: short, long, the payload alone
               ok.view(torch.int8), torch.zeros(N, K, dtype=torch.bfloat16),                     # dtype: int8, the bf16 weight itself
               torch.empty(ok.numel(), dtype=torch.uint8, device="meta"),                        # device
               ok.view(2, -1)]                                                                   # not one flat buffer
        for t in bad:
            with pytest.raises(ValueError, match=name):
                call(**{name: t})
    with pytest.raises(ValueError):
        call(w_o8=None)


@pytest.mark.parametrize("K", [2048, 4096])
def test_piece_to_block_map(K):
    """(64 j + lane) >> 4 == column // 128 for all eight columns of every piece; the pieces tile the row; the offsets are the format's"""
    cols, blk = C8.piece_columns(K), C8.piece_block(K)
    assert cols.shape == (K // 512, 64, 8) and blk.shape == (K // 512, 64)
    assert (cols // 128 == blk[..., None]).all()
    assert np.array_equal(np.sort(cols.reshape(-1)), np.arange(K))
    assert blk.max() == K // 128 - 1 and (blk == 4 * np.arange(K // 512)[:, None] + np.arange(64)[None, :] // 16).all()
    # against the packed buffer of tests/w8_rule.py: row 5 of an 8-row matrix whose payload bytes and scales number themselves
    N, row = 8, 5
    rng = np.random.default_rng(K)
    w = rng.standard_normal((N, K)) * np.exp2(rng.integers(-6, 6, (N, K // 128))).repeat(128, axis=1)
    packed = W8.pack(w)
    pay, s = W8.unpack(packed, N, K)
    off = C8.piece_payload_offset(K, row)
    assert (off % 8 == 0).all() and np.array_equal(packed[off[..., None] + np.arange(8)], pay[row][cols])
    soff = C8.piece_scale_offset(N, K, row)
    assert (soff % 4 == 0).all() and soff.max() + 4 <= packed.size
    got = np.ascontiguousarray(packed[soff[..., None] + np.arange(4)]).view(np.float32)[..., 0]
    assert np.array_equal(got, s[row][blk])


def test_revealing_exponents_differ_between_neighbours():
    for N, K, geglu in ((2048, 2048, None), (8192, 2048, 4096), (2048, 4096, None), (6144, 2048, None)):
        e = C8.scale_exponent(N, K)
        assert e.min() == -3 and e.max() == 3
        W8.assert_neighbours_differ(e, geglu_rows=geglu)
