"""The two rules of the prefix cache (include/db1_hip.h: db1_relattn_mem_ring_fwd, db1_ring_fork_rows) restated in NumPy, on top of
tests/kv8_rule.py: a memory that lives in the slots of a K/V ring -- a device-side origin, wrapping at cap, bf16 or fp8 -- read by an
attention call and forked, together with the call's new rows, into the rows of another ring.

bf16 form: a ring is [M, cap, 2, H, D] of any dtype (bit patterns or values), a slot is the (K row, V row) pair as it is.
fp8 form: a ring is uint8 [M, cap, 264 H], a slot is tests/kv8_rule.py's ``pack``; its value is payload * scale per (K | V, head) block.

``ring_memory``: logical key j < mlen of call row b is slot (origin + j) % cap of ring row base_rows[b] (None: b).  A base row outside
[0, M) is read as row 0, an origin outside [0, cap) as 0, and status bit 3 (value 8) is set.
``fork_rows``: destination i takes ring row rows[i] from call row s = src[i] (None: i) over base row r = base_rows[s] (None: s).  Logical
position j in [0, mlen) is row c = j + q of cat(memory of r, new rows of s): for c < mlen the SLOT of base slot (base origin + c) %
cap_base as it is (an fp8 slot keeps its bytes), otherwise new row c - mlen (fp8: ``pack``).  It goes to slot (origin + j) % cap.  Status:
bit 0 a row outside [0, M), bit 1 an origin outside [0, cap), bit 2 an s outside [0, n_src), bit 3 a base row outside [0, M_base) or a
base origin outside [0, cap_base); a destination with any of them is skipped.  Nothing else changes in either ring."""
import numpy as np

import kv8_rule as K8


def ring_memory(base, mlen, origin, base_rows=None, B=None, fp8=False, H=None):
    """-> (the linear memory [B, mlen, 2, H, D] -- fp8: the dequantised values, float64 --, the status word)"""
    base = np.asarray(base)
    M, cap = base.shape[0], base.shape[1]
    assert 1 <= mlen < cap
    rows = list(range(B)) if base_rows is None else [int(r) for r in base_rows]
    status = 0
    if not 0 <= origin < cap:
        origin, status = 0, 8
    out = []
    for r in rows:
        if not 0 <= r < M:
            r, status = 0, 8
        slots = base[r, (origin + np.arange(mlen)) % cap]
        out.append(K8.dequantize(*K8.unpack(slots, H)) if fp8 else slots)
    return np.stack(out), status


def fork_rows(ring, base, new_kv, mlen, origin, origin_base, rows, src=None, base_rows=None, fp8=False):
    """-> (the destination ring after the launch, the status word).  Neither ring is modified.  ``new_kv`` [n_src, q, 2, H, D] (fp8: bf16
    values held as floats), ``rows`` / ``src`` integer sequences of one length, ``base_rows`` one of length n_src."""
    ring, base, new_kv = np.array(ring, copy=True), np.asarray(base), np.asarray(new_kv)
    M, cap, M_base, cap_base = ring.shape[0], ring.shape[1], base.shape[0], base.shape[1]
    n_src, q, H = new_kv.shape[0], new_kv.shape[1], new_kv.shape[3]
    assert 1 <= mlen < cap and mlen < cap_base and q >= 1 and ring.shape[2:] == base.shape[2:] and ring.dtype == base.dtype
    if fp8:
        assert ring.dtype == np.uint8 and ring.shape[2:] == (K8.slot_bytes(H),)
    else:
        assert ring.shape[2:] == new_kv.shape[2:]
    status = 0
    for i, row in enumerate(rows):
        s = i if src is None else int(src[i])
        bad = (1 if not 0 <= row < M else 0) | (2 if not 0 <= origin < cap else 0) | (4 if not 0 <= s < n_src else 0)
        r = None
        if not bad & 4:
            r = s if base_rows is None else int(base_rows[s])
        if (r is not None and not 0 <= r < M_base) or not 0 <= origin_base < cap_base:
            bad |= 8
        if bad:
            status |= bad
            continue
        for j in range(mlen):
            c = j + q
            if c < mlen:
                slot = base[r, (origin_base + c) % cap_base]
            else:
                slot = K8.pack(new_kv[s, c - mlen]) if fp8 else new_kv[s, c - mlen]
            ring[row, (origin + j) % cap] = slot
    return ring, status
