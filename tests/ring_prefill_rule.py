"""db1_ring_prefill_rows (include/db1_hip.h, "Prefill straight into the ring") restated in NumPy: the ring slots of new tenants written from
(a K/V memory of mlen rows, a call's own q rows of K/V).

For destination i: row = rows[i], s = src[i] (src None: s = i).  Logical position j in [0, mlen) is position j of the LAST mlen rows of
cat(memory of s, new rows of s): memory row j + q while j + q < mlen, else new row j + q - mlen.  It goes to slot (origin + j) % cap of ring
row ``row``.  Status: bit 0 for a row outside [0, M) (skipped), bit 1 for an origin outside [0, cap) (nothing written), bit 2 for an s
outside [0, n_src) (skipped).  Nothing else in the ring changes.
bf16 form: the ring is [M, cap, 2, H, D] of any dtype (bit patterns or values) and the slot is the (K row, V row) pair as it is.
fp8 form: the ring is uint8 [M, cap, 264 H], the keys / values are bf16 values held as floats, the slot is tests/kv8_rule.py's ``pack``."""
import numpy as np

import kv8_rule as K8


def prefill_rows(ring, mem_kv, new_kv, mlen, origin, rows, src=None, fp8=False):
    """-> (the ring after the launch, the status word).  ``ring`` is not modified.  ``mem_kv`` [n_src or 1, mlen or 1, 2, H, D] (a dimension
    of size 1 stands for every index), ``new_kv`` [n_src, q, 2, H, D], ``rows`` / ``src`` integer sequences of one length."""
    ring = np.array(ring, copy=True)
    M, cap = ring.shape[0], ring.shape[1]
    new_kv, mem_kv = np.asarray(new_kv), np.asarray(mem_kv)
    n_src, q = new_kv.shape[0], new_kv.shape[1]
    H = new_kv.shape[3]
    assert 1 <= mlen < cap and q >= 1
    assert mem_kv.shape[0] in (1, n_src) and mem_kv.shape[1] in (1, mlen) and mem_kv.shape[2:] == new_kv.shape[2:]
    if fp8:
        assert ring.dtype == np.uint8 and ring.shape[2:] == (K8.slot_bytes(H),)
    else:
        assert ring.shape[2:] == new_kv.shape[2:]
    status = 0
    for i, row in enumerate(rows):
        s = i if src is None else int(src[i])
        bad = (1 if not 0 <= row < M else 0) | (2 if not 0 <= origin < cap else 0) | (4 if not 0 <= s < n_src else 0)
        if bad:
            status |= bad
            continue
        mem = np.broadcast_to(mem_kv[s if mem_kv.shape[0] > 1 else 0], (mlen,) + mem_kv.shape[2:])
        for j in range(mlen):
            c = j + q
            kv = mem[c] if c < mlen else new_kv[s, c - mlen]
            ring[row, (origin + j) % cap] = K8.pack(kv) if fp8 else kv
    return ring, status
