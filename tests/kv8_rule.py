"""The fp8 K/V ring format of include/db1_hip.h ("fp8 K/V ring") restated in NumPy, with its own e4m3 rounding in integer steps (no torch, no
library): the scale rule, the payload rule, the slot layout, and -- for the probes of tests/attn_probe.py -- rings with CRAFTED scales and the
scale mutants of the closed form that tests/test_kv8_rule_cpu.py proves detectable.

Slot (one key position of one batch row): H * 128 bytes of K payload, H * 128 bytes of V payload, H fp32 K scales, H fp32 V scales = 264 H bytes.
Scale of a block (the 128 elements of one (row, position, K or V, head)): amax = the largest magnitude among its finite elements; s = the
smallest power of two with amax <= 448 s; amax == 0 gives s = 1; the exponent of s is at least -126.
Payload = rne_e4m3(x / s) (OCP e4m3fn: 1-4-3, bias 7, largest finite 448, NaN = 0x7f / 0xff); a non-finite element is stored as 0x7f and takes no
part in amax.  Dequantised value = payload * s."""
import numpy as np

import attn_probe as A

D = 128
E4M3_MAX = 448.0
NAN_BYTE = 0x7F


def slot_bytes(H):
    return 264 * H


# ------------------------------------------------------------------------------------------------------------------ the number format
def e4m3_value(b):
    """the value of every byte of ``b`` (uint8) as float64; 0x7f / 0xff are NaN"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2((e - 10).astype(np.float64)))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(b & 0x80, -mag, mag)


def rne_e4m3(y):
    """round to nearest even e4m3 byte (uint8) of finite ``y`` with |y| <= 448: the spacing is 2^-9 below 2^-6 (subnormals) and
    2^(e - 3) in the binade 2^e; the tie rule is that of np.rint"""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    assert np.isfinite(a).all() and (a <= E4M3_MAX).all()
    _, ex = np.frexp(a)                                  # a = m 2^ex, m in [0.5, 1): binade e = ex - 1
    e = np.maximum(ex - 1, -6)                           # (-6: the subnormal spacing is the first normal binade's)
    q = np.rint(a / np.exp2((e - 3).astype(np.float64))).astype(np.int64)   # in units of the spacing: 0 .. 16
    byte = np.where(q < 8, q, ((e + 7) << 3) + (q - 8))  # (q == 16 carries into the next binade by itself: (e + 7) * 8 + 8)
    return (byte | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the rule
def scale_exponent(amax):
    """the exponent of the canonical scale of blocks with largest finite magnitude ``amax``"""
    amax = np.asarray(amax, np.float64)
    m, ex = np.frexp(amax)                               # 448 = 0.875 * 2^9
    e = np.where(m > 0.875, ex - 8, ex - 9)
    return np.where(amax == 0, 0, np.maximum(e, -126)).astype(np.int64)


def quantize(x, scales=None):
    """x [..., 128] (bf16 values as floats) -> (payload uint8 [..., 128], scales float32 [...]).  ``scales``: use these (powers of two)
    instead of the canonical ones"""
    x = np.asarray(x, np.float64)
    fin = np.isfinite(x)
    xf = np.where(fin, x, 0.0)
    if scales is None:
        s = np.exp2(scale_exponent(np.abs(xf).max(-1)).astype(np.float64))
    else:
        s = np.broadcast_to(np.asarray(scales, np.float64), x.shape[:-1])
    pay = rne_e4m3(xf / s[..., None])
    return np.where(fin, pay, NAN_BYTE).astype(np.uint8), s.astype(np.float32)


def dequantize(payload, scales):
    return e4m3_value(payload) * np.asarray(scales, np.float64)[..., None]


def pack(kv, scales=None):
    """kv [..., 2, H, 128] -> slots uint8 [..., 264 H]"""
    kv = np.asarray(kv, np.float64)
    H, lead = kv.shape[-2], kv.shape[:-3]
    pay, s = quantize(kv, scales)
    return np.concatenate([pay.reshape(lead + (2 * H * D,)), np.ascontiguousarray(s.reshape(lead + (2 * H,))).view(np.uint8).reshape(lead + (8 * H,))], -1)


def unpack(slots, H):
    """slots uint8 [..., 264 H] -> (payload uint8 [..., 2, H, 128], scales float32 [..., 2, H])"""
    slots = np.ascontiguousarray(slots, np.uint8)
    lead = slots.shape[:-1]
    assert slots.shape[-1] == slot_bytes(H)
    pay = slots[..., :2 * H * D].reshape(lead + (2, H, D))
    s = np.ascontiguousarray(slots[..., 2 * H * D:]).view(np.float32).reshape(lead + (2, H))
    return pay, s


# ------------------------------------------------------------------------------------------------------------------ probes with crafted scales
K_CANON, V_CANON = 2.0 ** -4, 2.0 ** -8     # the canonical scales of the probes' keys (one-hot 16) and values (largest entry 1)
SCALE_MUTANTS = ("head+1", "row+1", "k_for_v", "v_for_k", "ignored")


def crafted_multipliers(cap, seed=0):
    """[B, cap, 2, H]: a multiplier from {1, 2, 4, 8} for every block of a probe ring, seeded, such that the ring row behind a row (cyclically)
    and the other head always carry another one -- so that a scale taken from the wrong row or head is a wrong scale.  (K's and V's scales
    differ by construction: K_CANON * {1 .. 8} and V_CANON * {1 .. 8} do not meet.)"""
    rng = np.random.default_rng([seed, cap, 88])
    step = rng.integers(1, 4, (A.B, cap, 2))                               # row r + 1 differs from row r ...
    for b in range(A.B if cap > 1 else 0):
        for kv in range(2):
            while step[b, 1:, kv].sum() % 4 == 0:                           # ... and row 0 from row cap - 1
                step[b, 1, kv] = step[b, 1, kv] % 3 + 1
    t = np.cumsum(step, 1)
    head = rng.integers(1, 4, (A.B, 1, 2, 1)) * (np.arange(A.H) % 2)        # ... and head h + 1 from head h
    return np.exp2(((t[..., None] + head) % 4).astype(np.float64))


def crafted_scales(cap, seed=0):
    """[B, cap, 2, H]: the scale of every block of a probe ring: {1, 2, 4, 8} x the canonical scale of a probe key / value"""
    return crafted_multipliers(cap, seed) * np.array([K_CANON, V_CANON])[None, None, :, None]


def ring_seen(p, ring0, scales, start, mutant=None):
    """the probe as a kernel sees it over the ring ``ring0`` [B, cap, 2, H, D] packed under ``scales`` [B, cap, 2, H]: the memory keys / values
    dequantised -- with the scale a kernel under ``mutant`` would use -- and the call's own rows as they are.
        head+1    the scale of head h + 1          row+1     the scale of ring row r + 1
        k_for_v   K's scale used for V             v_for_k   V's scale used for K          ignored   no scale at all"""
    mlen, cap = p["mlen"], ring0.shape[1]
    rows = A.ring_rows(start, 0, mlen, cap)
    pay = e4m3_value(quantize(ring0, scales)[0])
    s = np.asarray(scales, np.float64)
    if mutant == "head+1":
        s = np.roll(s, -1, axis=3)
    elif mutant == "row+1":
        s = np.roll(s, -1, axis=1)
    elif mutant == "k_for_v":
        s = s[:, :, [0, 0]]
    elif mutant == "v_for_k":
        s = s[:, :, [1, 1]]
    elif mutant == "ignored":
        s = np.ones_like(s)
    elif mutant is not None:
        raise KeyError(mutant)
    deq = pay * s[..., None]
    seen = dict(p)
    seen["k"] = np.concatenate([deq[:, rows, 0], p["k"][:, mlen:]], 1)
    seen["v"] = np.concatenate([deq[:, rows, 1], p["v"][:, mlen:]], 1)
    return seen
