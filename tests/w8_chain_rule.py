"""The lane, piece and scale map of the fp8 persistent chain (include/db1_hip.h, "fp8 weights in the persistent chain") restated in NumPy
(no torch, no library), and the index-revealing weights of its kernel tests.

A worker wave holds one row of a packed [N, K] weight (tests/w8_rule.py: N K payload bytes, then N K / 128 fp32 scales).  Piece j
(0 .. K / 512 - 1) of the row for lane l (0 .. 63) is columns (64 j + l) 8 .. + 7, i.e. the 8 payload bytes at row K + (64 j + l) 8; the
piece's scale is block (64 j + l) >> 4 = 4 j + l // 16 of the row."""
import numpy as np

BLOCK = 128
LANES = 64


def pieces(K):
    assert K % (LANES * 8) == 0
    return K // (LANES * 8)


def piece_columns(K):
    """[pieces, 64, 8]: the columns of piece j for lane l"""
    j, l, e = np.meshgrid(np.arange(pieces(K)), np.arange(LANES), np.arange(8), indexing="ij")
    return (64 * j + l) * 8 + e


def piece_payload_offset(K, row):
    """[pieces, 64]: the byte offset of piece j of ``row`` for lane l inside the packed buffer"""
    j, l = np.meshgrid(np.arange(pieces(K)), np.arange(LANES), indexing="ij")
    return row * K + (64 * j + l) * 8


def piece_block(K):
    """[pieces, 64]: the scale block of piece j for lane l, as the header states it"""
    j, l = np.meshgrid(np.arange(pieces(K)), np.arange(LANES), indexing="ij")
    b = (64 * j + l) >> 4
    assert (b == 4 * j + l // 16).all()
    return b


def piece_scale_offset(N, K, row):
    """[pieces, 64]: the byte offset of that scale inside the packed buffer"""
    return N * K + 4 * (row * (K // BLOCK) + piece_block(K))


def scale_exponent(N, K):
    """[N, K / 128]: e(row, block) = (3 row + 5 block) % 7 - 3 of the kernel tests' weights"""
    n, b = np.arange(N)[:, None], np.arange(K // BLOCK)[None, :]
    return (3 * n + 5 * b) % 7 - 3


def revealing_factor(N, K):
    """[N, K] float64: 2^e(row, block) per element -- times 0.02 randn these are the index-revealing weights: no two neighbouring rows share
    an exponent, nor two neighbouring blocks of a row, nor (N = 2 * 4096 GEGLU rows) a value row and its gate row (3 * 4096 % 7 = 3)"""
    return np.repeat(np.exp2(scale_exponent(N, K).astype(np.float64)), BLOCK, axis=1)
