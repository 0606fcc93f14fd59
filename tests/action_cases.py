"""The seeded inputs of the db1_select_actions kernel test (tests/test_action_kernels_gpu.py), made on the host so that the CPU suite
(tests/test_action_cpu.py) can hold the ambiguity cap on exactly the rows the GPU test draws from."""
import numpy as np
import torch

# (V, act_lo, act_hi): a small vocabulary; DB1's continuous bins behind the text ids (overlapping discrete ids) and its discrete ids; the
# bins of a vocabulary whose discrete ids do not overlap the text ids (the window starts inside a 1024-column block: two blocks)
WINDOWS = [(200, 150, 199), (33025, 32000, 33024), (33025, 0, 6), (34049, 33024, 34048)]
ROWS = [1, 3, 64]
DTYPES = ["f32", "bf16"]
STEPS = [(1, 0), (3, 0), (3, 1), (3, 2)]          # (act_len, i)
SAMPLING = dict(greedy=False, temperature=0.7, top_k=5, top_p=0.9)
SEED, STEP_BASE, ENV_STEP = 0x5EED_AC71_0115, 11, 2
TD = {"f32": torch.float32, "bf16": torch.bfloat16}


def ld_of(V):
    return V + (64 - V % 64) % 64 + 64


def n_mask_of(lo, hi):
    """the mask covers the whole window where that is small, and all but its last 5 columns else"""
    return hi - lo if hi - lo <= 64 else hi - lo - 5


def make(V, lo, hi, M, dt):
    """-> (x float32 [M, ld] as the dtype rounds it, mask uint8 [M, n_mask], stream ids int32 [M]).  Every row: the window's maximum planted
    three times (the lowest column must win), a NaN, a +inf and a -inf inside the window, columns outside the window and the padding far
    above it (a pick from there is caught); with M >= 3 row 1 has no allowed column that is finite"""
    rng = np.random.default_rng(V * 131 + lo * 7 + M)
    ld, w = ld_of(V), hi - lo
    x = np.full((M, ld), 1e4, np.float32)
    x[:, :V] = rng.standard_normal((M, V)).astype(np.float32) * 3.0
    x[:, :lo] += 50.0
    x[:, hi:V] += 50.0
    for r in range(M):
        c = lo + rng.choice(w, size=min(3, w), replace=False)
        x[r, c] = x[r, lo:hi].max() + 1.0
        if w > 8:
            free = np.setdiff1d(np.arange(lo, hi), c)
            odd = rng.choice(free, size=3, replace=False)
            x[r, odd] = [np.nan, np.inf, -np.inf]
    n_mask = n_mask_of(lo, hi)
    mask = (rng.random((M, n_mask)) < 0.7).astype(np.uint8)
    if M >= 3:
        mask[1] = 0
        x[1, lo + n_mask:hi] = -np.inf
    x = torch.from_numpy(x).to(TD[dt]).float().numpy()          # (the values the kernel reads)
    sids = rng.integers(0, 2 ** 31, M).astype(np.int32)
    return x, mask, sids
