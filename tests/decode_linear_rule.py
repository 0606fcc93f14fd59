"""The rule the fused inference linear maps (csrc/gemm_skinny.hip: db1_linear_decode, db1_linear_decode_attn) and the persistent one-token
launch (csrc/decode_chain.hip: db1_decode_chain) are tested by: probe inputs, a float64 reference written from the definition, per-element
bounds, an fp32 transcription, one-mistake mutants of the REFERENCE (never of a kernel) and the case table that the CPU proof
(test_decode_linear_rule_cpu.py) and the GPU tests (test_decode_linear_kernels_gpu.py, test_decode_chain_probe_gpu.py) share.
NumPy only: neither torch nor the library is imported here.

NO CONSTANT BELOW CAME FROM RUNNING A KERNEL UNDER TEST.  Every c is a count of fp32 roundings read from the kernel's code; the two free
constants are the project's: the fp32 transcription may use HALF of an allowance, a mutant must move an element by TEN bounds.

Designs.
  exact    gemm_probe's `dense` (x, W integers in [-3, 3], bias in [-64, 64]) and `bounded` (x rows with 32 nonzeros of +-1, W in [-2, 2], bias
           in [-32, 32]).  Every product and partial sum is an integer below 2^24 (gemm_probe.check, asserted per case up to K = 16384): the
           MFMA accumulators, the 4-wave LDS add, the split-K partial tiles and the bias add are exact in any order, a bf16 output is the
           exact value rounded ONCE.  Expected bits, zero tolerance.  dense shows a lost k-step, wave share or slice whatever M is (every
           product is nonzero with probability 36/49); bounded keeps |y| <= 96, exact in bf16, so that ONE lost product changes bits.
  geglu    bounded x scaled by 1/8 (+-1/8), W integers in [-2, 2] whose value rows n and gate rows N + n come from different seeds, biases
           k/8 with integers k in [-16, 16] from different seeds per half: z = x.W^T + b is a multiple of 1/8 with |z| <= 10, exact in fp32
           and in bf16, so the kernel's bf16 z is known on the host and the activation is defined on it.  8 z has standard deviation
           sqrt(32 * 2 + 16 * 17 / 3) = 12.4: gates have sigma 1.55, 99 % in [-4, 4] (asserted: >= 90 %, and >= 10 % on each side of 0).
  pre      res and x Gaussian bf16, alpha = 1.5: alpha * res has 10 significant bits, so alpha * res + x is ONE fp32 rounding whether or
           not the compiler contracts it, and s = bf16(fp32(alpha res + x)) is known on the host.  W rows carry 32 nonzeros of +-1 (or +-1/4
           through GEGLU, to keep the gates in range) at k = (n s + j K / 32) mod K: the transposed `bounded` pattern.  The normalised rows
           are compared with float64 LN(s); y with the float64 product over the rows AS STORED (pre_out, itself checked).
  merge    attention partials [B H][nunit][64][130], rows >= q of every unit NaN.  Per (row, head) ONE live unit (index cycling over
           (b, i, h) from slot nunit - 1 downwards, so the last slot is always live somewhere) with l a power of two and O = l * integers in [-4, 4]; the others are dead -- the producer's contract (., -1e30, 0) --
           or low (m at least 200 below the live one, l in [1, 40]), all carrying finite decoys of magnitude 64.  __expf of an argument
           <= -200 is 0 in fp32 and __expf(0) is 1, so the merged row is the integers whatever the last place of __expf or of the division
           is (a relative 1e-7 on a small integer rounds back to it in bf16), and y = sum of 32 of them (+-), |y| <= 128, is exact again.
           `gauss`: O Gaussian, m = 3 N(0, 1), l in [0.5, 40], one unit dead: bounded, see below.

Bounds (stream_rule.bound: half an output ulp + k c 2^-24 A, k = 2 for a bf16 store, A = sum |terms|); c read from the code:
  y after an inexact input       c = 64 per + 4: the products of a wave's share (per = ceil(K / 64 / S / 4) k-steps of 64, each one fp32
                                 accumulation), three wave adds (gemm_skinny.hip `acc[t][j] += v[j]`, w = 0 .. 2), the bias (`acc + bv`).
  pre_out (LayerNorm prologue)   c = 29.  mean: 8 thread-serial adds (`sum += xv`), 6 butterfly steps (wave_sum), 3 wave adds (rowpart[0]),
                                 the division = 18.  rstd: x - mu (1), square (1), the same 8 + 6 + 3 and the division (18), + eps (1), rsqrtf
                                 (<= 2 ulp: 4) = 25, which carries the mean's error as stream_rule's `ln rstd` does.  The store adds x - mu, * rs,
                                 * gamma, + beta = 4.  A = rs |gamma| (|s| + |mu| + mean |s|) + |beta|, as stream_rule's `ln y`.
  ln_out (LayerNorm tail)        stream_rule's `ln y` (c = L(N) + 17): the tail IS ln_row.h on s = bf16(fp32(alpha res + y)), y as stored.
  geglu on an exact z            stream_rule's geglu bound (c = 13 on the bf16 path).
  geglu on an inexact z          z = bf16(fp32 sum) is not stored.  Where the float64 z is further than 2 c 2^-24 A from a bf16 rounding
                                 boundary the kernel's z is the reference's and the geglu bound holds; elsewhere z may be either neighbour
                                 and the bound is widened by the largest change of a * gelu(g) over the candidate roundings of both.
  merge (gauss)                  per unit: m - mx (inside __expf's argument), __expf relative 3 + 4 |a| (embed_ce_rule's charge: v_exp 2, the
                                 product with log2 e 1, the argument's roundings 4 |a|), its product with O or l (1), <= nunit adds; then the
                                 division (<= 2): |dv| <= 2^-24 [E_o / l + |v| (E_l / l + 2)], E_o = sum_c |O_c| w_c (4 + 4 |a_c| + nunit), E_l
                                 the same over l_c.  The merged row is rounded to bf16 in LDS and not stored: b_v = half_ulp(v) + 2 |dv|,
                                 and y carries sum_k |W[n, k]| b_v[k] next to its own summation allowance.
  chain (decode_chain.hip)       a dot product is an fmaf chain of 8 NL per lane (dc_fma8, NL = 4 for K = 2048, 8 for K = 4096) and dc_wave_sum:
                                 4 DPP adds and 2 levels of readlane adds = 6; + 1 for a bias: c = 8 NL + 6 (+ 1).  dc_ln_stats is ln_row_stats
                                 with the division as a product by 1 / 2048 (exact scaling): stream_rule's `ln y` at d = 2048.

Mutants and where they apply (`applies`): the product mutants at the exact plain / split-K cases (dense: any M; drop_product at bounded
and at dense with K <= 2112 -- beyond, |y| passes 2048, a bf16 ulp is 16 and a single product of magnitude <= 9 can round away); x_row0 at
M >= 2 and out_tile0 at M > 16; the bias mutants where there is a bias; bias_gate_from_value, geglu_swap and gate_next_wg at GEGLU; the
LayerNorm mutants at tail and pre cases (ln_row_m4: M >= 5; ln_unwritten_group: tail only); the merge mutants at the merge cases
(unit_plus / unit_minus: nunit >= 2; nunit_short: nunit >= 2 in the one-live-unit design, whose slot nunit - 1 is the live one of (0, 0, 0) --
a Gaussian last unit may carry almost no weight; wrong_q: B q == 2; dead_counted: cases with dead units)."""
import math
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_probe as G  # noqa: E402
import stream_rule as S  # noqa: E402
from stream_rule import _d  # noqa: E402

U = S.U
ALPHA = 1.5               # of every residual LayerNorm here: alpha * res is exact in fp32 (10 significant bits)
EPS = 1e-5
TEN = 10.0                # a mutant must move an element by ten bounds
HALF = 0.5                # the fp32 transcription may use half of an allowance
DD = 128                  # d_head
PART_ROWS, PART_LD = 64, DD + 2
TICKETS = 2048            # DB1_SKINNY_TICKETS
OK, BAD_SHAPE, BAD_ALIGN, BAD_DTYPE, WS_SMALL, UNSUPPORTED = 0, -1, -2, -3, -4, -6


# ------------------------------------------------------------------------------------------------ dispatcher arithmetic (as in the .hip)
def split(N, K, geglu=False, never=False):
    """skinny_fused_split"""
    if geglu or never:
        return 1
    groups, ksteps, s = N // 16, K // 64, 1
    while groups * s < 256 and ksteps % (2 * s) == 0 and ksteps // (2 * s) >= 32:
        s *= 2
    return s


def workspace_bytes(M, N, K, geglu=False):
    s = split(N, K, geglu)
    return 0 if s == 1 else (N // 16) * s * ((M + 15) // 16) * 64 * 16


def supported(M, N, K, geglu=False, tail=False, pre=False):
    """db1_linear_decode_supported"""
    if M < 1 or M > 64 or K % 64 or N % 16 or N < 16:
        return False
    if (tail or (not pre and split(N, K, geglu) > 1)) and N // (8 if geglu else 16) + 1 > TICKETS:
        return False
    if tail and N not in (512, 1024, 2048):
        return False
    if pre and (M > 16 or K % 256 or K > 2048):
        return False
    return True


def attn_supported(B, q, H, D, nunit, N):
    return (B >= 1 and q >= 1 and B * q <= 2 and D == 128 and H * D <= 2048 and (H * D) % 256 == 0 and 1 <= nunit <= 12 and N % 16 == 0 and N >= 16
            and N // 16 + 1 <= TICKETS)


def geometry(case, never=False):
    """(S, k-steps per slice, k-steps per wave) of the launch"""
    s = 1 if (case.get("pre") or case["kind"] == "merge") else split(case["N"], case["K"], case.get("geglu", False), never)
    kps = case["K"] // 64 // s
    return s, kps, (kps + 3) // 4


def wave_steps(case, sp, w):
    """the k-steps [ks0, ks1) of wave w in slice sp (empty: ks1 <= ks0)"""
    _, kps, per = geometry(case)
    ks0 = sp * kps + w * per
    return ks0, min(ks0 + per, (sp + 1) * kps)


def wg_rows(case, nb):
    """the W rows of workgroup nb: 16 output columns, or 8 value rows and their 8 gate rows"""
    if case.get("geglu"):
        a = np.arange(nb * 8, nb * 8 + 8)
        return np.concatenate([a, case["N"] + a])
    return np.arange(nb * 16, nb * 16 + 16)


def instantiation(case):
    """(TBIAS, TP, MT, GEGLU, PRO) of gemm_skinny_fused_kernel as linear_decode_launch / linear_decode_attn_launch pick them"""
    if case["kind"] == "merge":
        return ("float", "float", 1, False, -case["M"])
    params = bool(case.get("tail") or case.get("pre"))
    tb = "bf16" if case["bias"] == "bf16" else "float"
    tp = "bf16" if params and case["pdt"] == "bf16" else "float"
    pre = bool(case.get("pre"))
    return (tb, tp, 1 if pre else (case["M"] + 15) // 16, bool(case.get("geglu")), pre_rows(case["M"]) if pre else 0)


def all_instantiations():
    """every bf16-weight instantiation the two dispatchers can pick"""
    T = ("bf16", "float")
    return ({(tb, tp, mt, g, 0) for tb in T for tp in T for mt in (1, 2, 3, 4) for g in (False, True)} |
            {(tb, tp, 1, g, pro) for tb in T for tp in T for g in (False, True) for pro in (1, 4, 16)} | {("float", "float", 1, False, -1), ("float", "float", 1, False, -2)})


def pre_rows(M):
    """the LayerNorm prologue's instantiation (rows held per thread)"""
    return 1 if M == 1 else (4 if M <= 4 else 16)


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case, salt=0):
    return np.random.default_rng([zlib.crc32(case["id"].encode()), salt])


def _gauss16(rng, shape, scale=1.0, shift=0.0):
    return S.bf16(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale) + np.float32(shift))


def sparse_rows(R, K, seed, scale=1.0):
    """[R, K] float32: row n has 32 nonzeros of +-scale at k = (n s + j K / 32) mod K (gemm_probe's bounded pattern)"""
    return G.build("bounded", R, 1, K, seed)["A"].astype(np.float32) * np.float32(scale)


def _ln_params(rng, d, pdt):
    return S.rnd(rng.standard_normal(d, dtype=np.float32) * np.float32(0.1) + np.float32(1.0), pdt), S.rnd(rng.standard_normal(d, dtype=np.float32) * np.float32(0.1), pdt)


def merge_part(case, rng):
    """the attention partials of a merge case, float32 [B H, nunit, 64, 130]"""
    B, q, H, nu, others = case["B"], case["q"], case["H"], case["nunit"], case["others"]
    part = np.full((B * H, nu, PART_ROWS, PART_LD), np.nan, np.float32)
    for b in range(B):
        for i in range(q):
            for h in range(H):
                u = part[b * H + h, :, i]
                if others == "gauss":
                    u[:, :DD] = rng.standard_normal((nu, DD), dtype=np.float32)
                    u[:, DD] = 3.0 * rng.standard_normal(nu, dtype=np.float32)
                    u[:, DD + 1] = rng.uniform(0.5, 40.0, nu).astype(np.float32)
                    dead = (b + i + h) % nu
                    if nu > 1:
                        u[dead, DD], u[dead, DD + 1] = -1.0e30, 0.0
                        u[dead, :DD] = 64.0
                    continue
                live = (nu - 1 - ((b * q + i) * H + h)) % nu          # from the last slot downwards: (0, 0, 0) has it
                m_live = np.float32(3.0 * rng.standard_normal())
                u[:, :DD] = 64.0 * (rng.integers(0, 2, (nu, DD)) * 2 - 1)                      # decoys
                if others == "dead":
                    u[:, DD], u[:, DD + 1] = -1.0e30, 0.0
                else:
                    u[:, DD] = m_live - np.float32(200.0) - rng.uniform(0.0, 50.0, nu).astype(np.float32)
                    u[:, DD + 1] = rng.integers(1, 41, nu).astype(np.float32)
                l = np.float32(2.0 ** ((b + i + h) % 5 - 1))
                u[live, :DD] = l * rng.integers(-4, 5, DD).astype(np.float32)
                u[live, DD], u[live, DD + 1] = m_live, l
    return part


def inputs(case):
    """every operand as float32 holding values its storage format holds exactly: x [M, K], W [R, K], bias [R] or None, ..."""
    kind, M, N, K = case["kind"], case["M"], case["N"], case["K"]
    rng = _rng(case)
    geglu = case.get("geglu", False)
    R = 2 * N if geglu else N
    inp = {}
    if kind == "merge":
        inp["part"] = merge_part(case, rng)
        inp["W"] = sparse_rows(N, K, 3)
        inp["bias"] = None
    elif case.get("pre"):
        inp["x"], inp["pre_res"] = _gauss16(rng, (M, K)), _gauss16(rng, (M, K), 1.0, 0.25)
        inp["pre_gamma"], inp["pre_beta"] = _ln_params(rng, K, case["pdt"])
        if geglu:
            inp["W"] = np.concatenate([sparse_rows(N, K, 0, 0.25), sparse_rows(N, K, 1, 0.25)])
            b = np.concatenate([_rng(case, 1).integers(-16, 17, N), _rng(case, 2).integers(-16, 17, N)]).astype(np.float32) / np.float32(8)
        else:
            inp["W"] = sparse_rows(N, K, 0)
            b = rng.integers(-32, 33, N).astype(np.float32)
        inp["bias"] = b if case["bias"] != "none" else None
    elif geglu:
        p0, p1 = G.build("bounded", M, N, K, 0), G.build("bounded", M, N, K, 1)
        inp["x"] = p0["A"].astype(np.float32) / np.float32(8)
        inp["W"] = np.concatenate([p0["B"].T, p1["B"].T]).astype(np.float32)
        b = np.concatenate([_rng(case, 1).integers(-16, 17, N), _rng(case, 2).integers(-16, 17, N)]).astype(np.float32) / np.float32(8)
        inp["bias"] = b if case["bias"] != "none" else None
    else:
        G.check(case["design"], M, N, K, 1.0, 0.0, case["bias"] != "none")                       # the fp32 (dense) / bf16 (bounded) headroom
        p = G.build(case["design"], M, N, K, 0)
        inp["x"], inp["W"] = p["A"].astype(np.float32), np.ascontiguousarray(p["B"].T).astype(np.float32)
        inp["bias"] = p["bias"].astype(np.float32) if case["bias"] != "none" else None
    if case.get("tail"):
        r2 = _rng(case, 7)
        inp["res"] = _gauss16(r2, (M, N), 1.0, 0.25)
        inp["gamma"], inp["beta"] = _ln_params(r2, N, case["pdt"])
    assert inp["W"].shape == (R, K)
    return inp


# ------------------------------------------------------------------------------------------------ mutants
PRODUCT_MUTANTS = ("drop_product", "drop_kstep", "drop_wave_last", "drop_wave", "drop_slice", "dup_slice", "swap_halves_w")
ROW_MUTANTS = ("x_row0", "out_tile0")
BIAS_MUTANTS = ("bias_shift1", "bias_shift4", "bias_gate_from_value")
GEGLU_MUTANTS = ("geglu_swap", "gate_next_wg")
LN_MUTANTS = ("ln_no_alpha", "ln_swap_gamma_beta", "ln_row_m4", "ln_unwritten_group")
MERGE_MUTANTS = ("unit_plus", "unit_minus", "head_plus", "head_minus", "wrong_q", "dead_counted", "nunit_short")
MUTANTS = PRODUCT_MUTANTS + ROW_MUTANTS + BIAS_MUTANTS + GEGLU_MUTANTS + LN_MUTANTS + MERGE_MUTANTS


def applies(mutant, case):
    """does the mutant change what this case computes?  (the inapplicable cases, explicitly)"""
    kind, M = case["kind"], case["M"]
    exact_map = kind in ("plain", "split")
    if mutant == "drop_product":
        return exact_map and (case["design"] == "bounded" or case["K"] <= 2112)
    if mutant in ("drop_kstep", "drop_wave_last", "drop_wave", "swap_halves_w"):
        return exact_map and case["design"] == "dense"
    if mutant in ("drop_slice", "dup_slice"):
        return exact_map and case["design"] == "dense" and geometry(case)[0] > 1
    if mutant == "x_row0":
        return exact_map and M >= 2
    if mutant == "out_tile0":
        return exact_map and M > 16
    if mutant in ("bias_shift1", "bias_shift4"):
        return kind in ("plain", "split", "geglu") and case["bias"] != "none"
    if mutant == "bias_gate_from_value":
        return kind == "geglu" and case["bias"] != "none"
    if mutant in GEGLU_MUTANTS:
        return kind == "geglu"
    if mutant in LN_MUTANTS:
        if not (case.get("tail") or case.get("pre")):
            return False
        if mutant == "ln_row_m4":
            return M >= 5
        if mutant == "ln_unwritten_group":
            return bool(case.get("tail"))
        return True
    if mutant in MERGE_MUTANTS:
        if kind != "merge":
            return False
        if mutant in ("unit_plus", "unit_minus"):
            return case["nunit"] >= 2
        if mutant == "nunit_short":                 # (a Gaussian last unit may carry almost no weight: the index is judged on the one-live-unit design)
            return case["nunit"] >= 2 and case["others"] != "gauss"
        if mutant == "wrong_q":
            return case["B"] * case["q"] == 2
        if mutant == "dead_counted":
            return case["nunit"] >= 2 and case["others"] in ("dead", "gauss")
        return True
    raise KeyError(mutant)


# ------------------------------------------------------------------------------------------------ the reference
def _kcols(ks0, ks1):
    return slice(ks0 * 64, ks1 * 64)


def product(x, W, case, mutant=None):
    """x . W^T in float64 ([M, R]), under one product mutant:
    drop_product    the product at one (m, k) with x[m, k] != 0 is lost, in every column
    drop_kstep      the last 64-wide k-step is lost in the last workgroup
    drop_wave_last  the last k-step of wave 0's share (slice 0) is lost in workgroup 0
    drop_wave       the share of the last wave that has one (last slice) is lost in workgroup 0
    drop_slice      split slice 1 never arrives;  dup_slice: the last slice is added twice
    swap_halves_w   the two 8-element halves of every lane's 16 elements of k-step 0 change places, on W only"""
    x, W = _d(x), _d(W)
    M, K = x.shape
    nwg = W.shape[0] // 16
    if mutant == "swap_halves_w":
        W = W.copy()
        W[:, :64] = W[:, :64].reshape(-1, 4, 2, 8)[:, :, ::-1].reshape(-1, 64)
    P = x @ W.T
    s, kps, per = geometry(case)
    if mutant == "drop_product":
        m = M // 2
        k = int(np.flatnonzero(x[m])[-1])
        P[m] -= x[m, k] * W[:, k]
    elif mutant == "drop_kstep":
        rows, c = wg_rows(case, nwg - 1), _kcols(K // 64 - 1, K // 64)
        P[:, rows] -= x[:, c] @ W[rows, c].T
    elif mutant in ("drop_wave_last", "drop_wave"):
        rows = wg_rows(case, 0)
        if mutant == "drop_wave_last":
            ks0, ks1 = wave_steps(case, 0, 0)
            c = _kcols(ks1 - 1, ks1)
        else:
            w = max(w for w in range(4) if wave_steps(case, s - 1, w)[1] > wave_steps(case, s - 1, w)[0])
            c = _kcols(*wave_steps(case, s - 1, w))
        P[:, rows] -= x[:, c] @ W[rows, c].T
    elif mutant in ("drop_slice", "dup_slice"):
        sp = 1 if mutant == "drop_slice" else s - 1
        c = _kcols(sp * kps, (sp + 1) * kps)
        P += (-1.0 if mutant == "drop_slice" else 1.0) * (x[:, c] @ W[:, c].T)
    return P


def gelu64(x):
    return S.O.gelu(x)


def merge_ref(case, inp, mutant=None):
    """(v, b_v): the merged rows [B q, H 128] in float64 before the rounding to bf16, and the bound of their bf16 value (zeros: exact)"""
    B, q, H, nu = case["B"], case["q"], case["H"], case["nunit"]
    part = _d(inp["part"])
    v, bv = np.zeros((B * q, H * DD)), np.zeros((B * q, H * DD))
    for m in range(B * q):
        qq = q
        if mutant == "wrong_q":
            qq = 2 if q == 1 else 1
        b, i = (m // qq) % B, m % qq
        for h in range(H):
            hs = (h + (mutant == "head_plus") - (mutant == "head_minus")) % H
            u = part[b * H + hs, :, i]
            n_use = nu - 1 if mutant == "nunit_short" else nu
            mm, ll = u[:n_use, DD], u[:n_use, DD + 1]
            src = np.clip(np.arange(n_use) + (mutant == "unit_plus") - (mutant == "unit_minus"), 0, nu - 1)
            Ou = u[src, :DD]
            mx = max(-1.0e30, mm.max()) if n_use else -1.0e30
            with np.errstate(under="ignore", invalid="ignore"):
                a = mm - mx
                wt = np.where(ll > 0, np.exp(a), 1.0 if mutant == "dead_counted" else 0.0)
                l = (ll * wt).sum()
                o = (Ou * wt[:, None]).sum(0)
                cs = slice(h * DD, (h + 1) * DD)
                if not l > 0:
                    v[m, cs] = 0.0 if l == 0 else np.nan
                    continue
                v[m, cs] = o / l
                if case["others"] == "gauss":
                    ch = 4.0 + 4.0 * np.abs(np.where(ll > 0, a, 0.0)) + nu
                    Eo = (np.abs(Ou) * (wt * ch)[:, None]).sum(0)
                    El = (ll * wt * ch).sum()
                    dv = S.SHARE * U * (Eo / l + np.abs(v[m, cs]) * (El / l + 2.0))
                    bv[m, cs] = S.half_ulp(v[m, cs], "bf16") + 2.0 * dv
    return v, bv


def merged_rows(case, inp, mutant=None):
    """the merged rows as the bf16 values the kernel keeps: a relative 1e-7 (or a low unit's 1e-87) rounds back to the integer"""
    with np.errstate(invalid="ignore"):
        return S.bf16(np.asarray(merge_ref(case, inp, mutant)[0], np.float32)).astype(np.float64)


def _ln64(s, gamma, beta):
    mu = s.mean(-1, keepdims=True)
    rs = 1.0 / np.sqrt(((s - mu) ** 2).mean(-1, keepdims=True) + EPS)
    return (s - mu) * rs * gamma + beta, mu, rs


def s_rows(res, y, alpha=ALPHA):
    """s = bf16(fp32(alpha res + y)) as float64: alpha res is exact in fp32, so the sum is ONE fp32 rounding, contracted or not"""
    return S.bf16(np.asarray(alpha * _d(res) + _d(y), np.float32)).astype(np.float64)


def ln_expect(res, y, gamma, beta, c, mutant=None, group=None):
    """LN(alpha res + y) gamma + beta in float64 with its per-element bound, under one LayerNorm mutant:
    ln_no_alpha  alpha taken as 1;  ln_swap_gamma_beta;  ln_row_m4: rows m >= 4 computed from row m - 4;
    ln_unwritten_group: the columns of one column group of y (``group``, a slice) not yet written: zero"""
    res, y, gamma, beta = _d(res), _d(y), _d(gamma), _d(beta)
    if mutant == "ln_unwritten_group":
        y = y.copy()
        y[:, group] = 0.0
    s = s_rows(res, y, 1.0 if mutant == "ln_no_alpha" else ALPHA)
    if mutant == "ln_row_m4":
        s = np.concatenate([s[:4], s[:-4]])
    if mutant == "ln_swap_gamma_beta":
        gamma, beta = beta, gamma
    ref, mu, rs = _ln64(s, gamma, beta)
    A = rs * np.abs(gamma) * (np.abs(s) + np.abs(mu) + np.abs(s).mean(-1, keepdims=True)) + np.abs(beta)
    return ref, S.bound(ref, A, c, "bf16")


PRE_LN_C = 29             # see the header: 25 for rstd (which carries the mean's 18) + the 4 of the store


def tail_c(N):
    return S.L(N, 8) + 17   # stream_rule's `ln y`


def bf16_neighbours(z):
    """(lo, hi): the bf16 values below / above z (both z where z is a bf16 value)"""
    z32 = np.asarray(z, np.float32)
    t = (z32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)      # towards zero
    ulp = 2.0 * S.half_ulp(np.where(t == 0, 2.0 ** -126, t), "bf16")
    away = np.where(np.asarray(z) == t, t, t + np.copysign(ulp, z))
    return np.minimum(t, away), np.maximum(t, away)


def geglu_expect(z, Az, c, N):
    """a * gelu(g) of z = [a | g] (float64 [M, 2 N]) through the kernel's bf16 z, with the per-element bound.  Az None: z is exact (and a
    bf16 value); else |z_kernel - z| <= c 2^-24 Az before the rounding, see `geglu on an inexact z` in the header."""
    z = _d(z)
    zb = S.bf16(np.asarray(z, np.float32)).astype(np.float64)
    if Az is None:
        assert np.array_equal(zb, z), "the geglu design's z must be a bf16 value"
    a, g = zb[:, :N], zb[:, N:]
    ref = a * gelu64(g)
    with np.errstate(over="ignore", under="ignore"):
        e = np.abs(S._erf(g / math.sqrt(2.0)))
    bnd = S.bound(ref, np.abs(a) * 0.5 * np.abs(g) * (1.0 + e), S.GELU_C["bf16"] + 1, "bf16")
    if Az is None:
        return ref, bnd
    lo, hi = bf16_neighbours(z)
    mid = 0.5 * (lo + hi)
    unsafe = (lo != hi) & (np.abs(_d(z) - mid) <= 2.0 * S.SHARE * c * U * _d(Az))
    cand = lambda k: np.where(unsafe, (lo, hi)[k], zb)
    wide = np.zeros_like(ref)
    for ka in (0, 1):
        for kg in (0, 1):
            wide = np.maximum(wide, np.abs(cand(ka)[:, :N] * gelu64(cand(kg)[:, N:]) - ref))
    return ref, bnd + wide


def expect(case, inp, got, mutant=None):
    """{output name: (float64 reference, per-element bound; zero = expected bits)} of a case of the linear maps.  ``got`` supplies the stored
    intermediates that later results are defined on (pre_out for y, y for ln_out), never the result under comparison itself."""
    kind, M, N, K = case["kind"], case["M"], case["N"], case["K"]
    geglu = case.get("geglu", False)
    W = _d(inp["W"])
    bias = None if inp["bias"] is None else _d(inp["bias"])
    out = {}
    xb = None                                       # bound of the unstored bf16 input rows (merge / gauss)
    exact = True
    if kind == "merge":
        v, bv = merge_ref(case, inp, mutant)
        if case["others"] == "gauss":
            x, xb, exact = v, bv, False
        else:
            x = merged_rows(case, inp, mutant)
    elif case.get("pre"):
        ref, bnd = ln_expect(inp["pre_res"], inp["x"], inp["pre_gamma"], inp["pre_beta"], PRE_LN_C, mutant)
        out["pre_out"] = (ref, bnd)
        x, exact = _d(got["pre_out"]), False
    else:
        x = _d(inp["x"])
        if mutant == "x_row0":
            x = x.copy()
            x[M - 1] = x[0]
    z = product(x, W, case, mutant if mutant in PRODUCT_MUTANTS else None)
    Az = np.abs(np.nan_to_num(x)) @ np.abs(W).T
    if bias is not None:
        if mutant in ("bias_shift1", "bias_shift4"):
            bias = np.roll(bias, -1 if mutant == "bias_shift1" else -4)
        if mutant == "bias_gate_from_value":
            bias = np.concatenate([bias[:N], bias[:N]])
        z = z + bias
        Az = Az + np.abs(bias)
    if geglu:
        if mutant == "geglu_swap":
            z = np.concatenate([z[:, N:], z[:, :N]], 1)
        if mutant == "gate_next_wg":
            z = np.concatenate([z[:, :N], np.roll(z[:, N:], -8, axis=1)], 1)
    c_lin = 64 * geometry(case)[2] + 4
    if geglu:
        y = geglu_expect(z, None if exact else Az, c_lin, N)
    elif exact:
        y = (G.bf16_rne(z) if np.isfinite(z).all() else z, np.zeros(z.shape))
    else:
        extra = 0.0 if xb is None else xb @ np.abs(W).T
        y = (z, np.maximum(S.half_ulp(z, "bf16") + 2.0 * (S.SHARE * c_lin * U * Az + extra), S.TINY))
    if mutant == "out_tile0":
        n = min(16, M - 16)                         # rows 16 .. 16 + n - 1 hold what tile 0 computed
        y = tuple(np.concatenate([a[:16], a[:n], a[16 + n:]]) for a in y)
    out["y"] = y
    if case.get("tail"):
        group = slice(8, 16) if geglu else slice(16, 32)
        out["ln_out"] = ln_expect(inp["res"], got["y"], inp["gamma"], inp["beta"], tail_c(N), mutant, group)
    return out


def geglu_z(case, inp):
    """the exact z of a geglu-design case, float32 [M, 2 N] (what the GPU test uploads for db1_ffn_act_fwd)"""
    z = _d(inp["x"]) @ _d(inp["W"]).T + (0.0 if inp["bias"] is None else _d(inp["bias"]))
    assert np.array_equal(z * 8, np.round(z * 8)) and np.abs(z).max() <= 10.0
    return z.astype(np.float32)


def gate_condition(z, N):
    """the range condition on the gates of a GEGLU reference: (share in [-4, 4], share below 0, share above 0)"""
    g = _d(z)[:, N:]
    return float((np.abs(g) <= 4).mean()), float((g < 0).mean()), float((g > 0).mean())


# ------------------------------------------------------------------------------------------------ the fp32 transcription
def _sum32(a):
    """row sums in float32 by halving (ANOTHER order than the device's lanes -> butterfly -> waves)"""
    a = np.asarray(a, np.float32)
    n = 1 << (a.shape[-1] - 1).bit_length()
    t = np.zeros(a.shape[:-1] + (n,), np.float32)
    t[..., :a.shape[-1]] = a
    while t.shape[-1] > 1:
        t = t[..., ::2] + t[..., 1::2]
    return t[..., 0]


def _ln32(res, y, gamma, beta):
    f = np.float32
    s = S.bf16(f(ALPHA) * np.asarray(res, f) + np.asarray(y, f))
    d = f(s.shape[-1])
    mu = (_sum32(s) / d)[:, None]
    c = s - mu
    rs = (f(1.0) / np.sqrt(_sum32(c * c) / d + f(EPS)))[:, None]
    return S.bf16(c * rs * np.asarray(gamma, f) + np.asarray(beta, f))


def _dot32(x, W):
    """x . W^T in float32, k in blocks of 64 added by halving"""
    x, W = np.asarray(x, np.float32), np.asarray(W, np.float32)
    K = x.shape[1]
    parts = np.stack([x[:, k:k + 64] @ W[:, k:k + 64].T for k in range(0, K, 64)], -1)
    return _sum32(parts)


def merge32(case, inp):
    B, q, H, nu = case["B"], case["q"], case["H"], case["nunit"]
    f, part = np.float32, inp["part"]
    v = np.zeros((B * q, H * DD), f)
    for m in range(B * q):
        b, i = m // q, m % q
        for h in range(H):
            u = part[b * H + h, :, i]
            mx = max(f(-1.0e30), u[:, DD].max())
            with np.errstate(under="ignore"):
                wt = np.where(u[:, DD + 1] > 0, np.exp((u[:, DD] - mx).astype(np.float64)).astype(f), f(0))
            l, o = f(0), np.zeros(DD, f)
            for c in range(nu):
                l = l + u[c, DD + 1] * wt[c]
                o = o + u[c, :DD] * wt[c]
            v[m, h * DD:(h + 1) * DD] = o / l if l > 0 else 0
    return S.bf16(v)


def model(case, inp):
    """what the launch stores, in float32 arithmetic (summation orders of its own)"""
    N, geglu, f = case["N"], case.get("geglu", False), np.float32
    got = {}
    if case["kind"] == "merge":
        x = merge32(case, inp)
    elif case.get("pre"):
        x = got["pre_out"] = _ln32(inp["pre_res"], inp["x"], inp["pre_gamma"], inp["pre_beta"])
    else:
        x = inp["x"]
    z = _dot32(x, inp["W"])
    if inp["bias"] is not None:
        z = z + inp["bias"]
    if geglu:
        zb = S.bf16(z)
        got["y"] = S.bf16(zb[:, :N] * S._gelu_both(zb[:, N:], "bf16")[0])
    else:
        got["y"] = S.bf16(z)
    if case.get("tail"):
        got["ln_out"] = _ln32(inp["res"], got["y"], inp["gamma"], inp["beta"])
    return got


# ------------------------------------------------------------------------------------------------ the cases
def _mk(kind, **kw):
    kw["kind"] = kind
    kw["id"] = kind + "-" + "-".join(f"{k}{v}" if not isinstance(v, str) else v for k, v in kw.items() if k != "kind")
    return kw


BIASES = ("none", "bf16", "f32")
PLAIN_M = (1, 15, 16, 17, 32, 33, 48, 49, 64)
PLAIN_NK = ((16, 64), (16, 128), (48, 320), (32, 576), (16, 2112))
SPLIT_NK = ((16, 4096, 2), (48, 8192, 4), (16, 16384, 8), (16, 4032, 1), (4096, 4096, 1))       # (N, K, S)
MERGE_BQ = ((1, 1), (1, 2), (2, 1))


def _cases():
    C = []
    for N, K in PLAIN_NK:                                   # x and y strided (ldx = K + 8, ldy = N + 24)
        for M in PLAIN_M:
            for bias in BIASES:
                C.append(_mk("plain", design="dense", M=M, N=N, K=K, bias=bias))
        for M in (1, 17, 64):
            C.append(_mk("plain", design="bounded", M=M, N=N, K=K, bias="bf16"))
    for j, (N, K, s) in enumerate(SPLIT_NK):
        for i, M in enumerate((1, 17, 64) if N < 4096 else (1,)):
            C.append(_mk("split", design="dense", M=M, N=N, K=K, bias=BIASES[(i + j) % 3]))
        if N < 4096:
            C.append(_mk("split", design="bounded", M=17, N=N, K=K, bias="bf16"))
    n = 0
    for N, K in ((512, 64), (1024, 64), (2048, 64), (512, 4096)):
        for M in (1, 4, 5, 17, 64):
            for pdt in ("bf16", "f32"):
                C.append(_mk("tail", design="bounded", M=M, N=N, K=K, bias=BIASES[n % 3], pdt=pdt, tail=True))
                n += 1
    for N in (16, 48):
        for K in (64, 320):
            for M in (1, 16, 17, 64):
                for bias in BIASES:
                    C.append(_mk("geglu", M=M, N=N, K=K, bias=bias, geglu=True))
    for bias in BIASES:                                     # (MT = 3 through the GEGLU epilogue)
        C.append(_mk("geglu", M=33, N=16, K=64, bias=bias, geglu=True))
    for M in (1, 17, 33, 64):                               # every (TBIAS, TP, MT) of the GEGLU kernel that a LayerNorm tail can follow
        for bias in ("bf16", "f32"):
            for pdt in ("bf16", "f32"):
                C.append(_mk("geglu", M=M, N=512, K=64, bias=bias, geglu=True, pdt=pdt, tail=True))
                if M == 33:                                 # ... and MT = 3 of the plain one
                    C.append(_mk("tail", design="bounded", M=M, N=512, K=64, bias=bias, pdt=pdt, tail=True))
    for K in (256, 512, 1792, 2048):
        for M in (1, 2, 3, 4, 5, 15, 16):
            for pdt in ("bf16", "f32"):
                C.append(_mk("pre", M=M, N=48, K=K, bias=BIASES[n % 3], pdt=pdt, pre=True))
                C.append(_mk("pre", M=M, N=16, K=K, bias=BIASES[(n + 1) % 3], pdt=pdt, pre=True, geglu=True))
                n += 1
    C.append(_mk("pre", M=5, N=512, K=256, bias="bf16", pdt="bf16", pre=True, tail=True))
    for B, q in MERGE_BQ:
        for H in (2, 16):
            for nunit in (1, 2, 11, 12):
                for others in ("dead", "low"):
                    C.append(_mk("merge", M=B * q, N=48, K=H * DD, B=B, q=q, H=H, nunit=nunit, others=others))
    C.append(_mk("merge", M=2, N=48, K=16 * DD, B=1, q=2, H=16, nunit=12, others="gauss"))
    C.append(_mk("merge", M=2, N=48, K=2 * DD, B=2, q=1, H=2, nunit=11, others="gauss"))
    return C


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def cases(*kinds):
    return [c for c in CASES if c["kind"] in kinds]


def cheap(case):
    """small enough for the CPU proof (the 32 MB no-split case runs on the GPU only; its neighbours keep every formula)"""
    return case["N"] * case["K"] <= (1 << 21)


# one refusal per clause of db1_linear_decode_supported (M, N, K, geglu, tail, pre) and db1_linear_decode_attn_supported (B, q, H, D, nunit, N)
REFUSALS = (
    ("M=65", dict(M=65, N=16, K=64)), ("K%64", dict(M=4, N=16, K=96)), ("N%16", dict(M=4, N=24, K=64)),
    ("tail N=768", dict(M=4, N=768, K=64, tail=True)),
    ("pre M=17", dict(M=17, N=48, K=256, pre=True)), ("pre K=2304", dict(M=4, N=48, K=2304, pre=True)), ("pre K=384", dict(M=4, N=48, K=384, pre=True)),
    ("tickets: geglu tail N=16384", dict(M=1, N=16384, K=64, geglu=True, tail=True)),
)
ATTN_REFUSALS = (("13 units", dict(B=1, q=1, H=2, D=128, nunit=13, N=48)), ("B q = 3", dict(B=3, q=1, H=2, D=128, nunit=2, N=48)),
                 ("H D = 384", dict(B=1, q=1, H=3, D=128, nunit=2, N=48)))


# ------------------------------------------------------------------------------------------------ the persistent chain (decode_chain.hip)
CHAIN_D, CHAIN_DFF, CHAIN_H = 2048, 4096, 16
CHAIN_UNITS = (1, 9, 10, 12)


def chain_c(K, bias=False):
    """fp32 roundings of a dot product of the chain: the fmaf chain of a lane (8 per 16-byte piece, K / 512 pieces), dc_wave_sum (6), the bias"""
    return 8 * (K // 512) + 6 + (1 if bias else 0)


def chain_weights():
    """the weights of the chain probe, float32 holding bf16 values: w_o, w2 and w_qkv from the sparse +-1 pattern, w1 from the GEGLU design
    (value and gate halves from different seeds, +-1/4 so that the gates stay in range; biases k / 8 from different seeds)"""
    d, dff = CHAIN_D, CHAIN_DFF
    rng = np.random.default_rng(20)
    w = dict(w_o=sparse_rows(d, d, 4), w1=np.concatenate([sparse_rows(dff, d, 5, 0.25), sparse_rows(dff, d, 6, 0.25)]), w2=sparse_rows(d, dff, 7, 0.5),
             w_qkv=sparse_rows(3 * d, d, 8))
    w["b1"] = np.concatenate([np.random.default_rng(21).integers(-16, 17, dff), np.random.default_rng(22).integers(-16, 17, dff)]).astype(np.float32) / np.float32(8)
    w["b2"] = rng.integers(-32, 33, d).astype(np.float32) / np.float32(8)
    w["g1"], w["be1"] = _ln_params(rng, d, "bf16")
    w["g2"], w["be2"] = _ln_params(rng, d, "bf16")
    w["x_res"] = _gauss16(rng, (1, d))
    return w


def chain_part(nunit, others):
    case = _mk("merge", M=1, N=CHAIN_D, K=CHAIN_D, B=1, q=1, H=CHAIN_H, nunit=nunit, others=others)
    return case, merge_part(case, _rng(case))


def chain_expect(w, case, part, got):
    """{stage: (reference, bound)} of one chain launch; every stage from the STORED input of that stage (got: y_o, h1, act, f, x_next)"""
    d, dff = CHAIN_D, CHAIN_DFF
    out = {}
    merged = merged_rows(case, dict(part=part))
    y_o = merged @ _d(w["w_o"]).T
    out["y_o"] = (G.bf16_rne(y_o), np.zeros(y_o.shape))
    out["h1"] = ln_expect(w["x_res"], got["y_o"], w["g1"], w["be1"], tail_c(d))
    h1 = _d(got["h1"])
    z = h1 @ _d(w["w1"]).T + _d(w["b1"])
    Az = np.abs(h1) @ np.abs(_d(w["w1"])).T + np.abs(_d(w["b1"]))
    out["act"] = geglu_expect(z, Az, chain_c(d, True), dff)
    act = _d(got["act"])
    f = act @ _d(w["w2"]).T + _d(w["b2"])
    out["f"] = (f, S.bound(f, np.abs(act) @ np.abs(_d(w["w2"])).T + np.abs(_d(w["b2"])), chain_c(dff, True), "bf16"))
    if "x_next" in got:
        out["x_next"] = ln_expect(got["h1"], got["f"], w["g2"], w["be2"], tail_c(d))
        xn = _d(got["x_next"])
        qkv = xn @ _d(w["w_qkv"]).T
        out["qkv_next"] = (qkv, S.bound(qkv, np.abs(xn) @ np.abs(_d(w["w_qkv"])).T, chain_c(d), "bf16"))
    return out


def chain_model(w, case, part):
    """the chain's stores in float32 (orders of its own): y_o, h1, act, f, x_next, qkv_next"""
    d, dff = CHAIN_D, CHAIN_DFF
    got = {}
    got["y_o"] = S.bf16(_dot32(merge32(case, dict(part=part)), w["w_o"]))
    got["h1"] = _ln32(w["x_res"], got["y_o"], w["g1"], w["be1"])
    zb = S.bf16(_dot32(got["h1"], w["w1"]) + w["b1"])
    got["act"] = S.bf16(zb[:, :dff] * S._gelu_both(zb[:, dff:], "bf16")[0])
    got["f"] = S.bf16(_dot32(got["act"], w["w2"]) + w["b2"])
    got["x_next"] = _ln32(got["h1"], got["f"], w["g2"], w["be2"])
    got["qkv_next"] = S.bf16(_dot32(got["x_next"], w["w_qkv"]))
    return got
