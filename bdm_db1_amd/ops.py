"""Thin torch-tensor -> C-ABI adapters.  Tensors are containers only: every function passes
``tensor.data_ptr()`` + sizes to libdb1_hip.so on the current HIP stream.  No arithmetic happens in
Python or in torch ops here, and nothing falls back to torch when a call fails."""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from typing import Optional

import numpy as np
import torch

from . import lib
from .lib import DB1_BF16, DB1_F32, ACT_CODES

_vp = ctypes.c_void_p


def dt_code(t) -> int:
    dt = t if isinstance(t, torch.dtype) else t.dtype
    if dt == torch.float32:
        return DB1_F32
    if dt == torch.bfloat16:
        return DB1_BF16
    raise lib.Db1Error(f"unsupported dtype {dt} (float32 / bfloat16 only)")


def P(t: Optional[torch.Tensor]):
    if t is None:
        return _vp(0)
    if not t.is_cuda:
        raise lib.Db1Error("the DB1 kernels need device tensors (no CPU path)")
    return _vp(t.data_ptr())


_tls = threading.local()   # .scope = (raw handle, c_void_p, device index) of the stream a model call runs on, while it runs -- per host thread
_DEBUG_STREAM = bool(int(os.environ.get("DB1_DEBUG_STREAM", "0")))


def _scope():
    return getattr(_tls, "scope", None)


class stream_scope:
    """``with ops.stream_scope():`` around a model forward / backward: the current stream is looked up ONCE (torch.cuda.current_stream()
    costs ~7 us of host time and every launch asks for it: a quarter of the host time of an eager inference call).  Nothing inside may
    switch streams or devices -- the model's own code never does; ``DB1_DEBUG_STREAM=1`` checks every launch against torch's current
    stream.  The scope is thread-local (one host thread per GPU / rank is the contract of include/db1_hip.h; two threads driving two
    models never see each other's stream or scratch buffer)."""

    def __enter__(self):
        self.prev = _scope()
        h = torch.cuda.current_stream().cuda_stream
        _tls.scope = (h, _vp(h), torch.cuda.current_device())
        return self

    def __exit__(self, *exc):
        _tls.scope = self.prev
        return False


def stream():
    sc = _scope()
    if sc is not None:
        if _DEBUG_STREAM and (torch.cuda.current_device() != sc[2] or torch.cuda.current_stream().cuda_stream != sc[0]):
            raise lib.Db1Error("the current stream / device changed inside an ops.stream_scope()")
        return sc[1]
    return _vp(torch.cuda.current_stream().cuda_stream)


class _Workspace:
    """The scratch the C ABI asks its caller for (include/db1_hip.h: ``db1_<op>_workspace_bytes``): one torch buffer per (device,
    stream), grown on demand by the caching allocator (stream-ordered: no device synchronisation, no hipMalloc inside an entry
    point).  Every op that needs scratch is finished with it when its work on the stream is done, and ops of one stream run in
    order, so one buffer of the largest size requested so far serves them all.  Under hipGraph capture the capturing stream gets its
    own buffer from the graph's private pool (torch allows allocation there), which lives as long as this cache references it."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device):
        if nbytes <= 0:
            return _vp(0), 0
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               _scope()[0] if _scope() is not None else torch.cuda.current_stream(device).cuda_stream)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return _vp(buf.data_ptr()), buf.numel()


_workspace = _Workspace()
_ws_query_cache = {}


def reserve_workspace(nbytes: int, device=None):
    """pre-size the current stream's scratch buffer (so that a timed region never contains its first allocation)"""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _workspace.get(int(nbytes), device)


def _ws(query: str, args: tuple, device):
    """(ws pointer, ws_bytes) for one call: size from the library's own query (memoised per shape)"""
    key = (query, args)
    n = _ws_query_cache.get(key)
    if n is None:
        n = int(getattr(lib.load(), query)(*args))
        _ws_query_cache[key] = n
    return _workspace.get(n, device)


def _strides2(t: torch.Tensor):
    assert t.dim() == 2
    return t.stride(0), t.stride(1)


class KernelTimer:
    """HIP-event timing of individual launches for bench.py's roofline legs: one event pair per launch, recorded on the stream the
    kernel is launched on; nothing is synchronised until ``summary()``.  ``work`` is the ALGORITHMIC work of the launch: FLOPs actually
    executed for the MFMA-bound families ("gemm", "flash_fwd", "flash_bwd"), bytes for the HBM-bound kernels."""

    def __init__(self, only=None):
        self.rec = {}   # family -> [event pairs, summed work, launches]
        self.only = None if only is None else set(only)   # time these families only (the others run uninstrumented)

    def wrap(self, family: str, work: float, fn):
        if self.only is not None and family not in self.only:
            fn()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        r = self.rec.setdefault(family, [[], 0.0, 0])
        r[0].append((e0, e1))
        r[1] += work
        r[2] += 1

    def summary(self):
        """{family: (total ms, work, launches)}"""
        torch.cuda.synchronize()
        return {k: (float(sum(a.elapsed_time(b) for a, b in v[0])), v[1], v[2]) for k, v in self.rec.items()}


_gemm_timer: Optional[KernelTimer] = None


def set_gemm_timer(t: Optional[KernelTimer]):
    global _gemm_timer
    _gemm_timer = t


def _timed(family: str, work: float, run):
    if _gemm_timer is not None:
        _gemm_timer.wrap(family, work, run)
    else:
        run()


def marker(tag: int):
    """an empty kernel named db1_marker_kernel on the current stream (include/db1_hip_test.h): cuts a kernel trace to a region"""
    lib.call("db1_test_marker", int(tag), stream())


def _tri_fraction(M: int, K: int, mode: int, period: int, tm: int = 256, tk: int = 64) -> float:
    """share of the k-tiles a tile GEMM executes under a structural-zero hint for A (db1_gemm_strided_tri): a k-tile is skipped when
    it is zero for EVERY row of the m-tile (mode 1: k > m; mode 2: (k mod period) < m)"""
    if mode == 0:
        return 1.0
    done = total = 0
    for m0 in range(0, M, tm):
        m1 = min(m0 + tm, M) - 1
        for k0 in range(0, K, tk):
            total += 1
            if mode == 1:
                done += 0 if k0 > m1 else 1
            else:
                done += 0 if (k0 % period) + tk - 1 < m0 else 1
    return done / max(total, 1)


def _is_tile_gemm(M, N, K, a, b, out, sa, sb, so) -> bool:
    return bool(lib.load().db1_gemm_would_use_fast(M, N, K, dt_code(a), dt_code(b), dt_code(out), sa[0], sa[1], sb[0], sb[1], so[0], so[1]))


def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
         alpha: float = 1.0, beta: float = 0.0, useful_flops: Optional[float] = None):
    """out[m,n] = alpha * a[m,k] @ b[k,n] + beta*out + bias[n]; a, b, out are 2-D VIEWS with any strides
    (pass ``w.t()`` for y = x W^T).  Optional leading batch dims are not handled here (see gemm_batched).
    ``useful_flops``: what the timer counts when part of the product is padding (the vocabulary pad of the tied head)."""
    M, K = a.shape
    K2, N = b.shape
    assert K == K2 and out.shape == (M, N), (a.shape, b.shape, out.shape)

    def run():
        ws, wsn = _ws("db1_gemm_workspace_bytes", (M, N, K, dt_code(a), dt_code(b), dt_code(out), a.stride(0), a.stride(1), b.stride(0), b.stride(1),
                                                    out.stride(0), out.stride(1), 1, 1), out.device)
        lib.call("db1_gemm_strided", P(a), P(b), P(out), P(bias), M, N, K, dt_code(a), dt_code(b), dt_code(out),
                 dt_code(bias) if bias is not None else 0, a.stride(0), a.stride(1), b.stride(0), b.stride(1),
                 out.stride(0), out.stride(1), 1, 1, 0, 0, 0, 0, 0, 0, alpha, beta, ws, wsn, stream())

    if _gemm_timer is not None and _is_tile_gemm(M, N, K, a, b, out, a.stride(), b.stride(), out.stride()):
        _gemm_timer.wrap("gemm", 2.0 * M * N * K if useful_flops is None else useful_flops, run)
    else:
        run()
    return out


def gemm_nt_headbias_supported(M, N, K, split_n) -> bool:
    return bool(lib.load().db1_gemm_nt_headbias_supported(M, N, K, split_n))


def gemm_nt_headbias(x, w, out, qu, qv, bias_u, bias_v, split_n):
    """out[:, split_n:] = (x w^T)[:, split_n:];  qu = (x w^T)[:, :split_n] + bias_u, qv = ... + bias_v (bf16; out[:, :split_n] is NOT written)"""
    M, K = x.shape
    N = w.shape[0]
    assert x.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1 and qu.is_contiguous() and qv.is_contiguous()
    assert x.dtype == w.dtype == out.dtype == qu.dtype == bias_u.dtype == torch.bfloat16 and bias_u.numel() == split_n == bias_v.numel()

    def run():
        lib.call("db1_gemm_nt_headbias", P(x), P(w), P(out), P(qu), P(qv), P(bias_u), P(bias_v), M, N, K, split_n, x.stride(0), w.stride(0),
                 out.stride(0), split_n, stream())

    _timed("gemm", 2.0 * M * N * K, run)


def gemm_batched(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, beta: float = 0.0, tri=(0, 0)):
    """4-D views [z0, z1, rows, cols] with arbitrary strides (stride 0 broadcasts).
    ``tri`` = (mode, period): structural-zero hint for ``a`` (db1_gemm_strided_tri), an optimisation only."""
    Z0, Z1, M, K = a.shape
    _, _, K2, N = b.shape
    assert K == K2 and out.shape == (Z0, Z1, M, N) and b.shape[:2] == (Z0, Z1), (a.shape, b.shape, out.shape)

    def run():
        ws, wsn = _ws("db1_gemm_workspace_bytes", (M, N, K, dt_code(a), dt_code(b), dt_code(out), a.stride(2), a.stride(3), b.stride(2), b.stride(3),
                                                    out.stride(2), out.stride(3), Z0, Z1), out.device)
        lib.call("db1_gemm_strided_tri", P(a), P(b), P(out), _vp(0), M, N, K, dt_code(a), dt_code(b), dt_code(out), 0,
                 a.stride(2), a.stride(3), b.stride(2), b.stride(3), out.stride(2), out.stride(3), Z0, Z1,
                 a.stride(0), a.stride(1), b.stride(0), b.stride(1), out.stride(0), out.stride(1), alpha, beta, int(tri[0]), int(tri[1]),
                 ws, wsn, stream())

    # the batched contractions of the attention backward (dq_r, dR) run on the same tile kernels: timed with the FLOPs they execute
    # (k-tiles skipped under the structural-zero hint are not counted)
    if _gemm_timer is not None and _is_tile_gemm(M, N, K, a, b, out, a.stride()[2:], b.stride()[2:], out.stride()[2:]):
        _gemm_timer.wrap("gemm", 2.0 * M * N * K * Z0 * Z1 * _tri_fraction(M, K, int(tri[0]), int(tri[1])), run)
    else:
        run()
    return out


def relattn_dqr_supported(B, L, H, D, dtype) -> bool:
    return bool(lib.load().db1_relattn_dqr_supported(B, L, H, D, dt_code(dtype)))


def _dqr_bf16_only(who, *tensors):
    if any(t.dtype != torch.bfloat16 for t in tensors):
        raise lib.Db1Error(f"{who}: bf16 operands only")     # (the entry point takes no dtype: refused here, nothing launched)


def relattn_dqr(dT, R, dqv):
    """dqv[b, i, h, :] = sum_dist dT[h, b, i, dist] R[dist, h, :]  (dT [H,B,L,L] bf16 zero above the causal diagonal, R [L, H*D], dqv [B,L,H,D])"""
    H, B, L, _ = dT.shape
    D = dqv.shape[-1]
    assert dT.is_contiguous() and R.stride(1) == 1 and dqv.stride(3) == 1 and dqv.stride(2) == D
    _dqr_bf16_only("relattn_dqr", dT, R, dqv)
    ws, wsn = _ws("db1_relattn_dqr_workspace_bytes", (L, H), dT.device)
    # algorithmic bytes: the causal half of dT read once + the output written
    _timed("relattn_dqr", 2.0 * (H * B * L * (L + 1) / 2 + dqv.numel()),
           lambda: lib.call("db1_relattn_dqr", P(dT), P(R), R.stride(0), P(dqv), dqv.stride(1), dqv.stride(0), B, L, H, D, ws, wsn, stream()))


NO_DROP = (0.0, 0, 0, 0)   # (p, seed, site, step[, device step counter: the step used is step + *counter, read when the kernel runs[, rows per step]])


def _drop_dev(drop):
    return P(drop[4]) if len(drop) > 4 and drop[4] is not None else _vp(0)


def _drop_step(drop) -> int:
    return int(drop[3]) & 0xFFFFFFFF     # (a window backward passes first-step offsets below zero on top of a device counter: modulo 2^32 like the kernel's add)


def _drop_rps(drop) -> int:
    """rows per micro-step when the rows are a whole accumulation window's (db1_layernorm_residual_bwd: drop_rows_per_step), else 0"""
    return int(drop[5]) if len(drop) > 5 and drop[5] else 0


def dropout(x, y, drop):
    """y = dropout(x) with the counter-based keep decisions of ``drop = (p, seed, site, step)`` (y may alias x; also its own backward)"""
    p, seed, site, step = drop[:4]
    lib.call("db1_dropout", P(x), P(y), x.numel(), float(p), int(seed), int(site), _drop_step(drop), _drop_dev(drop), dt_code(x), stream())


def relattn_dqr_fused(dT, R, dq, du_acc, dv_acc):
    """dq[b,i,h,:] += sum_dist dT[h,b,i,dist] R[dist,h,:] (dq: a [B,L,H,D] view, e.g. the q slot of dqkv), du_acc += colsum of the incoming dq
    (the (q+u).k branch), dv_acc += colsum of the added term"""
    H, B, L, _ = dT.shape
    D = dq.shape[-1]
    assert dT.is_contiguous() and R.stride(1) == 1 and dq.stride(3) == 1 and dq.stride(2) == D and dq.shape == (B, L, H, D)
    assert du_acc.dtype == torch.float32 and dv_acc.dtype == torch.float32 and du_acc.numel() == H * D == dv_acc.numel()
    _dqr_bf16_only("relattn_dqr_fused", dT, R, dq)
    ws, wsn = _ws("db1_relattn_dqr_workspace_bytes", (L, H), dT.device)
    # algorithmic bytes: the causal half of dT read once, dq read and written
    _timed("relattn_dqr", 2.0 * (H * B * L * (L + 1) / 2 + 2 * dq.numel()),
           lambda: lib.call("db1_relattn_dqr_fused", P(dT), P(R), R.stride(0), P(dq), dq.stride(1), dq.stride(0), P(du_acc), P(dv_acc),
                            B, L, H, D, ws, wsn, stream()))


def relattn_dqr_groups_supported(B, L, H, D, dtype, ngroups) -> bool:
    return bool(lib.load().db1_relattn_dqr_groups_supported(B, L, H, D, dt_code(dtype), int(ngroups)))


def relattn_dqr_fused_groups(dT, Rg, dq, du_acc, dv_acc):
    """relattn_dqr_fused over a batch of ng = Rg.shape[0] blocks of B / ng sequences, block g with its own R = Rg[g] ([ng, L, H*D] view: a
    whole accumulation window's attention backward in one launch)"""
    H, B, L, _ = dT.shape
    D = dq.shape[-1]
    ng = Rg.shape[0]
    assert dT.is_contiguous() and Rg.dim() == 3 and Rg.stride(2) == 1 and dq.stride(3) == 1 and dq.stride(2) == D and dq.shape == (B, L, H, D)
    assert du_acc.dtype == torch.float32 and dv_acc.dtype == torch.float32 and du_acc.numel() == H * D == dv_acc.numel()
    _dqr_bf16_only("relattn_dqr_fused_groups", dT, Rg, dq)
    ws, wsn = _ws("db1_relattn_dqr_groups_workspace_bytes", (L, H, ng), dT.device)
    _timed("relattn_dqr", 2.0 * (H * B * L * (L + 1) / 2 + 2 * dq.numel()),
           lambda: lib.call("db1_relattn_dqr_fused_groups", P(dT), P(Rg), Rg.stride(1), Rg.stride(0), ng, P(dq), dq.stride(1), dq.stride(0), P(du_acc), P(dv_acc),
                            B, L, H, D, ws, wsn, stream()))


def relattn_dqr_parts_rows(H: int) -> int:
    return int(lib.load().db1_relattn_dqr_parts_rows(int(H)))


def relattn_dqr_fused_parts(dT, R, dq, parts):
    """relattn_dqr_fused without its two reduces: parts [2, rows, H * D] float32 receives the per-workgroup column sums (du half, dv half)"""
    H, B, L, _ = dT.shape
    D = dq.shape[-1]
    assert dT.is_contiguous() and R.stride(1) == 1 and dq.stride(3) == 1 and dq.stride(2) == D and dq.shape == (B, L, H, D)
    _dqr_bf16_only("relattn_dqr_fused_parts", dT, R, dq)
    assert parts.dtype == torch.float32 and parts.is_contiguous() and parts.shape == (2, relattn_dqr_parts_rows(H), H * D)
    ws, wsn = _ws("db1_relattn_dqr_workspace_bytes", (L, H), dT.device)
    _timed("relattn_dqr", 2.0 * (H * B * L * (L + 1) / 2 + 2 * dq.numel()),
           lambda: lib.call("db1_relattn_dqr_fused_parts", P(dT), P(R), R.stride(0), P(dq), dq.stride(1), dq.stride(0), P(parts),
                            B, L, H, D, ws, wsn, stream()))


def layernorm_residual_fwd(x, r, alpha, gamma, beta, y, s_out, mean, rstd, eps, drop=NO_DROP):
    rows, d = x.numel() // x.shape[-1], x.shape[-1]
    nstreams = 2 + (r is not None) + (s_out is not None)   # x [, r] in; y [, s] out
    _timed("layernorm_fwd", float(rows * d * x.element_size() * nstreams),
           lambda: lib.call("db1_layernorm_residual_fwd", P(x), P(r), float(alpha), P(gamma), P(beta), P(y), P(s_out), P(mean), P(rstd),
                            rows, d, float(eps), float(drop[0]), int(drop[1]), int(drop[2]), int(drop[3]), _drop_dev(drop), dt_code(x), dt_code(gamma), stream()))


def layernorm_residual_bwd(dy, s, gamma, mean, rstd, ds, dgamma_acc, dbeta_acc, dr_out=None, drop=NO_DROP):
    """``dr_out``: gradient of the (dropped) residual input r = ds under the forward's keep decisions; None when nothing was dropped"""
    rows, d = dy.numel() // dy.shape[-1], dy.shape[-1]
    ws, wsn = _ws("db1_layernorm_residual_bwd_workspace_bytes", (rows, d, dt_code(dy)), dy.device)
    _timed("layernorm_bwd", float(rows * d * dy.element_size() * (3 + (dr_out is not None))),   # dy, s in; ds [, dr] out
           lambda: lib.call("db1_layernorm_residual_bwd", P(dy), P(s), P(gamma), P(mean), P(rstd), P(ds), P(dr_out), P(dgamma_acc), P(dbeta_acc),
                            rows, d, float(drop[0]), int(drop[1]), int(drop[2]), _drop_step(drop), _drop_dev(drop), _drop_rps(drop), dt_code(dy), dt_code(gamma),
                            ws, wsn, stream()))


def layernorm_bwd_parts_numel(rows: int, d: int, dtype) -> int:
    """floats of the partial-sum matrix [blocks, 2 d] of db1_layernorm_residual_bwd_parts (0: this shape has no partials form)"""
    return int(lib.load().db1_layernorm_residual_bwd_workspace_bytes(int(rows), int(d), dt_code(dtype))) // 4


def layernorm_residual_bwd_parts(dy, s, gamma, mean, rstd, ds, parts, dr_out=None, drop=NO_DROP):
    """layernorm_residual_bwd without the parameter reduce: parts [blocks, 2 d] float32 receives the per-block (dgamma | dbeta) partial sums"""
    rows, d = dy.numel() // dy.shape[-1], dy.shape[-1]
    assert parts.dtype == torch.float32 and parts.is_contiguous()
    _timed("layernorm_bwd", float(rows * d * dy.element_size() * (3 + (dr_out is not None))),
           lambda: lib.call("db1_layernorm_residual_bwd_parts", P(dy), P(s), P(gamma), P(mean), P(rstd), P(ds), P(dr_out), P(parts), parts.numel() * 4,
                            rows, d, float(drop[0]), int(drop[1]), int(drop[2]), _drop_step(drop), _drop_dev(drop), _drop_rps(drop), dt_code(dy), dt_code(gamma),
                            stream()))


def ffn_act_fwd(z, out, act: str):
    rows, n = out.numel() // out.shape[-1], out.shape[-1]
    _timed("ffn_act_fwd", float((z.numel() + out.numel()) * z.element_size()),
           lambda: lib.call("db1_ffn_act_fwd", P(z), P(out), rows, n, ACT_CODES[act], dt_code(z), stream()))


def ffn_act_bwd(z, dout, dz, act: str):
    rows, n = dout.numel() // dout.shape[-1], dout.shape[-1]
    lib.call("db1_ffn_act_bwd", P(z), P(dout), P(dz), rows, n, ACT_CODES[act], dt_code(z), stream())


def ffn_act_bwd_bias(z, dout, dz, dbias_acc, act: str):
    """activation backward + dbias_acc += column sums of dz, one pass"""
    rows, n = dout.numel() // dout.shape[-1], dout.shape[-1]
    assert dbias_acc.dtype == torch.float32 and dbias_acc.numel() == dz.shape[-1]
    ws, wsn = _ws("db1_ffn_act_bwd_bias_workspace_bytes", (rows, n, ACT_CODES[act]), z.device)
    _timed("ffn_act_bwd", float((z.numel() + dout.numel() + dz.numel()) * z.element_size()),
           lambda: lib.call("db1_ffn_act_bwd_bias", P(z), P(dout), P(dz), P(dbias_acc), rows, n, ACT_CODES[act], dt_code(z), ws, wsn, stream()))


def gemm_nt_geglu_fused(M: int, dff: int, K: int, dtype, lda=None, ldw=None, ldz=None, ldact=None) -> bool:
    """does db1_gemm_nt_geglu run the activation inside the GEMM's epilogue at this shape (else: separate launches)"""
    return bool(lib.load().db1_gemm_nt_geglu_fused(M, dff, K, dt_code(dtype), lda or K, ldw or K, ldz or 2 * dff, ldact or dff))


def gemm_nn_geglu_bwd_fused(M: int, dff: int, K: int, dtype, lddy=None, ldw=None, ldz=None, lddz=None) -> bool:
    return bool(lib.load().db1_gemm_nn_geglu_bwd_fused(M, dff, K, dt_code(dtype), lddy or K, ldw or dff, ldz or 2 * dff, lddz or 2 * dff))


def gemm_nt_geglu(x, w1, bias, z, act):
    """z = x w1^T + bias  [M, 2 dff]   and   act = z[:, :dff] * gelu(z[:, dff:])  [M, dff]   (PositionwiseFF's first half, one launch where fused)"""
    M, K = x.shape
    dff = act.shape[1]
    assert w1.shape == (2 * dff, K) and z.shape == (M, 2 * dff) and x.stride(1) == 1 and w1.stride(1) == 1 and z.stride(1) == 1 and act.stride(1) == 1
    assert bias is None or bias.dtype == x.dtype
    ws, wsn = _ws("db1_gemm_workspace_bytes", (M, 2 * dff, K, dt_code(x), dt_code(w1), dt_code(z), x.stride(0), 1, 1, w1.stride(0), z.stride(0), 1, 1, 1), x.device)
    _timed("gemm", 2.0 * M * 2 * dff * K,
           lambda: lib.call("db1_gemm_nt_geglu", P(x), P(w1), P(bias), P(z), P(act), M, dff, K, x.stride(0), w1.stride(0), z.stride(0), act.stride(0),
                            dt_code(x), ws, wsn, stream()))


def gemm_nn_geglu_bwd(dy, w2, z, dz, dbias_acc):
    """dz = GEGLU'(z) applied to dact = dy w2 (w2 [K, dff] row-major; dact is never stored); dbias_acc [2 dff] fp32 += column sums of dz"""
    M, K = dy.shape
    dff = w2.shape[1]
    assert w2.shape[0] == K and z.shape == (M, 2 * dff) and dz.shape == (M, 2 * dff) and dbias_acc.dtype == torch.float32 and dbias_acc.numel() == 2 * dff
    assert dy.stride(1) == 1 and w2.stride(1) == 1 and z.stride(1) == 1 and dz.stride(1) == 1
    ws, wsn = _ws("db1_gemm_nn_geglu_bwd_workspace_bytes", (M, dff, K, dt_code(dy), dy.stride(0), w2.stride(0), z.stride(0), dz.stride(0)), dy.device)
    _timed("gemm", 2.0 * M * dff * K,
           lambda: lib.call("db1_gemm_nn_geglu_bwd", P(dy), P(w2), P(z), P(dz), P(dbias_acc), M, dff, K, dy.stride(0), w2.stride(0), z.stride(0), dz.stride(0),
                            dt_code(dy), ws, wsn, stream()))


def gemm_nn_geglu_bwd_parts(dy, w2, z, dz, parts):
    """gemm_nn_geglu_bwd without the bias reduce (fused shapes): parts [M / 128, 2 dff] float32 receives the column sums of dz per 128-row block"""
    M, K = dy.shape
    dff = w2.shape[1]
    assert w2.shape[0] == K and z.shape == (M, 2 * dff) and dz.shape == (M, 2 * dff) and parts.dtype == torch.float32 and parts.shape == (M // 128, 2 * dff)
    assert dy.stride(1) == 1 and w2.stride(1) == 1 and z.stride(1) == 1 and dz.stride(1) == 1 and parts.is_contiguous()
    _timed("gemm", 2.0 * M * dff * K,
           lambda: lib.call("db1_gemm_nn_geglu_bwd_parts", P(dy), P(w2), P(z), P(dz), P(parts), M, dff, K, dy.stride(0), w2.stride(0), z.stride(0), dz.stride(0),
                            dt_code(dy), stream()))


def colsum_acc(x2d, out_acc):
    rows, cols = x2d.shape
    assert x2d.stride(1) == 1 and out_acc.dtype == torch.float32
    ws, wsn = _ws("db1_colsum_acc_workspace_bytes", (rows, cols), x2d.device)
    lib.call("db1_colsum_acc", P(x2d), P(out_acc), rows, cols, x2d.stride(0), dt_code(x2d), ws, wsn, stream())


def add(a, b, y):
    lib.call("db1_add", P(a), P(b), P(y), a.numel(), dt_code(a), stream())


def add2d(a2d, b2d, y2d):
    """y = a + b on 2-D views with unit inner stride (y may alias b)."""
    rows, cols = y2d.shape
    assert a2d.stride(1) == 1 and b2d.stride(1) == 1 and y2d.stride(1) == 1 and b2d.dtype == y2d.dtype
    lib.call("db1_add2d", P(a2d), a2d.stride(0), P(b2d), b2d.stride(0), P(y2d), y2d.stride(0), rows, cols,
             dt_code(a2d), dt_code(y2d), stream())


def add2d_colsums(a2d, b2d, y2d, sum_a_acc, sum_b_acc):
    """y = a + b (y may alias b) and the float32 column sums of a and of b accumulated into sum_a_acc / sum_b_acc, one pass."""
    rows, cols = y2d.shape
    assert a2d.stride(1) == 1 and b2d.stride(1) == 1 and y2d.stride(1) == 1 and a2d.dtype == y2d.dtype == b2d.dtype
    assert sum_a_acc.dtype == torch.float32 and sum_b_acc.dtype == torch.float32
    ws, wsn = _ws("db1_add2d_colsums_workspace_bytes", (rows, cols), y2d.device)
    _timed("add2d_colsums", float(3 * rows * cols * y2d.element_size()),
           lambda: lib.call("db1_add2d_colsums", P(a2d), a2d.stride(0), P(b2d), b2d.stride(0), P(y2d), y2d.stride(0), P(sum_a_acc), P(sum_b_acc),
                            rows, cols, dt_code(y2d), ws, wsn, stream()))


def zero_segments(base, segments):
    """base[off : off + len] = 0 for every row (off, len) of the int64 device table ``segments`` [n, 2]; one launch"""
    assert base.dtype == torch.float32 and segments.dtype == torch.int64 and segments.dim() == 2 and segments.shape[1] == 2 and segments.is_contiguous()
    lib.call("db1_zero_segments", P(base), P(segments), segments.shape[0], stream())


def cast(x, y):
    lib.call("db1_cast", P(x), P(y), x.numel(), dt_code(x), dt_code(y), stream())


def embed_gather(table, ids, out2d):
    n, d = out2d.shape
    assert ids.dtype == torch.int64 and ids.numel() == n and out2d.stride(1) == 1
    lib.call("db1_embed_gather_fwd", P(table), P(ids), P(out2d), n, d, out2d.stride(0), table.shape[0], dt_code(table), dt_code(out2d), stream())


def vision_pos_add(out2d, row_table, col_table, row_ids, col_ids):
    """out[t] += row_table[row_ids[t]] + col_table[col_ids[t]] (db1_vision_pos_add)"""
    n, d = out2d.shape
    assert out2d.is_contiguous() and row_table.shape == col_table.shape and row_table.shape[1] == d and row_table.dtype == col_table.dtype
    assert row_ids.dtype == torch.int64 and col_ids.dtype == torch.int64 and row_ids.numel() == n == col_ids.numel()
    lib.call("db1_vision_pos_add", P(out2d), P(row_table), P(col_table), P(row_ids), P(col_ids), n, d, row_table.shape[0], dt_code(row_table), dt_code(out2d), stream())


def embed_scatter_add(dout2d, ids, dtable_acc):
    n, d = dout2d.shape
    assert ids.dtype == torch.int64 and dtable_acc.dtype == torch.float32 and dout2d.stride(1) == 1
    ws, wsn = _ws("db1_embed_scatter_add_workspace_bytes", (n,), dout2d.device)
    lib.call("db1_embed_scatter_add_bwd", P(dout2d), P(ids), P(dtable_acc), n, d, dout2d.stride(0), dtable_acc.shape[0], dt_code(dout2d), ws, wsn, stream())


def rl_assemble_fwd(word_table, pos_table, vis, ids, position_id, labels, out):
    B, L, d = out.shape
    nvis = 0 if vis is None else vis.shape[1]
    lib.call("db1_rl_assemble_fwd", P(word_table), P(pos_table), P(vis), P(ids), P(position_id), P(labels), P(out),
             B, L, d, nvis, word_table.shape[0], pos_table.shape[0], dt_code(word_table), dt_code(out), stream())


def rl_assemble_bwd(dout, ids, position_id, dword_acc, dpos_acc, dvis):
    B, L, d = dout.shape
    nvis = 0 if dvis is None else dvis.shape[1]
    ws, wsn = _ws("db1_rl_assemble_bwd_workspace_bytes", (B, L), dout.device)
    lib.call("db1_rl_assemble_bwd", P(dout), P(ids), P(position_id), P(dword_acc), P(dpos_acc), P(dvis), B, L, d, nvis,
             dword_acc.shape[0], dpos_acc.shape[0], dt_code(dout), ws, wsn, stream())


def masked_ce_fwd(logits2d, labels, mask, lse, sums, V):
    T, ld = logits2d.shape[0], logits2d.stride(0)
    ws, wsn = _ws("db1_masked_ce_fwd_workspace_bytes", (T,), logits2d.device)
    _timed("masked_ce_fwd", float(T * V * logits2d.element_size()),
           lambda: lib.call("db1_masked_ce_fwd", P(logits2d), P(labels), P(mask), P(lse), P(sums), T, V, ld, dt_code(logits2d), ws, wsn, stream()))


def masked_ce_bwd(logits2d, labels, mask, lse, sums, dlogits2d, V, gscale=1.0):
    T, ld = logits2d.shape[0], logits2d.stride(0)
    assert dlogits2d.stride(0) == ld
    _timed("masked_ce_bwd", float(2 * T * V * logits2d.element_size()),
           lambda: lib.call("db1_masked_ce_bwd", P(logits2d), P(labels), P(mask), P(lse), P(sums), P(dlogits2d), T, V, ld, float(gscale),
                            dt_code(logits2d), stream()))


def masked_ce_fwd_bwd(logits2d, labels, mask, lse, sums, norm, V, gscale=1.0):
    """lse, sums += (loss, mask) and logits2d overwritten by dlogits in ONE pass (db1_masked_ce_fwd_bwd); norm[1] = the loss normaliser"""
    T, ld = logits2d.shape[0], logits2d.stride(0)
    ws, wsn = _ws("db1_masked_ce_fwd_workspace_bytes", (T,), logits2d.device)
    lib.call("db1_masked_ce_fwd_bwd", P(logits2d), P(labels), P(mask), P(lse), P(sums), P(norm), T, V, ld, float(gscale), dt_code(logits2d), ws, wsn, stream())


DB1_ERR_BAD_SHAPE, DB1_ERR_UNSUPPORTED_DTYPE, DB1_ERR_UNSUPPORTED = -1, -3, -6


# The argument checks of the capturable wrappers below (selection, beam step, ring reorder, scoring): each raises ValueError, naming the
# function (``who``) and the argument, before anything is launched.
def _check_window(who, V, vocab_lo, vocab_hi):
    vocab_hi = V if vocab_hi is None else int(vocab_hi)
    vocab_lo = int(vocab_lo)
    if not 0 <= vocab_lo < vocab_hi <= V:
        raise ValueError(f"{who}: vocabulary window [{vocab_lo}, {vocab_hi}) is empty or outside [0, {V})")
    return vocab_lo, vocab_hi


def _check_logits(who, logits2d, V, vocab_lo, vocab_hi, supported):
    """``logits2d`` [M, ld] fp32 / bf16 with unit column stride, its first V columns valid (``V`` None: all of them), ``supported(V, ld)`` (the
    kernel's own predicate) and the window inside [0, V) -> (M, ld, V, vocab_lo, vocab_hi)"""
    if logits2d.dim() != 2 or logits2d.stride(1) != 1:
        raise ValueError(f"{who}: logits must be a 2-D tensor with unit column stride")
    if logits2d.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: logits dtype {logits2d.dtype} (float32 / bfloat16)")
    M, ld = logits2d.shape[0], logits2d.stride(0)
    V = logits2d.shape[1] if V is None else int(V)
    if not 0 < V <= logits2d.shape[1] or not supported(V, ld):
        raise ValueError(f"{who}: V={V} unsupported for logits of shape {tuple(logits2d.shape)}, row stride {ld}")
    return (M, ld, V) + _check_window(who, V, vocab_lo, vocab_hi)


def _check_tensor(who, name, x, dtype, shape, dev):
    """``x``: a contiguous ``dtype`` tensor on ``dev`` of ``shape`` -- an int: that many elements; a tuple: that shape, -1 for any size"""
    if isinstance(shape, int):
        ok = x.numel() == shape
    else:
        xs = tuple(x.shape)
        ok = xs == shape or (len(xs) == len(shape) and all(n in (-1, m) for n, m in zip(shape, xs)))
    if not ok or x.dtype != dtype or not x.is_contiguous() or x.device != dev:
        what = f"of {shape} elements" if isinstance(shape, int) else f"of shape {shape}"
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor {what} on {dev}")


def _check_next_ids(who, next_ids, M, dev):
    if next_ids.dtype != torch.int64 or next_ids.shape[0] != M or next_ids.numel() != M or next_ids.device != dev:
        raise ValueError(f"{who}: next_ids must be an int64 tensor of {M} rows (one element each) on {dev}")


def _check_sampling(who, greedy, temperature, top_k, top_p):
    if not greedy:
        if not (temperature > 0 and temperature < float("inf")):
            raise ValueError(f"{who}: temperature {temperature} must be > 0 when sampling")
        if not 0 < top_p <= 1:
            raise ValueError(f"{who}: top_p {top_p} must lie in (0, 1]")
        if top_k < 0:
            raise ValueError(f"{who}: top_k {top_k} must be >= 0")


def _check_rings(who, rings):
    """``rings``: contiguous 16-byte aligned [M, cap, ...] tensors of one shape, dtype and device -> (M, cap, the bytes of one slot, device)"""
    if not rings:
        raise ValueError(f"{who}: no rings")
    r0 = rings[0]
    if r0.dim() < 3:
        raise ValueError(f"{who}: rings must be [M, cap, ...] tensors")
    for r in rings:
        if r.shape != r0.shape or r.dtype != r0.dtype or not r.is_contiguous() or r.device != r0.device or r.data_ptr() % 16:
            raise ValueError(f"{who}: the rings must be contiguous 16-byte aligned tensors of one shape, dtype and device")
    return r0.shape[0], r0.shape[1], int(r0[0, 0].numel() * r0.element_size()), r0.device


def _check_logprobs(who, logprob, sum_logprob, rows, max_new, dev) -> bool:
    """the optional log-prob outputs of the selection wrappers: both None (False: the plain entry point) or both given (True: the ``_lp`` one),
    float32, contiguous, on ``dev``, ``logprob`` [rows, max_new] and ``sum_logprob`` [rows]"""
    if logprob is None and sum_logprob is None:
        return False
    if logprob is None or sum_logprob is None:
        raise ValueError(f"{who}: logprob and sum_logprob go together (one of them is None)")
    _check_tensor(who, "logprob", logprob, torch.float32, (rows, max_new), dev)
    _check_tensor(who, "sum_logprob", sum_logprob, torch.float32, (rows,), dev)
    return True


MAX_TOP_N = 16


def _check_top(who, top_n, top_ids, top_logprob, shape, dev) -> int:
    """the optional top-n outputs: all of ``top_n`` / ``top_ids`` / ``top_logprob`` unset (0: the entry point without them) or all given
    (``top_n``, 1 .. 16): int32 and float32, contiguous, on ``dev``, of ``shape + (top_n,)``"""
    if top_n is None and top_ids is None and top_logprob is None:
        return 0
    if top_n is None or top_ids is None or top_logprob is None:
        raise ValueError(f"{who}: top_n, top_ids and top_logprob go together (one of them is None)")
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or not 1 <= int(top_n) <= MAX_TOP_N:
        raise ValueError(f"{who}: top_n {top_n!r} must be an integer in [1, {MAX_TOP_N}]")
    _check_tensor(who, "top_ids", top_ids, torch.int32, tuple(shape) + (int(top_n),), dev)
    _check_tensor(who, "top_logprob", top_logprob, torch.float32, tuple(shape) + (int(top_n),), dev)
    return int(top_n)


def _check_slots(who, M, S, row_map, dev) -> int:
    """``S`` slots behind ``M`` logits rows -> S: with a ``row_map`` (int32 [M]) at least M of them; without one, row i is slot i and S = M"""
    if row_map is not None:
        _check_tensor(who, "row_map", row_map, torch.int32, M, dev)
        if S < M:
            raise ValueError(f"{who}: {M} logits rows for {S} slots")
    elif S != M:
        raise ValueError(f"{who}: hist holds {S} rows for {M} logits rows (no row_map)")
    return S


def _check_vectors(who, dev, n, optional=(), **vectors):
    """each of ``vectors`` (name=tensor, in the order given) is a contiguous int32 vector of ``n`` elements; one named in ``optional`` may be None"""
    for name, x in vectors.items():
        if x is not None or name not in optional:
            _check_tensor(who, name, x, torch.int32, n, dev)


def _check_outputs(who, rows, max_new, dev, next_ids, logprob, sum_logprob, top_n, top_ids, top_logprob):
    """what a selection or stop launch writes per row next to ``out`` [rows, max_new]: ``next_ids``, the optional log-prob outputs and the
    optional top-n outputs, which need the log-prob ones -> (lp: whether those are there, top: the top-n count or 0)"""
    _check_next_ids(who, next_ids, rows, dev)
    lp = _check_logprobs(who, logprob, sum_logprob, rows, max_new, dev)
    top = _check_top(who, top_n, top_ids, top_logprob, (rows, max_new), dev)
    if top and not lp:
        raise ValueError(f"{who}: top_n needs logprob and sum_logprob")
    return lp, top


def _output_args(lp, top, logprob, sum_logprob, top_ids, top_logprob):
    """the five log-prob / top-n arguments of an entry point that always takes them (``lp, top`` from ``_check_outputs``): NULL, 0 for what is off"""
    return (P(logprob) if lp else _vp(0), P(sum_logprob) if lp else _vp(0), top, P(top_ids) if top else _vp(0), P(top_logprob) if top else _vp(0))


def _own_output_args(lp, top, *outputs):
    """those of the plain / ``_lp`` / ``_top`` entry points, each of which takes only its own: none, the first two, all five"""
    args = _output_args(lp, top, *outputs)
    return (args[:2] if lp else ()) + (args[2:] if top else ())


def _check_hist(who, hist, dev):
    """``hist`` is a 2-D tensor -> (S, max_new), its shape; dtype, layout and device are looked at with the rows (``_check_constrain_rows``)"""
    if not torch.is_tensor(hist) or hist.dim() != 2:
        raise ValueError(f"{who}: hist must be a contiguous {torch.int32} tensor of shape (slots, max_new) on {dev}")
    return hist.shape


def _check_max_new(who, mx):
    if not 1 <= mx <= 4096:
        raise ValueError(f"{who}: max_new {mx} (the columns of hist) must lie in [1, 4096]")


def _check_constrain_rows(who, logits2d, V, hist, row_map, supported):
    """what the two constrain wrappers share once their lists are measured: the logits, the history and the slots behind the rows -> (M, ld, V)"""
    M, ld, V, _, _ = _check_logits(who, logits2d, V, 0, None, supported)
    _check_tensor(who, "hist", hist, torch.int32, tuple(hist.shape), logits2d.device)
    _check_slots(who, M, hist.shape[0], row_map, logits2d.device)
    return M, ld, V


def select_tokens_supported(V: int, ld: int, dtype) -> bool:
    return bool(lib.load().db1_select_tokens_supported(int(V), int(ld), dt_code(dtype)))


def select_tokens(logits2d, t, finished, lengths, out, next_ids, status, *, V=None, vocab_lo=0, vocab_hi=None, greedy=True, temperature=1.0,
                  top_k=0, top_p=1.0, seed=0, eos_id=-1, pad_id=0, step_base=0, stream_id=None, logprob=None, sum_logprob=None, top_n=None,
                  top_ids=None, top_logprob=None):
    """one token per row of ``logits2d`` [M, ld] (fp32 / bf16, the first V columns valid) on the device (db1_select_tokens): greedy, or
    Gumbel-max sampling at ``temperature`` after top-k / top-p, over the columns [vocab_lo, vocab_hi).  ``t`` (int32 [1], device): the token
    index within the generation, READ only; ``finished`` / ``lengths`` / ``status`` (int32 [M]) updated; the token goes to ``out`` [M, max_new]
    (int32) at column t and to ``next_ids`` (int64, [M] or a column of [M, q]: row stride taken from the tensor).  ``logprob`` (float32
    [M, max_new]) and ``sum_logprob`` (float32 [M]), both or neither: the chosen token's log-probability over the window goes to column t and is
    added to the row's sum (db1_select_tokens_lp; the choice itself is bit-identical).  ``top_n`` (1 .. 16), ``top_ids`` (int32) and
    ``top_logprob`` (float32), both [M, max_new, top_n], all or none and only with the log-prob outputs: the row's ``top_n`` most likely
    tokens and their log-probabilities go to [row, t, :] (db1_select_tokens_top, rule in include/db1_hip.h; everything else is
    bit-identical).  Capturable; raises ValueError on bad arguments before anything is launched."""
    who, dev = "select_tokens", logits2d.device
    M, ld, V, vocab_lo, vocab_hi = _check_logits(who, logits2d, V, vocab_lo, vocab_hi,
                                                 lambda V, ld: select_tokens_supported(V, max(ld, V), logits2d.dtype))
    _check_sampling(who, greedy, temperature, top_k, top_p)
    _check_vectors(who, dev, M, finished=finished, lengths=lengths, status=status)
    _check_vectors(who, dev, 1, t=t)
    _check_vectors(who, dev, M, optional=("stream_id",), stream_id=stream_id)
    _check_tensor(who, "out", out, torch.int32, (M, -1), dev)
    lp, top = _check_outputs(who, M, out.shape[1], dev, next_ids, logprob, sum_logprob, top_n, top_ids, top_logprob)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lib.call("db1_select_tokens_top" if top else "db1_select_tokens_lp" if lp else "db1_select_tokens", P(logits2d), M, V, max(ld, V), dt_code(logits2d), vocab_lo, vocab_hi,
             float(temperature), int(top_k), float(top_p), int(bool(greedy)), seed & 0xFFFFFFFF, seed >> 32, int(eos_id), int(pad_id),
             int(step_base), P(t), P(stream_id), P(finished), P(lengths), P(out), out.shape[1], P(next_ids), next_ids.stride(0), P(status),
             *_own_output_args(lp, top, logprob, sum_logprob, top_ids, top_logprob), _vp(0), 0, stream())


def select_tokens_slots_supported(V: int, ld: int, dtype) -> bool:
    return bool(lib.load().db1_select_tokens_slots_supported(int(V), int(ld), dt_code(dtype)))


def select_tokens_slots(logits2d, t, limit, finished, lengths, out, next_ids, status, *, V=None, vocab_lo=0, vocab_hi=None, greedy=True,
                        temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_id=-1, pad_id=0, step_base=0, stream_id=None, row_map=None, logprob=None,
                        sum_logprob=None, top_n=None, top_ids=None, top_logprob=None):
    """``select_tokens`` over SLOTS (db1_select_tokens_slots): ``t`` and ``limit`` are int32 [S], one token counter and one token limit per
    slot; a live slot's token goes to ``out`` [S, max_new] at column t[slot], then the launch sets t[slot] += 1 and, at t[slot] == limit[slot],
    finished[slot].  A slot with finished != 0 is vacant: it only gets ``pad_id`` in ``next_ids``.  ``row_map`` (int32 [M], distinct slots) says
    which slot each row of ``logits2d`` [M, ld] belongs to; None: row i is slot i and S = M.  ``finished`` / ``lengths`` / ``status`` /
    ``stream_id`` are int32 [S], ``next_ids`` int64 ([S] or a column of [S, q]).  ``logprob`` (float32 [S, max_new]) and ``sum_logprob``
    (float32 [S]), both or neither, as ``select_tokens`` takes them, indexed by the slot (db1_select_tokens_slots_lp); ``top_n``, ``top_ids``
    and ``top_logprob`` ([S, max_new, top_n]) likewise (db1_select_tokens_slots_top).  Capturable; raises ValueError on bad arguments
    before anything is launched."""
    _select_slots("select_tokens_slots", logits2d, None, (vocab_lo, vocab_hi, greedy, temperature, top_k, top_p, seed), t, limit, finished, lengths,
                  out, next_ids, status, V, eos_id, pad_id, step_base, stream_id, row_map, logprob, sum_logprob, top_n, top_ids, top_logprob)


def _select_slots(who, logits2d, params, sampling, t, limit, finished, lengths, out, next_ids, status, V, eos_id, pad_id, step_base, stream_id,
                  row_map, logprob, sum_logprob, top_n, top_ids, top_logprob):
    """the body of ``select_tokens_slots`` (``sampling``: the seven scalars every slot shares) and ``select_tokens_slots_per`` (None: ``params``)"""
    dev, per = logits2d.device, sampling is None
    supported = lambda V, ld: select_tokens_slots_supported(V, max(ld, V), logits2d.dtype)
    if per:
        M, ld, V, _, _ = _check_logits(who, logits2d, V, 0, None, supported)
    else:
        vocab_lo, vocab_hi, greedy, temperature, top_k, top_p, seed = sampling
        M, ld, V, vocab_lo, vocab_hi = _check_logits(who, logits2d, V, vocab_lo, vocab_hi, supported)
        _check_sampling(who, greedy, temperature, top_k, top_p)
    S = _check_slots(who, M, int(t.numel()) if row_map is not None else M, row_map, dev)
    _check_vectors(who, dev, S, optional=("stream_id",), t=t, limit=limit, finished=finished, lengths=lengths, status=status, stream_id=stream_id)
    if per:
        if params is None:
            raise ValueError(f"{who}: params is None")
        _check_tensor(who, "params", params, torch.int32, (S, SLOT_PARAM_WORDS), dev)
        if params.data_ptr() % 32:
            raise ValueError(f"{who}: params must be 32-byte aligned")
    _check_tensor(who, "out", out, torch.int32, (S, -1), dev)
    lp, top = _check_outputs(who, S, out.shape[1], dev, next_ids, logprob, sum_logprob, top_n, top_ids, top_logprob)
    head = (P(logits2d), M, V, max(ld, V), dt_code(logits2d))
    slots = (int(eos_id), int(pad_id), int(step_base), P(t), P(limit), P(stream_id), P(finished), P(lengths), P(out), out.shape[1], P(next_ids),
             next_ids.stride(0), P(status), P(row_map), S)
    outputs = (lp, top, logprob, sum_logprob, top_ids, top_logprob)
    if per:
        lib.call("db1_select_tokens_slots_per", *head, P(params), *slots, *_output_args(*outputs), _vp(0), 0, stream())
        return
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lib.call("db1_select_tokens_slots_top" if top else "db1_select_tokens_slots_lp" if lp else "db1_select_tokens_slots", *head, vocab_lo, vocab_hi,
             float(temperature), int(top_k), float(top_p), int(bool(greedy)), seed & 0xFFFFFFFF, seed >> 32, *slots, *_own_output_args(*outputs), _vp(0), 0, stream())


SLOT_PARAM_WORDS = 8


def pack_slot_params(greedy, temperature, top_k, top_p, seed, vocab_lo, vocab_hi) -> np.ndarray:
    """one slot's record of ``select_tokens_slots_per`` (db1_select_tokens_slots_per, include/db1_hip.h) -> int32 [8]; THE place the layout
    is written down on the host: word 0 ``greedy`` (0 / 1), 1 ``top_k``, 2 ``vocab_lo``, 3 ``vocab_hi``, 4 / 5 the low / high 32 bits of
    ``seed``, 6 the fp32 bits of ``1 / temperature`` (one fp32 division, the one the scalar forms do at the launch; 1.0 when greedy, as
    there), 7 the fp32 bits of ``top_p``.  Pure NumPy; nothing is validated here (``SamplingParams.resolve`` does that, and the kernel
    refuses a bad record slot by slot)."""
    w = np.zeros(SLOT_PARAM_WORDS, np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_t = np.float32(1) if greedy else np.float32(1) / np.float32(temperature)
    w[0] = 1 if greedy else 0
    w[1:4] = np.array([top_k, vocab_lo, vocab_hi], np.int64).astype(np.int32).view(np.uint32)
    w[4], w[5] = seed & 0xFFFFFFFF, seed >> 32
    w[6:8] = np.array([inv_t, top_p], np.float32).view(np.uint32)
    return w.view(np.int32)


def select_tokens_slots_per(logits2d, params, t, limit, finished, lengths, out, next_ids, status, *, V=None, eos_id=-1, pad_id=0, step_base=0,
                            stream_id=None, row_map=None, logprob=None, sum_logprob=None, top_n=None, top_ids=None, top_logprob=None):
    """``select_tokens_slots`` with every slot's OWN sampling parameters (db1_select_tokens_slots_per): ``params`` (int32 [S, 8], contiguous,
    on the device, 32-byte aligned; one ``pack_slot_params`` record per slot, indexed by the slot like ``t``) takes the place of
    ``vocab_lo, vocab_hi, greedy, temperature, top_k, top_p, seed``; everything else is as ``select_tokens_slots`` takes it, and a slot comes
    out exactly as that would leave it under the slot's values.  The records are device data, so the KERNEL checks them: a live slot whose
    window is not ``0 <= vocab_lo < vocab_hi <= V``, or which samples with ``1 / temperature`` not finite and positive, ``top_k < 0`` or
    ``top_p`` outside (0, 1], gets status bit 2 (value 4), ``finished`` = 1 and ``pad_id`` in ``next_ids``, nothing else of it touched; a
    greedy slot ignores words 1 and 4 .. 7.  Capturable; raises ValueError on bad arguments before anything is launched."""
    _select_slots("select_tokens_slots_per", logits2d, params, None, t, limit, finished, lengths, out, next_ids, status, V, eos_id, pad_id,
                  step_base, stream_id, row_map, logprob, sum_logprob, top_n, top_ids, top_logprob)


def constrain_logits_supported(V: int, ld: int, max_new: int, n_bad: int, dtype) -> bool:
    return bool(lib.load().db1_constrain_logits_supported(int(V), int(ld), int(max_new), int(n_bad), dt_code(dtype)))


def constrain_logits_pen_supported(V: int, ld: int, max_new: int, n_bad: int, n_bias: int, dtype) -> bool:
    return bool(lib.load().db1_constrain_logits_pen_supported(int(V), int(ld), int(max_new), int(n_bad), int(n_bias), dt_code(dtype)))


def constrain_logits(logits2d, t, hist, *, V=None, finished=None, row_map=None, repetition_penalty=1.0, no_repeat_ngram_size=0, bad=None,
                     eos_id=-1, min_new=0, frequency_penalty=0.0, presence_penalty=0.0, bias_ids=None, bias_val=None):
    """the decoding constraints of one step, IN PLACE on ``logits2d`` [M, ld] (fp32 / bf16, the first V columns valid) before a selection
    or beam step reads it (db1_constrain_logits, rule in include/db1_hip.h): the repetition penalty over each row's history, the no-repeat
    n-gram ban, the banned ids ``bad`` (int32, device; None: none) and EOS banned while t < ``min_new``; a ban is a -inf.  ``hist`` (int32
    [S, max_new]): the tokens every slot has generated so far; ``t`` (int32, device, READ only): [1], one counter for all rows, or [S], one
    per slot; ``finished`` (int32 [S] or None): rows left alone; ``row_map`` (int32 [M]) as ``select_tokens_slots`` takes it, None: row i is
    slot i and S = M.  ``frequency_penalty`` / ``presence_penalty`` (finite, 0 = off) and the bias list ``bias_ids`` (int32) / ``bias_val``
    (float32), device vectors of one length <= 1024 with DISTINCT ids, both or neither: with any of them set the call goes to
    db1_constrain_logits_pen (freq * count + pres off every generated token's logit, the biases added after; the rule is stated with the
    prototype), else to db1_constrain_logits exactly as before.  Capturable; raises ValueError on bad arguments before anything is launched."""
    who, dev, i32 = "constrain_logits", logits2d.device, torch.int32
    S, mx = _check_hist(who, hist, dev)
    if not torch.is_tensor(t) or not (bad is None or torch.is_tensor(bad)):
        raise ValueError(f"{who}: t and bad must be {i32} tensors on {dev} (bad: or None)")
    n_bad = 0 if bad is None else int(bad.numel())
    _check_max_new(who, mx)
    if n_bad > 1024:
        raise ValueError(f"{who}: {n_bad} banned ids (at most 1024)")
    M, ld, V = _check_constrain_rows(who, logits2d, V, hist, row_map,
                                     lambda V, ld: constrain_logits_supported(V, max(ld, V), mx, n_bad, logits2d.dtype))
    if t.numel() not in (1, S):
        raise ValueError(f"{who}: t must hold 1 or {S} elements")
    _check_vectors(who, dev, int(t.numel()), t=t)
    _check_vectors(who, dev, S, optional=("finished",), finished=finished)
    _check_vectors(who, dev, n_bad, optional=("bad",), bad=bad)
    theta = float(repetition_penalty)
    if not 0.0 < theta < float("inf"):
        raise ValueError(f"{who}: repetition_penalty {repetition_penalty} must be finite and > 0")
    theta32 = float(np.float32(theta))
    if not 0.0 < theta32 < float("inf") or not 0.0 < float(np.float32(1.0 / theta32)) < float("inf"):
        raise ValueError(f"{who}: repetition_penalty {repetition_penalty} and its inverse must be finite and > 0 in float32")
    if int(no_repeat_ngram_size) < 0 or int(min_new) < 0:
        raise ValueError(f"{who}: no_repeat_ngram_size {no_repeat_ngram_size} and min_new {min_new} must be >= 0")
    with np.errstate(over="ignore"):
        freq, pres = float(np.float32(frequency_penalty)), float(np.float32(presence_penalty))
    if not (abs(freq) < float("inf") and abs(pres) < float("inf")):
        raise ValueError(f"{who}: frequency_penalty {frequency_penalty} and presence_penalty {presence_penalty} must be finite in float32")
    if (bias_ids is None) != (bias_val is None):
        raise ValueError(f"{who}: bias_ids and bias_val go together (one of them is None)")
    n_bias = 0
    if bias_ids is not None:
        if not torch.is_tensor(bias_ids) or not torch.is_tensor(bias_val) or bias_ids.numel() != bias_val.numel():
            raise ValueError(f"{who}: bias_ids ({i32}) and bias_val (float32) must be device vectors of one length")
        n_bias = int(bias_ids.numel())
        if n_bias > 1024:
            raise ValueError(f"{who}: {n_bias} biases (at most 1024)")
        _check_tensor(who, "bias_ids", bias_ids, i32, n_bias, dev)
        _check_tensor(who, "bias_val", bias_val, torch.float32, n_bias, dev)
    head = (P(logits2d), M, V, max(ld, V), dt_code(logits2d), P(t), int(t.numel() == S and S > 1), P(hist), mx, P(finished), P(row_map), S,
            theta32, float(np.float32(1.0 / theta32)), min(int(no_repeat_ngram_size), 2 ** 31 - 1), P(bad if n_bad else None), n_bad,
            max(int(eos_id), -1), min(int(min_new), 2 ** 31 - 1))
    if freq != 0.0 or pres != 0.0 or n_bias:
        if not constrain_logits_pen_supported(V, max(ld, V), mx, n_bad, n_bias, logits2d.dtype):
            raise ValueError(f"{who}: db1_constrain_logits_pen does not support these shapes")
        lib.call("db1_constrain_logits_pen", *head, freq, pres, P(bias_ids if n_bias else None), P(bias_val if n_bias else None), n_bias,
                 _vp(0), 0, stream())
        return
    lib.call("db1_constrain_logits", *head, _vp(0), 0, stream())


MAX_STOP_SEQUENCES = 16
MAX_STOP_LEN = 16


def stop_match_supported(n_stop: int, max_new: int) -> bool:
    return bool(lib.load().db1_stop_match_supported(int(n_stop), int(max_new)))


def pack_stop_sequences(seqs):
    """stop sequences (1 .. 16 of 1 .. 16 token ids >= 0 each) -> (``stop_tok`` int32 [n, 16], sequence k in row k from column 0, the rest
    -1; ``stop_len`` int32 [n]): THE place the layout db1_stop_match reads is written down on the host.  Pure NumPy; raises ValueError."""
    seqs = [[int(v) for v in q] for q in seqs]
    if not 1 <= len(seqs) <= MAX_STOP_SEQUENCES:
        raise ValueError(f"pack_stop_sequences: {len(seqs)} sequences (1 .. {MAX_STOP_SEQUENCES})")
    tok = np.full((len(seqs), MAX_STOP_LEN), -1, np.int32)
    for k, q in enumerate(seqs):
        if not 1 <= len(q) <= MAX_STOP_LEN or min(q) < 0 or max(q) >= 2 ** 31:
            raise ValueError(f"pack_stop_sequences: sequence {k} must hold 1 .. {MAX_STOP_LEN} token ids >= 0")
        tok[k, :len(q)] = q
    return tok, np.array([len(q) for q in seqs], np.int32)


def stop_match(stop_tok, stop_len, lengths, checked, finished, stop_hit, out, next_ids, *, pad_id=0, row_map=None, logprob=None,
               sum_logprob=None, top_n=None, top_ids=None, top_logprob=None):
    """the stop sequences of one step, after its selection launch (db1_stop_match, rule in include/db1_hip.h): a slot whose ``lengths`` moved
    since the last look (``checked``) and whose output now ends in one of the sequences ``stop_tok`` int32 [n, 16] / ``stop_len`` int32 [n]
    (device, ``pack_stop_sequences``) loses the matched tokens (``pad_id`` in ``out`` [S, max_new] and in ``next_ids``), gets ``finished`` = 1,
    ``stop_hit`` = the sequence's index + 1 and ``lengths`` = ``checked`` = what is kept.  ``lengths`` / ``checked`` / ``finished`` /
    ``stop_hit``: int32 [S]; ``row_map`` (int32 [M]) as ``select_tokens_slots`` takes it, None: every slot.  ``logprob`` / ``sum_logprob``
    and ``top_n`` / ``top_ids`` / ``top_logprob`` as the selection takes them: the removed positions get 0 and -1 / -inf, the sum is rebuilt.
    Capturable; raises ValueError on bad arguments before anything is launched."""
    _stop_match("stop_match", False, stop_tok, stop_len, lengths, checked, finished, stop_hit, out, next_ids, pad_id, row_map, logprob,
                sum_logprob, top_n, top_ids, top_logprob)


def _stop_match(who, per, stop_tok, stop_len, lengths, checked, finished, stop_hit, out, next_ids, pad_id, row_map, logprob, sum_logprob, top_n,
                top_ids, top_logprob):
    """the body of ``stop_match`` (one list [n, 16] / [n]; n goes to the launch) and ``stop_match_per`` (``per``: [S, 16, 16] / [S, 16])"""
    i32 = torch.int32
    if not torch.is_tensor(out) or out.dim() != 2:
        raise ValueError(f"{who}: out must be a contiguous {i32} tensor of shape (slots, max_new)")
    dev, (S, mx) = out.device, out.shape
    if per:
        if not torch.is_tensor(stop_tok) or not torch.is_tensor(stop_len):
            raise ValueError(f"{who}: stop_tok [slots, {MAX_STOP_SEQUENCES}, {MAX_STOP_LEN}] and stop_len [slots, {MAX_STOP_SEQUENCES}] must be "
                             f"{i32} tensors on {dev}")
        if mx < 1:
            raise ValueError(f"{who}: max_new {mx}")
        n_arg, tok_shape, len_shape = (), (S, MAX_STOP_SEQUENCES, MAX_STOP_LEN), (S, MAX_STOP_SEQUENCES)
    else:
        if not torch.is_tensor(stop_tok) or not torch.is_tensor(stop_len) or stop_tok.dim() != 2:
            raise ValueError(f"{who}: stop_tok [n, {MAX_STOP_LEN}] and stop_len [n] must be {i32} tensors on {dev}")
        n = int(stop_tok.shape[0])
        if not 1 <= n <= MAX_STOP_SEQUENCES or not stop_match_supported(n, mx):
            raise ValueError(f"{who}: {n} stop sequences (1 .. {MAX_STOP_SEQUENCES}), max_new {mx}")
        n_arg, tok_shape, len_shape = (n,), (n, MAX_STOP_LEN), (n,)
    _check_tensor(who, "stop_tok", stop_tok, i32, tok_shape, dev)
    _check_tensor(who, "stop_len", stop_len, i32, len_shape, dev)
    _check_tensor(who, "out", out, i32, (S, mx), dev)
    _check_vectors(who, dev, S, lengths=lengths, checked=checked, finished=finished, stop_hit=stop_hit)
    M = S
    if row_map is not None:
        M = int(row_map.numel())
        _check_tensor(who, "row_map", row_map, i32, M, dev)
        if not 1 <= M <= S:
            raise ValueError(f"{who}: {M} rows for {S} slots")
    lp, top = _check_outputs(who, S, mx, dev, next_ids, logprob, sum_logprob, top_n, top_ids, top_logprob)
    lib.call("db1_stop_match_per" if per else "db1_stop_match", P(stop_tok), P(stop_len), *n_arg, int(pad_id), P(lengths), P(checked), P(finished),
             P(stop_hit), P(out), mx, P(next_ids), next_ids.stride(0), P(row_map), M, S,
             *_output_args(lp, top, logprob, sum_logprob, top_ids, top_logprob), stream())


SLOT_CONS_WORDS = 8
MAX_SLOT_LIST = 1024      # the most a slot's banned-id or bias row can hold (db1_constrain_logits_slots_supported)


def pack_slot_constraints(cons, eos_id, bad_cap: int, bias_cap: int):
    """one slot's constraints as ``constrain_logits_slots_per`` and ``stop_match_per`` read them (include/db1_hip.h) -> (``rec`` int32 [8],
    ``bad`` int32 [bad_cap], ``bias_ids`` int32 [bias_cap], ``bias_val`` float32 [bias_cap], ``stop_tok`` int32 [16, 16], ``stop_len``
    int32 [16]); THE place the record's layout is written down on the host: word 0 the fp32 bits of ``theta`` (the repetition penalty), 1
    those of ``1 / theta`` (one fp32 division, the one the scalar forms do), 2 ``ngram``, 3 ``min_new`` (0 when ``eos_id`` is None or
    negative), 4 / 5 the fp32 bits of the frequency / presence penalty, 6 ``n_bad``, 7 ``n_bias``.  Unused list entries are -1 (ids) and
    0.0 (bias values); the stop table is ``pack_stop_sequences``' with length 0 in the unused entries.  ``cons``: a ``DecodingConstraints``
    or None (the record that edits nothing).  Pure NumPy; raises ValueError for what the kernel's guard would refuse and for lists beyond
    the capacities."""
    bad_cap, bias_cap = int(bad_cap), int(bias_cap)
    if not (0 <= bad_cap <= MAX_SLOT_LIST and 0 <= bias_cap <= MAX_SLOT_LIST):
        raise ValueError(f"pack_slot_constraints: capacities {bad_cap}, {bias_cap} must lie in [0, {MAX_SLOT_LIST}]")
    theta, ngram, min_new, freq, pres, ids, bias, stops = 1.0, 0, 0, 0.0, 0.0, (), (), ()
    if cons is not None:
        theta, ngram, min_new = cons.repetition_penalty, cons.no_repeat_ngram_size, cons.min_new_tokens
        freq, pres, ids, bias, stops = cons.frequency_penalty, cons.presence_penalty, cons.bad_token_ids, cons.logit_bias, cons.stop_sequences
    if len(ids) > bad_cap:
        raise ValueError(f"pack_slot_constraints: {len(ids)} banned ids for a capacity of {bad_cap}")
    if len(bias) > bias_cap:
        raise ValueError(f"pack_slot_constraints: {len(bias)} biases for a capacity of {bias_cap}")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        f = np.array([theta, 0.0, freq, pres], np.float32)
        f[1] = np.float32(1) / f[0]
    if not (np.isfinite(f).all() and f[0] > 0 and f[1] > 0):
        raise ValueError(f"pack_slot_constraints: repetition_penalty {theta} and its inverse must be finite and > 0, frequency_penalty {freq} "
                         f"and presence_penalty {pres} finite, all in float32")
    if int(ngram) < 0 or int(min_new) < 0:
        raise ValueError(f"pack_slot_constraints: no_repeat_ngram_size {ngram} and min_new_tokens {min_new} must be >= 0")
    if eos_id is None or int(eos_id) < 0:
        min_new = 0
    w = np.zeros(SLOT_CONS_WORDS, np.uint32)
    w[0:2] = f[0:2].view(np.uint32)
    w[2:4] = np.minimum(np.array([ngram, min_new], np.int64), 2 ** 31 - 1).astype(np.int32).view(np.uint32)
    w[4:6] = f[2:4].view(np.uint32)
    w[6], w[7] = len(ids), len(bias)
    bad = np.full(bad_cap, -1, np.int32)
    bad[:len(ids)] = np.asarray(ids, np.int64)
    bias_ids, bias_val = np.full(bias_cap, -1, np.int32), np.zeros(bias_cap, np.float32)
    bias_ids[:len(bias)] = [k for k, _ in bias]
    bias_val[:len(bias)] = [b for _, b in bias]
    stop_tok, stop_len = np.full((MAX_STOP_SEQUENCES, MAX_STOP_LEN), -1, np.int32), np.zeros(MAX_STOP_SEQUENCES, np.int32)
    if stops:
        tok, n = pack_stop_sequences(stops)
        stop_tok[:len(n)], stop_len[:len(n)] = tok, n
    return w.view(np.int32), bad, bias_ids, bias_val, stop_tok, stop_len


def constrain_logits_slots_supported(V: int, ld: int, max_new: int, bad_cap: int, bias_cap: int, dtype) -> bool:
    return bool(lib.load().db1_constrain_logits_slots_supported(int(V), int(ld), int(max_new), int(bad_cap), int(bias_cap), dt_code(dtype)))


def constrain_logits_slots_per(logits2d, cons, t, hist, finished, status, *, V=None, row_map=None, bad=None, bias_ids=None, bias_val=None,
                               eos_id=-1):
    """``constrain_logits`` with every slot's OWN constraints (db1_constrain_logits_slots_per, rule in include/db1_hip.h): ``cons`` (int32
    [S, 8], contiguous, on the device, 32-byte aligned; one ``pack_slot_constraints`` record per slot, indexed by the slot like ``t``), the
    banned ids ``bad`` (int32 [S, bad_cap]) and the biases ``bias_ids`` (int32) / ``bias_val`` (float32) [S, bias_cap], row s the lists of
    slot s (None: a capacity of 0), take the place of the scalars and the shared lists; ``t`` int32 [S], ``hist`` int32 [S, max_new].  A
    valid slot's row comes out exactly as ``constrain_logits`` would leave it under the slot's values.  The records are device data, so the
    KERNEL checks them: a live slot whose record it refuses gets status bit 3 (value 8) in ``status`` and ``finished`` = 1 (both int32 [S],
    written), its logits untouched.  Capturable; raises ValueError on bad arguments before anything is launched."""
    who, dev, i32 = "constrain_logits_slots_per", logits2d.device, torch.int32
    S, mx = _check_hist(who, hist, dev)
    _check_max_new(who, mx)
    caps = []
    for name, x in (("bad", bad), ("bias_ids", bias_ids), ("bias_val", bias_val)):
        if x is not None and (not torch.is_tensor(x) or x.dim() != 2):
            raise ValueError(f"{who}: {name} must be a tensor of shape (slots, capacity) on {dev}, or None")
        caps.append(0 if x is None else int(x.shape[1]))
    bad_cap, bias_cap = caps[0], caps[1]
    if caps[1] != caps[2]:
        raise ValueError(f"{who}: bias_ids and bias_val must have one shape (or both be None)")
    if bad_cap > MAX_SLOT_LIST or bias_cap > MAX_SLOT_LIST:
        raise ValueError(f"{who}: capacities {bad_cap}, {bias_cap} (at most {MAX_SLOT_LIST})")
    M, ld, V = _check_constrain_rows(who, logits2d, V, hist, row_map,
                                     lambda V, ld: constrain_logits_slots_supported(V, max(ld, V), mx, bad_cap, bias_cap, logits2d.dtype))
    for name, x in (("t", t), ("finished", finished), ("status", status), ("cons", cons)):
        if not torch.is_tensor(x):      # (none of them is optional here: the guard writes finished and status)
            raise ValueError(f"{who}: {name} must be a {i32} tensor on {dev}, got {type(x).__name__}")
    _check_vectors(who, dev, S, t=t, finished=finished, status=status)
    _check_tensor(who, "cons", cons, i32, (S, SLOT_CONS_WORDS), dev)
    if cons.data_ptr() % 32:
        raise ValueError(f"{who}: cons must be 32-byte aligned")
    if bad_cap:
        _check_tensor(who, "bad", bad, i32, (S, bad_cap), dev)
    if bias_cap:
        _check_tensor(who, "bias_ids", bias_ids, i32, (S, bias_cap), dev)
        _check_tensor(who, "bias_val", bias_val, torch.float32, (S, bias_cap), dev)
    lib.call("db1_constrain_logits_slots_per", P(logits2d), M, V, max(ld, V), dt_code(logits2d), P(t), P(hist), mx, P(finished), P(status),
             P(row_map), S, P(cons), P(bad if bad_cap else None), bad_cap, P(bias_ids if bias_cap else None),
             P(bias_val if bias_cap else None), bias_cap, max(int(eos_id), -1), _vp(0), 0, stream())


def stop_match_per(stop_tok, stop_len, lengths, checked, finished, stop_hit, out, next_ids, *, pad_id=0, row_map=None, logprob=None,
                   sum_logprob=None, top_n=None, top_ids=None, top_logprob=None):
    """``stop_match`` with every slot's OWN list (db1_stop_match_per, rule in include/db1_hip.h): ``stop_tok`` int32 [S, 16, 16] and
    ``stop_len`` int32 [S, 16] (device; slot s's ``pack_slot_constraints`` table at [s]; an unused entry has length 0), everything else as
    ``stop_match`` takes it, and a slot comes out exactly as that would leave it under the slot's list.  Capturable; raises ValueError on
    bad arguments before anything is launched."""
    _stop_match("stop_match_per", True, stop_tok, stop_len, lengths, checked, finished, stop_hit, out, next_ids, pad_id, row_map, logprob,
                sum_logprob, top_n, top_ids, top_logprob)


SPEC_MAX_Q = 16           # 1 + the most draft tokens of a speculative step (db1_spec_pick)
SPEC_MAX_HIST = 4096      # the prompt text + max_new tokens a row's draft lookup can stage (db1_spec_accept)
SPEC_MAX_NGRAM = 8


def _check_spec_width(who, M, q_in, Q):
    """the widths every speculative launch shares (pure Python: nothing is loaded): 2 <= Q <= 16, 1 <= q_in <= Q, M * Q <= 65535"""
    for name, v in (("Q", Q), ("q_in", q_in)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: {name} {v!r} must be an integer")
    if not 2 <= int(Q) <= SPEC_MAX_Q:
        raise ValueError(f"{who}: Q {Q} must lie in [2, {SPEC_MAX_Q}] (1 + the number of draft tokens)")
    if not 1 <= int(q_in) <= int(Q):
        raise ValueError(f"{who}: q_in {q_in} must lie in [1, Q = {Q}]")
    if not 1 <= int(M) or int(M) * int(Q) > 65535:
        raise ValueError(f"{who}: {M} rows of Q = {Q} positions (1 <= M, M * Q <= 65535)")


def spec_supported(V: int, ld: int, dtype, Q: int, ctx_cap: int, max_new: int, ngram_min: int = 1, ngram_max: int = 3, cap: int = 1) -> bool:
    """whether the three launches of a speculative step (db1_spec_pick / _accept / _commit) take these sizes"""
    L = lib.load()
    return bool(L.db1_spec_pick_supported(int(V), int(ld), dt_code(dtype), int(Q)) and
                L.db1_spec_accept_supported(int(Q), int(ctx_cap), int(max_new), int(ngram_min), int(ngram_max)) and
                L.db1_spec_commit_supported(int(Q), int(cap)))


def spec_pick(logits2d, t, finished, ids, sel, hit, *, q_in, V=None, vocab_lo=0, vocab_hi=None, greedy=True, temperature=1.0, top_k=0, top_p=1.0,
              seed=0, pad_id=0, step_base=0, stream_id=None, lp=None, max_new):
    """launch 1 of a speculative step (db1_spec_pick, rule in include/db1_hip.h): for row r and position i < ``q_in``, logits row r * q_in + i
    of ``logits2d`` [M * q_in, ld], the token ``select_tokens`` would pick at token index ``t`` + i goes to ``sel`` [M, Q] (int32; -1: no
    candidate, -2: the row is finished or the index is past ``max_new``), ``hit`` [M, Q] says whether column i + 1 of ``ids`` (int64 [M, Q],
    contiguous; READ only) holds that token, and ``lp`` (float32 [M, Q], optional) receives its log-probability.  ``t`` int32 [1] and
    ``finished`` int32 [M] are only read.  Capturable; raises ValueError on bad arguments before the library is loaded."""
    who, dev = "spec_pick", logits2d.device
    if not torch.is_tensor(ids) or ids.dim() != 2:
        raise ValueError(f"{who}: ids must be a contiguous {torch.int64} tensor of shape (rows, Q)")
    M, Q = int(ids.shape[0]), int(ids.shape[1])
    _check_spec_width(who, M, q_in, Q)
    q_in = int(q_in)
    if logits2d.dim() != 2 or logits2d.stride(1) != 1 or logits2d.shape[0] != M * q_in:
        raise ValueError(f"{who}: logits must be a 2-D tensor of {M} * {q_in} rows with unit column stride")
    if logits2d.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: logits dtype {logits2d.dtype} (float32 / bfloat16)")
    if int(max_new) < 1:
        raise ValueError(f"{who}: max_new {max_new} must be >= 1")
    ld = logits2d.stride(0)
    V = logits2d.shape[1] if V is None else int(V)
    if not 0 < V <= logits2d.shape[1]:
        raise ValueError(f"{who}: V={V} for logits of shape {tuple(logits2d.shape)}")
    vocab_lo, vocab_hi = _check_window(who, V, vocab_lo, vocab_hi)
    _check_sampling(who, greedy, temperature, top_k, top_p)
    _check_tensor(who, "ids", ids, torch.int64, (M, Q), dev)
    _check_vectors(who, dev, M, finished=finished)
    _check_vectors(who, dev, 1, t=t)
    _check_vectors(who, dev, M, optional=("stream_id",), stream_id=stream_id)
    _check_tensor(who, "sel", sel, torch.int32, (M, Q), dev)
    _check_tensor(who, "hit", hit, torch.int32, (M, Q), dev)
    if lp is not None:
        _check_tensor(who, "lp", lp, torch.float32, (M, Q), dev)
    if not lib.load().db1_spec_pick_supported(V, max(ld, V), dt_code(logits2d), Q):
        raise ValueError(f"{who}: V={V} unsupported for logits of shape {tuple(logits2d.shape)}, row stride {ld}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lib.call("db1_spec_pick", P(logits2d), M, q_in, Q, V, max(ld, V), dt_code(logits2d), vocab_lo, vocab_hi, float(temperature), int(top_k),
             float(top_p), int(bool(greedy)), seed & 0xFFFFFFFF, seed >> 32, int(pad_id), int(step_base), P(t), P(stream_id), P(finished),
             int(max_new), P(ids), P(sel), P(hit), P(lp), stream())


def spec_accept(t, sel, hit, finished, lengths, out, status, ids, n_acc, *, q_in, V, eos_id=-1, pad_id=0, lp=None, logprob=None, sum_logprob=None,
                ctx=None, ctx_len=None, script=None, ngram_min=1, ngram_max=3):
    """launch 2 of a speculative step (db1_spec_accept): from ``sel`` / ``hit`` [M, Q] the accepted count goes to ``n_acc`` (int32 [1]), every
    row commits that many tokens into ``out`` [M, max_new] at column ``t`` on (``lengths`` / ``finished`` / ``status`` int32 [M] and, with
    ``lp`` [M, Q], ``logprob`` [M, max_new] / ``sum_logprob`` [M] updated), its last token goes to column 0 of ``ids`` (int64 [M, Q]) and the
    next Q - 1 drafts to the other columns: from ``script`` (int32 [M, max_new]) if given, else by n-gram lookup (``ngram_max`` down to
    ``ngram_min``) over ``ctx`` (int32 [M, ctx_cap], ``ctx_len`` int32 [M]; both or neither) followed by the row's output.  ``t`` is only read.
    Capturable; raises ValueError on bad arguments before the library is loaded."""
    who = "spec_accept"
    i32 = torch.int32
    if not torch.is_tensor(ids) or ids.dim() != 2:
        raise ValueError(f"{who}: ids must be a contiguous {torch.int64} tensor of shape (rows, Q)")
    if not torch.is_tensor(out) or out.dim() != 2:
        raise ValueError(f"{who}: out must be a contiguous {i32} tensor of shape (rows, max_new)")
    dev, (M, Q), mx = out.device, (int(ids.shape[0]), int(ids.shape[1])), int(out.shape[1])
    _check_spec_width(who, M, q_in, Q)
    for name, v in (("ngram_min", ngram_min), ("ngram_max", ngram_max)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= SPEC_MAX_NGRAM:
            raise ValueError(f"{who}: {name} {v!r} must be an integer in [1, {SPEC_MAX_NGRAM}]")
    if int(ngram_min) > int(ngram_max):
        raise ValueError(f"{who}: ngram_min {ngram_min} exceeds ngram_max {ngram_max}")
    if int(V) < 1 or mx < 1:
        raise ValueError(f"{who}: V={V}, max_new={mx}")
    if (ctx is None) != (ctx_len is None):
        raise ValueError(f"{who}: ctx and ctx_len go together (one of them is None)")
    ctx_cap = 0
    if ctx is not None:
        if not torch.is_tensor(ctx) or ctx.dim() != 2 or ctx.shape[1] < 1:
            raise ValueError(f"{who}: ctx must be a contiguous {i32} tensor of shape (rows, ctx_cap >= 1)")
        ctx_cap = int(ctx.shape[1])
    if ctx_cap + mx > SPEC_MAX_HIST:
        raise ValueError(f"{who}: ctx_cap {ctx_cap} + max_new {mx} exceeds {SPEC_MAX_HIST}, the history a row's lookup can stage")
    if (lp is None) != (logprob is None) or (logprob is None) != (sum_logprob is None):
        raise ValueError(f"{who}: lp, logprob and sum_logprob go together (all or none)")
    _check_tensor(who, "ids", ids, torch.int64, (M, Q), dev)
    _check_tensor(who, "out", out, i32, (M, mx), dev)
    _check_tensor(who, "sel", sel, i32, (M, Q), dev)
    _check_tensor(who, "hit", hit, i32, (M, Q), dev)
    _check_vectors(who, dev, M, finished=finished, lengths=lengths, status=status)
    _check_vectors(who, dev, 1, t=t, n_acc=n_acc)
    if lp is not None:
        _check_tensor(who, "lp", lp, torch.float32, (M, Q), dev)
        _check_logprobs(who, logprob, sum_logprob, M, mx, dev)
    if ctx is not None:
        _check_tensor(who, "ctx", ctx, i32, (M, ctx_cap), dev)
        _check_vectors(who, dev, M, ctx_len=ctx_len)
    if script is not None:
        _check_tensor(who, "script", script, i32, (M, mx), dev)
    lib.call("db1_spec_accept", M, int(q_in), Q, int(eos_id), int(pad_id), int(V), mx, P(t), P(sel), P(hit), P(lp), P(finished), P(lengths), P(out),
             P(status), P(logprob), P(sum_logprob), P(ids), P(ctx), P(ctx_len), ctx_cap, P(script), int(ngram_min), int(ngram_max), P(n_acc), stream())


def spec_commit(t, n_acc, *, q_in, Q, hist=None, ring_state=None, cap=0):
    """launch 3 of a speculative step (db1_spec_commit, one thread): ``t`` += ``n_acc`` (both int32 [1]); ``ring_state`` (int32 [1], optional)
    goes back by the ``q_in`` - n_acc positions that were not kept, modulo ``cap``; ``hist`` (int32 [Q + 1], optional) counts the step under
    its accepted count.  Capturable; raises ValueError on bad arguments before the library is loaded."""
    who, dev = "spec_commit", t.device
    _check_spec_width(who, 1, q_in, Q)
    _check_vectors(who, dev, 1, t=t, n_acc=n_acc)
    if hist is not None:
        _check_tensor(who, "hist", hist, torch.int32, (int(Q) + 1,), dev)
    if ring_state is not None:
        _check_vectors(who, dev, 1, ring_state=ring_state)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or int(cap) <= 0 or int(cap) < int(q_in):
            raise ValueError(f"{who}: cap {cap!r} must be a positive integer, at least q_in = {q_in}")
    lib.call("db1_spec_commit", P(t), P(n_acc), P(hist), int(q_in), int(Q), P(ring_state), int(cap), stream())


def beam_step_supported(V: int, ld: int, W: int, dtype) -> bool:
    return bool(lib.load().db1_beam_step_supported(int(V), int(ld), int(W), dt_code(dtype)))


def beam_step_diverse_supported(V: int, ld: int, W: int, D: int, dtype) -> bool:
    """``W``: the beams of ONE sub-group (W'), ``D`` sub-groups per prompt"""
    return bool(lib.load().db1_beam_step_diverse_supported(int(V), int(ld), int(W), int(D), dt_code(dtype)))


def _beam_step(who, logits2d, t, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done, switches, next_ids,
               status, W, D, lam, V, vocab_lo, vocab_hi, eos_id, pad_id, length_penalty):
    """``beam_step`` (D = 1, lam = 0) and ``beam_step_diverse``: every host check over the Q = M / W (sub-)groups of W beams, then the
    library's own predicate, then db1_<who> (the diverse symbols take D, and lambda, next to W)"""
    dev, W, D, lam, i32, f32 = logits2d.device, int(W), int(D), float(lam), torch.int32, torch.float32
    d = (D,) if who == "beam_step_diverse" else ()
    if W < 1 or D < 1 or D * W > 16:
        raise ValueError(f"{who}: W={W} beams in each of D={D} sub-groups: both must be >= 1 and D * W <= 16")
    if not 0 <= lam < float("inf"):
        raise ValueError(f"{who}: diversity_penalty {lam} must be finite and >= 0")
    M, ld, V, vocab_lo, vocab_hi = _check_logits(who, logits2d, V, vocab_lo, vocab_hi, lambda V, ld: True)      # (the library's predicate: below)
    if M % (D * W) != 0 or M == 0:
        raise ValueError(f"{who}: D * W = {D * W} must divide the {M} rows")
    G, Q = M // (D * W), M // W
    lp = float(length_penalty)
    if not abs(lp) < float("inf"):
        raise ValueError(f"{who}: length_penalty {length_penalty} must be finite")
    _check_tensor(who, "tokens", tokens, i32, (M, -1), dev)
    mx = tokens.shape[1]
    if mx < 1:
        raise ValueError(f"{who}: max_new must be >= 1")
    for name, x, shape, dt in (("t", t, (1,), i32), ("beam_score", beam_score, (M,), f32), ("parent", parent, (M,), i32),
                               ("pool_tokens", pool_tokens, (Q, W, mx), i32), ("pool_len", pool_len, (Q, W), i32),
                               ("pool_score", pool_score, (Q, W), f32), ("pool_slot", pool_slot, (Q, W), i32),
                               ("pool_count", pool_count, (Q,), i32), ("done", done, (Q,), i32), ("switches", switches, (Q,), i32),
                               ("status", status, (Q,), i32)):
        _check_tensor(who, name, x, dt, shape, dev)
    _check_next_ids(who, next_ids, M, dev)
    if M > 65535:
        raise ValueError(f"{who}: {M} rows (at most 65535)")
    sym, code, ld = "db1_" + who, dt_code(logits2d), max(ld, V)
    if not getattr(lib.load(), sym + "_supported")(V, ld, W, *d, code):      # (the library's own predicate, after every host check)
        raise ValueError(f"{who}: V={V} unsupported for logits of shape {tuple(logits2d.shape)}, row stride {logits2d.stride(0)}")
    ws, wsn = _ws(sym + "_workspace_bytes", (M, V, W, *d, mx, code), dev)
    lib.call(sym, P(logits2d), G, *((D, W, lam) if d else (W,)), V, ld, code, vocab_lo, vocab_hi, int(eos_id), int(pad_id), lp, P(t), mx,
             P(beam_score), P(parent), P(tokens), P(pool_tokens), P(pool_len), P(pool_score), P(pool_slot), P(pool_count), P(done), P(switches),
             P(next_ids), next_ids.stride(0), P(status), ws, wsn, stream())


def beam_step(logits2d, t, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done, switches, next_ids, status,
              *, W, V=None, vocab_lo=0, vocab_hi=None, eos_id=-1, pad_id=0, length_penalty=1.0):
    """one beam-search step over ``logits2d`` [M, ld] (fp32 / bf16, the first V columns valid, M = G * W rows) on the device
    (db1_beam_step, rule in include/db1_hip.h): ``t`` (int32 [1]) READ only; beam_score (float32 [M]), parent (int32 [M]), tokens (int32
    [M, max_new]), the pool (pool_tokens int32 [G, W, max_new], pool_len / pool_slot int32 [G, W], pool_score float32 [G, W]) and pool_count /
    done / switches / status (int32 [G]) updated; the next ids go to ``next_ids`` (int64, [M] or a column of [M, q]).  Capturable; raises
    ValueError on bad arguments before anything is launched."""
    _beam_step("beam_step", logits2d, t, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done, switches,
               next_ids, status, W, 1, 0.0, V, vocab_lo, vocab_hi, eos_id, pad_id, length_penalty)


def beam_step_diverse(logits2d, t, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done, switches, next_ids,
                      status, *, W, D, diversity_penalty, V=None, vocab_lo=0, vocab_hi=None, eos_id=-1, pad_id=0, length_penalty=1.0):
    """one diverse (group) beam-search step over ``logits2d`` [M, ld] (M = G * D * W rows: G prompts, ``D`` sub-groups of ``W`` beams each,
    row (g * D + d) * W + j) on the device (db1_beam_step_diverse, rule in include/db1_hip.h): every state tensor is what ``beam_step`` takes
    for G * D groups of ``W`` beams; a token chosen by an earlier sub-group of the prompt in this step costs a later one
    ``diversity_penalty`` per earlier choice in the ranking, never in a stored score.  Capturable; raises ValueError on bad arguments before
    anything is launched."""
    _beam_step("beam_step_diverse", logits2d, t, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done,
               switches, next_ids, status, W, D, diversity_penalty, V, vocab_lo, vocab_hi, eos_id, pad_id, length_penalty)


def ring_pointers(rings) -> torch.Tensor:
    """the device array of ring base pointers db1_ring_reorder takes (int64 [n_layers])"""
    return torch.tensor([r.data_ptr() for r in rings], dtype=torch.int64).to(rings[0].device)


def ring_reorder(rings, ptrs, state, mlen, t, max_t, parent, W=1, done=None):
    """copy the last t keys of every row from row parent[b] (same group of W rows) in every ring of ``rings`` (bf16 [M, cap, 2, H, D],
    contiguous; ``ptrs`` = ring_pointers(rings)) -- db1_ring_reorder.  ``t`` (int32 [1]) READ only, at most ``max_t`` (<= mlen);
    ``done`` (int32 [M / W] or None): groups left alone.  Capturable; raises ValueError on bad arguments before anything is launched."""
    M, cap, slot_bytes, dev = _check_rings("ring_reorder", rings)
    if not lib.load().db1_ring_reorder_supported(slot_bytes):
        raise ValueError(f"ring_reorder: a slot of {slot_bytes} bytes (a multiple of 16 expected)")
    W, mlen, max_t = int(W), int(mlen), int(max_t)
    if W < 1 or M % W:
        raise ValueError(f"ring_reorder: W={W} must divide the {M} rows")
    if not 1 <= max_t <= mlen < cap:
        raise ValueError(f"ring_reorder: needs 1 <= max_t ({max_t}) <= mlen ({mlen}) < cap ({cap})")
    _check_tensor("ring_reorder", "ptrs (ring_pointers)", ptrs, torch.int64, (len(rings),), dev)
    for name, x, n in (("state", state, 1), ("t", t, 1), ("parent", parent, M)) + ((("done", done, M // W),) if done is not None else ()):
        _check_tensor("ring_reorder", name, x, torch.int32, n, dev)
    ws, wsn = _ws("db1_ring_reorder_workspace_bytes", (len(rings), M, max_t, slot_bytes), dev)
    lib.call("db1_ring_reorder", P(ptrs), len(rings), M, W, cap, slot_bytes, P(state), mlen, P(t), max_t, P(parent), P(done), ws, wsn, stream())


def ring_load_rows(rings, ptrs, src, state, mlen, rows, status):
    """the projected keys / values ``src`` (per layer a contiguous tensor [n, mlen, ...] of the rings' dtype and slot) of n new requests go to
    rows ``rows`` (int32 [n], distinct, on the device) of every ring of ``rings`` ([M, cap, ...], ``ptrs`` = ring_pointers(rings)), logical key
    j to slot (state + j) % cap -- db1_ring_load_rows, one launch, nothing else written.  ``state`` (int32 [1]) READ only.  ``status`` (int32
    [1]) |= 1 for a row outside [0, M) (skipped), |= 2 for an origin outside [0, cap).  Raises ValueError on bad arguments before anything is
    launched."""
    who = "ring_load_rows"
    M, cap, slot_bytes, dev = _check_rings(who, rings)
    if len(src) != len(rings) or src[0].dim() < 3:
        raise ValueError(f"{who}: one source tensor [n, mlen, ...] per ring expected")
    r0, n, mlen = rings[0], src[0].shape[0], int(mlen)
    for x in src:
        if tuple(x.shape) != (n, mlen) + tuple(r0.shape[2:]) or x.dtype != r0.dtype or not x.is_contiguous() or x.device != dev or \
                (n and x.data_ptr() % 16):
            raise ValueError(f"{who}: every source must be a contiguous 16-byte aligned {r0.dtype} tensor of shape "
                             f"{(n, mlen) + tuple(r0.shape[2:])} on {dev}")
    if not lib.load().db1_ring_load_rows_supported(slot_bytes, mlen, cap):
        raise ValueError(f"{who}: a slot of {slot_bytes} bytes (a multiple of 16 expected) with 0 < mlen ({mlen}) < cap ({cap})")
    if n > M:
        raise ValueError(f"{who}: {n} source rows for a ring of {M} rows")
    _check_tensor(who, "ptrs (ring_pointers)", ptrs, torch.int64, (len(rings),), dev)
    for name, x, k in (("state", state, 1), ("rows", rows, n), ("status", status, 1)):
        _check_tensor(who, name, x, torch.int32, k, dev)
    if n == 0:
        return
    sp = ring_pointers(src)
    lib.call("db1_ring_load_rows", P(ptrs), P(sp), len(rings), M, n, cap, slot_bytes, P(state), mlen, P(rows), P(status), stream())


def lmhead_ce(h2d, W, labels, mask, lse, sums, V, dh=None, dW_acc=None, beta_dw=1.0, gscale=1.0, chunk_rows=0):
    """tied head + masked CE without the logits tensor (db1_lmhead_ce_fwd / _fwd_bwd): ``dh`` and ``dW_acc`` given -> the training sweep"""
    T, d = h2d.shape
    rows = W.shape[0]
    assert h2d.is_contiguous() and W.is_contiguous() and W.shape[1] == d and h2d.dtype == W.dtype and rows >= V
    train = dh is not None
    assert (dW_acc is not None) == train and (not train or (dh.is_contiguous() and dW_acc.dtype == torch.float32 and dW_acc.shape == (rows, d)))
    ws, wsn = _ws("db1_lmhead_ce_workspace_bytes", (T, rows, d, int(chunk_rows), dt_code(h2d), int(train)), h2d.device)
    flops = 2.0 * T * V * d * (3 if train else 1)

    def run():
        if train:
            lib.call("db1_lmhead_ce_fwd_bwd", P(h2d), P(W), P(labels), P(mask), P(lse), P(sums), P(dh), P(dW_acc), float(beta_dw), float(gscale),
                     T, V, rows, d, int(chunk_rows), dt_code(h2d), ws, wsn, stream())
        else:
            lib.call("db1_lmhead_ce_fwd", P(h2d), P(W), P(labels), P(mask), P(lse), P(sums), T, V, rows, d, int(chunk_rows), dt_code(h2d), ws, wsn, stream())

    _timed("lmhead_ce", flops, run)   # (GEMM-dominated: reported as its own MFMA-bound family by bench.py)


def score_rows_supported(V: int, ld: int, dtype) -> bool:
    return bool(lib.load().db1_score_rows_supported(int(V), int(ld), dt_code(dtype)))


def _check_score_outputs(who, T, dev, labels, lse, logprob, top1, rank, status):
    for name, x, dt in (("labels", labels, torch.int64), ("lse", lse, torch.float32), ("logprob", logprob, torch.float32),
                        ("top1", top1, torch.int32), ("rank", rank, torch.int32), ("status", status, torch.int32)):
        _check_tensor(who, name, x, dt, T, dev)


def score_rows(logits2d, labels, lse, logprob, top1, rank, status, *, V=None, vocab_lo=0, vocab_hi=None, top_n=None, top_ids=None,
               top_logprob=None):
    """log-probability, arg-max and rank of ``labels`` (int64 [T]) under every row of ``logits2d`` [T, ld] (fp32 / bf16, the first V columns
    valid) over the columns [vocab_lo, vocab_hi) (db1_score_rows, rule in include/db1_hip.h): lse / logprob (float32 [T]) and top1 / rank /
    status (int32 [T]) are written, the logits are only read.  ``top_n`` (1 .. 16), ``top_ids`` (int32 [T, top_n]) and ``top_logprob``
    (float32 [T, top_n]), all or none: every row's ``top_n`` best candidates and their log-probabilities (db1_score_rows_top; the other
    outputs are bit-identical).  Capturable; raises ValueError on bad arguments before anything is launched."""
    T, ld, V, vocab_lo, vocab_hi = _check_logits("score_rows", logits2d, V, vocab_lo, vocab_hi,
                                                 lambda V, ld: score_rows_supported(V, ld, logits2d.dtype))      # (ld itself, not max(ld, V))
    if T < 1 or logits2d.data_ptr() % 16:
        raise ValueError(f"score_rows: logits of shape {tuple(logits2d.shape)} at {logits2d.data_ptr():#x}: at least one row, 16-byte aligned")
    _check_score_outputs("score_rows", T, logits2d.device, labels, lse, logprob, top1, rank, status)
    top = _check_top("score_rows", top_n, top_ids, top_logprob, (T,), logits2d.device)
    _timed("score_rows", float(T * V * logits2d.element_size()),
           lambda: lib.call("db1_score_rows_top" if top else "db1_score_rows", P(logits2d), P(labels), P(lse), P(logprob), P(top1), P(rank),
                            P(status), T, V, ld, dt_code(logits2d), *((top, P(top_ids), P(top_logprob)) if top else ()), vocab_lo, vocab_hi,
                            stream()))


def lmhead_score(h2d, W, labels, lse, logprob, top1, rank, status, *, V, vocab_lo=0, vocab_hi=None, chunk_rows=0, top_n=None, top_ids=None,
                 top_logprob=None):
    """``score_rows`` on the logits ``h2d`` [T, d] x ``W`` [rows >= V, d]^T, ``chunk_rows`` rows of logits at a time (0: 16 384) in the workspace
    (db1_lmhead_score): the logits tensor never exists.  ``top_n``, ``top_ids`` and ``top_logprob`` as ``score_rows`` takes them
    (db1_lmhead_score_top).  Capturable; raises ValueError on bad arguments before anything is launched."""
    if h2d.dim() != 2 or W.dim() != 2 or not h2d.is_contiguous() or not W.is_contiguous() or W.shape[1] != h2d.shape[1]:
        raise ValueError("lmhead_score: h [T, d] and W [rows, d] must be contiguous 2-D tensors of one width")
    if h2d.dtype not in (torch.float32, torch.bfloat16) or W.dtype != h2d.dtype or W.device != h2d.device:
        raise ValueError(f"lmhead_score: h and W must share one dtype (float32 / bfloat16) and device, got {h2d.dtype} / {W.dtype}")
    (T, d), rows, V, chunk_rows = h2d.shape, W.shape[0], int(V), int(chunk_rows)
    if T < 1 or not 0 < V <= rows or not score_rows_supported(V, rows, h2d.dtype):
        raise ValueError(f"lmhead_score: V={V} unsupported for a head of {rows} rows (at most 34 816, a multiple of 16 bytes)")
    if chunk_rows < 0:
        raise ValueError(f"lmhead_score: chunk_rows {chunk_rows} must be >= 0")
    vocab_lo, vocab_hi = _check_window("lmhead_score", V, vocab_lo, vocab_hi)
    _check_score_outputs("lmhead_score", T, h2d.device, labels, lse, logprob, top1, rank, status)
    top = _check_top("lmhead_score", top_n, top_ids, top_logprob, (T,), h2d.device)
    ws, wsn = _ws("db1_lmhead_score_workspace_bytes", (T, rows, d, chunk_rows, dt_code(h2d)), h2d.device)
    _timed("lmhead_score", 2.0 * T * V * d,
           lambda: lib.call("db1_lmhead_score_top" if top else "db1_lmhead_score", P(h2d), P(W), P(labels), P(lse), P(logprob), P(top1), P(rank),
                            P(status), T, V, rows, d, vocab_lo, vocab_hi, chunk_rows, dt_code(h2d),
                            *((top, P(top_ids), P(top_logprob)) if top else ()), ws, wsn, stream()))


def score_segments(logprob, rank, labels, mask, out, *, V):
    """per-sequence sums of ``score_rows`` results (db1_score_segments): ``out`` float32 [n_seg, 3] = {sum(mask * logprob), sum(mask),
    sum(mask * (rank == 0))} over segments of ``numel / n_seg`` consecutive rows; rows whose label lies outside [0, V) count as mask 0.
    Capturable; raises ValueError on bad arguments before anything is launched."""
    dev = logprob.device
    _check_tensor("score_segments", "out", out, torch.float32, (-1, 3), dev)
    n_seg, n = out.shape[0], logprob.numel()
    if n_seg < 1 or n < 1 or n % n_seg or int(V) < 1:
        raise ValueError(f"score_segments: {n} rows do not split into {n_seg} segments (V={V})")
    for name, x, dt in (("logprob", logprob, torch.float32), ("rank", rank, torch.int32), ("labels", labels, torch.int64), ("mask", mask, torch.float32)):
        _check_tensor("score_segments", name, x, dt, n, dev)
    lib.call("db1_score_segments", P(logprob), P(rank), P(labels), P(mask), P(out), n_seg, n // n_seg, int(V), stream())


def relattn_add_head_bias(qkv, u, vb, qu, qv, B, Lq, Lk, H, D):
    lib.call("db1_relattn_add_head_bias", P(qkv), P(u), P(vb), P(qu), P(qv), B, Lq, Lk, H, D, dt_code(qkv), dt_code(u), stream())


def relattn_softmax_fwd(AC, T, lse, H, B, Lq, Lk, nd, mlen, shift, scale):
    lib.call("db1_relattn_softmax_fwd", P(AC), P(T), P(lse), H, B, Lq, Lk, nd, mlen, shift, float(scale), stream())


def relattn_softmax_bwd(Pm, dP, dT, H, B, Lq, Lk, nd, mlen, shift, scale):
    lib.call("db1_relattn_softmax_bwd", P(Pm), P(dP), P(dT), H, B, Lq, Lk, nd, mlen, shift, float(scale), stream())


def relattn_decode_supported(B, q, klen, H, D, dtype) -> bool:
    return bool(lib.load().db1_relattn_decode_supported(B, q, klen, H, D, dt_code(dtype)))


def relattn_decode_fwd(qu, qv, k, v, R, out, B, q, klen, mlen, H, D, shift, scale):
    """k, v: views [B, klen, H, D] (any row / batch stride, unit stride inside a head row)"""
    assert k.stride(3) == 1 and k.stride(2) == D and v.stride() == k.stride()
    ws, wsn = _ws("db1_relattn_decode_workspace_bytes", (B, q, klen, H), out.device)
    lib.call("db1_relattn_decode_fwd", P(qu), P(qv), P(k), P(v), k.stride(1), k.stride(0), P(R), R.shape[0], P(out),
             B, q, klen, mlen, H, D, shift, float(scale), ws, wsn, stream())


def relattn_mem_supported(B, q, klen, mlen, H, D, shift, dtype, kv_row_stride=None, kv_batch_stride=None) -> bool:
    """db1_relattn_mem_supported, and (when given) the key / value strides the entry point accepts: multiples of 8 elements"""
    if any(s is not None and int(s) % 8 for s in (kv_row_stride, kv_batch_stride)):
        return False
    return bool(lib.load().db1_relattn_mem_supported(B, q, klen, mlen, H, D, shift, dt_code(dtype)))


def relattn_mem_fwd(qu, qv, k, v, R, out, lse, B, q, klen, mlen, H, D, shift, scale):
    """attention of q new queries (any number up to 8192) over klen = mlen + q keys in one launch (db1_relattn_mem_fwd).
    k, v: views [B, klen, H, D] (any row / batch stride, unit stride inside a head row); lse: float32 [B, H, q] or None"""
    assert k.stride(3) == 1 and k.stride(2) == D and v.stride() == k.stride()
    if any(t.dtype != torch.bfloat16 for t in (qu, qv, k, v, R, out)) or (lse is not None and lse.dtype != torch.float32):
        raise lib.Db1Error("relattn_mem_fwd: bf16 operands (float32 lse) only")     # (the entry point takes no dtype: refused here, nothing launched)
    lib.call("db1_relattn_mem_fwd", P(qu), P(qv), P(k), P(v), k.stride(1), k.stride(0), P(R), R.shape[0], P(out), P(lse),
             B, q, klen, mlen, H, D, shift, float(scale), _vp(0), 0, stream())


def _kv_strides(who, name, x, B, rows, H, D, may_broadcast):
    """(row stride, batch stride) in elements of a key / value view ``x`` [B, rows, H, D] (unit stride inside a head row); with
    ``may_broadcast`` a dimension of size 1 (or an expanded one) stands for every index: stride 0"""
    if x.dim() != 4 or x.shape[2] != H or x.shape[3] != D or x.stride(3) != 1 or x.stride(2) != D:
        raise ValueError(f"{who}: {name} must be a [batch, rows, {H}, {D}] view with unit stride inside a head row")
    nb, nr = x.shape[0], x.shape[1]
    if not (nb == B or (may_broadcast and nb == 1)) or not (nr == rows or (may_broadcast and nr == 1)):
        raise ValueError(f"{who}: {name} of shape {tuple(x.shape)} for {B} sequences of {rows} rows")
    return (x.stride(1) if nr > 1 else 0) if may_broadcast else x.stride(1), (x.stride(0) if nb > 1 else 0) if may_broadcast else x.stride(0)


def relattn_mem_kv_supported(B, q, mlen, H, D, shift, dtype) -> bool:
    """db1_relattn_mem_kv_supported: what relattn_mem_supported supports at klen = mlen + q, with mlen >= 1"""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(lib.load().db1_relattn_mem_kv_supported(int(B), int(q), int(mlen), int(H), int(D), int(shift), dt_code(dtype)))


def relattn_mem_kv_fwd(qu, qv, k_new, v_new, k_mem, v_mem, R, out, lse, B, q, mlen, H, D, shift, scale):
    """relattn_mem_fwd with the keys / values in two places (db1_relattn_mem_kv_fwd): key j < mlen is row j of the memory ``k_mem`` /
    ``v_mem``, key j >= mlen row j - mlen of the call's own ``k_new`` / ``v_new`` -- bit for bit relattn_mem_fwd over the concatenation.
    k_new, v_new: views [B, q, H, D] (e.g. of qkv_new [B, q, 3, H, D]); k_mem, v_mem: views [B or 1, mlen or 1, H, D] -- a dimension of
    size 1 (or an expanded one) is passed with stride 0: one row for every position, one memory for every sequence.
    lse: float32 [B, H, q] or None."""
    who = "relattn_mem_kv_fwd"
    if any(t.dtype != torch.bfloat16 for t in (qu, qv, k_new, v_new, k_mem, v_mem, R, out)) or (lse is not None and lse.dtype != torch.float32):
        raise lib.Db1Error(f"{who}: bf16 operands (float32 lse) only")     # (the entry point takes no dtype: refused here, nothing launched)
    n_rs, n_bs = _kv_strides(who, "k_new", k_new, B, q, H, D, False)
    m_rs, m_bs = _kv_strides(who, "k_mem", k_mem, B, mlen, H, D, True)
    if v_new.shape != k_new.shape or v_new.stride() != k_new.stride() or v_mem.shape != k_mem.shape or v_mem.stride() != k_mem.stride():
        raise ValueError(f"{who}: the values must have the keys' shape and strides")
    lib.call("db1_relattn_mem_kv_fwd", P(qu), P(qv), P(k_new), P(v_new), n_rs, n_bs, P(k_mem), P(v_mem), m_rs, m_bs, P(R), R.shape[0], P(out), P(lse),
             B, q, mlen, H, D, shift, float(scale), _vp(0), 0, stream())


def ring_prefill_rows(ring, k_new, v_new, k_mem, v_mem, state, mlen, rows, src, status):
    """the ring slots of new tenants of ONE layer from (a K/V memory, a call's own K/V) -- db1_ring_prefill_rows, one launch.  ``ring``:
    [M, cap, 2, H, D] bf16 or an fp8 ring [M, cap, 264 H] uint8, contiguous; k_new, v_new: views [n_src, q, H, D]; k_mem, v_mem: views
    [n_src or 1, mlen or 1, H, D] (size 1 = stride 0, as relattn_mem_kv_fwd takes them).  Destination i takes ring row ``rows[i]`` (int32
    [n_dst], distinct, on the device) from source ``src[i]`` (int32 [n_dst]; None: i): position j of the last mlen rows of cat(memory,
    new) goes to slot (state + j) % cap.  ``state`` (int32 [1]) READ only; ``status`` (int32 [1]) |= 1 for a row outside [0, M), |= 2 for
    an origin outside [0, cap), |= 4 for a source outside [0, n_src) (each skipped).  Raises ValueError on bad arguments before anything
    is launched."""
    who = "ring_prefill_rows"
    if k_new.dim() != 4:
        raise ValueError(f"{who}: k_new must be a [n_src, q, H, D] view")
    n_src, q, H, D = (int(v) for v in k_new.shape)
    dev, mlen = ring.device, int(mlen)
    fp8 = ring.dtype == torch.uint8
    slot = (264 * H,) if fp8 else (2, H, D)
    if ring.dtype not in (torch.uint8, torch.bfloat16) or ring.dim() != 2 + len(slot) or tuple(ring.shape[2:]) != slot or not ring.is_contiguous() or \
            ring.data_ptr() % 16:
        raise ValueError(f"{who}: the ring must be a contiguous 16-byte aligned bf16 [M, cap, 2, {H}, {D}] or uint8 [M, cap, {264 * H}] tensor")
    M, cap = int(ring.shape[0]), int(ring.shape[1])
    if any(t.dtype != torch.bfloat16 or t.device != dev for t in (k_new, v_new, k_mem, v_mem)):
        raise ValueError(f"{who}: the keys / values must be bf16 tensors on {dev}")
    if not lib.load().db1_ring_prefill_rows_supported(int(fp8), q, mlen, cap, H, D):
        raise ValueError(f"{who}: needs d_head 128, an even number of heads on an fp8 ring and 1 <= mlen ({mlen}) < cap ({cap}) (H={H}, D={D}, q={q})")
    n_rs, n_bs = _kv_strides(who, "k_new", k_new, n_src, q, H, D, False)
    m_rs, m_bs = _kv_strides(who, "k_mem", k_mem, n_src, mlen, H, D, True)
    if v_new.shape != k_new.shape or v_new.stride() != k_new.stride() or v_mem.shape != k_mem.shape or v_mem.stride() != k_mem.stride():
        raise ValueError(f"{who}: the values must have the keys' shape and strides")
    if any(s % 8 for s in (n_rs, n_bs, m_rs, m_bs)) or any(t.data_ptr() % 16 for t in (k_new, v_new, k_mem, v_mem)):
        raise ValueError(f"{who}: the keys / values must be 16-byte aligned with strides that are multiples of 8 elements")
    if rows.dim() != 1:
        raise ValueError(f"{who}: rows must be an int32 vector")
    n_dst = int(rows.numel())
    if n_dst > M:
        raise ValueError(f"{who}: {n_dst} destinations for a ring of {M} rows")
    for name, x, k in (("state", state, 1), ("rows", rows, n_dst), ("status", status, 1)) + ((("src", src, n_dst),) if src is not None else ()):
        _check_tensor(who, name, x, torch.int32, k, dev)
    if src is None and n_dst > n_src:
        raise ValueError(f"{who}: {n_dst} destinations from {n_src} sources need a src map")
    if n_dst == 0:
        return
    lib.call("db1_ring_prefill_rows", P(ring), int(fp8), M, cap, P(k_new), P(v_new), n_rs, n_bs, P(k_mem), P(v_mem), m_rs, m_bs, P(state), P(rows),
             P(src), n_dst, n_src, q, mlen, H, D, P(status), stream())


def _ring_layer(who, name, ring, H, D):
    """(fp8, M, cap) of a K/V ring's layer buffer: contiguous, 16-byte aligned, bf16 [M, cap, 2, H, D] or uint8 [M, cap, 264 H]"""
    fp8 = ring.dtype == torch.uint8
    slot = (264 * H,) if fp8 else (2, H, D)
    if ring.dtype not in (torch.uint8, torch.bfloat16) or ring.dim() != 2 + len(slot) or tuple(ring.shape[2:]) != slot or not ring.is_contiguous() or \
            ring.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be a contiguous 16-byte aligned bf16 [M, cap, 2, {H}, {D}] or uint8 [M, cap, {264 * H}] tensor")
    return fp8, int(ring.shape[0]), int(ring.shape[1])


def relattn_mem_ring_supported(B, q, mlen, cap_base, fp8, H, D, shift, dtype) -> bool:
    """db1_relattn_mem_ring_supported: what relattn_mem_kv_supported supports, with 1 <= mlen < cap_base and an even H on an fp8 ring"""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(lib.load().db1_relattn_mem_ring_supported(int(B), int(q), int(mlen), int(cap_base), int(bool(fp8)), int(H), int(D), int(shift), dt_code(dtype)))


def relattn_mem_ring_fwd(qu, qv, k_new, v_new, base, state_base, base_rows, status, R, out, lse, B, q, mlen, H, D, shift, scale):
    """relattn_mem_kv_fwd with the memory in the slots of a K/V ring (db1_relattn_mem_ring_fwd): key j < mlen of call row b is slot
    (state_base + j) % cap of row ``base_rows[b]`` of ``base`` -- one layer of a ring, bf16 [M, cap, 2, H, D] or fp8 uint8 [M, cap, 264 H],
    dequantised on the way -- bit for bit relattn_mem_kv_fwd over the unpacked, linearised memory.  ``state_base`` int32 [1] (read on the
    device); ``base_rows`` int32 [B] or None (the identity; repeats are allowed); ``status`` int32 [1], |= 8 when a base row or the origin
    was out of range (read as 0: do not trust the output then).  k_new, v_new, lse as relattn_mem_kv_fwd takes them."""
    who = "relattn_mem_ring_fwd"
    if any(t.dtype != torch.bfloat16 for t in (qu, qv, k_new, v_new, R, out)) or (lse is not None and lse.dtype != torch.float32):
        raise lib.Db1Error(f"{who}: bf16 operands (float32 lse) only")     # (the entry point takes no dtype: refused here, nothing launched)
    fp8, M_base, cap_base = _ring_layer(who, "base", base, H, D)
    n_rs, n_bs = _kv_strides(who, "k_new", k_new, B, q, H, D, False)
    if v_new.shape != k_new.shape or v_new.stride() != k_new.stride():
        raise ValueError(f"{who}: the values must have the keys' shape and strides")
    dev = base.device
    for name, x, k in (("state_base", state_base, 1), ("status", status, 1)) + ((("base_rows", base_rows, B),) if base_rows is not None else ()):
        _check_tensor(who, name, x, torch.int32, k, dev)
    if base_rows is None and B > M_base:
        raise ValueError(f"{who}: {B} call rows over a base ring of {M_base} rows need base_rows")
    lib.call("db1_relattn_mem_ring_fwd", P(qu), P(qv), P(k_new), P(v_new), n_rs, n_bs, P(base), int(fp8), M_base, cap_base, P(state_base), P(base_rows),
             P(status), P(R), R.shape[0], P(out), P(lse), B, q, mlen, H, D, shift, float(scale), _vp(0), 0, stream())


def ring_fork_rows_supported(fp8, q, mlen, cap_base, cap, H, D) -> bool:
    """db1_ring_fork_rows_supported: what db1_ring_prefill_rows supports at the destination's cap, with mlen < cap_base"""
    return bool(lib.load().db1_ring_fork_rows_supported(int(bool(fp8)), int(q), int(mlen), int(cap_base), int(cap), int(H), int(D)))


def ring_fork_rows(ring, base, state_base, base_rows, k_new, v_new, state, mlen, rows, src, status):
    """ring_prefill_rows with a ring as the memory (db1_ring_fork_rows, one launch per layer): destination i takes row ``rows[i]`` of
    ``ring`` from call row s = ``src[i]`` (None: i) over row ``base_rows[s]`` (None: s) of ``base``: position j of the last mlen rows of
    cat(the base row's mlen slots from ``state_base``, the call's q new rows) goes to slot (state + j) % cap.  Base slots are copied byte
    for byte (an fp8 slot is never requantised), new rows are copied (bf16) or quantised (fp8).  ``ring`` and ``base``: layer buffers of
    one format and H (cap may differ) that do not overlap; the int32 vectors on the device; ``status`` |= 1 / 2 / 4 as ring_prefill_rows,
    |= 8 for a base row or base origin out of range (skipped).  Raises ValueError on bad arguments before anything is launched."""
    who = "ring_fork_rows"
    if k_new.dim() != 4:
        raise ValueError(f"{who}: k_new must be a [n_src, q, H, D] view")
    n_src, q, H, D = (int(v) for v in k_new.shape)
    dev, mlen = ring.device, int(mlen)
    fp8, M, cap = _ring_layer(who, "the ring", ring, H, D)
    fp8b, M_base, cap_base = _ring_layer(who, "base", base, H, D)
    if fp8 != fp8b or base.device != dev:
        raise ValueError(f"{who}: the base ring and the destination ring must have one format and one device")
    lo, hi = ring.data_ptr(), ring.data_ptr() + ring.numel() * ring.element_size()
    blo, bhi = base.data_ptr(), base.data_ptr() + base.numel() * base.element_size()
    if lo < bhi and blo < hi:
        raise ValueError(f"{who}: the base ring and the destination ring overlap")
    if any(t.dtype != torch.bfloat16 or t.device != dev for t in (k_new, v_new)):
        raise ValueError(f"{who}: the keys / values must be bf16 tensors on {dev}")
    if not ring_fork_rows_supported(fp8, q, mlen, cap_base, cap, H, D):
        raise ValueError(f"{who}: needs d_head 128, an even number of heads on fp8 rings and 1 <= mlen ({mlen}) < cap ({cap}) and cap_base ({cap_base}) "
                         f"(H={H}, D={D}, q={q})")
    n_rs, n_bs = _kv_strides(who, "k_new", k_new, n_src, q, H, D, False)
    if v_new.shape != k_new.shape or v_new.stride() != k_new.stride():
        raise ValueError(f"{who}: the values must have the keys' shape and strides")
    if n_rs % 8 or n_bs % 8 or k_new.data_ptr() % 16 or v_new.data_ptr() % 16:
        raise ValueError(f"{who}: the keys / values must be 16-byte aligned with strides that are multiples of 8 elements")
    if rows.dim() != 1:
        raise ValueError(f"{who}: rows must be an int32 vector")
    n_dst = int(rows.numel())
    if n_dst > M:
        raise ValueError(f"{who}: {n_dst} destinations for a ring of {M} rows")
    for name, x, k in (("state", state, 1), ("state_base", state_base, 1), ("rows", rows, n_dst), ("status", status, 1)) + \
            ((("src", src, n_dst),) if src is not None else ()) + ((("base_rows", base_rows, n_src),) if base_rows is not None else ()):
        _check_tensor(who, name, x, torch.int32, k, dev)
    if src is None and n_dst > n_src:
        raise ValueError(f"{who}: {n_dst} destinations from {n_src} sources need a src map")
    if base_rows is None and n_src > M_base:
        raise ValueError(f"{who}: {n_src} call rows over a base ring of {M_base} rows need base_rows")
    if n_dst == 0:
        return
    lib.call("db1_ring_fork_rows", P(ring), int(fp8), M, cap, P(base), M_base, cap_base, P(state_base), P(base_rows), P(k_new), P(v_new), n_rs, n_bs,
             P(state), P(rows), P(src), n_dst, n_src, q, mlen, H, D, P(status), stream())


_tickets = {}


def decode_tickets(device) -> torch.Tensor:
    """the ticket counters of the fused inference launches (db1_linear_decode_tickets_bytes): zero once, every launch leaves them zero.
    One buffer per device: the inference path of a device runs on one stream at a time."""
    t = _tickets.get(device)
    if t is None:
        t = torch.zeros(int(lib.load().db1_linear_decode_tickets_bytes()) // 4, dtype=torch.int32, device=device)
        _tickets[device] = t
    return t


def relattn_decode_ring_fwd(qkv_new, u, vb, kv_ring, state, R, out, B, q, mlen, H, D, shift, scale, fused_merge=False, part=None):
    """attention of q new tokens over a ring of cached K / V (db1_relattn_decode_ring_fwd): kv_ring [B, cap, 2, H, D], state int32[1].
    out None + part (a float tensor of relattn_decode_ring_part_numel elements): the per-chunk partial results only (for linear_decode_attn).
    fused_merge: the chunk that finishes last merges inside the launch (ticket hand-off) instead of a second launch -- measured SLOWER inside
    a graph (q = 1: 13.1 vs 9.3 us, q = 22: 23.9 vs 13.2 us: the drain + ticket + dependent reads cost more than a launch boundary), so off"""
    cap = kv_ring.shape[1]
    if part is not None:
        ws, wsn = P(part), part.numel() * 4
    else:
        ws, wsn = _ws("db1_relattn_decode_ring_workspace_bytes", (B, q, mlen + q, H), qkv_new.device)
    lib.call("db1_relattn_decode_ring_fwd", P(qkv_new), P(u), P(vb), P(kv_ring), P(state), cap, P(R), R.shape[0], P(out), B, q, mlen, H, D, shift,
             float(scale), ws, wsn, P(decode_tickets(qkv_new.device)) if (fused_merge and out is not None) else _vp(0), stream())


# ---- the grouped K/V ring (include/db1_hip.h, "grouped K/V ring"): one base row per group, one short tail per row
GROUP_MAX_W, GROUP_MAX_KLEN, GROUP_MAX_TAIL = 64, 2048, 4096


def relattn_decode_group_supported(G, W, mlen, Lt, cap_b, cap_t, H, D, dtype) -> bool:
    return bool(lib.load().db1_relattn_decode_group_supported(int(G), int(W), int(mlen), int(Lt), int(cap_b), int(cap_t), int(H), int(D), dt_code(dtype)))


def relattn_decode_group_fwd(qkv_new, u, vb, base, state_b, tail, state_t, n_tail, Lt, R, out, G, W, mlen, H, D, shift, scale, status):
    """one new token per row over a group's shared base ring and the row's own tail (db1_relattn_decode_group_fwd): qkv_new [G W, 1, 3, H, D]
    (or [G W, 3 H D]), base [G, cap_b, 2, H, D], tail [G W, cap_t, 2, H, D], out [G W, 1, H, D], all bf16; state_b, state_t, n_tail, status
    int32 [1] on the device.  The call's own key / value is appended to the tail.  Everything is checked here, on the host: ValueError
    before the library is called."""
    who = "relattn_decode_group_fwd"
    G, W, mlen, Lt, H, D, shift = int(G), int(W), int(mlen), int(Lt), int(H), int(D), int(shift)
    if D != 128 or not 1 <= W <= GROUP_MAX_W or G < 1 or H < 1 or not 1 <= mlen < GROUP_MAX_KLEN or not 1 <= Lt <= GROUP_MAX_TAIL or shift < 0:
        raise ValueError(f"{who}: needs d_head 128, 1 <= W <= {GROUP_MAX_W}, 1 <= mlen <= {GROUP_MAX_KLEN - 1}, 1 <= Lt <= {GROUP_MAX_TAIL} and shift >= 0 "
                         f"(got G={G}, W={W}, mlen={mlen}, Lt={Lt}, H={H}, D={D}, shift={shift})")
    M, dev = G * W, qkv_new.device
    for name, x, lead in (("base", base, G), ("tail", tail, M)):
        if x.dim() != 5 or x.shape[0] != lead or tuple(x.shape[2:]) != (2, H, D) or x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"{who}: {name} must be a contiguous bf16 [{lead}, cap, 2, {H}, {D}] tensor on {dev}")
    cap_b, cap_t = int(base.shape[1]), int(tail.shape[1])
    if cap_b < mlen or cap_t < Lt + 1:
        raise ValueError(f"{who}: the base ring needs mlen ({mlen}) slots and the tail ring Lt + 1 ({Lt + 1}) (got {cap_b} and {cap_t})")
    if qkv_new.dtype != torch.bfloat16 or not qkv_new.is_contiguous() or qkv_new.numel() != M * 3 * H * D:
        raise ValueError(f"{who}: qkv_new must be a contiguous bf16 tensor of {M} x 3 x {H} x {D} elements")
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() != M * H * D or out.device != dev:
        raise ValueError(f"{who}: out must be a contiguous bf16 tensor of {M} x {H} x {D} elements on {dev}")
    for name, x in (("u", u), ("vb", vb)):
        _check_tensor(who, name, x, torch.bfloat16, H * D, dev)
    if R.dim() < 2 or R.shape[0] < 1 or R.dtype != torch.bfloat16 or not R.is_contiguous() or R.numel() != R.shape[0] * H * D or R.device != dev:
        raise ValueError(f"{who}: R must be a contiguous bf16 [nd, {H}, {D}] tensor on {dev}")
    for name, x in (("state_b", state_b), ("state_t", state_t), ("n_tail", n_tail), ("status", status)):
        _check_tensor(who, name, x, torch.int32, 1, dev)
    if any(x.data_ptr() % 16 for x in (qkv_new, u, vb, base, tail, R, out)):
        raise ValueError(f"{who}: operands must be 16-byte aligned")
    ws, wsn = _ws("db1_relattn_decode_group_workspace_bytes", (G, W, mlen, Lt, H), dev)
    lib.call("db1_relattn_decode_group_fwd", P(qkv_new), P(u), P(vb), P(base), P(state_b), cap_b, P(tail), P(state_t), cap_t, P(n_tail), Lt, P(R),
             int(R.shape[0]), P(out), G, W, mlen, H, D, shift, float(scale), P(status), ws, wsn, stream())


def group_ring_advance(state_t, n_tail, cap_t, Lt, mlen):
    lib.call("db1_group_ring_advance", P(state_t), P(n_tail), int(cap_t), int(Lt), int(mlen), stream())


def relattn_decode_ring_part_numel(B, q, klen, H) -> int:
    return int(lib.load().db1_relattn_decode_ring_workspace_bytes(int(B), int(q), int(klen), int(H))) // 4


# ---- the fp8 K/V ring (include/db1_hip.h, "fp8 K/V ring"): rings are uint8 [B, cap, kv8_slot_bytes(H, D)]
def kv8_slot_bytes(H, D) -> int:
    """bytes of one fp8 slot (db1_kv8_slot_bytes: 264 H), 0 where the format is not defined (d_head != 128, an odd number of heads)"""
    return int(lib.load().db1_kv8_slot_bytes(int(H), int(D)))


def relattn_decode_ring_kv8_supported(B, q, klen, H, D) -> bool:
    return bool(lib.load().db1_relattn_decode_ring_kv8_supported(int(B), int(q), int(klen), int(H), int(D)))


def relattn_decode_ring_kv8_fwd(qkv_new, u, vb, kv_ring, state, R, out, B, q, mlen, H, D, shift, scale, fused_merge=False, part=None):
    """relattn_decode_ring_fwd over an fp8 ring (db1_relattn_decode_ring_kv8_fwd): kv_ring uint8 [B, cap, kv8_slot_bytes(H, D)]; every other
    operand, ``part`` and ``fused_merge`` as there.  The call's own keys / values are appended quantised."""
    if kv_ring.dtype != torch.uint8 or kv_ring.dim() != 3 or not kv_ring.is_contiguous() or kv_ring.shape[0] != B or \
            kv_ring.shape[2] != kv8_slot_bytes(H, D):
        raise ValueError(f"relattn_decode_ring_kv8_fwd: the ring must be a contiguous uint8 [{B}, cap, {kv8_slot_bytes(H, D)}] tensor")
    cap = kv_ring.shape[1]
    if part is not None:
        ws, wsn = P(part), part.numel() * 4
    else:
        ws, wsn = _ws("db1_relattn_decode_ring_kv8_workspace_bytes", (B, q, mlen + q, H), qkv_new.device)
    lib.call("db1_relattn_decode_ring_kv8_fwd", P(qkv_new), P(u), P(vb), P(kv_ring), P(state), cap, P(R), R.shape[0], P(out), B, q, mlen, H, D, shift,
             float(scale), ws, wsn, P(decode_tickets(qkv_new.device)) if (fused_merge and out is not None) else _vp(0), stream())


def kv8_quantize(src, dst):
    """projected keys / values ``src`` (bf16 [n, mlen, 2, H, D], contiguous) -> fp8 slots ``dst`` (uint8 [n, mlen, slot]; the row stride is
    free, e.g. ``ring[:, :mlen]``) -- db1_kv8_quantize, one launch"""
    if src.dim() != 5 or src.shape[2] != 2 or src.dtype != torch.bfloat16 or not src.is_contiguous():
        raise ValueError("kv8_quantize: src must be a contiguous bf16 [n, mlen, 2, H, D] tensor")
    n, mlen, _, H, D = src.shape
    slot = kv8_slot_bytes(H, D)
    if not slot:
        raise ValueError(f"kv8_quantize: no fp8 slot for H={H}, D={D} (d_head 128 and an even number of heads expected)")
    if dst.dtype != torch.uint8 or tuple(dst.shape) != (n, mlen, slot) or dst.device != src.device or dst.stride(2) != 1 or dst.stride(1) != slot:
        raise ValueError(f"kv8_quantize: dst must be a uint8 [{n}, {mlen}, {slot}] tensor (or such a view of a ring) on {src.device}")
    if n == 0:
        return
    lib.call("db1_kv8_quantize", P(src), P(dst), n, mlen, H, D, dst.stride(0) if n > 1 else max(dst.stride(0), mlen * slot), stream())


def _kv8_scale_exp(amax):
    """the exponent of the canonical scale: the smallest power of two s with amax <= 448 s; 0 for amax == 0; at least -126"""
    m, e = torch.frexp(amax)                         # amax = m 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    se = torch.where(m > 0.875, e - 8, e - 9).clamp(min=-126)
    return torch.where(amax == 0, torch.zeros_like(se), se)


def kv8_pack(kv, scales=None):
    """host side (tests, debugging): keys / values ``kv`` [..., 2, H, 128] (CPU, any float dtype holding bf16 values) -> slots uint8
    [..., 264 H] by the rule of include/db1_hip.h.  ``scales`` [..., 2, H] (powers of two with |x| <= 448 s): use these instead of the
    canonical ones."""
    x = kv.detach().to("cpu", torch.float64)
    if x.dim() < 3 or x.shape[-3] != 2 or x.shape[-1] != 128 or x.shape[-2] % 2:
        raise ValueError("kv8_pack: kv must be [..., 2, H, 128] with an even H")
    H, lead = x.shape[-2], tuple(x.shape[:-3])
    fin = torch.isfinite(x)
    if scales is None:
        s = torch.ldexp(torch.ones(lead + (2, H), dtype=torch.float64), _kv8_scale_exp(torch.where(fin, x.abs(), torch.zeros_like(x)).amax(-1)))
    else:
        s = scales.detach().to("cpu", torch.float64).expand(lead + (2, H))
        m, e = torch.frexp(s)
        if not bool(((m == 0.5) & (e >= -125) & (e <= 128)).all()):
            raise ValueError("kv8_pack: every scale must be a power of two that is a normal fp32 (2^-126 .. 2^127)")
    y = torch.where(fin, x / s[..., None], torch.zeros_like(x))
    if float(y.abs().max()) > 448.0:
        raise ValueError("kv8_pack: a scale is too small for its block (|x / s| > 448)")
    pay = y.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    pay = torch.where(fin, pay, torch.full_like(pay, 0x7F))
    return torch.cat([pay.reshape(lead + (2 * H * 128,)), s.to(torch.float32).reshape(lead + (2 * H,)).contiguous().view(torch.uint8).reshape(lead + (8 * H,))], -1)


def kv8_unpack(slots, H):
    """host side: slots uint8 [..., 264 H] -> (the dequantised keys / values, bf16 [..., 2, H, 128]; the scales, float32 [..., 2, H])"""
    sl = slots.detach().to("cpu").contiguous()
    H = int(H)
    if sl.dtype != torch.uint8 or sl.shape[-1] != 264 * H:
        raise ValueError(f"kv8_unpack: slots must be uint8 [..., {264 * H}]")
    lead = tuple(sl.shape[:-1])
    pay = sl[..., :256 * H].contiguous().view(torch.float8_e4m3fn).to(torch.float32).reshape(lead + (2, H, 128))
    s = sl[..., 256 * H:].contiguous().view(torch.float32).reshape(lead + (2, H))
    return (pay * s[..., None]).to(torch.bfloat16), s


def linear_decode_attn_supported(B, q, H, D, klen, N) -> bool:
    return bool(lib.load().db1_linear_decode_attn_supported(int(B), int(q), int(H), int(D), (int(klen) + 127) // 128, int(N)))


def linear_decode_attn(part, klen, B, q, H, D, W, y):
    """y = merge(part) W^T (db1_linear_decode_attn): part from relattn_decode_ring_fwd(out=None, part=...)"""
    assert W.dtype == torch.bfloat16 and W.is_contiguous() and y.dtype == torch.bfloat16 and y.stride(1) == 1 and W.shape == (y.shape[1], H * D)
    lib.call("db1_linear_decode_attn", P(part), (int(klen) + 127) // 128, B, q, H, D, P(W), P(y), y.stride(0), y.shape[1], stream())


_chain_scratch = {}


def decode_chain_supported(d, dff, H, D, klen) -> bool:
    return bool(lib.load().db1_decode_chain_supported(int(d), int(dff), int(H), int(D), (int(klen) + 127) // 128))


def _chain_key(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()   # "cuda" and "cuda:0" are one device
    sc = _scope()
    return idx, (sc[0] if sc is not None else torch.cuda.current_stream(idx).cuda_stream)


class chain_scratch_scope:
    """``with ops.chain_scratch_scope(scratch, pinned_word):`` -- the chain launches and flag fetches inside use THIS scratch / pinned word
    instead of the (device, stream) ones.  For hipGraph captures (GraphedRingStep): a capture runs on torch's shared capture stream, whose
    key would be new -- its scratch would be allocated AND zero-filled inside the capture, i.e. every replay would start by wiping the
    scratch including the sticky error flag, and every graph captured on that stream would share one scratch whatever stream replays it.
    The owner creates both eagerly (``new_chain_scratch``) before it captures.  Thread-local."""

    def __init__(self, scratch, host_word):
        self.pair = (scratch, host_word)

    def __enter__(self):
        self.prev = getattr(_tls, "chain_override", None)
        _tls.chain_override = self.pair
        return self

    def __exit__(self, *exc):
        _tls.chain_override = self.prev
        return False


def _chain_pinned_word():
    global _chain_flag_pool
    if _chain_flag_pool is None:
        if torch.cuda.is_current_stream_capturing():
            raise lib.Db1Error("db1_decode_chain: the first one-token call must run eagerly (GraphedRingStep warms up before it captures)")
        _chain_flag_pool = [torch.zeros(256, dtype=torch.int32).pin_memory(), list(range(255, -1, -1))]
    pool, free = _chain_flag_pool
    if not free:
        raise lib.Db1Error("db1_decode_chain: more than 256 scratch owners (device x stream pairs + captured steps) decode through the persistent launch")
    i = free.pop()
    word = pool[i:i + 1]
    word.zero_()
    # the word goes back to the free list when its owner (a GraphedRingStep, or whoever holds a new_chain_scratch result) is collected
    weakref.finalize(word, free.append, i)
    return word


def new_chain_scratch(device):
    """(zeroed scratch, pinned host word) owned by the caller -- a captured step; must be called eagerly (never under capture)"""
    if torch.cuda.is_current_stream_capturing():
        raise lib.Db1Error("new_chain_scratch under hipGraph capture: the scratch of a captured step is created before the capture")
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return torch.zeros(int(lib.load().db1_decode_chain_scratch_bytes()), dtype=torch.uint8, device=torch.device("cuda", idx)), _chain_pinned_word()


def decode_chain_scratch(device):
    """the scratch of db1_decode_chain (tagged hand-off rows + error flag): one buffer per (device, STREAM) like every other scratch
    buffer here -- the tag of a word is only the layer index, so two models decoding at the same time on two streams must not see each
    other's rows (or each other's sticky error flag) -- or the one a chain_scratch_scope supplies.  Zeroed once, when it is created:
    never inside a capture (a zero-fill node would wipe the flag at every replay)."""
    ov = getattr(_tls, "chain_override", None)
    if ov is not None:
        return ov[0]
    key = _chain_key(device)
    t = _chain_scratch.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise lib.Db1Error("db1_decode_chain under hipGraph capture without a chain_scratch_scope: the scratch (and its error flag) would be "
                               "allocated and zero-filled inside the graph")
        t = torch.zeros(int(lib.load().db1_decode_chain_scratch_bytes()), dtype=torch.uint8, device=torch.device("cuda", key[0]))
        _chain_scratch[key] = t
    return t


_chain_flag_host = {}
_chain_flag_pool = None


def decode_chain_flag_fetch(device):
    """enqueue a copy of the chain's error flag into pinned host memory behind the launches issued so far (4 bytes, no synchronisation,
    legal under hipGraph capture) -> (pinned int32 tensor, the scratch it watches): the pinned word holds the flag once the stream has
    passed this point"""
    ov = getattr(_tls, "chain_override", None)
    if ov is not None:
        h = ov[1]
    else:
        key = _chain_key(device)
        h = _chain_flag_host.get(key)
        if h is None:
            # one pinned word per (device, stream), handed out from a small pool that is allocated on the first EAGER call: a stream that is
            # capturing a graph may not allocate pinned memory (hipHostMalloc invalidates the capture)
            h = _chain_pinned_word()
            _chain_flag_host[key] = h
    sc = decode_chain_scratch(device)
    off = int(lib.load().db1_decode_chain_error_offset())
    h.copy_(sc[off:off + 4].view(torch.int32), non_blocking=True)
    return h, sc


def decode_chain_clear_error(watch):
    h, sc = watch
    off = int(lib.load().db1_decode_chain_error_offset())
    sc[off:off + 4].zero_()
    h.zero_()


def decode_chain(part, klen, H, x_res, w_o, w1, b1, w2, b2, w_qkv_next, g1, be1, g2, be2, alpha, eps, h1_out, f_out, x_next, qkv_next, slot, w_o_next=None):
    """one new token through o_net (merge of the attention partials) -> LN -> ff1 + GEGLU -> ff2 -> LN -> the next layer's qkv projection, one
    launch (db1_decode_chain); w_qkv_next None = last layer (h1_out and f_out come back for the head's input LayerNorm).  Consecutive launches
    need different ``slot`` values (the layer index)."""
    d, dff = w_o.shape[0], w2.shape[1]
    for t in (x_res, w_o, w1, b1, w2, b2, g1, be1, g2, be2):
        assert t.dtype == torch.bfloat16 and t.is_contiguous()
    lib.call("db1_decode_chain", P(part), (int(klen) + 127) // 128, int(H), P(x_res), P(w_o), P(w1), P(b1), P(w2), P(b2), P(w_qkv_next), P(w_o_next), P(g1), P(be1), P(g2), P(be2),
             float(alpha), float(eps), P(h1_out), P(f_out), P(x_next), P(qkv_next), P(decode_chain_scratch(x_res.device)), int(slot), int(d), int(dff), stream())


def decode_chain_error(device) -> bool:
    """did a hand-off poll of a chain launch run into its limit (results invalid)?  Synchronises."""
    off = int(lib.load().db1_decode_chain_error_offset())
    return bool(decode_chain_scratch(device)[off:off + 4].view(torch.int32).item())


def linear_decode_supported(M, N, K, geglu=False, ln=False, pre=False) -> bool:
    return bool(lib.load().db1_linear_decode_supported(int(M), int(N), int(K), int(geglu), int(bool(ln)) | (2 if pre else 0)))


def linear_decode(x, W, bias, y, geglu=False, ln=None, pre=None):
    """y = x W^T + bias for M <= 64 rows (bf16), optionally through GEGLU (W [2N, K]); inside the same launch (db1_linear_decode)
    pre = (res, alpha, gamma, beta, eps, out): the input rows are x_eff = LayerNorm(alpha * res + x) * gamma + beta, also stored to out;
    ln  = (res, alpha, gamma, beta, eps, out): out = LayerNorm(alpha * res + y) * gamma + beta"""
    _linear_decode(x, W, bias, y, geglu, ln, pre, False)


def _linear_decode(x, W, bias, y, geglu, ln, pre, w8):
    """linear_decode (W: the bf16 weight) and linear_decode_w8 (W: its packed fp8 buffer): one argument block"""
    M, K = x.shape
    N = y.shape[1]
    assert x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
    if w8:
        _w8_check(W, 2 * N if geglu else N, K, y.device, "linear_decode_w8")
    else:
        assert W.dtype == torch.bfloat16 and W.is_contiguous() and W.shape == ((2 * N if geglu else N), K)
    assert x.stride(1) == 1 and y.stride(1) == 1
    ws, wsn = _ws("db1_linear_decode_workspace_bytes", (M, N, K, int(geglu)), y.device)
    dtp = 0

    def pack(t):
        nonlocal dtp
        if t is None:
            return (_vp(0), 0, 1.0, _vp(0), _vp(0), 0.0, _vp(0), 0)
        res, alpha, gamma, beta, eps, out = t
        assert res.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and gamma.dtype == beta.dtype and res.stride(1) == 1 and out.stride(1) == 1
        assert dtp in (0, dt_code(gamma.dtype) + 100)
        dtp = dt_code(gamma.dtype) + 100
        return (P(res), res.stride(0), float(alpha), P(gamma), P(beta), float(eps), P(out), out.stride(0))
    a_pre, a_ln = pack(pre), pack(ln)
    lib.call("db1_linear_decode_w8" if w8 else "db1_linear_decode", P(x), x.stride(0), P(W), P(bias), dt_code(bias.dtype) if bias is not None else 0, P(y),
             y.stride(0), M, N, K, int(geglu), *a_pre, *a_ln, max(dtp - 100, 0), P(decode_tickets(y.device)), ws, wsn, stream())


# ---- fp8 decode weights (include/db1_hip.h, "fp8 decode weights"): a weight [N, K] is ONE uint8 buffer of w8_bytes(N, K) bytes
def w8_bytes(N, K) -> int:
    """bytes of the packed form of a [N, K] weight (db1_w8_bytes: N K payload bytes + N K / 128 fp32 scales), 0 where K % 128 != 0"""
    return int(lib.load().db1_w8_bytes(int(N), int(K)))


def w8_quantize(W, out=None):
    """a bf16 weight ``W`` [N, K] on the device (rows may be strided: ``W.stride(0) >= K``) -> its packed buffer (uint8 [w8_bytes(N, K)],
    ``out`` or a new tensor) -- db1_w8_quantize, one launch"""
    if W.dim() != 2 or W.dtype != torch.bfloat16 or W.stride(1) != 1 or not W.is_cuda:
        raise ValueError("w8_quantize: W must be a bf16 [N, K] device tensor with contiguous rows")
    N, K = W.shape
    nb = w8_bytes(N, K)
    if not nb:
        raise ValueError(f"w8_quantize: no fp8 form for N={N}, K={K} (K % 128 == 0 expected)")
    if out is None:
        out = torch.empty(nb, dtype=torch.uint8, device=W.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != nb or out.device != W.device or not out.is_contiguous():
        raise ValueError(f"w8_quantize: out must be a contiguous uint8 [{nb}] tensor on {W.device}")
    lib.call("db1_w8_quantize", P(W), W.stride(0), N, K, P(out), stream())
    return out


def w8_pack(W):
    """host side (tests, debugging): a weight ``W`` [N, K] (CPU, any float dtype holding bf16 values, K % 128 == 0) -> the packed buffer uint8
    [N K + 4 N K / 128] by the rule of include/db1_hip.h: every block of 128 k of a row is a block of kv8_pack"""
    x = W.detach().to("cpu", torch.float64)
    if x.dim() != 2 or x.shape[1] == 0 or x.shape[1] % 128 or x.shape[0] == 0:
        raise ValueError("w8_pack: W must be [N, K] with K % 128 == 0")
    N, K = x.shape
    xb = x.reshape(N, K // 128, 128)
    fin = torch.isfinite(xb)
    s = torch.ldexp(torch.ones(N, K // 128, dtype=torch.float64), _kv8_scale_exp(torch.where(fin, xb.abs(), torch.zeros_like(xb)).amax(-1)))
    y = torch.where(fin, xb / s[..., None], torch.zeros_like(xb))
    pay = y.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    pay = torch.where(fin, pay, torch.full_like(pay, 0x7F))
    return torch.cat([pay.reshape(-1), s.to(torch.float32).reshape(-1).contiguous().view(torch.uint8)])


def w8_unpack(buf, N, K):
    """host side: a packed buffer -> (the dequantised weight, bf16 [N, K]; the scales, float32 [N, K / 128])"""
    b = buf.detach().to("cpu").contiguous()
    N, K = int(N), int(K)
    if K <= 0 or K % 128 or N <= 0 or b.dtype != torch.uint8 or b.dim() != 1 or b.numel() != N * K + 4 * N * (K // 128):
        raise ValueError(f"w8_unpack: buf must be uint8 [{N * K + 4 * N * (K // 128) if K % 128 == 0 else '?'}] (N K payload bytes, then N K / 128 fp32 scales; K % 128 == 0)")
    pay = b[:N * K].view(torch.float8_e4m3fn).to(torch.float32).reshape(N, K // 128, 128)
    s = b[N * K:].clone().view(torch.float32).reshape(N, K // 128)
    return (pay * s[..., None]).reshape(N, K).to(torch.bfloat16), s


def linear_decode_w8_supported(M, N, K, geglu=False, ln=False, pre=False) -> bool:
    return bool(lib.load().db1_linear_decode_w8_supported(int(M), int(N), int(K), int(geglu), int(bool(ln)) | (2 if pre else 0)))


def linear_decode_w8(x, W8, bias, y, geglu=False, ln=None, pre=None):
    """linear_decode with the weight in its fp8 form (db1_linear_decode_w8): ``W8`` is the packed buffer of the [N, K] (geglu: [2 N, K]) weight
    from w8_quantize.  Bit for bit linear_decode over w8_unpack(W8)."""
    _linear_decode(x, W8, bias, y, geglu, ln, pre, True)


def linear_decode_attn_w8_supported(B, q, H, D, klen, N) -> bool:
    return bool(lib.load().db1_linear_decode_attn_w8_supported(int(B), int(q), int(H), int(D), (int(klen) + 127) // 128, int(N)))


def linear_decode_attn_w8(part, klen, B, q, H, D, W8, y):
    """linear_decode_attn with the [N, H D] weight in its fp8 form (db1_linear_decode_attn_w8)"""
    assert y.dtype == torch.bfloat16 and y.stride(1) == 1
    _w8_check(W8, y.shape[1], H * D, y.device, "linear_decode_attn_w8")
    lib.call("db1_linear_decode_attn_w8", P(part), (int(klen) + 127) // 128, B, q, H, D, P(W8), P(y), y.stride(0), y.shape[1], stream())


def decode_chain_w8_supported(d, dff, H, D, klen) -> bool:
    return bool(lib.load().db1_decode_chain_w8_supported(int(d), int(dff), int(H), int(D), (int(klen) + 127) // 128))


def decode_chain_w8(part, klen, H, x_res, w_o8, w1_8, b1, w2_8, b2, w_qkv_next8, g1, be1, g2, be2, alpha, eps, h1_out, f_out, x_next, qkv_next, slot, w_o_next=None):
    """decode_chain with o_net, ff1, ff2, the next layer's qkv_net and ``w_o_next`` as packed fp8 buffers (w8_quantize of the [d, d],
    [2 dff, d], [d, dff], [3 d, d] and [d, d] weights; db1_decode_chain_w8): bit for bit decode_chain over w8_unpack of them.  d and dff are
    read from the bf16 operands (x_res, b1); the same scratch and slot rule as decode_chain."""
    for t in (x_res, b1, b2, g1, be1, g2, be2):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError("decode_chain_w8: the input row, the biases and the LayerNorm parameters must be contiguous bf16 tensors")
    d, dff, dev = x_res.numel(), b1.numel() // 2, x_res.device
    for name, t, N, K in (("w_o8", w_o8, d, d), ("w1_8", w1_8, 2 * dff, d), ("w2_8", w2_8, d, dff), ("w_qkv_next8", w_qkv_next8, 3 * d, d), ("w_o_next", w_o_next, d, d)):
        if t is None and name in ("w_qkv_next8", "w_o_next"):
            continue
        # (the size is the format's own rule, N K + 4 N K / 128: a wrong buffer is refused before the library is touched)
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.device != dev or K % 128 or
                t.numel() != N * K + 4 * N * (K // 128)):
            raise ValueError(f"decode_chain_w8: {name} must be the packed uint8 buffer of a [{N}, {K}] matrix on {dev} (w8_quantize; K % 128 == 0)")
    lib.call("db1_decode_chain_w8", P(part), (int(klen) + 127) // 128, int(H), P(x_res), P(w_o8), P(w1_8), P(b1), P(w2_8), P(b2), P(w_qkv_next8), P(w_o_next), P(g1), P(be1),
             P(g2), P(be2), float(alpha), float(eps), P(h1_out), P(f_out), P(x_next), P(qkv_next), P(decode_chain_scratch(x_res.device)), int(slot), int(d), int(dff), stream())


def _w8_check(W8, N, K, device, who):
    if W8.dtype != torch.uint8 or W8.dim() != 1 or not W8.is_contiguous() or W8.device != device or K % 128 or W8.numel() != w8_bytes(N, K):
        raise ValueError(f"{who}: the weight must be the packed uint8 buffer of a [{N}, {K}] matrix on {device} (w8_quantize; K % 128 == 0)")


def ring_advance(state, q, cap):
    lib.call("db1_ring_advance", P(state), int(q), int(cap), stream())


def relattn_flash_supported(B, L, H, D, dtype) -> bool:
    return bool(lib.load().db1_relattn_flash_supported(B, L, H, D, dt_code(dtype)))


def relattn_flash_probs_tiles(L: int) -> int:
    """1 KiB fragment images per (batch, head) of the kept probabilities: the tiles (key block of 32, 16-query tile) on or below the causal
    diagonal, stored as a triangle (db1_relattn_flash_probs_bytes)"""
    return int(lib.load().db1_relattn_flash_probs_bytes(1, int(L), 1)) // 1024


def relattn_flash_probs_full(probs, L: int):
    """(tests / tools) the triangle of kept-probability images [B*H, tiles, 512] expanded to [B*H, L/32, L/16, 512]; tiles above the causal
    diagonal, which do not exist, read NaN"""
    nkb, nt = L // 32, L // 16
    full = torch.full((probs.shape[0], nkb, nt, 512), float("nan"), device=probs.device, dtype=probs.dtype)
    for jb in range(nkb):
        i0 = 2 * jb + jb * (nt - 1 - jb)
        full[:, jb, 2 * jb:] = probs[:, i0:i0 + nt - 2 * jb]
    return full


def relattn_flash_fwd(qu, qv, qkv5, R, out, lse, B, L, H, D, shift, scale, probs=None, mblk=None):
    """qkv5: the packed activations viewed [B, L, 3, H, D]; k / v are addressed inside it by stride.
    probs [B*H, relattn_flash_probs_tiles(L), 512] bf16 + mblk [B*H, L/32, L] f32 (optional): the unnormalised probabilities (a triangle of
    fragment images, see the header) and their reference maxima, kept for the stored-probabilities backward."""
    assert probs is None or probs.numel() * 2 == int(lib.load().db1_relattn_flash_probs_bytes(B, L, H)), "probs: db1_relattn_flash_probs_bytes(B, L, H) bytes"
    k, v = qkv5[:, :, 1], qkv5[:, :, 2]
    vis = L * (L + 1) / 2 if shift >= L else (shift * (shift + 1) / 2 + (L - shift) * shift)   # visible (query, key) pairs
    _timed("flash_fwd", 3 * 2.0 * B * H * vis * D,   # (q+u).k, (q+v).R, P.v over the visible pairs
           lambda: lib.call("db1_relattn_flash_fwd", P(qu), P(qv), P(k), P(v), k.stride(1), k.stride(0), P(R), P(out), P(lse),
                            B, L, H, D, shift, float(scale), P(probs) if probs is not None else _vp(0), P(mblk) if mblk is not None else _vp(0), stream()))


def relattn_flash_bwd(qu, qv, qkv5, R, out, dout, lse, delta, dqkv5, dT, B, L, H, D, shift, scale, store_probs=True, probs=None, mblk=None):
    """probs + mblk (from relattn_flash_fwd): nothing is recomputed.  Otherwise store_probs: give the library the scratch for P and dS
    (the key side then runs without recomputation); False = both sides recompute (no scratch)."""
    k, v = qkv5[:, :, 1], qkv5[:, :, 2]
    if probs is not None:
        ws, wsn = _ws("db1_relattn_flash_bwd_workspace_bytes", (B, L, H, 1), out.device)
    else:
        ws, wsn = _ws("db1_relattn_flash_bwd_workspace_bytes", (B, L, H, 0), out.device) if store_probs else (_vp(0), 0)
    dq, dk, dv = dqkv5[:, :, 0], dqkv5[:, :, 1], dqkv5[:, :, 2]
    vis = L * (L + 1) / 2 if shift >= L else (shift * (shift + 1) / 2 + (L - shift) * shift)
    _timed("flash_bwd", 6 * 2.0 * B * H * vis * D,   # twice the forward's algorithmic work (bwd_q + bwd_kv; dq_r / dR run as separate kernels)
           lambda: lib.call("db1_relattn_flash_bwd", P(qu), P(qv), P(k), P(v), k.stride(1), k.stride(0), P(R), P(out), P(dout), P(lse), P(delta),
                            P(dq), P(dk), P(dv), dq.stride(1), dq.stride(0), P(dT), B, L, H, D, shift, float(scale),
                            P(probs) if probs is not None else _vp(0), P(mblk) if mblk is not None else _vp(0), ws, wsn, stream()))


def patch_normalize(pixels, patches, p):
    n, C, Hh, Ww = pixels.shape
    lib.call("db1_patch_normalize", P(pixels), P(patches), n, C, Hh, Ww, p, dt_code(pixels), dt_code(patches), stream())


def im2col3x3(x, cols, N, C, p):
    lib.call("db1_im2col3x3", P(x), P(cols), N, C, p, cols.shape[-1], dt_code(x), stream())


def col2im3x3(dcols, dx, N, C, p):
    lib.call("db1_col2im3x3", P(dcols), P(dx), N, C, p, dcols.shape[-1], dt_code(dx), stream())


def nhwc_to_nchw(x, y, N, C, hw):
    lib.call("db1_nhwc_to_nchw", P(x), P(y), N, C, hw, dt_code(x), stream())


def nchw_to_nhwc(x, y, N, C, hw):
    lib.call("db1_nchw_to_nhwc", P(x), P(y), N, C, hw, dt_code(x), stream())


def groupnorm_gelu_fwd(x, gamma, beta, y, mean, rstd, N, C, hw, groups=32, eps=1e-5):
    lib.call("db1_groupnorm_gelu_fwd", P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), N, C, hw, groups, float(eps),
             dt_code(x), dt_code(gamma), stream())


def groupnorm_gelu_bwd(dy, x, gamma, beta, mean, rstd, dx, dgamma_acc, dbeta_acc, N, C, hw, groups=32):
    lib.call("db1_groupnorm_gelu_bwd", P(dy), P(x), P(gamma), P(beta), P(mean), P(rstd), P(dx), P(dgamma_acc), P(dbeta_acc),
             N, C, hw, groups, dt_code(x), dt_code(gamma), stream())


# ---- channels-last vision pipeline (bf16 path)
def patch_normalize_nhwc(pixels, patches, p):
    n, C, Hh, Ww = pixels.shape
    lib.call("db1_patch_normalize_nhwc", P(pixels), P(patches), n, C, Hh, Ww, p, dt_code(pixels), dt_code(patches), stream())


def im2col3x3_nhwc(x, cols, N, C, p):
    lib.call("db1_im2col3x3_nhwc", P(x), P(cols), N, C, p, cols.shape[-1], dt_code(x), stream())


def col2im3x3_nhwc(dcols, dx, N, C, p):
    lib.call("db1_col2im3x3_nhwc", P(dcols), P(dx), N, C, p, dcols.shape[-1], dt_code(dx), stream())


def conv_weight_permute(w, wp, Cout, Cin):
    lib.call("db1_conv_weight_permute", P(w), P(wp), Cout, Cin, wp.shape[-1], dt_code(w), dt_code(wp), stream())


def conv_wgrad_unpermute(gp, g_acc, Cout, Cin):
    assert gp.dtype == torch.float32 and g_acc.dtype == torch.float32
    lib.call("db1_conv_wgrad_unpermute", P(gp), P(g_acc), Cout, Cin, gp.shape[-1], stream())


def conv_weight_permute_t(w, wp, Cout, Cin):
    lib.call("db1_conv_weight_permute_t", P(w), P(wp), Cout, Cin, dt_code(w), dt_code(wp), stream())


def conv3x3_implicit_fwd(x, w_op, bias, y, n_patches, sign=1, res=None):
    """64 -> 64 channel 3x3 conv on 16x16 patches, channels-last bf16, no column matrix (sign=-1: data gradient)"""
    if res is not None:   # y = conv + bias + res
        assert res.dtype == torch.bfloat16 and res.is_contiguous()
        lib.call("db1_conv3x3_implicit_fwd_res", P(x), P(w_op), P(bias), P(res), P(y), n_patches, sign, dt_code(bias) if bias is not None else 0, stream())
        return
    lib.call("db1_conv3x3_implicit_fwd", P(x), P(w_op), P(bias), P(y), n_patches, sign, dt_code(bias) if bias is not None else 0, stream())


def conv1_fused_fwd(x_cl, w_op, bias, cols, y, n_patches):
    """3 -> 64 channel 3x3 conv on 16x16 patches + its column matrix in one kernel (db1_conv1_fused_fwd)"""
    assert x_cl.dtype == torch.bfloat16 and w_op.shape == (64, 32) and cols.shape[1] == 32 and y.shape[1] == 64
    lib.call("db1_conv1_fused_fwd", P(x_cl), P(w_op), P(bias), P(cols), P(y), n_patches, dt_code(bias) if bias is not None else 0, stream())


def conv3x3_implicit_wgrad(dy, x, gp_acc, n_patches, gbias_acc=None):
    assert gp_acc.dtype == torch.float32 and gp_acc.shape[-1] == 576
    ws, wsn = _ws("db1_conv3x3_implicit_wgrad_workspace_bytes", (int(n_patches),), dy.device)   # fixed-order partial sums: bit-reproducible
    lib.call("db1_conv3x3_implicit_wgrad", P(dy), P(x), P(gp_acc), P(gbias_acc), n_patches, ws, wsn, stream())


def groupnorm_gelu_nhwc_fwd(x, gamma, beta, y, mean, rstd, N, C, hw, groups=32, eps=1e-5):
    lib.call("db1_groupnorm_gelu_nhwc_fwd", P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), N, C, hw, groups, float(eps),
             dt_code(x), dt_code(gamma), stream())


def groupnorm_gelu_nhwc_bwd(dy, x, gamma, beta, mean, rstd, dx, dgamma_acc, dbeta_acc, N, C, hw, groups=32, res=None):
    """``res``: added to dx in fp32 before its rounding (the residual branch's gradient), instead of a separate add pass"""
    assert res is None or (res.shape == dx.shape and res.dtype == dx.dtype and res.is_contiguous() and res.data_ptr() != dx.data_ptr())
    ws, wsn = _ws("db1_groupnorm_gelu_nhwc_bwd_workspace_bytes", (int(N),), x.device)   # per-sample rows, summed in a fixed order (no atomics)
    lib.call("db1_groupnorm_gelu_nhwc_bwd", P(dy), P(x), P(gamma), P(beta), P(mean), P(rstd), P(dx), P(res) if res is not None else _vp(0), P(dgamma_acc), P(dbeta_acc),
             N, C, hw, groups, dt_code(x), dt_code(gamma), ws, wsn, stream())


def sumsq_acc(x, acc):
    _timed("sumsq", float(x.numel() * x.element_size()), lambda: lib.call("db1_sumsq_acc", P(x), P(acc), x.numel(), dt_code(x), stream()))


def grad_norm_sq(x, acc):
    """acc[0] = sum(x^2), deterministic (db1_grad_norm_sq: fixed-order partial sums, no atomics): what the engine's global-norm clip uses"""
    ws, wsn = _ws("db1_grad_norm_sq_workspace_bytes", (x.numel(),), x.device)
    _timed("sumsq", float(x.numel() * x.element_size()), lambda: lib.call("db1_grad_norm_sq", P(x), P(acc), x.numel(), dt_code(x), ws, wsn, stream()))


def adam_step(p32, g, m, v, p_work, lr, beta1, beta2, eps, wd, adamw, step, gscale=1.0, clip=0.0, norm_sq=None):
    # p, m, v read + written (24 B), g read, bf16 working copy written
    _timed("adam", float(p32.numel() * (24 + g.element_size() + (2 if p_work is not None else 0))),
           lambda: lib.call("db1_adam_step", P(p32), P(g), P(m), P(v), P(p_work), p32.numel(), float(lr), float(beta1), float(beta2), float(eps),
                            float(wd), int(bool(adamw)), int(step), float(gscale), float(clip), P(norm_sq), dt_code(g),
                            dt_code(p_work) if p_work is not None else 0, stream()))


def mulaw_discretize(x, ids, is_action, num_bins=1024, mu=100.0, M=256.0):
    assert x.dtype == torch.float32 and ids.dtype == torch.int32
    lib.call("db1_mulaw_discretize", P(x), P(ids), x.numel(), int(bool(is_action)), num_bins, float(mu), float(M), stream())


def mulaw_decode(ids, out, is_action, num_bins=1024, mu=100.0, M=256.0, oob_flag=None):
    assert ids.dtype in (torch.int32, torch.int64) and out.dtype == torch.float32 and ids.numel() == out.numel()
    assert oob_flag is None or oob_flag.dtype == torch.int32
    lib.call("db1_mulaw_decode", P(ids), P(out), ids.numel(), int(ids.dtype == torch.int64), int(bool(is_action)), num_bins, float(mu),
             float(M), P(oob_flag), stream())


ACT_MAX_WINDOW, ACT_MAX_LEN = 4096, 64     # db1_select_actions: the widest action window, the longest action


def select_actions_supported(V: int, ld: int, dtype, act_lo: int, act_hi: int) -> bool:
    return bool(lib.load().db1_select_actions_supported(int(V), int(ld), dt_code(dtype), int(act_lo), int(act_hi)))


def select_actions(logits2d, ctr, bins, next_ids, status, *, act_lo, act_hi, V=None, mask=None, values=None, num_bins=1024, greedy=True,
                   temperature=1.0, top_k=0, top_p=1.0, seed=0, step_base=0, stream_id=None):
    """one action token per row of ``logits2d`` [M, ld] (fp32 / bf16, the first V columns valid) on the device (db1_select_actions, rule in
    include/db1_hip.h): ``select_tokens``' choice over the columns [act_lo, act_hi) (at most 4096) that ``mask`` (uint8 [M, n_mask], 1 =
    allowed, the columns from act_lo on; None: all) leaves.  ``ctr`` (int32 [2], device) = {env_step, i}, READ only; for i < act_len =
    ``bins.shape[1]``: the bin token - act_lo goes to ``bins`` [M, act_len] (int32) at column i, its decoded action value to ``values``
    (float32 [M, act_len] or None) and the token to ``next_ids`` (int64, [M] or a column of [M, q]); i == act_len writes nothing; ``status``
    (int32 [M]) |= 1 for a row without a candidate, |= 2 for i out of range.  Capturable; raises ValueError on bad arguments before anything
    is launched."""
    who, dev = "select_actions", logits2d.device
    M, ld, V, act_lo, act_hi = _check_logits(who, logits2d, V, act_lo, act_hi, lambda V, ld: True)
    if act_hi - act_lo > ACT_MAX_WINDOW:
        raise ValueError(f"{who}: the window [{act_lo}, {act_hi}) is wider than {ACT_MAX_WINDOW} columns")
    _check_sampling(who, greedy, temperature, top_k, top_p)
    if not torch.is_tensor(bins) or bins.dim() != 2 or not 1 <= bins.shape[1] <= ACT_MAX_LEN:
        raise ValueError(f"{who}: bins must be a contiguous {torch.int32} tensor of shape ({M}, act_len) with act_len in [1, {ACT_MAX_LEN}] on {dev}")
    act_len = bins.shape[1]
    _check_tensor(who, "bins", bins, torch.int32, (M, act_len), dev)
    if values is not None:
        _check_tensor(who, "values", values, torch.float32, (M, act_len), dev)
    _check_vectors(who, dev, 2, ctr=ctr)
    _check_vectors(who, dev, M, status=status)
    _check_vectors(who, dev, M, optional=("stream_id",), stream_id=stream_id)
    _check_next_ids(who, next_ids, M, dev)
    n_mask = 0
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dim() != 2 or not 1 <= mask.shape[1] <= act_hi - act_lo:
            raise ValueError(f"{who}: mask must be a contiguous {torch.uint8} tensor of shape ({M}, n) with 1 <= n <= {act_hi - act_lo} on {dev}")
        n_mask = mask.shape[1]
        _check_tensor(who, "mask", mask, torch.uint8, (M, n_mask), dev)
    if int(num_bins) < 1:
        raise ValueError(f"{who}: num_bins {num_bins} must be >= 1")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lib.call("db1_select_actions", P(logits2d), M, V, max(ld, V), dt_code(logits2d), act_lo, act_hi, P(mask), n_mask, float(temperature), int(top_k),
             float(top_p), int(bool(greedy)), seed & 0xFFFFFFFF, seed >> 32, int(step_base), P(ctr), P(stream_id), act_len, int(num_bins), P(bins),
             P(values), P(next_ids), next_ids.stride(0), P(status), stream())


def obs_tokens(x, ids, *, bin_base, sep_id, num_bins=1024, mu=100.0, M=256.0):
    """float observations ``x`` [rows, obs_dim] (float32, contiguous) -> ``ids`` [rows, >= obs_dim + 1] (int64, unit column stride; a view of
    the observation call's static input ids): column j < obs_dim = ``bin_base`` + the tokenizer's observation bin of x[:, j]
    (``mulaw_discretize(is_action=False)``, the same ids), column obs_dim = ``sep_id`` (db1_obs_tokens).  Capturable; raises ValueError on bad
    arguments before anything is launched."""
    who = "obs_tokens"
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: x must be a contiguous {torch.float32} tensor of shape (rows, obs_dim)")
    rows, obs_dim = x.shape
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[0] != rows or ids.shape[1] < obs_dim + 1 or \
            ids.stride(1) != 1 or ids.stride(0) < obs_dim + 1 or ids.device != x.device:
        raise ValueError(f"{who}: ids must be an {torch.int64} tensor of shape ({rows}, >= {obs_dim + 1}) with unit column stride on {x.device}")
    if int(num_bins) < 1 or int(bin_base) < 0 or int(sep_id) < 0:
        raise ValueError(f"{who}: num_bins {num_bins} must be >= 1, bin_base {bin_base} and sep_id {sep_id} >= 0")
    lib.call("db1_obs_tokens", P(x), rows, obs_dim, P(ids), ids.stride(0), int(bin_base), int(sep_id), int(num_bins), float(mu), float(M), stream())


GEMM_KERNELS = {0: "strided-fp32", 1: "tile128", 2: "tile256", 3: "pp-k64", 4: "pp-k32", 5: "w4", 6: "skinny", 7: "w4n"}


def gemm_kernel_choice(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, beta: float = 0.0, ws_bytes: int = -1):
    """(kernel name, split-K?, tail-call?) that ``gemm(a, b, out)`` would take (db1_gemm_kernel_choice)"""
    M, K = a.shape
    N = b.shape[1]
    code = lib.load().db1_gemm_kernel_choice(M, N, K, dt_code(a), dt_code(b), dt_code(out), a.stride(0), a.stride(1), b.stride(0), b.stride(1),
                                             out.stride(0), out.stride(1), 1, 1, float(beta), int(ws_bytes))
    return GEMM_KERNELS[code & 15], bool(code & 16), bool(code & 32)


def gemm_force_generic(on: bool):
    """test hook (include/db1_hip_test.h), thread-local"""
    lib.load().db1_test_gemm_force_generic(1 if on else 0)


def gemm_tile_override(tile: int):
    """test / tuning hook (include/db1_hip_test.h), thread-local: 0 = measured heuristics; 128 / 256 / 512 / 1024 pin one bf16 tile kernel"""
    lib.load().db1_test_gemm_tile_override(int(tile))


def flash_fwd2(mode):
    """test hook (include/db1_hip_test.h), thread-local: 0 / False = the compiled key-block loop, 1 / True = the default (hand-scheduled
    4-wave forward), 2 = the hand-scheduled 8-wave forward"""
    lib.load().db1_test_flash_fwd2(int(mode))
