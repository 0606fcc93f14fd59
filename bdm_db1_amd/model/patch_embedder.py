"""The ResNet-style image-patch embedder of the vision encoder (the reference's vision_embedding.py:65-180), per 16 x 16 patch:
conv1 -> GroupNorm + GELU -> conv -> GroupNorm + GELU -> conv -> + conv1's output -> projection to d_model -> + position embeddings.
A plain object the model builds once; its parameters stay in the model's arena under the reference's names.  Two pipelines:
  * channels-last (bf16, 16 x 16 patches, ``model.use_channels_last``): activations [N * 256, 64], tap-major weight operands, no layout
    shuffle between the convolutions (vision.hip); the 64 -> 64 convolutions are implicit GEMMs (conv_implicit.hip) unless
    ``model.use_implicit_conv`` is off, which keeps explicit column matrices (a reference path of the tests);
  * NCHW (fp32, other patch sizes, or ``use_channels_last`` off): the reference's layout end to end, im2col + GEMM.
Which kernel a convolution takes follows from the pipeline and its input channels alone.  There is no torch-op fallback."""
import weakref
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from .. import ops

PE = "vision_encoder.patch_embeddings."
CONVS = (PE + "conv1", PE + "residual_path.2", PE + "residual_path.5")
NORMS = (PE + "residual_path.0", PE + "residual_path.3")
PROJ = PE + "projection"
ROW_TABLE, COL_TABLE = "vision_encoder.row_position_embeddings.weight", "vision_encoder.col_position_embeddings.weight"


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass
class ConvSaved:
    implicit: bool            # True: no column matrix was built, ``x`` is the convolution's input [N * hw, 64]
    x: torch.Tensor           # False: ``x`` is the column matrix [N * hw, kpad]


@dataclass
class PatchCtx:
    """what one forward keeps for its backward"""
    channels_last: bool       # which pipeline ran
    n_img: int
    N: int                    # patches
    Np: int                   # rows of the projection's operand (N, or N padded to whole 256-row tiles)
    C: int                    # input channels
    convs: List[ConvSaved] = field(default_factory=list)     # conv1, residual_path.2, residual_path.5
    # residual_path.0, residual_path.3: (the GroupNorm's input = a convolution's output, [N * hw, 64] channels-last or [N, 64, hw] NCHW; mean; rstd)
    norms: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = field(default_factory=list)
    y: Optional[torch.Tensor] = None         # the projection's input [Np, 64 * hw]: (pixel, channel) columns channels-last, (channel, pixel) NCHW
    row_ids: Optional[torch.Tensor] = None   # [N] int64
    col_ids: Optional[torch.Tensor] = None


class PatchEmbedder:
    def __init__(self, model):
        self.m = weakref.proxy(model)    # (not a strong reference: a model <-> embedder cycle would keep a dropped model's arena until the collector runs)
        self.hw = model.patch_size * model.patch_size
        self._operands = {}              # (tag, weight version | "static") -> weight in the layout a kernel wants: operand()

    def position_ids(self, h0: int, w0: int, n_img: int):
        """eval: midpoint rule; train: uniform pick in [low, high) per (image, position) (vision_embedding.py:134-172)."""
        vocab = self.m.vision_position_vocab_size
        seq = torch.arange(h0 * w0)
        row = torch.div(seq, w0, rounding_mode="trunc")
        col = seq % w0
        col_hi = ((col + 1) / w0 * vocab).to(torch.int32)
        col_lo = (col / w0 * vocab).to(torch.int32)
        row_hi = ((row + 1) / h0 * vocab).to(torch.int32)
        row_lo = (row / h0 * vocab).to(torch.int32)
        if self.m.training:
            r = (torch.rand(n_img, h0 * w0) * (row_hi - row_lo) + row_lo).floor().to(torch.int64)
            c = (torch.rand(n_img, h0 * w0) * (col_hi - col_lo) + col_lo).floor().to(torch.int64)
        else:
            r = ((row_lo + row_hi) / 2).int().to(torch.int64).unsqueeze(0).expand(n_img, -1)
            c = ((col_lo + col_hi) / 2).int().to(torch.int64).unsqueeze(0).expand(n_img, -1)
        return r.contiguous(), c.contiguous()

    # ------------------------------------------------------------------ weight operands
    def operand(self, tag: str, wname: str, shape, fill) -> torch.Tensor:
        """weight ``wname`` in the layout a kernel wants: ``fill(weight, buffer)`` writes it into a ``shape`` buffer.  One rule for every
        kind: built once per weight version, and the entries of older versions go when a new one is built; in a captured training step
        (``_graph_static``) one fixed buffer per tag, refilled by every call -- a replay reads the weights of ITS step at the same address."""
        m = self.m
        key = (tag, "static" if m._graph_static else m._wversion)
        buf = self._operands.get(key)
        if buf is None:
            self._operands = {k: v for k, v in self._operands.items() if k[1] in (m._wversion, "static")}
            buf = self._operands[key] = torch.empty(*shape, device=m.dev, dtype=m.compute_dtype)
            fill(m.W(wname), buf)
        elif m._graph_static:
            fill(m.W(wname), buf)
        return buf

    def _conv_operand(self, k: int, Cin: int) -> torch.Tensor:
        """GEMM operand [64, kpad] (tap-major columns, zero padded to a multiple of 8) of a 3x3 conv weight"""
        wname = CONVS[k] + ".weight"
        return self.operand(wname, wname, (64, _round_up(9 * Cin, 8)), lambda w, out: ops.conv_weight_permute(w, out, 64, Cin))

    def _proj_operand(self) -> torch.Tensor:
        """the patch projection weight [d, 64 * hw] with its columns in (pixel, channel) order: the channels-last convolution output
        [N * hw, 64] IS [N, hw * 64], so the projection (and its data gradient) needs no layout shuffle of the activations -- a 67 MB
        copy of the weight per optimizer step instead of two passes over [N, 16 384] per batch"""
        d, hw = self.m.d_model, self.hw
        return self.operand(PROJ + ".weight^cl", PROJ + ".weight", (d, hw * 64), lambda w, out: ops.nchw_to_nhwc(w, out, d, 64, hw))

    # ------------------------------------------------------------------ forward
    def forward(self, pixels: torch.Tensor, row_ids=None, col_ids=None):
        """pixels [n_img, C, H, W] -> (emb [n_img, h0 * w0, d], ctx)"""
        m = self.m
        pixels = pixels.to(device=m.dev, dtype=torch.float32).contiguous()
        n_img, C, Hh, Ww = pixels.shape
        h0, w0 = Hh // m.patch_size, Ww // m.patch_size
        N = n_img * h0 * w0
        cl = m.compute_dtype == torch.bfloat16 and self.hw == 256 and m.use_channels_last
        ctx = PatchCtx(channels_last=cl, n_img=n_img, N=N, Np=N, C=C)
        emb = self._forward_cl(pixels, ctx) if cl else self._forward_nchw(pixels, ctx)
        if row_ids is None:
            row_ids, col_ids = self.position_ids(h0, w0, n_img)
        ctx.row_ids, ctx.col_ids = m._dev_ids(row_ids).reshape(-1), m._dev_ids(col_ids).reshape(-1)
        assert ctx.row_ids.numel() == N
        # emb += row_position_embeddings[row_ids] + col_position_embeddings[col_ids] (vision_embedding.py:170-178) in one pass over emb
        ops.vision_pos_add(emb.view(N, m.d_model), m.W(ROW_TABLE), m.W(COL_TABLE), ctx.row_ids, ctx.col_ids)
        return emb.view(n_img, h0 * w0, m.d_model), ctx

    def _norm_fwd(self, ctx: PatchCtx, k: int, x):
        """GroupNorm + GELU k on a convolution's output, in the pipeline's layout"""
        m, N = self.m, ctx.N
        a, mean, rstd = m._new(*x.shape), m._new(N * 32, dtype=torch.float32), m._new(N * 32, dtype=torch.float32)
        fwd = ops.groupnorm_gelu_nhwc_fwd if ctx.channels_last else ops.groupnorm_gelu_fwd
        fwd(x, m.W(NORMS[k] + ".weight"), m.W(NORMS[k] + ".bias"), a, mean, rstd, N, 64, self.hw)
        ctx.norms.append((x, mean, rstd))
        return a

    def _conv_fwd_cl(self, ctx: PatchCtx, k: int, x_cl, Cin: int, out=None, res=None):
        """convolution k of the channels-last pipeline -> [N * 256, 64]; ``out`` / ``res``: write into this buffer / add this residual in
        the epilogue (implicit convolutions only)"""
        m, N = self.m, ctx.N
        wp, bias = self._conv_operand(k, Cin), m.W(CONVS[k] + ".bias")
        if Cin == 64 and m.use_implicit_conv:  # implicit GEMM: the shifted pixels are gathered by the LDS-DMA, no column matrix
            out = m._new(N * 256, 64) if out is None else out
            ops.conv3x3_implicit_fwd(x_cl, wp, bias, out, N, sign=1, res=res)
            ctx.convs.append(ConvSaved(True, x_cl))
            return out
        assert out is None and res is None, "only an implicit convolution writes into a given buffer or adds a residual"
        out, cols = m._new(N * 256, 64), m._new(N * 256, wp.shape[1])
        if Cin == 3:   # one streaming kernel: column matrix (27 + 5 zero columns) + convolution
            ops.conv1_fused_fwd(x_cl, wp, bias, cols, out, N)
        else:
            ops.im2col3x3_nhwc(x_cl, cols, N, Cin, m.patch_size)
            ops.gemm(cols, wp.t(), out, bias=bias)
        ctx.convs.append(ConvSaved(False, cols))
        return out

    def _forward_cl(self, pixels, ctx: PatchCtx):
        m, N, hw = self.m, ctx.N, self.hw
        patches = m._new(N * hw, ctx.C)
        ops.patch_normalize_nhwc(pixels, patches, m.patch_size)
        c1 = self._conv_fwd_cl(ctx, 0, patches, ctx.C)
        a0 = self._norm_fwd(ctx, 0, c1)
        a1 = self._norm_fwd(ctx, 1, self._conv_fwd_cl(ctx, 1, a0, 64))
        # (y, x, c) flattening against the column-permuted projection weight.  The patch count of a mixed batch is whatever the data gives
        # (4116, 20 680 ...): rows are padded with zeros to a multiple of 256 so that the K = 16 384 projection and its two gradients take
        # the 256 x 256 kernels (the 128-tile / generic kernels ran them at 0.24 PFLOP/s)
        ctx.Np = Np = _round_up(N, 256) if N >= 512 else N
        ypad = m._new(Np * hw, 64)
        if m.use_implicit_conv:   # the last convolution adds the residual in its epilogue and writes straight into the padded operand
            self._conv_fwd_cl(ctx, 2, a1, 64, out=ypad[:N * hw], res=c1)
        else:
            ops.add(c1, self._conv_fwd_cl(ctx, 2, a1, 64), ypad[:N * hw])
        if Np > N:
            ypad[N * hw:].zero_()
        ctx.y = ypad.view(Np, hw * 64)
        emb_pad = m._new(Np, m.d_model)
        ops.gemm(ctx.y, self._proj_operand().t(), emb_pad, bias=m.W(PROJ + ".bias"))
        return emb_pad[:N]

    # ---- NCHW pipeline: the reference's order end to end (the fp32 parity path; bf16 with use_channels_last off)
    def _conv_weight(self, k: int, K: int, Kp: int):
        """[64, Kp] view of a 3x3 conv weight in the compute dtype (zero-padded copy when Cin*9 is not a multiple of 8)"""
        w = self.m.W(CONVS[k] + ".weight").view(64, K)
        if Kp == K:
            return w
        wp = torch.zeros(64, Kp, device=self.m.dev, dtype=self.m.compute_dtype)
        ops.add2d(w, wp[:, :K], wp[:, :K])
        return wp

    def _conv_fwd_nchw(self, ctx: PatchCtx, k: int, x_nchw, Cin: int):
        """per-patch 3x3 conv as im2col + GEMM; returns the NHWC output [N * hw, 64]"""
        m, N = self.m, ctx.N
        K = Cin * 9
        Kp = _round_up(K, 8)  # conv1: 27 -> 32 zero-padded columns so its weight gradient can use the MFMA tile kernel (split-K)
        cols = m._new(N * self.hw, Kp)
        ops.im2col3x3(x_nchw, cols, N, Cin, m.patch_size)
        out = m._new(N * self.hw, 64)
        ops.gemm(cols, self._conv_weight(k, K, Kp).t(), out, bias=m.W(CONVS[k] + ".bias"))
        ctx.convs.append(ConvSaved(False, cols))
        return out

    def _relayout(self, shuffle, x, N: int, *shape):
        """ops.nhwc_to_nchw / ops.nchw_to_nhwc of a 64-channel activation into a new tensor of ``shape``"""
        y = self.m._new(*shape)
        shuffle(x, y, N, 64, self.hw)
        return y

    def _forward_nchw(self, pixels, ctx: PatchCtx):
        m, N, hw = self.m, ctx.N, self.hw
        patches = m._new(N, ctx.C, m.patch_size, m.patch_size)
        ops.patch_normalize(pixels, patches, m.patch_size)
        c1 = self._conv_fwd_nchw(ctx, 0, patches, ctx.C)
        a0 = self._norm_fwd(ctx, 0, self._relayout(ops.nhwc_to_nchw, c1, N, N, 64, hw))
        c2 = self._conv_fwd_nchw(ctx, 1, a0, 64)
        a1 = self._norm_fwd(ctx, 1, self._relayout(ops.nhwc_to_nchw, c2, N, N, 64, hw))
        c3 = self._conv_fwd_nchw(ctx, 2, a1, 64)
        ops.add(c1, c3, c3)                                                   # residual (NHWC)
        ctx.y = self._relayout(ops.nhwc_to_nchw, c3, N, N, 64 * hw)           # NCHW flatten = projection weight layout
        emb = m._new(N, m.d_model)
        ops.gemm(ctx.y, m.W(PROJ + ".weight").view(m.d_model, 64 * hw).t(), emb, bias=m.W(PROJ + ".bias"))
        return emb

    # ------------------------------------------------------------------ backward
    def backward(self, demb: torch.Tensor, ctx: PatchCtx):
        """demb [N, d] (compute dtype, contiguous): accumulates the gradients of the embedder's parameters and of the two position tables"""
        ops.embed_scatter_add(demb, ctx.row_ids, self.m.G(ROW_TABLE))
        ops.embed_scatter_add(demb, ctx.col_ids, self.m.G(COL_TABLE))
        (self._backward_cl if ctx.channels_last else self._backward_nchw)(demb, ctx)

    def _norm_bwd(self, ctx: PatchCtx, k: int, da, **kw):
        m, (x, mean, rstd) = self.m, ctx.norms[k]
        dx = m._new(*x.shape)
        bwd = ops.groupnorm_gelu_nhwc_bwd if ctx.channels_last else ops.groupnorm_gelu_bwd
        bwd(da, x, m.W(NORMS[k] + ".weight"), m.W(NORMS[k] + ".bias"), mean, rstd, dx,
            m.G(NORMS[k] + ".weight"), m.G(NORMS[k] + ".bias"), ctx.N, 64, self.hw, **kw)
        return dx

    def _conv_bwd_cl(self, ctx: PatchCtx, k: int, dy, Cin: int, need_dx: bool):
        m, N, sv = self.m, ctx.N, ctx.convs[k]
        wname, bname = CONVS[k] + ".weight", CONVS[k] + ".bias"
        wp = self._conv_operand(k, Cin)
        gp = torch.zeros(64, wp.shape[1], device=m.dev, dtype=torch.float32)
        if sv.implicit:   # (the bias gradient -- column sums of dy -- comes out of the same kernel)
            ops.conv3x3_implicit_wgrad(dy, sv.x, gp, N, gbias_acc=m.G(bname))
        else:
            ops.gemm(dy.t(), sv.x, gp, beta=1.0)
            ops.colsum_acc(dy, m.G(bname))
        ops.conv_wgrad_unpermute(gp, m.G(wname), 64, Cin)
        if not need_dx:
            return None
        dx = m._new(N * 256, Cin)
        if sv.implicit:   # the same kernel against the data-gradient operand [c_in, tap*64 + c_out]
            wt = self.operand(wname + "^T", wname, (64, 576), lambda w, out: ops.conv_weight_permute_t(w, out, 64, 64))
            ops.conv3x3_implicit_fwd(dy, wt, None, dx, N, sign=-1)
        else:
            dcols = m._new(sv.x.shape[0], wp.shape[1])
            ops.gemm(dy, wp, dcols)
            ops.col2im3x3_nhwc(dcols, dx, N, Cin, m.patch_size)
        return dx

    def _backward_cl(self, demb, ctx: PatchCtx):
        m, N, Np, d, hw = self.m, ctx.N, ctx.Np, self.m.d_model, self.hw
        # the weight gradient comes out with (pixel, channel) columns: shuffled back per weight row and added (fp32, two passes over 134 MB),
        # the data gradient [N, hw * 64] is channels-last already
        dpad = demb
        if Np > N:                                             # zero rows for the padded patches
            dpad = m._new(Np, d)
            dpad[:N].copy_(demb)
            dpad[N:].zero_()
        gp = torch.empty(d, hw * 64, device=m.dev, dtype=torch.float32)
        ops.gemm(dpad.t(), ctx.y, gp)
        gpt = torch.empty(d, 64 * hw, device=m.dev, dtype=torch.float32)
        ops.nhwc_to_nchw(gp, gpt, d, 64, hw)
        gw = m.G(PROJ + ".weight").view(d, 64 * hw)
        ops.add(gpt, gw, gw)
        ops.colsum_acc(demb, m.G(PROJ + ".bias"))
        dy_pad = m._new(Np * hw, 64)
        ops.gemm(dpad, self._proj_operand(), dy_pad.view(Np, hw * 64))
        dy = dy_pad[:N * hw]                                   # gradient w.r.t. the residual sum, channels-last
        da1 = self._conv_bwd_cl(ctx, 2, dy, 64, True)
        da0 = self._conv_bwd_cl(ctx, 1, self._norm_bwd(ctx, 1, da1), 64, True)
        dc1 = self._norm_bwd(ctx, 0, da0, res=dy)              # + the residual branch's gradient, in the same pass
        self._conv_bwd_cl(ctx, 0, dc1, ctx.C, False)

    def _conv_bwd_nchw(self, ctx: PatchCtx, k: int, dy_nhwc, Cin: int, need_dx: bool):
        m, N, cols = self.m, ctx.N, ctx.convs[k].x
        wname, bname = CONVS[k] + ".weight", CONVS[k] + ".bias"
        K, Kp = Cin * 9, cols.shape[1]
        if Kp == K:
            ops.gemm(dy_nhwc.t(), cols, m.G(wname).view(64, K), beta=1.0)
        else:  # padded columns: reduce into a [64, Kp] float32 scratch, then add its first K columns to the gradient
            gp = torch.zeros(64, Kp, device=m.dev, dtype=torch.float32)
            ops.gemm(dy_nhwc.t(), cols, gp, beta=1.0)
            g = m.G(wname).view(64, K)
            ops.add2d(gp[:, :K], g, g)
        ops.colsum_acc(dy_nhwc, m.G(bname))
        if not need_dx:
            return None
        dcols = m._new(cols.shape[0], Kp)
        ops.gemm(dy_nhwc, self._conv_weight(k, K, Kp), dcols)
        dx = m._new(N, Cin, self.hw)
        ops.col2im3x3(dcols, dx, N, Cin, m.patch_size)
        return dx

    def _backward_nchw(self, demb, ctx: PatchCtx):
        m, N, d, hw = self.m, ctx.N, self.m.d_model, self.hw
        ops.gemm(demb.t(), ctx.y, m.G(PROJ + ".weight").view(d, 64 * hw), beta=1.0)
        ops.colsum_acc(demb, m.G(PROJ + ".bias"))
        dy = m._new(N, 64 * hw)
        ops.gemm(demb, m.W(PROJ + ".weight").view(d, 64 * hw), dy)
        dy_nhwc = self._relayout(ops.nchw_to_nhwc, dy, N, N * hw, 64)
        da1 = self._conv_bwd_nchw(ctx, 2, dy_nhwc, 64, True)
        dc2 = self._relayout(ops.nchw_to_nhwc, self._norm_bwd(ctx, 1, da1), N, N * hw, 64)
        da0 = self._conv_bwd_nchw(ctx, 1, dc2, 64, True)
        dc1 = self._relayout(ops.nchw_to_nhwc, self._norm_bwd(ctx, 0, da0), N, N * hw, 64)
        ops.add(dc1, dy_nhwc, dc1)                             # residual branch
        self._conv_bwd_nchw(ctx, 0, dc1, ctx.C, False)
