"""The image-patch embedder (bdm_db1_amd/model/patch_embedder.py) driven directly at d = 64: which kernels each pipeline launches, the two bf16
pipelines against each other, the padded projection rows, and the weight-operand cache.  The kernels themselves are pinned bit for bit by
test_vision_kernels_gpu.py and the model-level paths to the oracle by test_model_gpu.py / test_geometry_vision_gpu.py; this file pins the
orchestration between them.  Every output of these paths was bit-equal between two runs of the same code (profiles/patch_embedder_refactor.txt,
part A: the kernels reduce in a fixed order), so the equalities here are torch.equal."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from golden_util import CASES, case_cfg, make_params  # noqa: E402

DEV = "cuda"
PE = "vision_encoder.patch_embeddings."
WEIGHTS = [PE + "conv1.weight", PE + "residual_path.2.weight", PE + "residual_path.5.weight", PE + "projection.weight"]
COUNTED = ["patch_normalize", "patch_normalize_nhwc", "conv1_fused_fwd", "im2col3x3", "im2col3x3_nhwc", "col2im3x3", "col2im3x3_nhwc",
           "conv3x3_implicit_fwd", "conv3x3_implicit_wgrad", "groupnorm_gelu_fwd", "groupnorm_gelu_nhwc_fwd", "groupnorm_gelu_bwd",
           "groupnorm_gelu_nhwc_bwd", "add", "gemm", "nchw_to_nhwc", "nhwc_to_nchw", "conv_weight_permute", "conv_weight_permute_t"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def build(dtype=torch.bfloat16, state=None, **over):
    from bdm_db1_amd import TransformerXL
    cfg = case_cfg("small_mixed")
    cfg.update(over)
    model = TransformerXL(SimpleNamespace(**cfg), compute_dtype=dtype)
    if state is None:
        state = {k: torch.from_numpy(v) for k, v in make_params(cfg, 100 + list(CASES).index("small_mixed")).items()}
    model.load_state_dict(state, strict=False)
    model.eval()       # (the midpoint rule for the position ids: no random draw)
    return model


def inputs(shape, d=64):
    g = torch.Generator().manual_seed(shape[0] * 131 + shape[1])
    n = shape[0] * (shape[2] // 16) * (shape[3] // 16)
    return (torch.rand(*shape, generator=g) * 255.0).to(DEV), torch.randn(n, d, generator=g).to(DEV)


def vision_grads(model):
    return {n: model.G(n).detach().clone() for n in model.arena.offsets if n.startswith("vision_encoder.")}


def run(model, pixels, demb):
    """forward + backward on zeroed gradient accumulators -> (emb, the 14 gradients the backward writes)"""
    model.arena.grad.zero_()
    emb, ctx = model.patch_embedder.forward(pixels)
    emb = emb.detach().clone()
    model.patch_embedder.backward(demb.to(model.compute_dtype).contiguous(), ctx)
    torch.cuda.synchronize()
    return emb, vision_grads(model)


class Counter:
    """call counts of ops.<name> (and the calls' positional arguments), as test_geometry_vision_gpu.py counts them"""

    def __init__(self, monkeypatch):
        from bdm_db1_amd import ops
        self.calls = {n: [] for n in COUNTED}
        for name in COUNTED:
            def wrapped(*a, _o=getattr(ops, name), _n=name, **k):
                self.calls[_n].append(a)
                return _o(*a, **k)
            monkeypatch.setattr(ops, name, wrapped)

    def take(self):
        """counts since the last take"""
        out = {n: len(v) for n, v in self.calls.items() if v}
        args = {n: list(v) for n, v in self.calls.items()}
        for v in self.calls.values():
            del v[:]
        return out, args


def rel_err(got, ref):
    got, ref = got.double().cpu().numpy(), ref.double().cpu().numpy()
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


_nchw_ref = {}


def nchw_reference(shape):
    """the bf16 NCHW pipeline on the same inputs (computed once per input shape)"""
    if shape not in _nchw_ref:
        model = build(**({"vision_num_input_channels": shape[1]} if shape[1] != 3 else {}))
        model.use_channels_last = False
        _nchw_ref[shape] = run(model, *inputs(shape))
    return _nchw_ref[shape]


# channels-last, implicit 64 -> 64 convolutions, conv1 as the fused streaming kernel; nothing but the projection weight goes through a layout shuffle
CL_FWD = {"patch_normalize_nhwc": 1, "conv_weight_permute": 3, "conv1_fused_fwd": 1, "groupnorm_gelu_nhwc_fwd": 2, "conv3x3_implicit_fwd": 2,
          "nchw_to_nhwc": 1, "gemm": 1}
CL_BWD = {"gemm": 3, "nhwc_to_nchw": 1, "add": 1, "conv3x3_implicit_wgrad": 2, "conv_weight_permute_t": 2, "conv3x3_implicit_fwd": 2,
          "groupnorm_gelu_nhwc_bwd": 2}
# explicit columns for the 64 -> 64 convolutions: two more column matrices and GEMMs, the residual added by ops.add into the padded operand
EXPLICIT_FWD = {"patch_normalize_nhwc": 1, "conv_weight_permute": 3, "conv1_fused_fwd": 1, "groupnorm_gelu_nhwc_fwd": 2, "im2col3x3_nhwc": 2,
                "add": 1, "nchw_to_nhwc": 1, "gemm": 3}
EXPLICIT_BWD = {"gemm": 7, "nhwc_to_nchw": 1, "add": 1, "col2im3x3_nhwc": 2, "groupnorm_gelu_nhwc_bwd": 2}
# NCHW: im2col + GEMM per convolution, three activation shuffles each way, the residual adds as ops.add
NCHW_FWD = {"patch_normalize": 1, "im2col3x3": 3, "gemm": 4, "nhwc_to_nchw": 3, "groupnorm_gelu_fwd": 2, "add": 1}
NCHW_BWD = {"gemm": 7, "nchw_to_nhwc": 3, "col2im3x3": 2, "groupnorm_gelu_bwd": 2, "add": 1}
# one input channel: conv1 through a column matrix + GEMM instead of the fused kernel
C1_FWD = {**{k: v for k, v in CL_FWD.items() if k != "conv1_fused_fwd"}, "im2col3x3_nhwc": 1, "gemm": 2}

PATHS = [
    # id, dtype, input shape, model switches, forward counts, backward counts, rows of the projection GEMM
    ("1-defaults-8", torch.bfloat16, (2, 3, 32, 32), {}, CL_FWD, CL_BWD, 8),
    ("2-defaults-592-padded", torch.bfloat16, (37, 3, 64, 64), {}, CL_FWD, CL_BWD, 768),
    ("3-defaults-512", torch.bfloat16, (32, 3, 64, 64), {}, CL_FWD, CL_BWD, 512),
    ("4-explicit-columns-592", torch.bfloat16, (37, 3, 64, 64), {"use_implicit_conv": False}, EXPLICIT_FWD, EXPLICIT_BWD, 768),
    ("5-bf16-nchw-8", torch.bfloat16, (2, 3, 32, 32), {"use_channels_last": False}, NCHW_FWD, NCHW_BWD, 8),
    ("6-fp32-8", torch.float32, (2, 3, 32, 32), {}, NCHW_FWD, NCHW_BWD, 8),
    ("7-one-channel-8", torch.bfloat16, (2, 1, 32, 32), {}, C1_FWD, CL_BWD, 8),
]


@pytest.mark.parametrize("case", PATHS, ids=[p[0] for p in PATHS])
def test_which_kernels_ran(case, monkeypatch):
    _, dtype, shape, switches, want_fwd, want_bwd, proj_rows = case
    model = build(dtype, **({"vision_num_input_channels": shape[1]} if shape[1] != 3 else {}))
    for k, v in switches.items():
        assert hasattr(model, k)
        setattr(model, k, v)
    pixels, demb = inputs(shape)
    counter = Counter(monkeypatch)
    model.arena.grad.zero_()
    emb, ctx = model.patch_embedder.forward(pixels)
    fwd, fwd_args = counter.take()
    emb = emb.detach().clone()
    model.patch_embedder.backward(demb.to(dtype).contiguous(), ctx)
    torch.cuda.synchronize()
    bwd, bwd_args = counter.take()
    assert fwd == want_fwd, fwd
    assert bwd == want_bwd, bwd
    channels_last = dtype == torch.bfloat16 and switches.get("use_channels_last", True)
    assert ctx.channels_last == channels_last and ctx.N == demb.shape[0] and ctx.Np == proj_rows
    implicit = channels_last and switches.get("use_implicit_conv", True)
    assert [c.implicit for c in ctx.convs] == [False, implicit, implicit]
    # the projection is the last GEMM of the forward and the first two of the backward: all three over the padded row count
    assert fwd_args["gemm"][-1][0].shape[0] == proj_rows and fwd_args["gemm"][-1][2].shape[0] == proj_rows
    assert bwd_args["gemm"][0][0].shape[1] == proj_rows and bwd_args["gemm"][1][0].shape[0] == proj_rows
    if channels_last:      # no layout shuffle of an activation: the only nchw_to_nhwc is the projection weight's, the only nhwc_to_nchw its fp32 gradient's
        assert [tuple(a[0].shape) for a in fwd_args["nchw_to_nhwc"]] == [(64, 64, 16, 16)]
        assert [(tuple(a[0].shape), a[0].dtype) for a in bwd_args["nhwc_to_nchw"]] == [((64, 64 * 256), torch.float32)]
        # ... and the result against the bf16 NCHW pipeline on the same inputs: 3e-2 of each tensor's max, the bound
        # test_bf16_channels_last_vision_path_matches_nchw_path_and_oracle states for these two pipelines (same maths, different rounding points)
        ref_emb, ref_grads = nchw_reference(shape)
        grads = vision_grads(model)
        errs = {"emb": rel_err(emb, ref_emb), **{n: rel_err(grads[n], ref_grads[n]) for n in ref_grads}}
        print({k: f"{v:.2e}" for k, v in errs.items()})
        assert len(ref_grads) == 14 and max(errs.values()) < 3e-2, errs


def test_padded_projection_rows_have_no_effect(monkeypatch):
    """592 patches -> 768 projection rows.  Every buffer the embedder takes from the model is filled with NaN before it is handed out -- the
    176 pad rows of the projection's operand with it -- and the embedding and all 14 gradients come out bit-equal to the plain run: the pad
    rows are zeroed by the forward, contribute zero rows to the weight gradient, and nothing else reads memory it did not write"""
    shape = (37, 3, 64, 64)
    pixels, demb = inputs(shape)
    model = build()
    emb, grads = run(model, pixels, demb)
    plain_new = model._new

    def poisoned(*sh, dtype=None):
        return plain_new(*sh, dtype=dtype).fill_(float("nan"))
    monkeypatch.setattr(model, "_new", poisoned)
    assert torch.isnan(model._new(4, 4)).all()
    emb_p, grads_p = run(model, pixels, demb)
    assert torch.equal(emb, emb_p) and not torch.isnan(emb_p).any()
    for n in grads:
        assert torch.equal(grads[n], grads_p[n]), n
        assert torch.isfinite(grads_p[n]).all(), n


def edit_weights(model):
    with torch.no_grad():
        for i, n in enumerate(WEIGHTS):
            model.arena.view(model.arena.master, n).mul_(1.0 + 0.125 * (i + 1))


def test_operand_cache_follows_the_weight_version(monkeypatch):
    shape = (2, 3, 32, 32)
    pixels, demb = inputs(shape)
    model = build()
    pe = model.patch_embedder
    counter = Counter(monkeypatch)
    run(model, pixels, demb)
    first, _ = counter.take()
    assert first["conv_weight_permute"] == 3 and first["conv_weight_permute_t"] == 2 and first["nchw_to_nhwc"] == 1
    v0 = model._wversion
    assert sorted(k[1] for k in pe._operands) == [v0] * 6          # three tap-major operands, two transposed ones, the projection's
    # a second forward + backward on unchanged weights permutes nothing
    run(model, pixels, demb)
    second, _ = counter.take()
    assert not {"conv_weight_permute", "conv_weight_permute_t", "nchw_to_nhwc"} & set(second), second
    # edited weights, work copy synced (a version bump): the next forward equals a fresh model's on the edited weights ...
    edit_weights(model)
    model.sync_work_params()
    assert model._wversion == v0 + 1
    emb, ctx = pe.forward(pixels)
    assert sorted(k[1] for k in pe._operands) == [v0 + 1] * 4      # ... the old version's entries are gone with the first rebuild, the transposed ones too
    fresh = build(state=model.state_dict())
    emb_f, grads_f = run(fresh, pixels, demb)
    assert torch.equal(emb, emb_f)
    emb2, grads = run(model, pixels, demb)
    assert torch.equal(emb2, emb_f)
    for n in grads:
        assert torch.equal(grads[n], grads_f[n]), n
    assert sorted(k[1] for k in pe._operands) == [v0 + 1] * 6


def test_operand_cache_in_a_captured_step_refills_fixed_buffers():
    """_graph_static (set by GraphedTrainStep): no version bump happens between replays, so every call refills the operand -- always in the
    same buffer, whose address the captured graph holds"""
    shape = (2, 3, 32, 32)
    pixels, demb = inputs(shape)
    model = build()
    pe = model.patch_embedder
    model._graph_static = True
    run(model, pixels, demb)
    assert sorted(k[1] for k in pe._operands) == ["static"] * 6
    ptrs = {k: v.data_ptr() for k, v in pe._operands.items()}
    edit_weights(model)
    model.arena.sync_work()                # the working copy follows the edit; the weight version does not move
    emb, grads = run(model, pixels, demb)
    assert {k: v.data_ptr() for k, v in pe._operands.items()} == ptrs
    fresh = build(state=model.state_dict())
    emb_f, grads_f = run(fresh, pixels, demb)
    assert torch.equal(emb, emb_f)
    for n in grads:
        assert torch.equal(grads[n], grads_f[n]), n
