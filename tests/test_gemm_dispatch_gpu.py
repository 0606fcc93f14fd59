"""Every branch of the GEMM dispatcher (gemm_plan, bdm_db1_amd/csrc/gemm.hip) executed: one shape per branch (the list of
tools/gemm_dispatch_table.py, each the smallest that reaches its branch), the kernel the plan names and the product against the strided
fp32-MFMA kernel on the same bf16 operands; and the structural-zero hint, which now reaches the plan through the shape."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

torch = pytest.importorskip("torch")
import gemm_dispatch_table as gdt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _operands(layout, M, N, K, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    r = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    if layout == "nt":
        return r(M, K), r(N, K).t()
    if layout == "nn":
        return r(M, K), r(K, N)
    return r(K, M).t(), r(K, N)


def _gemm(ops, lib, a, b, out, bias, beta, offer):
    """ops.gemm with the workspace the case offers ("none": the call is made without one)"""
    if offer != "none":
        return ops.gemm(a, b, out, bias=bias, beta=beta)
    M, K = a.shape
    N = b.shape[1]
    lib.call("db1_gemm_strided", ops.P(a), ops.P(b), ops.P(out), ops.P(bias), M, N, K, ops.dt_code(a), ops.dt_code(b), ops.dt_code(out),
             ops.dt_code(bias) if bias is not None else 0, a.stride(0), a.stride(1), b.stride(0), b.stride(1), out.stride(0), out.stride(1),
             1, 1, 0, 0, 0, 0, 0, 0, 1.0, beta, None, 0, ops.stream())


@pytest.mark.parametrize("case", gdt.BRANCH_CASES, ids=lambda c: "%dx%dx%d-%s-%s-%s" % (c[0] + (c[1], "%s%d" % c[4] if c[4] else "default", c[5])))
def test_every_plan_branch_runs_the_kernel_it_names(case):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops, lib
    (M, N, K), layout, _, _, knob, offer, want_choice = case
    try:
        if knob:
            lib.set_knob(*knob)
        ops._ws_query_cache.clear()          # (the workspace query depends on the knobs)
        a, b = _operands(layout, M, N, K, 11)
        for odt, beta, with_bias in ((torch.bfloat16, 0.0, True), (torch.float32, 1.0, False)):
            bias = (torch.randn(N, device=DEV) * 0.3).to(torch.bfloat16) if with_bias else None
            c0 = (torch.randn(M, N, device=DEV) * 0.2).to(odt)
            got, want = c0.clone(), c0
            choice = ops.gemm_kernel_choice(a, b, got, beta=beta, ws_bytes={"any": -1, "none": 0}[offer])
            assert choice == want_choice, (case, odt, choice)
            _gemm(ops, lib, a, b, got, bias, beta, offer)
            ops.gemm_force_generic(True)
            ops.gemm(a, b, want, bias=bias, beta=beta)
            ops.gemm_force_generic(False)
            scale = float(want.abs().max())
            err = float((got - want).abs().max()) / scale
            print(f"{case[:6]} {odt}: {choice} err {err:.2e}")
            assert err <= (6e-3 if odt == torch.bfloat16 else 2e-5), (case, odt, beta, err)
            del got, want, c0
    finally:
        ops.gemm_force_generic(False)
        lib.load().db1_test_clear_knobs()
        ops._ws_query_cache.clear()


def test_structural_zero_hint_through_the_plan_is_bit_identical_to_the_unhinted_call():
    """hint 2 (A[m, k] == 0 for (k mod period) < m) on one column of tiles -- the per-head dR contraction, 12 tiles x 8 slices with and
    without the hint: the hinted call skips k-tiles of exact zeros, so every partial sum and the result are the same bits"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bdm_db1_amd import ops
    H, B, L, D = 3, 8, 1024, 128
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    i = torch.arange(L, device=DEV)[:, None]
    dd = torch.arange(L, device=DEV)[None, :]
    dT = torch.randn(H, B, L, L, device=DEV, generator=g).to(torch.bfloat16).masked_fill_(dd > i, 0)
    qv = torch.randn(B, L, H, D, device=DEV, generator=g).to(torch.bfloat16)
    outs = []
    for tri in ((0, 0), (2, L)):
        dR = torch.full((L, H * D), float("nan"), device=DEV, dtype=torch.float32)
        ops.gemm_batched(dT.view(H, B * L, L).transpose(1, 2).unsqueeze(1), qv.view(B * L, H, D).permute(1, 0, 2).unsqueeze(1),
                         dR.view(L, H, D).permute(1, 0, 2).unsqueeze(1), tri=tri)
        outs.append(dR)
    ref = torch.einsum("hbik,bihd->khd", dT.double(), qv.double()).reshape(L, H * D)
    assert torch.isfinite(outs[0]).all()
    assert float((outs[0] - ref).abs().max() / ref.abs().max()) < 2e-5
    assert torch.equal(outs[0], outs[1]), "the hinted call differs from the unhinted one"
