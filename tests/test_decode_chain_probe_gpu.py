"""db1_decode_chain and db1_decode_chain_w8 (csrc/decode_chain.hip) against the rule of tests/decode_linear_rule.py at the one geometry the kernel
has (d 2048, dff 4096, H 16): one-live-unit attention partials, w_o / w2 / w_qkv from the sparse +-1 pattern, w1 from the GEGLU design.
Every stage is checked per element from the STORED input of that stage: the scratch row y_o bit for bit, h1_out under the LayerNorm bound
from the stored y_o, the scratch row act from h1_out, the scratch row f from act, x_next from (h1_out, f), qkv_next from x_next.  Both forms
of the launch run on alternating slots; their scratch rows are bit-equal, so h1_out of the last-layer form stands for the other form's
unstored row.  After every launch all tags equal slot + 1, the error flag is 0, and a second launch of a form gives the same bits.

Template instantiations of dc_launch and the case that reaches each:
  decode_chain_kernel<9, false>   bf16, nunit 1 and 9        decode_chain_kernel<12, false>   bf16, nunit 10 and 12
  decode_chain_kernel<9, true>    w8, nunit 1 and 9          decode_chain_kernel<12, true>    w8, nunit 10 and 12
(the probe's weights are 0, +-1/4, +-1/2, +-1: their e4m3 form with power-of-two block scales is lossless -- asserted --, so the fp8 launch
has the same expectations, stage by stage, and is not judged by its equality with the bf16 launch alone)"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_linear_rule as R  # noqa: E402
import stream_rule as S  # noqa: E402
from gpu_common import DEV, _need_gpu, dev, host  # noqa: E402,F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
D, DFF, H = R.CHAIN_D, R.CHAIN_DFF, R.CHAIN_H
_ratios = {}


@pytest.fixture(scope="module")
def chain():
    from bdm_db1_amd import ops
    if not ops.decode_chain_supported(D, DFF, H, 128, 128):
        pytest.skip("db1_decode_chain needs 256 CUs")
    w = R.chain_weights()
    t = {k: dev(v, "bf16") for k, v in w.items()}
    t8 = {k: ops.w8_quantize(t[k]) for k in ("w_o", "w1", "w2", "w_qkv")}
    for k, buf in t8.items():                                # the fp8 form of the probe's weights is lossless
        assert torch.equal(ops.w8_unpack(buf, *t[k].shape)[0], t[k].cpu()), k
    scratch, word = ops.new_chain_scratch(torch.device(DEV))
    yield dict(ops=ops, w=w, t=t, t8=t8, scratch=scratch, word=word)
    if _ratios:
        print("\nlargest observed ratio per chain stage: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_ratios.items())))


def _rows(chain, slot):
    ops = chain["ops"]
    off = int(ops.lib.load().db1_decode_chain_error_offset())
    w = chain["scratch"][:(2 * D + DFF) * 4].view(torch.int32)
    assert int(chain["scratch"][off:off + 4].view(torch.int32).item()) == 0, "a hand-off poll ran into its limit"
    tags = (w & 0xffff).unique().tolist()
    assert tags == [slot + 1], f"tags {tags[:4]} after the launch on slot {slot}"
    val = (w >> 16).to(torch.int16).view(torch.bfloat16).float().cpu().numpy()
    return dict(y_o=val[None, :D].copy(), act=val[None, D:D + DFF].copy(), f=val[None, D + DFF:].copy())


@pytest.mark.parametrize("form", ["bf16", "w8"])
@pytest.mark.parametrize("nunit,others", [(1, "dead"), (9, "dead"), (9, "low"), (10, "dead"), (10, "low"), (12, "low")])
def test_chain_stages(chain, nunit, others, form):
    ops, t = chain["ops"], chain["t"]
    case, part_h = R.chain_part(nunit, others)
    part = torch.from_numpy(part_h).to(DEV)
    wt = chain["t8"] if form == "w8" else t
    fn = ops.decode_chain_w8 if form == "w8" else ops.decode_chain
    new = lambda n: torch.full((1, n), NAN, device=DEV, dtype=torch.bfloat16)
    runs = []
    with ops.chain_scratch_scope(chain["scratch"], chain["word"]):
        for slot in (2, 3, 4, 5):                           # with the next layer's projection / last layer, alternating
            last = slot % 2 == 1
            h1o, fo, xn, qn = new(D), new(D), new(D), new(3 * D)
            fn(part, nunit * 128, H, t["x_res"], wt["w_o"], wt["w1"], t["b1"], wt["w2"], t["b2"], None if last else wt["w_qkv"], t["g1"], t["be1"], t["g2"], t["be2"],
               R.ALPHA, R.EPS, h1o if last else None, fo if last else None, None if last else xn, None if last else qn, slot, w_o_next=wt["w_o"])
            torch.cuda.synchronize()
            got = _rows(chain, slot)
            got.update(dict(h1=host(h1o), f_out=host(fo)) if last else dict(x_next=host(xn), qkv_next=host(qn)))
            runs.append(got)
    bits = lambda a: a.view(np.uint32)
    for a, b in ((runs[0], runs[2]), (runs[1], runs[3])):    # a second launch of a form: the same bits
        assert a.keys() == b.keys() and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
    for k in ("y_o", "act", "f"):                             # between the forms
        assert np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k
    assert np.array_equal(bits(runs[1]["f_out"]), bits(runs[1]["f"]))
    got = dict(runs[0], h1=runs[1]["h1"])
    assert all(np.isfinite(v).all() for v in got.values())
    worst = {}
    for name, (ref, bnd) in R.chain_expect(chain["w"], case, part_h, got).items():
        q = S.check(got[name], ref, bnd, f"chain {form} nunit {nunit} {others}: {name}")
        if bnd.any():
            hu = S.half_ulp(ref, "bf16")                     # next to it, the share of the fp32 allowance in use (the error beyond half an output ulp)
            with np.errstate(invalid="ignore", divide="ignore"):
                sh = max(0.0, float(np.where(bnd > hu, (np.abs(got[name] - ref) - hu) / (bnd - hu), 0.0).max()))
            worst[name], worst[name + " fp32"] = q, sh
            _ratios[name], _ratios[name + " fp32"] = max(_ratios.get(name, 0.0), q), max(_ratios.get(name + " fp32", 0.0), sh)
    print(f"chain-{form}-nunit{nunit}-{others}: max ratio = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
