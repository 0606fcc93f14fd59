"""What the GPU tests of generation, beam search and scoring (and of their kernels) share: the skip without a GPU, the upload helper, the small
fp32 model with its NumPy oracle, the small bf16 model with the ring path, and the prompt builder.  A plain module, imported like select_rule."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rule as S  # noqa: E402

DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(TD[dt])


def host(t):
    return t.detach().float().cpu().numpy().copy()      # bf16 -> float32 is exact


class Guarded:
    """a [rows, cols] tensor (row stride ld) in the middle of one allocation filled with the sentinel: margins of at least one row and 64
    elements before and after; ``off`` shifts the start by that many elements (an unaligned base)"""

    def __init__(self, rows, cols, dt, ld=None, fill=None, off=0):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.start = 64 * -(-max(self.ld, 64) // 64) + off
        self.buf = torch.full((2 * self.start + rows * self.ld,), S.SENT, device=DEV, dtype=TD[dt])
        self.t = self._body(self.buf)
        if fill is not None:
            self.t.copy_(dev(np.reshape(fill, (rows, cols)), dt))

    def _body(self, buf):
        return buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    @property
    def flat(self):
        assert self.ld == self.cols
        return self.buf[self.start:self.start + self.rows * self.cols]

    def np(self, flat=False):
        a = host(self.t)
        return a.reshape(-1) if flat else a

    def intact(self, name):
        chk = self.buf.clone()
        self._body(chk).fill_(S.SENT)
        bits = torch.int16 if chk.dtype == torch.bfloat16 else torch.int32
        bad = (chk.view(bits) != torch.full((1,), S.SENT, device=DEV, dtype=chk.dtype).view(bits)).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} guard elements changed, the first at offset {int(bad[0]) - self.start} from the output's start"


def _tdev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _model(name, dtype=torch.float32, seed=321):
    """(cfg, model, oracle) of the golden case ``name`` with seeded parameters"""
    from golden_util import case_cfg, make_params
    from oracle import db1_oracle as O
    from bdm_db1_amd import TransformerXL
    cfg = case_cfg(name)
    params = make_params(cfg, seed)
    model = TransformerXL(SimpleNamespace(**cfg), device=DEV, compute_dtype=dtype)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    params["pos_emb.inv_freq"] = model.pos_emb.inv_freq.cpu().numpy()
    model.eval()
    return cfg, model, O.OracleModel(O.OracleConfig(**cfg), params)


def _fp32_model():
    return _model("small_vqa")


def _bf16_model(seed=5, mem_len=40):
    from bdm_db1_amd import TransformerXL, synth
    cfg = synth.db1_config("tiny", n_embed=256, n_head=2, n_layer=2, n_position=128, mem_len=mem_len, fp16=True)
    torch.manual_seed(seed)
    model = TransformerXL(cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)
    model.eval()
    return cfg, model


def _prompt(rng, kind, G, vocab):
    """(model input, the prompt's fields) of G rows: nlp 6 tokens; ic 3 + 4 patches; vqa 3 + 4 patches + 5 question tokens"""
    from bdm_db1_amd.data import ICTaskInput, NLPTaskInput, VQATaskInput
    if kind == "nlp":
        ids = rng.integers(0, vocab, (G, 6))
        return NLPTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, text_seq=_tdev(ids), text_len=None), dict(text_seq=ids)
    prompt = rng.integers(0, vocab, (G, 3))
    img = rng.standard_normal((G, 3, 32, 32)).astype(np.float32)
    if kind == "ic":
        text = np.zeros((G, 0), np.int64)
        return ICTaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(prompt), img_seq=_tdev(img),
                           text_seq=_tdev(text)), dict(prompt_seq=prompt, img_seq=img, text_seq=text)
    q = rng.integers(1, vocab, (G, 5))
    return VQATaskInput(position_id=None, attention_mask=None, loss_mask=None, label=None, prompt_seq=_tdev(prompt), img_seq=_tdev(img),
                        text_seq=_tdev(q), img_id_seq=None, ques_id_seq=None, ques_len=None), dict(prompt_seq=prompt, img_seq=img, text_seq=q)
