"""Whole training micro-steps under both fills (tests/uninit.py): for every task model with a tiny golden batch, one eager
forward + backward - fp32 and bf16, packed and padded cross-modal encoder, dropout on and seeded identically - must give the
same bits for the losses and for EVERY parameter gradient whether the buffers the library allocates uninitialised held 0.0 or
NaN beforehand; one greedy TVC decode and one retrieval search must give identical outputs.  Needs a real MI355X (-m gpu)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import hero_oracle as O
from tests import uninit
from tests.test_oracle_golden import _task_batches, _vsm_batch
from tests.util import GOLDEN, load_tiny, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
P_DROP = 0.1


def _pretrain_batch(which):
    batch, _ = O.load_npz_case(os.path.join(GOLDEN, "case_pretrain.npz"))
    if which == "vsm":
        return _vsm_batch(batch)                                     # two queries per video
    mlm, mfm, fom = _task_batches(batch)
    return {"mlm": mlm, "mfm": mfm, "fom": fom}[which]


def _tiny():
    model, _, _ = load_tiny("cuda")
    return model


def _vsm(model, b):
    return sum(l.sum() for l in model(b, task="tvr", compute_loss=True))


def _videoqa(model, b):
    qa_loss, temporal_loss = model(b, task="tvqa", compute_loss=True)
    return qa_loss + 0.4 * temporal_loss


def _encoder_task(task):
    def step(model, b):
        if task.startswith("mf"):
            b = dict(b, c_v_feats=b["c_v_feats"].clone())            # forward_mfm writes the mask embedding into it
        return model.v_encoder(b, task, compute_loss=True).mean()
    return step


def _models():
    from tests import test_gpu_tvc as TT
    from tests import test_gpu_videoqa as TQ
    from tests import test_gpu_violin as TV
    return {
        "vsm": (_tiny, lambda: to_dev(_pretrain_batch("vsm"), "cuda"), _vsm),
        "videoqa": (TQ.load_model, lambda: TQ.load_batch("a5"), _videoqa),
        "violin": (TV.load_model, TV.load_batch, lambda m, b: m(b, task="violin", compute_loss=True)),
        "tvc": (TT.load_model, TT.load_batch, lambda m, b: m.caption_loss(b)),
        "mlm": (_tiny, lambda: to_dev(_pretrain_batch("mlm"), "cuda"), _encoder_task("mlm")),
        "mfm-nce": (_tiny, lambda: to_dev(_pretrain_batch("mfm"), "cuda"), _encoder_task("mfm-nce")),
        "mffr": (_tiny, lambda: to_dev(_pretrain_batch("mfm"), "cuda"), _encoder_task("mffr")),
        "fom": (_tiny, lambda: to_dev(_pretrain_batch("fom"), "cuda"), _encoder_task("fom")),
    }


@pytest.fixture()
def compute_dtype(request):
    import hero_amd
    from hero_amd import functional as HF
    old = hero_amd.compute_dtype()
    hero_amd.set_compute_dtype(request.param)
    HF.set_grad_sink(None)
    yield request.param
    hero_amd.set_compute_dtype(old)
    HF.clear_weight_cache()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("compute_dtype", DTYPES, ids=IDS, indirect=True)
@pytest.mark.parametrize("task", ["vsm", "videoqa", "violin", "tvc", "mlm", "mfm-nce", "mffr", "fom"])
def test_training_micro_step(task, compute_dtype, packed, monkeypatch):
    """Weight gradients run with ONE split of their reduction.  From 256 rows on (fp32; 512 in bf16) functional._split_for cuts
    the reduction across workgroups that merge their partial sums with fp32 atomics, in an order that differs from run to run:
    the last bit of those gradients is not reproducible under ANY fill, and bit-identity between two runs presupposes that each
    is reproducible.  Measured on an MI355X, fp32 video-QA batch (reductions of 420 and 791 rows, splits 3 and 6), three runs
    under the SAME fill: 14-15 of the 81 gradients - nn.Linear weights only - differ between two runs in their last bit, in
    other elements every time; with one split, 0 of 81.  One split runs the same kernels; the split launch itself - output from
    torch.empty, pre-scale, atomic merge - runs under the fills in test_gpu_uninit_kernels.py::test_wgrad_with_a_split_reduction,
    on integer operands whose sums are exact in any order."""
    from hero_amd import functional as HF
    monkeypatch.setattr(HF, "_split_for", lambda n_out, n_in, rows, bk: 1)
    from hero_amd.model.layers import BertEncoder
    from hero_amd.utils.misc import set_dropout
    load_model, load_batch, step = _models()[task]

    def build():
        HF.set_grad_sink(None)
        model = load_model()
        model.train()
        set_dropout(model, P_DROP)
        return model, load_batch()

    def run(inputs):
        model, b = inputs
        torch.manual_seed(11)
        HF.manual_seed(11, "cuda")
        loss = step(model, b)
        loss.backward()
        out = {"loss": loss.detach()}
        n = 0
        for name, prm in model.named_parameters():
            if prm.grad is not None:
                out["grad." + name] = prm.grad
                n += 1
        assert n >= 5, n
        return out

    BertEncoder.allow_packing = packed
    try:
        uninit.assert_fill_independent(build, run)
    finally:
        BertEncoder.allow_packing = True


@pytest.mark.parametrize("compute_dtype", DTYPES, ids=IDS, indirect=True)
def test_greedy_tvc_decode(compute_dtype):
    from hero_amd.model import TvcGenerator
    from tests import test_gpu_tvc as TT

    def build():
        model = TT.load_model(True)
        model.eval()
        return model, TT.load_batch()

    def run(inputs):
        model, b = inputs
        ids = TvcGenerator(model, 8, TT.DESC["bos"], int(TT.Z["greedy_eos"])).greedy_decode(b)
        width = max(len(r) for r in ids)
        return {"ids": torch.tensor([list(r) + [-1] * (width - len(r)) for r in ids]), "lengths": torch.tensor([len(r) for r in ids])}

    out = uninit.assert_fill_independent(build, run)
    if compute_dtype == torch.float32:
        want = json.loads(str(TT.Z["greedy"]))
        assert [r[:n].tolist() for r, n in zip(out["ids"], out["lengths"].tolist())] == want


@pytest.mark.parametrize("compute_dtype", DTYPES, ids=IDS, indirect=True)
def test_retrieval_search(compute_dtype):
    import hero_amd
    from tests import test_gpu_retrieval as TR
    case = TR.golden()
    alpha, k, min_l, max_l, top_n, max_clip_len, _ = (int(x) for x in case["cfg"])

    def build():
        model = _tiny()
        model.eval()
        q = [torch.from_numpy(case["in.query_" + n]).cuda() for n in ("input_ids", "pos_ids", "attn_masks")]
        return model, TR.golden_batches(case), q, torch.from_numpy(case["in.gt_vidx"]).cuda()

    def run(inputs):
        model, batches, q, gt = inputs
        index = hero_amd.encode_corpus(model, batches, max_clip_len)
        out = index.search(model, *q, max_before_nms=top_n, gt_vidx=gt, q2c_alpha=alpha, max_vcmr_video=k, min_pred_l=min_l, max_pred_l=max_l)
        res = {"search." + name: v for name, v in out.items() if torch.is_tensor(v)}
        assert len(res) >= 5, sorted(out)
        res["corpus"] = index.frame_embeddings
        return res

    out = uninit.assert_fill_independent(build, run)
    if compute_dtype == torch.float32:
        assert np.array_equal(out["search.vr_indices"].cpu().numpy(), case["vr_indices"])
