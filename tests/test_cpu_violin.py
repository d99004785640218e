"""VIOLIN without a GPU, against tests/golden/case_violin.npz - what the reference's own datasets, collates and model gave
(tests/golden/make_golden_violin.py):
  * hero_amd.collate.violin_item / violin_collate / violin_eval_collate rebuild the reference batches, every key, dtype and value;
  * the float64 restatement of the frame pool and the classifier tail (tests/violin_reference.py), which the GPU tests judge
    the kernels by, reproduces the reference's pooled output, gradients and loss;
  * HeroForViolin has the reference's state-dict keys; ViolinMeter.update_host gives the reference's validation figures;
  * hero_amd.step.VIOLIN_OPTS holds the recipe's numbers."""
import json
import os

import numpy as np
import pytest
import torch

from tests import violin_reference as R
from tests.util import GOLDEN

Z = np.load(os.path.join(GOLDEN, "case_violin.npz"))
DESC = json.loads(str(Z["desc"]))


def ref_batch(prefix):
    out = {}
    for k in Z.files:
        if k.startswith(prefix + "."):
            a = Z[k]
            out[k[len(prefix) + 1:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return out


def _video(C, v, s2f):
    feat = torch.from_numpy(Z["feat." + v["vid"]])
    return C.video_item(feat, [(sid, list(fr)) for sid, fr in s2f], v["sub_tokens"], sep=DESC["sep"], sub_ctx_len=DESC["sub_ctx_len"])


def rebuild_train():
    """Every item is the sampled statement and its paired one (ViolinDataset.getids, sampled by statement)."""
    from hero_amd import collate as C
    want = ref_batch("out")
    items = []
    for i, v in enumerate(DESC["videos"]):
        order = [v["sampled"], 1 - v["sampled"]]
        items.append(C.violin_item(_video(C, v, want["sub_idx2frame_idx"][2 * i]), [v["statements"][j] for j in order],
                                   [v["targets"][j] for j in order], sep=DESC["sep"], vid=v["vid"]))
    return C.violin_collate(items), want


def rebuild_eval():
    """One statement per item, all six (ViolinEvalDataset)."""
    from hero_amd import collate as C
    want = ref_batch("eval")
    items = []
    for i, v in enumerate(DESC["videos"]):
        for j in (0, 1):
            item = C.violin_item(_video(C, v, want["sub_idx2frame_idx"][2 * i + j]), [v["statements"][j]], [v["targets"][j]],
                                 sep=DESC["sep"], vid=v["vid"])
            items.append((["s%02d-%d" % (i, j)], item))
    return C.violin_eval_collate(items), want


@pytest.mark.parametrize("rebuild", [rebuild_train, rebuild_eval], ids=["train", "eval"])
def test_violin_collate_equals_reference_collate(rebuild):
    got, want = rebuild()
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.shape, w.shape, g.dtype, w.dtype)
            assert torch.equal(g, w), k
        else:
            assert json.loads(json.dumps(g)) == w, k
    assert set(got) - set(want) == {"lengths"}


def test_fixture_covers_masked_frames_both_labels_and_differing_statements():
    b, e = ref_batch("out"), ref_batch("eval")
    for x in (b, e):
        assert x["c_attn_masks"].shape[0] == 6 and x["targets"].shape == (6, 1) and x["targets"].dtype == torch.int64
        assert sorted(set(x["targets"].reshape(-1).tolist())) == [0, 1]
        assert int((x["c_attn_masks"] == 0).sum()) > 0
        assert len(set(x["q_attn_masks"].sum(1).tolist())) > 2                               # statement lengths differ
        assert sorted(set(x["c_attn_masks"].sum(1).tolist())) == [6, 9, 10]
    assert e["qids"] == ["s%02d-%d" % (v, i) for v in range(3) for i in (0, 1)]
    assert DESC["sub_ctx_len"] == 2
    assert float(np.abs(Z["logits"]).max()) < 8 and 0.0 < float(Z["val.acc"]) < 1.0


def test_float64_restatement_reproduces_the_reference_pool():
    """Forward and gradient of the pool in isolation, as the reference computed them in fp32 on the model's own tensors.
    Bound (that of tests/test_cpu_videoqa.py): the reference side is fp32 arithmetic over D = 128 and <= 10 frames: 1e-5 relative
    to each tensor's largest element is ~100 fp32 roundings; the parameter gradient relative to the size of its terms."""
    t = lambda k: torch.from_numpy(Z["pool." + k])        # noqa: E731
    X, m, w = t("X"), t("mask"), torch.from_numpy(Z["param.violin_pool.weight"])
    f = R.pool_forward(X, m, w)
    b = R.pool_backward(X, m, w, t("dpooled"))
    for name, got, want in (("pooled", f["pooled"], t("pooled")), ("dX", b["dX"], t("dX"))):
        err = float((got - want.double()).abs().max() / want.double().abs().max())
        assert err < 1e-5, (name, err)
    err = float(((b["dw"] - t("dw").reshape(-1).double()).abs() / b["dw_scale"]).max())
    print("dw error / scale %.3e" % err, " |dw| / scale %.3e" % float((b["dw"].abs() / b["dw_scale"]).max()))
    assert err < 1e-5, err
    masked = m == 0
    assert bool(masked.any()) and float(f["att"][masked].abs().max()) == 0.0
    n_valid = m.sum(1, keepdim=True).expand_as(m).double()
    assert float((f["att"] - 1.0 / n_valid)[~masked].abs().max()) > 0.05
    assert float(f["att"].sum(1).sub(1).abs().max()) < 1e-12


def test_float64_restatement_reproduces_the_reference_loss():
    """The capped stable loss from the fixture's LayerNorm output: inside |z| < 8 it is binary_cross_entropy(sigmoid(z), t).
    Bound: fp32 arithmetic over K = 256 on the reference side, 1e-5 as above."""
    w = torch.from_numpy(Z["param.violin_pred_head.linear_2.weight"])
    b = torch.from_numpy(Z["param.violin_pred_head.linear_2.bias"])
    f = R.head_forward(torch.from_numpy(Z["h"]), w, b, torch.from_numpy(Z["out.targets"]))
    want = torch.from_numpy(Z["logits"]).reshape(-1).double()
    assert float((f["logits"] - want).abs().max() / want.abs().max()) < 1e-5
    assert abs(float(f["loss"]) - float(Z["violin_loss"])) < 1e-5 * float(Z["violin_loss"])
    g = R.head_backward(torch.from_numpy(Z["h"]), w, b, torch.from_numpy(Z["out.targets"]))
    gw = torch.from_numpy(Z["grad.violin_pred_head.linear_2.weight"]).reshape(-1).double()
    assert float(((g["dw"] - gw).abs() / g["dw_scale"]).max()) < 1e-5
    assert abs(float(g["db"]) - float(Z["grad.violin_pred_head.linear_2.bias"].reshape(-1)[0])) < 1e-5 * float(g["db_scale"])


def test_restatement_gradients_are_the_derivatives_of_their_forwards():
    """Central differences in float64 on a small case with a masked tail."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(3, 5, 8, generator=g, dtype=torch.float64)
    m = torch.ones(3, 5, dtype=torch.float64)
    m[1, 3:] = 0
    w, dp = torch.randn(8, generator=g, dtype=torch.float64), torch.randn(3, 8, generator=g, dtype=torch.float64)
    loss = lambda X_, w_: float((R.pool_forward(X_, m, w_)["pooled"] * dp).sum())      # noqa: E731
    b = R.pool_backward(X, m, w, dp)
    eps = 1e-6
    for idx in [(0, 0, 0), (1, 1, 7), (1, 4, 3), (2, 3, 5)]:
        d = torch.zeros_like(X)
        d[idx] = eps
        num = (loss(X + d, w) - loss(X - d, w)) / (2 * eps)
        assert abs(num - float(b["dX"][idx])) < 1e-6 * max(1.0, abs(num)), (idx, num, float(b["dX"][idx]))
    for k in (0, 5):
        d = torch.zeros(8, dtype=torch.float64)
        d[k] = eps
        assert abs((loss(X, w + d) - loss(X, w - d)) / (2 * eps) - float(b["dw"][k])) < 1e-6
    h = torch.randn(5, 8, generator=g, dtype=torch.float64)
    w2, b2 = torch.randn(8, generator=g, dtype=torch.float64), torch.tensor([0.3], dtype=torch.float64)
    t = torch.tensor([1, 0, 0, 1, 1])
    hb = R.head_backward(h, w2, b2, t, dloss=0.7)
    hl = lambda h_, w_, b_: 0.7 * float(R.head_forward(h_, w_, b_, t)["loss"])         # noqa: E731
    for idx in [(0, 0), (3, 7), (4, 2)]:
        d = torch.zeros_like(h)
        d[idx] = eps
        assert abs((hl(h + d, w2, b2) - hl(h - d, w2, b2)) / (2 * eps) - float(hb["dh"][idx])) < 1e-6
    d = torch.zeros(8, dtype=torch.float64)
    d[4] = eps
    assert abs((hl(h, w2 + d, b2) - hl(h, w2 - d, b2)) / (2 * eps) - float(hb["dw"][4])) < 1e-6
    assert abs((hl(h, w2, b2 + eps) - hl(h, w2, b2 - eps)) / (2 * eps) - float(hb["db"])) < 1e-6


def test_restatement_loss_is_capped_and_its_gradient_is_not():
    h = torch.tensor([[200.0, 0, 0, 0], [-200.0, 0, 0, 0], [30.0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
    w, b = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    t = torch.tensor([0, 1, 0, 0])
    f, g = R.head_forward(h, w, b, t), R.head_backward(h, w, b, t)
    assert f["terms"].tolist()[:3] == [100.0, 100.0, 30.0 + float(torch.log1p(torch.exp(torch.tensor(-30.0, dtype=torch.float64))))]
    assert abs(float(f["terms"][3]) - float(torch.log(torch.tensor(2.0, dtype=torch.float64)))) < 1e-15
    assert float(f["right"]) == 1.0                                  # only the z == 0, t == 0 row: z == 0 predicts 0
    assert torch.allclose(g["dz"] * 4, torch.tensor([1.0, -1.0, 1.0, 0.5], dtype=torch.float64), atol=1e-12)


def test_state_dict_keys_equal_the_reference():
    from hero_amd.model import HeroForViolin
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    model = HeroForViolin.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), {}, vfeat_dim=int(z["__vfeat__"]),
                                          max_frm_seq_len=int(z["__max_frm__"]))
    assert sorted(model.state_dict().keys()) == json.loads(str(Z["state_keys"]))
    assert tuple(model.violin_pool.weight.shape) == (1, 128) and model.violin_pool.bias is None
    assert tuple(model.violin_pred_head.linear_2.weight.shape) == (1, 256)


def test_meter_host_path_gives_the_reference_validation_figures():
    from hero_amd.violin import ViolinMeter
    z, t = torch.from_numpy(Z["val.logits"]), torch.from_numpy(Z["eval.targets"])
    meter = ViolinMeter(device="cpu")
    meter.update_host(z[:4], t[:4])                                  # two batches: the sums accumulate
    meter.update_host(z[4:], t[4:])
    got = meter.compute()
    assert got["acc"] == float(Z["val.acc"])
    assert abs(got["loss"] - float(Z["val.loss"])) < 1e-6 * float(Z["val.loss"])
    results = {q: int(a) for q, a in zip(json.loads(str(Z["eval.qids"])), (z.reshape(-1) > 0).long().tolist())}
    assert results == json.loads(str(Z["val.results"]))


def test_violin_opts_are_the_recipe():
    from hero_amd import step
    o = step.VIOLIN_OPTS
    assert (o["learning_rate"], o["lr_mul"], o["warmup_steps"], o["num_train_steps"]) == (3e-5, 8.0, 600, 6000)
    assert (o["train_batch_size"], o["gradient_accumulation_steps"]) == (4, 2)
    assert (o["weight_decay"], o["grad_norm"], o["dropout"], o["betas"], o["optim"]) == (0.01, 1.0, 0.1, [0.9, 0.98], "adamw")
    assert "violin" in step.HEAD_LR_TASKS and step.QA_TASKS == ("tvqa", "how2qa")


def test_head_functions_on_cpu_tensors_raise():
    from hero_amd.violin import BceHeadFn, FramePoolFn, head_in_envelope, pool_in_envelope
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FramePoolFn.apply(torch.zeros(4, 6, 8), torch.ones(4, 5), torch.zeros(1, 8), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BceHeadFn.apply(torch.zeros(4, 8), torch.zeros(1, 8), torch.zeros(1), torch.zeros(4, dtype=torch.long))
    assert pool_in_envelope(256, 512, 1024) and not pool_in_envelope(257, 300, 64) and not pool_in_envelope(4, 513, 64)
    assert not pool_in_envelope(4, 3, 64) and not pool_in_envelope(4, 4, 6) and not pool_in_envelope(4, 4, 1028)
    assert head_in_envelope(1, 4) and head_in_envelope(67, 2048) and not head_in_envelope(0, 8) and not head_in_envelope(2, 2052)
    assert not head_in_envelope(2, 6)
