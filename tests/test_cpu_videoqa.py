"""Video QA (TVQA / How2QA) without a GPU, against tests/golden/case_videoqa.npz - what the reference's own dataset, collate
and model gave (tests/golden/make_golden_videoqa.py):
  * hero_amd.collate.videoqa_item / video_qa_collate rebuild the reference batch, every key, dtype and value;
  * the float64 restatement of the two attention pools (tests/qa_reference.py), which the GPU tests judge the kernels by,
    reproduces the reference's pooled outputs and gradients;
  * HeroForVideoQA has the reference's state-dict keys."""
import json
import os

import numpy as np
import pytest
import torch

from tests import qa_reference as R
from tests.util import GOLDEN

Z = np.load(os.path.join(GOLDEN, "case_videoqa.npz"))
CASES = json.loads(str(Z["__cases__"]))


def ref_batch(case):
    out = {}
    for k in Z.files:
        if k.startswith(case + ".out."):
            a = Z[k]
            out[k[len(case) + 5:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return out


def rebuild(case):
    """The raw per-video inputs of a case -> hero_amd.collate.video_qa_collate."""
    from hero_amd import collate as C
    desc = json.loads(str(Z[case + ".desc"]))
    want = ref_batch(case)
    A = len(desc["videos"][0]["answers"])
    items = []
    for i, v in enumerate(desc["videos"]):
        feat = torch.from_numpy(Z["%s.feat.%s" % (case, v["vid"])])
        s2f = [(sid, list(fr)) for sid, fr in want["sub_idx2frame_idx"][i * A]]      # as compute_sub2frames left them
        video = C.video_item(feat, s2f, v["sub_tokens"], sep=desc["sep"])
        items.append(C.videoqa_item(video, v["question"], v["answers"], v["target"], v["ts"], sep=desc["sep"],
                                    frame_interval=desc["frame_interval"]))
    return C.video_qa_collate(items), want


@pytest.mark.parametrize("case", CASES)
def test_qa_collate_equals_reference_collate(case):
    got, want = rebuild(case)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.shape, w.shape, g.dtype, w.dtype)
            assert torch.equal(g, w), k
        else:
            assert json.loads(json.dumps(g)) == w, k
    assert set(got) - set(want) == {"lengths"}


def test_fixture_covers_missing_labels_masked_frames_and_both_answer_counts():
    a5, a4 = ref_batch("a5"), ref_batch("a4")
    assert a5["c_attn_masks"].shape[0] == 15 and a4["c_attn_masks"].shape[0] == 12          # 3 videos x 5 / 4 answers
    for b in (a5, a4):
        assert b["targets"].shape == (3, 1) and b["ts_targets"].shape == (3, 2)
        assert int((b["targets"] == -1).sum()) == 1 and int((b["targets"] != -1).sum()) == 2
        assert int((b["ts_targets"][:, 0] == -1).sum()) == 1 and bool((b["ts_targets"][b["ts_targets"][:, 0] == -1] == -1).all())
        assert int((b["c_attn_masks"] == 0).sum()) > 0
        assert len(set(b["qa_attn_masks"].sum(1).tolist())) > 2                              # QA lengths differ
    assert sorted(set(a5["c_attn_masks"].sum(1).tolist())) == [6, 9, 10]


def test_float64_restatement_reproduces_the_reference_head():
    """Forward and gradient of the head in isolation, as the reference computed them in fp32 on the model's own tensors.
    Bound: the reference side is fp32 arithmetic over D = 128 (dot products, sums over <= 10 frames / 5 answers): 1e-5 relative
    to each tensor's largest element is ~100 fp32 roundings; the parameter gradients relative to the size of their terms."""
    t = lambda k: torch.from_numpy(Z["a5.pool." + k])        # noqa: E731
    X, m = t("X"), t("mask")
    wq, ws = torch.from_numpy(Z["param.qa_pool.weight"]), torch.from_numpy(Z["param.st_ed_pool.weight"])
    f = R.forward(X, m, wq, ws)
    b = R.backward(X, m, wq, ws, t("dqa"), t("dse"))
    for name, got, want in (("qa_pooled", f["qa_pooled"], t("qa_pooled")), ("se_pooled", f["se_pooled"], t("se_pooled")),
                            ("dX", b["dX"], t("dX"))):
        err = float((got - want.double()).abs().max() / want.double().abs().max())
        assert err < 1e-5, (name, err)
    # dw: a sum of cancelling terms, judged against the size of what is summed (tests/qa_reference.py `dw_*_scale`)
    for name in ("dw_qa", "dw_se"):
        err = float(((b[name] - t(name).reshape(-1).double()).abs() / b[name + "_scale"]).max())
        print(name, "error / scale %.3e" % err, " |dw| / scale %.3e" % float((b[name].abs() / b[name + "_scale"]).max()))
        assert err < 1e-5, (name, err)
    # a masked frame spreads its weight evenly over the answers; the attention tables are not uniform where frames are valid
    masked = m == 0
    assert bool(masked.any()) and float((f["att_se"][masked] - 1.0 / X.shape[1]).abs().max()) < 1e-12
    assert float((f["att_se"][~masked] - 1.0 / X.shape[1]).abs().max()) > 0.05
    assert float((f["att_qa"] * m.double()).sum(2).sub(1).abs().max()) < 1e-9


def test_restatement_gradient_is_the_derivative_of_its_forward():
    """Central differences in float64 on a small case with a masked tail (A = 3 is no power of two)."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64)
    m = torch.ones(2, 3, 5, dtype=torch.float64)
    m[1, :, 3:] = 0
    wq, ws = torch.randn(8, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    dqa, dse = torch.randn(2, 3, 8, generator=g, dtype=torch.float64), torch.randn(2, 5, 8, generator=g, dtype=torch.float64)

    def loss(X_, wq_, ws_):
        f = R.forward(X_, m, wq_, ws_)
        return float((f["qa_pooled"] * dqa).sum() + (f["se_pooled"] * dse).sum())
    b = R.backward(X, m, wq, ws, dqa, dse)
    eps = 1e-6
    for idx in [(0, 0, 0, 0), (1, 2, 1, 7), (1, 1, 4, 3), (0, 2, 3, 5)]:
        d = torch.zeros_like(X)
        d[idx] = eps
        num = (loss(X + d, wq, ws) - loss(X - d, wq, ws)) / (2 * eps)
        assert abs(num - float(b["dX"][idx])) < 1e-6 * max(1.0, abs(num)), (idx, num, float(b["dX"][idx]))
    for k in (0, 5):
        d = torch.zeros(8, dtype=torch.float64)
        d[k] = eps
        assert abs((loss(X, wq + d, ws) - loss(X, wq - d, ws)) / (2 * eps) - float(b["dw_qa"][k])) < 1e-6
        assert abs((loss(X, wq, ws + d) - loss(X, wq, ws - d)) / (2 * eps) - float(b["dw_se"][k])) < 1e-6


def test_state_dict_keys_equal_the_reference():
    from hero_amd.model import HeroForVideoQA
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    model = HeroForVideoQA.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), {}, vfeat_dim=int(z["__vfeat__"]),
                                           max_frm_seq_len=int(z["__max_frm__"]))
    assert sorted(model.state_dict().keys()) == json.loads(str(Z["state_keys"]))
    assert torch.equal(model.st_ed_pool.weight, model.qa_pool.weight)                  # initialised as a copy
    assert model.st_ed_pool.weight is not model.qa_pool.weight


def test_qa_pool_on_cpu_tensors_raises():
    from hero_amd.qa import QaPoolFn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QaPoolFn.apply(torch.zeros(4, 6, 8), torch.ones(4, 5), torch.zeros(1, 8), torch.zeros(1, 8), 2, 5)
