"""The pre-training batch boundary against the reference's OWN data code.

tests/golden/case_pretrain_collate.npz was produced by importing the reference's VideoMlmDataset / mlm_collate, MfmDataset /
mfm_collate, FomDataset / fom_collate and VsmDataset / vsm_collate (tests/golden/make_golden_pretrain_collate.py).  After
random.seed(the recorded seed), hero_amd.collate's host half must rebuild every tensor and list of the four batches bit for bit
from the raw description: the draws come from Python's `random` in the reference's order."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.util import GOLDEN

Z = np.load(os.path.join(GOLDEN, "case_pretrain_collate.npz"))
CASES = json.loads(str(Z["__cases__"]))
TASKS = ("mlm", "mfm", "fom", "vsm")


def ref_batch(case, task):
    pre, out = "%s.%s." % (case, task), {}
    for k in Z.files:
        if k.startswith(pre):
            a = Z[k]
            out[k[len(pre):]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return out


def rebuild(case, task):
    from hero_amd import collate as C
    d = json.loads(str(Z[case + ".desc"]))
    random.seed(d["py_seed"])
    items = []
    for v in d["videos"]:
        feat = torch.from_numpy(Z["%s.feat.%s" % (case, v["vid"])])
        s2f = [(sid, list(fr)) for sid, fr in v["sub2frames"]]
        if task == "mlm":
            items.append(C.mlm_item(feat, s2f, v["sub_tokens"], d["mask"], d["v_range"], cls_=d["cls"], mask_prob=d["mask_prob"],
                                    sub_ctx_len=d["sub_ctx_len"], max_txt_len=d["max_txt_len"]))
        elif task == "vsm":
            items.append(C.vsm_item(feat, s2f, v["sub_tokens"], v["vid"], d["query_per_video"], sep=d["sep"], cls_=d["cls"],
                                    sub_ctx_len=d["sub_ctx_len"], max_txt_len=d["max_txt_len"]))
        else:
            video = C.video_item(feat, s2f, v["sub_tokens"], sep=d["sep"], sub_ctx_len=d["sub_ctx_len"])
            items.append(C.mfm_item(video, d["mask_prob"]) if task == "mfm" else C.fom_item(video, d["reorder_p"]))
    return {"mlm": C.mlm_collate, "mfm": C.mfm_collate, "fom": C.fom_collate, "vsm": C.vsm_collate}[task](items)


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("case", CASES)
def test_host_pretrain_collate_equals_reference(case, task):
    got, want = rebuild(case, task), ref_batch(case, task)
    assert len(want) >= 7
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.shape, w.shape, g.dtype, w.dtype)
            assert torch.equal(g, w), k
        else:
            assert json.loads(json.dumps(g)) == w, k
    assert set(got) - set(want) == (set() if task == "mlm" else {"lengths"})


def test_fixture_has_the_cases_it_is_meant_to_have():
    n = ref_batch("narrow", "mlm")
    assert (n["attn_masks"][:, 0] == 0).any()                                        # a zero-frame subtitle
    assert n["txt_mask_tgt"].shape == n["attn_masks"].shape and n["txt_labels"].dim() == 1
    assert int(n["txt_mask_tgt"].sum()) == n["txt_labels"].numel()
    assert (n["input_ids"][:, 0] == 0).all()                                         # CLS, not SEP
    assert json.loads(str(Z["ctx1.desc"]))["sub_ctx_len"] == 1
    one = ref_batch("oneframe", "mfm")
    assert int(one["c_attn_masks"][0].sum()) == 1 and bool(one["c_v_masks"][0, 0])   # a one-frame video: its frame is masked
    # the at-least-one case: a row whose only label is its first token, which reads MASK (the generator asserts from the
    # draws that the rule, not a draw, put it there)
    a, d = ref_batch("atleast1", "mlm"), json.loads(str(Z["atleast1.desc"]))
    W = a["input_ids"].shape[1]
    slots = a["attn_masks"].shape[1] - W
    assert slots >= 0 and any(int(a["input_ids"][r, 1]) == d["mask"] for r in range(a["input_ids"].shape[0]))
    f = ref_batch("narrow", "fom")
    assert f["reordered_frame_idx"].numel() == 2 * f["binary_targets"].numel()
    v = ref_batch("rand3", "vsm")
    assert v["q_vidx"].numel() == 4 * len(v["vids"]) and v["targets"].shape == (v["q_vidx"].numel(), 2)


def test_eval_collate_adds_the_video_names():
    from hero_amd import collate as C
    d = json.loads(str(Z["narrow.desc"]))
    random.seed(3)
    items = []
    for v in d["videos"]:
        feat = torch.from_numpy(Z["narrow.feat.%s" % v["vid"]])
        video = C.video_item(feat, [(s, list(f)) for s, f in v["sub2frames"]], v["sub_tokens"], sep=d["sep"])
        items.append((v["vid"],) + C.fom_item(video, 0.5))
    got = C.fom_eval_collate(items)
    want = C.fom_collate([it[1:] for it in items])
    assert got["vids"] == [v["vid"] for v in d["videos"]]
    assert all(torch.equal(got[k], want[k]) for k in ("shuffled_orders", "targets", "reordered_frame_idx", "binary_targets"))
