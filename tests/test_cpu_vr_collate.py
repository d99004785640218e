"""The items and collates of video retrieval and of video-only corpora (hero_amd/collate.py) against the batches the reference's own
datasets and collates produced (tests/golden/case_vr.npz, written by tests/golden/make_golden_vr.py): every tensor and every
list, bit for bit.  And the refusals of hero_amd.retrieval.pack_gt_ts."""
import numpy as np
import pytest
import torch

from hero_amd import collate as C
from hero_amd.retrieval import pack_gt_ts
from tests import didemo_reference as DR

Z = DR.load_vr()
DESC = Z["desc"]
FEATS = {v["vid"]: torch.from_numpy(Z["feat." + v["vid"]]) for v in DESC["videos"]}


def video_only(vid):
    return C.video_only_item(FEATS[vid], cls_=DESC["cls"])


def video_sub(vid):
    v = next(v for v in DESC["videos"] if v["vid"] == vid)
    return C.video_item(FEATS[vid], [(si, list(fr)) for si, fr in v["subs"]], v["sub_tokens"], sep=DESC["sep"])


def rebuild(name):
    qs = DESC["queries"]
    if name == "vr_vonly":
        return C.vr_collate([C.vr_item(video_only(q["vid"]), q["vid"], [q["tokens"]], cls_=DESC["cls"]) for q in qs])
    if name == "vr_vonly_eval":
        return C.vr_eval_collate([([q["qid"]], C.vr_item(video_only(q["vid"]), q["vid"], [q["tokens"]])) for q in qs])
    if name == "vr_vonly_full":
        return C.vr_full_eval_collate([C.vr_full_eval_item(q["qid"], q["tokens"], q["vid"]) for q in qs])
    if name == "vr_sub":
        return C.vr_collate([C.vr_item(video_sub(q["vid"]), q["vid"], [q["tokens"]]) for q in qs])
    if name == "vcmr_vonly":
        return C.vcmr_collate([C.vcmr_item(video_only(q["vid"]), q["vid"], [(q["tokens"], q["ts"])], frame_interval=DESC["frame_interval"]) for q in qs])
    raise KeyError(name)


def same(a, b):
    if torch.is_tensor(b):
        return torch.is_tensor(a) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("name", DR.BATCHES)
def test_batch_equals_the_reference(name):
    mine, want = rebuild(name), DR.batch_of(Z, name)
    assert set(mine) - {"lengths"} == set(want), (sorted(mine), sorted(want))
    for k, v in want.items():
        assert same(mine[k], v), (name, k, mine[k], v)


def test_video_only_item_is_one_cls_row_with_every_frame():
    feat = FEATS["v00"]
    ids, feats, masks, clip, clip_mask, n_subs, sub2frames = C.video_only_item(feat, cls_=0)
    assert [t.tolist() for t in ids] == [[0]] and ids[0].dtype == torch.long                  # CLS, not SEP
    assert len(feats) == 1 and torch.equal(feats[0], feat) and torch.equal(clip, feat)
    assert masks[0].tolist() == [1] * (1 + feat.shape[0]) and clip_mask.tolist() == [1] * feat.shape[0]
    assert n_subs == 1 and sub2frames == [(0, list(range(feat.shape[0])))]
    b = C.video_collate([C.video_only_item(FEATS[v]) for v in sorted(FEATS)])
    lens = b["lengths"]
    assert lens["sub_ntok"].tolist() == [1, 1, 1] and lens["sub_nfrm"].tolist() == lens["vid_nfrm"].tolist() == [9, 6, 10]
    assert lens["vid_sub_off"].tolist() == [0, 1, 2, 3] and lens["sub_frm_off"].tolist() == [0, 9, 15, 25]


def test_full_eval_target_follows_the_timestamp():
    qid, rows = C.vcmr_full_eval_item("q", [5, 6], "v", ts=[3.2, 7.6], n_frames=9)
    assert qid == "q" and rows[0][3].tolist() == [2, 5] and rows[0][0].tolist() == [0, 5, 6]
    assert C.vcmr_full_eval_item("q", [5], "v")[1][0][3].tolist() == [-1, -1]
    assert C.vr_full_eval_item("q", [5], "v")[1][0][3].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        C.vcmr_full_eval_item("q", [5], "v", ts=[0.0, 1.0])


def test_pack_gt_ts():
    ts, n = pack_gt_ts([[1.5, 4.0], [[0, 5]] * 4, [[5, 10]] * 7, np.array([2.0, 3.0])])
    assert ts.dtype == torch.float32 and tuple(ts.shape) == (4, 7, 2) and n.dtype == torch.int32 and n.tolist() == [1, 4, 7, 1]
    assert ts[0, 0].tolist() == [1.5, 4.0] and ts[1, :4].tolist() == [[0.0, 5.0]] * 4 and float(ts[1, 4:].abs().sum()) == 0.0
    ts, n = pack_gt_ts([[1.0, 2.0]])
    assert tuple(ts.shape) == (1, 1, 2) and n.tolist() == [1]
    for bad in ([[[0, 5]] * 2], [[[0, 5]] * 3], [[[0, 5]] * 17], [[[0, 5]]], [[1.0, 2.0, 3.0]], []):
        with pytest.raises(ValueError):
            pack_gt_ts(bad)
    case = DR.didemo_cases(Z)["i15"]
    ts, n = pack_gt_ts(case["ts_list"])
    assert np.array_equal(ts.numpy(), case["gt_ts"]) and np.array_equal(n.numpy(), case["gt_n"]) and sorted(set(n.tolist())) == [4, 5, 7]
