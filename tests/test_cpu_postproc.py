"""What follows a search, on the host: `postprocess_host` and RecallMeter's arithmetic against the reference-made
tests/golden/case_postproc.npz (tests/golden/make_golden_postproc.py: the reference's post_processing_*_nms, get_submission_top_n
and eval_retrieval on synthetic candidate lists).  Everything is compared exactly: positions, counts, integers, the fp32
seconds bit for bit, and the metrics as dictionaries."""
import numpy as np
import pytest
import torch

import hero_amd
from hero_amd import retrieval as HR
from tests import postproc_reference as PR

CASES = PR.load_cases()


def host_post(case):
    cfg = case["cfg"]
    return HR.postprocess_host(case["out"], vfeat_interval=cfg["vfeat_interval"], nms_thd=cfg["nms_thd"], max_after_nms=cfg["max_after_nms"])


def check_post(post, case):
    """a `postprocess` result against the reference's survivors of the case"""
    out, ref, A = case["out"], case["ref"], case["cfg"]["max_after_nms"]
    for task in ("vcmr", "svmr"):
        keep, count = ref[task + "_keep"], ref[task + "_count"]
        none = keep < 0
        at = np.clip(keep, 0, None)
        assert np.array_equal(post[task + "_nms_count"].cpu().numpy(), count), task
        names = [("scores", 0), ("st", -1), ("ed", -1)] + ([("video", -1)] if task == "vcmr" else [])
        for name, empty in names:
            got = post["%s_nms_%s" % (task, name)].cpu()
            src = out["%s_%s" % (task, name)]
            assert got.dtype == src.dtype and tuple(got.shape) == (len(keep), A), (task, name)
            want = np.where(none, empty, np.take_along_axis(src.numpy(), at, 1))
            assert np.array_equal(got.numpy(), want), (task, name)
        for name in ("st_sec", "ed_sec"):
            got = post["%s_nms_%s" % (task, name)].cpu()
            assert got.dtype == torch.float32
            assert np.array_equal(got.numpy().view(np.int32), ref["%s_%s" % (task, name)].view(np.int32)), (task, name)      # bit for bit
        assert post[task + "_nms_count"].dtype == torch.int32
    assert post["vr_indices"] is out["vr_indices"]


def test_fixture_is_not_vacuous():
    a, b = CASES["a"], CASES["b"]
    assert a["out"]["vcmr_st"].shape == (80, 200) and b["out"]["svmr_st"].shape[1] == 400 and b["cfg"]["max_after_nms"] == 150
    assert a["ref"]["svmr_count"].sum() <= 0.75 * 80 * 200 and (a["ref"]["vcmr_count"] == 100).any()
    assert (b["ref"]["vcmr_count"] == 100).all()
    assert (CASES["c"]["out"]["vcmr_st"][:, -1] == -1).any() and CASES["e"]["out"]["vcmr_st"].shape[1] == 1
    assert CASES["f"]["cfg"]["nms_thd"] == -1 and CASES["g"]["cfg"]["vfeat_interval"] == 2
    assert CASES["d1"]["cfg"]["nms_thd"] == 0.6 and CASES["d2"]["cfg"]["nms_thd"] == 0.5


@pytest.mark.parametrize("name", PR.CASES)
def test_postprocess_host_reproduces_the_reference(name):
    check_post(host_post(CASES[name]), CASES[name])


@pytest.mark.parametrize("name", PR.CASES)
def test_metrics_equal_the_reference_dictionary(name):
    case = CASES[name]
    post = host_post(case)
    meter = hero_amd.RecallMeter(vfeat_interval=case["cfg"]["vfeat_interval"])
    PR.meter_from_lists(meter, post, case["gt_vidx"], case["gt_ts"], case["desc_type"])
    assert meter.compute() == case["metrics"]


def test_metrics_without_nms_keys_and_without_types():
    """the raw result dictionary of a search is accepted too (case f has no NMS: the same lists), and no *_by_type without types"""
    case = CASES["f"]
    meter = PR.meter_from_lists(hero_amd.RecallMeter(), case["out"], case["gt_vidx"], case["gt_ts"], None)
    got = meter.compute()
    assert set(got) == {"VCMR", "SVMR", "VR"}
    assert got == {k: case["metrics"][k] for k in got}


def test_three_uneven_chunks_accumulate_to_the_same_dictionary():
    case = CASES["a"]
    post = host_post(case)
    meter = hero_amd.RecallMeter()
    for lo, hi in ((0, 7), (7, 48), (48, 80)):
        part = {k: v[lo:hi] for k, v in post.items()}
        PR.meter_from_lists(meter, part, case["gt_vidx"][lo:hi], case["gt_ts"][lo:hi], case["desc_type"][lo:hi])
    assert meter.compute() == case["metrics"]
    meter.reset()
    assert meter.compute() == {}


def test_cap_and_ties_of_the_host_sweep():
    """per_video_cap is per video, not per row; an IoU equal to the threshold does not suppress, one above it does"""
    st = np.arange(0, 40, 2, dtype=np.int32).reshape(1, 20)
    video = (np.arange(20, dtype=np.int32) % 2).reshape(1, 20)
    keep, count = HR.nms_rows_host(video, st, st + 1, 0.5, 3, 20)
    assert count[0] == 6 and keep[0, :6].tolist() == [0, 1, 2, 3, 4, 5]
    one = np.zeros((1, 3), dtype=np.int32)
    keep, count = HR.nms_rows_host(one, np.array([[0, 2, 1]], dtype=np.int32), np.array([[4, 4, 4]], dtype=np.int32), 0.6, 100, 3)
    assert keep[0].tolist() == [0, 1, -1] and count[0] == 2            # 3/5 == 0.6 survives, 4/5 falls


def test_device_entry_points_refuse_cpu_tensors():
    z = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        HR.k_moment_nms(z, z, z, 0.5)
    with pytest.raises(RuntimeError):
        HR.k_first_hit(z, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        HR.postprocess(CASES["e"]["out"])
