"""Host restatements for the post-processing tests, and the loader of tests/golden/case_postproc.npz.

`first_hit` is eval_by_task_type's arithmetic (utils/tvr_standalone_eval.py:57-72, 148-179) reduced to what the metrics use: per
query, the rank of the first prediction in the ground-truth video and of the first one there whose fp32 IoU with the ground
truth reaches each threshold.  numpy >= 2 compares a float32 array with a Python float in float32; the thresholds are cast
to float32 here so that older numpy versions do the same."""
import json
import os

import numpy as np
import torch

from tests.util import GOLDEN

RESULT_KEYS = ("vr_scores", "vr_indices", "vcmr_scores", "vcmr_video", "vcmr_st", "vcmr_ed", "svmr_scores", "svmr_st", "svmr_ed")
CASES = ("a", "b", "c", "d1", "d2", "e", "f", "g")


def first_hit(video, st, ed, gt_video, gt_ts, interval, thds, n_pred):
    """int arrays [Nq, >= n_pred] (st, ed may be None), gt_video [Nq], gt_ts fp32 [Nq, 2] -> first [Nq, len(thds) + 1] int32."""
    video = np.asarray(video)[:, :n_pred]
    Nq, P = video.shape
    first = np.full((Nq, len(thds) + 1), P, dtype=np.int32)
    interval = np.float32(interval)
    for q in range(Nq):
        match = (video[q] >= 0) & (video[q] == gt_video[q])
        if st is not None:
            s, e = np.asarray(st)[q, :P], np.asarray(ed)[q, :P]
            match &= s >= 0
        if match.any():
            first[q, 0] = int(np.argmax(match))
        if st is None or not len(thds):
            continue
        p0, p1 = s.astype(np.float32) * interval, (e + 1).astype(np.float32) * interval
        g0, g1 = np.float32(gt_ts[q][0]), np.float32(gt_ts[q][1])
        inter = np.maximum(np.float32(0), np.minimum(p1, g1) - np.maximum(p0, g0))
        hull = np.maximum(p1, g1) - np.minimum(p0, g0)
        iou = np.divide(inter, hull, out=np.zeros_like(inter), where=hull != 0)
        assert iou.dtype == np.float32
        for t, thd in enumerate(thds):
            ok = match & (iou >= np.float32(thd))
            if ok.any():
                first[q, 1 + t] = int(np.argmax(ok))
    return first


def load_cases():
    """{case name: {"out": result dictionary of CPU tensors, "cfg": {...}, "gt_vidx", "gt_ts", "desc_type", "ref": {task_keep,
    task_count, task_st_sec, task_ed_sec}, "metrics": the reference's dictionary}}."""
    z = np.load(os.path.join(GOLDEN, "case_postproc.npz"), allow_pickle=False)
    cases = {}
    for name in CASES:
        pre = name + "."
        arr = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        cfg = json.loads(str(arr.pop("cfg")))
        metrics = json.loads(str(arr.pop("metrics")))
        out = {k: torch.from_numpy(arr[k]) for k in RESULT_KEYS if k in arr}
        ref = {k[len("ref_"):]: arr[k] for k in arr if k.startswith("ref_")}
        cases[name] = dict(out=out, cfg=cfg, gt_vidx=arr["gt_vidx"], gt_ts=arr["gt_ts"], desc_type=arr["desc_type"], ref=ref, metrics=metrics)
    return cases


def meter_from_lists(meter, d, gt_vidx, gt_ts, desc_type):
    """RecallMeter.update's bookkeeping on the host: `first_hit` above in place of the kernel, then the meter's own arithmetic."""
    gt_vidx, gt_ts = np.asarray(gt_vidx), np.asarray(gt_ts, dtype=np.float32)
    dt = None if desc_type is None else torch.as_tensor(np.asarray(desc_type))
    P = meter.max_pred_per_query
    for task in ("vcmr", "svmr"):
        pre = task + "_nms_" if task + "_nms_st" in d else task + "_"
        if pre + "st" not in d:
            continue
        st, ed = d[pre + "st"].cpu().numpy(), d[pre + "ed"].cpu().numpy()
        video = d[pre + "video"].cpu().numpy() if task == "vcmr" else np.where(st >= 0, gt_vidx.reshape(-1, 1), -1)
        first = first_hit(video, st, ed, gt_vidx, gt_ts, meter.vfeat_interval, meter.iou_thds, P)
        meter.add_first(task.upper(), torch.from_numpy(first), min(P, st.shape[1]), dt)
    if "vr_indices" in d:
        vi = d["vr_indices"].cpu().numpy()
        first = first_hit(vi, None, None, gt_vidx, gt_ts, meter.vfeat_interval, (), P)
        meter.add_first("VR", torch.from_numpy(first).expand(-1, len(meter.iou_thds) + 1), min(P, vi.shape[1]), dt)
    return meter
