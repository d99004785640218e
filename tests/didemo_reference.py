"""Host restatement of the reference's recall rule for ground truth with several annotators (DiDeMo), and the loader of
tests/golden/case_vr.npz.

`first_hit_multi` is eval_by_task_type's arithmetic (utils/tvr_standalone_eval.py:57-72, 148-181) reduced to what the metrics use,
written as tests/postproc_reference.first_hit is: fp32 throughout, the thresholds cast to fp32.  Per query it gives the rank of
the first prediction in the ground-truth video and, per threshold, of the first one there that enough annotators agree with:
from four timestamps on the reference asks for `least_n_overlap = 2` of them to have IoU >= the threshold, with fewer (one
[st, ed]) for that one.  `need` and `only_first` bend the rule on purpose, so that a test can show its cases tell the rules
apart."""
import json
import os

import numpy as np
import torch

from tests.util import GOLDEN

DIDEMO_CASES = ("i15", "i20")
BATCHES = ("vr_vonly", "vr_vonly_eval", "vr_vonly_full", "vr_sub", "vcmr_vonly")


def first_hit_multi(video, st, ed, gt_video, gt_ts, gt_n, interval, thds, n_pred, need=None, only_first=False):
    """int arrays [Nq, >= n_pred], gt_video [Nq], gt_ts fp32 [Nq, G, 2] (slots >= gt_n[q] are never read), gt_n [Nq]
    -> first [Nq, len(thds) + 1] int32.  need: the number of agreeing annotators asked for, whatever gt_n is; only_first: only
    annotator 0 is looked at."""
    video = np.asarray(video)[:, :n_pred]
    Nq, P = video.shape
    first = np.full((Nq, len(thds) + 1), P, dtype=np.int32)
    interval = np.float32(interval)
    for q in range(Nq):
        s, e = np.asarray(st)[q, :P], np.asarray(ed)[q, :P]
        match = (video[q] >= 0) & (video[q] == gt_video[q]) & (s >= 0)
        if match.any():
            first[q, 0] = int(np.argmax(match))
        if not len(thds):
            continue
        n = 1 if only_first else int(gt_n[q])
        least = (2 if n >= 4 else 1) if need is None else need
        p0, p1 = s.astype(np.float32) * interval, (e + 1).astype(np.float32) * interval
        reached = np.zeros((len(thds), P), dtype=np.int64)
        for g in range(n):
            g0, g1 = np.float32(gt_ts[q][g][0]), np.float32(gt_ts[q][g][1])
            inter = np.maximum(np.float32(0), np.minimum(p1, g1) - np.maximum(p0, g0))
            hull = np.maximum(p1, g1) - np.minimum(p0, g0)
            iou = np.divide(inter, hull, out=np.zeros_like(inter), where=hull != 0)
            assert iou.dtype == np.float32
            for t, thd in enumerate(thds):
                reached[t] += iou >= np.float32(thd)
        for t in range(len(thds)):
            ok = match & (reached[t] >= least)
            if ok.any():
                first[q, 1 + t] = int(np.argmax(ok))
    return first


def meter_from_rows(meter, case, **rule):
    """RecallMeter's bookkeeping on the host for one didemo.* case: VCMR from the rows as they are, SVMR from the rows in the
    ground-truth video (every other slot vacant - the reference ranks SVMR among the predictions of that video)."""
    gt, P = case["gt_vidx"], meter.max_pred_per_query
    for task, (video, st, ed) in (("VCMR", case["vcmr"]), ("SVMR", case["svmr"])):
        first = first_hit_multi(video, st, ed, gt, case["gt_ts"], case["gt_n"], meter.vfeat_interval, meter.iou_thds, P, **rule)
        meter.add_first(task, torch.from_numpy(first), min(P, st.shape[1]))
    return meter


def load_vr():
    """case_vr.npz as {key: array}; JSON strings decoded for the keys that hold them."""
    z = np.load(os.path.join(GOLDEN, "case_vr.npz"), allow_pickle=False)
    out = {}
    for k in z.files:
        v = z[k]
        out[k] = json.loads(str(v)) if v.dtype.kind == "U" and v.ndim == 0 else v
    return out


def batch_of(z, name):
    """One recorded reference batch: tensors back as tensors, lists as lists."""
    pre = "batch." + name + "."
    return {k[len(pre):]: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in z.items() if k.startswith(pre)}


def didemo_cases(z):
    """{case: {"vcmr": (video, st, ed), "svmr": (video, st, ed), gt_vidx, gt_ts [Nq, G, 2], gt_n, ts_list (ragged), interval, metrics}}"""
    return {name: _didemo_case(z, name) for name in DIDEMO_CASES}


def _didemo_case(z, name):
    pre = "didemo." + name + "."
    video, st, ed, gt = z[pre + "video"], z[pre + "st"], z[pre + "ed"], z[pre + "gt_vidx"]
    own = video == gt.reshape(-1, 1)
    svmr = (np.where(own, video, -1).astype(np.int32), np.where(own, st, -1).astype(np.int32), np.where(own, ed, -1).astype(np.int32))
    # the reference's SVMR rank counts only the predictions in the ground-truth video: pack them to the front
    order = np.argsort(~own, axis=1, kind="stable")
    svmr = tuple(np.take_along_axis(a, order, 1) for a in svmr)
    return dict(vcmr=(video, st, ed), svmr=svmr, gt_vidx=gt, gt_ts=z[pre + "gt_ts"], gt_n=z[pre + "gt_n"], ts_list=z[pre + "ts_list"],
                interval=float(z[pre + "cfg"]["vfeat_interval"]), metrics=z[pre + "metrics"])
