#!/usr/bin/env python3
"""A/B of the recall bookkeeping for ground truth with several annotators (DiDeMo): `RecallMeter.update` on the device
(hero_first_hit_multi; one HIP-event pair per batch) against the host statement on the same rows (the reference's arithmetic in
numpy, eval_by_task_type's per-query loop reduced to first-hit ranks; wall clock).  80 queries x 100 predictions x 4 annotators,
VCMR + SVMR rows, sides alternating, medians.  Prints one JSON line; it belongs verbatim in profiles/didemo_recall_ab.txt.

    python tools/bench_didemo_recall.py [--queries 80 --preds 100 --annotators 4 --batches 20 --warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_first_hit(video, st, ed, gt_video, gt_ts, gt_n, interval, thds):
    """utils/tvr_standalone_eval.py:148-181 per query, reduced to the rank of the first correct prediction per threshold."""
    Nq, P = video.shape
    first = np.full((Nq, len(thds) + 1), P, dtype=np.int32)
    for q in range(Nq):
        match = (video[q] >= 0) & (video[q] == gt_video[q]) & (st[q] >= 0)
        if match.any():
            first[q, 0] = int(np.argmax(match))
        p0, p1 = st[q].astype(np.float32) * np.float32(interval), (ed[q] + 1).astype(np.float32) * np.float32(interval)
        n = int(gt_n[q])
        reached = np.zeros((len(thds), P), dtype=np.int64)
        for g in range(n):
            g0, g1 = gt_ts[q, g]
            inter = np.maximum(np.float32(0), np.minimum(p1, g1) - np.maximum(p0, g0))
            hull = np.maximum(p1, g1) - np.minimum(p0, g0)
            iou = np.divide(inter, hull, out=np.zeros_like(inter), where=hull != 0)
            for t, thd in enumerate(thds):
                reached[t] += iou >= np.float32(thd)
        for t in range(len(thds)):
            ok = match & (reached[t] >= (2 if n >= 4 else 1))
            if ok.any():
                first[q, 1 + t] = int(np.argmax(ok))
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=80)
    ap.add_argument("--preds", type=int, default=100)
    ap.add_argument("--annotators", type=int, default=4)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from hero_amd import retrieval as HR
    rng = np.random.default_rng(0)
    Nq, P, G = args.queries, args.preds, args.annotators
    video = rng.integers(0, 8, size=(Nq, P)).astype(np.int32)
    st = rng.integers(0, 30, size=(Nq, P)).astype(np.int32)
    ed = (st + rng.integers(1, 8, size=(Nq, P))).astype(np.int32)
    gt = rng.integers(0, 8, size=Nq).astype(np.int32)
    g0 = rng.integers(0, 6, size=(Nq, G)) * 5.0
    gt_ts = np.stack([g0, g0 + 5.0 * rng.integers(1, 3, size=(Nq, G))], axis=2).astype(np.float32)
    gt_n = np.full(Nq, G, dtype=np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()                    # noqa: E731
    d = {"vcmr_video": dev(video), "vcmr_st": dev(st), "vcmr_ed": dev(ed), "svmr_st": dev(st), "svmr_ed": dev(ed)}
    dgt, dts, dn = dev(gt), dev(gt_ts), dev(gt_n)
    thds = (0.5, 0.7)
    sv_video = np.where(st >= 0, gt.reshape(-1, 1), -1)
    dev_ms, host_ms = [], []
    meter = HR.RecallMeter(device="cuda")
    for i in range(args.warmup + args.batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        meter.update(d, dgt, dts, gt_n=dn)
        e1.record()
        torch.cuda.synchronize()
        host = HR.RecallMeter()
        t0 = time.perf_counter()
        for task, v in (("VCMR", video), ("SVMR", sv_video)):
            host.add_first(task, torch.from_numpy(host_first_hit(v, st, ed, gt, gt_ts, gt_n, 1.5, thds)), P)
        t1 = time.perf_counter()
        if i >= args.warmup:
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append((t1 - t0) * 1e3)
    one = HR.RecallMeter(device="cuda")
    one.update(d, dgt, dts, gt_n=dn)
    same = one.compute() == host.compute()
    med = lambda x: float(np.median(x))                           # noqa: E731
    print(json.dumps({"bench": "didemo_recall_ab", "queries": Nq, "preds": P, "annotators": G, "tasks": ["VCMR", "SVMR"], "batches": args.batches,
                      "device_ms": round(med(dev_ms), 4), "device_ms_min_max": [round(min(dev_ms), 4), round(max(dev_ms), 4)],
                      "host_ms": round(med(host_ms), 3), "host_over_device": round(med(host_ms) / med(dev_ms), 1),
                      "timer": "device: one HIP-event pair around RecallMeter.update; host: wall clock of the numpy statement + add_first",
                      "same_metrics": bool(same), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
