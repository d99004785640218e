#!/usr/bin/env python3
"""A/B of the pre-training batch draw at the D3 shape (32 videos x 60 frames, 15 subtitles x (4 frames + 20 tokens), D = 4352):
hero_amd.pretrain_data.PretrainMasker.draw (kernels over one clean device batch: MLM + MFM + FOM) against the host collates of
hero_amd.collate (mlm_collate + mfm_collate + fom_collate, the reference's DataLoader-side draws restated) on the same videos.

Device side: HIP-event pairs around `--inner` back-to-back draw() calls (one draw is too short a window for the events), the
median over `--runs` pairs after warm-up, per draw - for the three tasks together and for each task alone.  The masked copy's
achieved GB/s is its own byte count (every destination row written once: clip copy, subtitle copy, compact targets; every row
that is not a row of zeros read once) over the time of the MFM draw, whose small mask kernel is included in that time.
Host side: wall clock of building the three task batches from the raw videos in one process (items + collates, the features
already in memory), the median over `--host-runs` runs.  Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASK_ID, V_RANGE, CLS, SEP = 50264, (5, 50265), 0, 2
VIDEOS, FRAMES, SUBS, FPS, TOKS, D = 32, 60, 15, 4, 20, 4352


def make_videos(seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(VIDEOS):
        feat = torch.randn(FRAMES, D, generator=g)
        s2f = [(s, list(range(s * FPS, (s + 1) * FPS))) for s in range(SUBS)]
        toks = [torch.randint(V_RANGE[0], V_RANGE[1], (TOKS - 1,), generator=g).tolist() for _ in range(SUBS)]
        out.append((feat, s2f, toks))
    return out


def host_batches(videos, p):
    from hero_amd import collate as C
    mlm = C.mlm_collate([C.mlm_item(f, s, t, MASK_ID, V_RANGE, cls_=CLS, mask_prob=p) for f, s, t in videos])
    mfm = C.mfm_collate([C.mfm_item(C.video_item(f, s, t, sep=SEP), p) for f, s, t in videos])
    fom = C.fom_collate([C.fom_item(C.video_item(f, s, t, sep=SEP), p) for f, s, t in videos])
    return mlm, mfm, fom


def device_us(fn, a):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / a.inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--prob", type=float, default=0.15)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain_mask: needs a GPU (nothing is measured without one)")
    from hero_amd import collate as C
    from hero_amd.pretrain_data import PretrainMasker
    videos = make_videos(1)
    host = C.video_collate([C.video_item(f, s, t, sep=SEP) for f, s, t in videos])
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items() if k != "lengths"}
    ln = {k: torch.as_tensor(v, dtype=torch.int32).cuda() for k, v in host["lengths"].items()}
    m = PretrainMasker.for_batch(host, "cuda", MASK_ID, V_RANGE, CLS, mlm_prob=a.prob, mfm_prob=a.prob, fom_prob=a.prob).set_seed(2024)
    times = {"all": device_us(lambda: m.draw(dev, ln), a)}
    for task in ("mlm", "mfm", "fom"):
        times[task] = device_us(lambda: m.draw(dev, ln, tasks=(task,)), a)
    m.draw(dev, ln)
    n_tok, n_frm = m._counts()
    src = m._row_src.cpu()
    copy_bytes = (int(src.numel()) + int((src >= 0).sum())) * D * 4
    host_s = []
    for i in range(a.host_runs):
        random.seed(i)
        t0 = time.perf_counter()
        host_batches(videos, a.prob)
        host_s.append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    T, max_sl = host["f_sub_input_ids"].shape
    line = json.dumps({
        "bench": "pretrain_mask_ab", "shape": {"videos": VIDEOS, "frames": FRAMES, "subs": SUBS, "frames_per_sub": FPS, "tokens_per_sub": TOKS,
                                               "D": D, "rows": T, "max_sl": max_sl, "prob": a.prob},
        "device_timer": "HIP events around %d back-to-back draw() calls, per draw, median of %d" % (a.inner, a.runs),
        "host_timer": "wall clock, one process: mlm + mfm + fom items and collates of hero_amd.collate from the raw videos; median of %d" % a.host_runs,
        "draw_all_us_median": round(med["all"], 2), "draw_all_us_min": round(min(times["all"]), 2),
        "draw_mlm_us_median": round(med["mlm"], 2), "draw_mfm_us_median": round(med["mfm"], 2), "draw_fom_us_median": round(med["fom"], 2),
        "masked_tokens": n_tok, "masked_frames": n_frm, "masked_copy_bytes": copy_bytes,
        "masked_copy_gb_per_s_over_mfm_draw": round(copy_bytes / (med["mfm"] * 1e-6) / 1e9, 1),
        "host_collates_ms_median": round(statistics.median(host_s) * 1e3, 2), "host_collates_ms_min": round(min(host_s) * 1e3, 2),
        "host_over_device": round(statistics.median(host_s) * 1e6 / med["all"], 1), "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
