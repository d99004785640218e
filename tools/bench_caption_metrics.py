#!/usr/bin/env python3
"""A/B of the caption scorer: hero_amd.caption.k_caption_score (one HIP launch over device id rows) against the host scorers of
tests/caption_reference.py (plain Python, float64: the reference's pycocoevalcap restated on integers) on the same rows.

Two shapes, each with 4 references of about 15 tokens per clip and Tcap 30: 200 rows (40 clips x 5 samples - the reward of a
self-critical step) and 4096 rows (a validation set, one row per clip).  Captions are a reference with a quarter of the tokens
replaced, over a Zipf-like vocabulary of 2000 ids.

Device side: HIP-event pairs around `--inner` back-to-back launches (one launch is too short a window for the events), the
median over `--runs` pairs after warm-up, per launch.  Host side: wall clock of the device-to-host copy of the id rows, the cut
at eos and the scoring of every row, document frequencies built beforehand; the median over `--host-runs` runs.  Both sides'
results are compared (BLEU integers equal, CIDEr-D within 1e-5 * max(1, |reference|)).  Prints one JSON line; `--out FILE` also
writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EOS, TCAP, VOCAB = 2, 30, 2000


def make_case(clips, per_clip, seed):
    rng = np.random.RandomState(seed)

    def sent(n):
        return [int(t) for t in np.minimum(rng.zipf(1.3, n) + 2, VOCAB - 1)]
    refs = [[sent(int(rng.randint(10, 21))) for _ in range(4)] for _ in range(clips)]
    rows, clip = [], []
    for c in range(clips):
        for _ in range(per_clip):
            h = list(refs[c][int(rng.randint(4))])
            for i in rng.choice(len(h), len(h) // 4, replace=False):
                h[i] = int(rng.randint(3, VOCAB))
            rows.append(h)
            clip.append(c)
    ids = torch.full((len(rows), TCAP), EOS, dtype=torch.int32)
    for i, h in enumerate(rows):
        ids[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
    return refs, ids, clip


def measure(clips, per_clip, a):
    from hero_amd.caption import CaptionRefs, k_caption_score
    from tests import caption_reference as R
    refs, ids, clip = make_case(clips, per_clip, seed=clips)
    table = CaptionRefs(refs, device="cuda")
    d_ids, d_clip = ids.cuda(), torch.tensor(clip, dtype=torch.int32).cuda()
    M = ids.shape[0]
    out = (torch.empty((M, 10), dtype=torch.int32, device="cuda"), torch.empty((M,), device="cuda"), torch.empty((M,), device="cuda"))
    for _ in range(10):
        k_caption_score(d_ids, d_clip, table, EOS, out=out)
    torch.cuda.synchronize()
    dev = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            k_caption_score(d_ids, d_clip, table, EOS, out=out)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / a.inner)
    df, n = R.document_frequency(refs)
    host, want = [], None
    for _ in range(a.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = d_ids.cpu().tolist()
        want = [R.score_clip(R.cut(r, EOS), refs[c], df, n) for r, c in zip(rows, clip)]
        host.append((time.perf_counter() - t0) * 1e6)
    stats_equal = out[0].cpu().tolist() == [R.stats_row(w) for w in want]
    ref = torch.tensor([w["cider"] for w in want], dtype=torch.float64)
    cider_err = float((out[2].double().cpu() - ref).abs().max())
    if not stats_equal or bool(((out[2].double().cpu() - ref).abs() > 1e-5 * ref.abs().clamp(min=1.0)).any()):
        raise SystemExit("bench_caption_metrics: the two sides disagree (stats equal %s, CIDEr-D error %.3e)" % (stats_equal, cider_err))
    return {"rows": M, "clips": clips, "refs_per_clip": 4, "tcap": TCAP, "kernel_us_median": round(statistics.median(dev), 2),
            "kernel_us_min": round(min(dev), 2), "host_us_median": round(statistics.median(host), 1), "host_us_min": round(min(host), 1),
            "host_over_kernel": round(statistics.median(host) / statistics.median(dev), 1), "stats_equal": stats_equal,
            "cider_max_abs_err": float("%.3e" % cider_err)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_caption_metrics: needs a GPU (nothing is measured without one)")
    line = json.dumps({"bench": "caption_metrics_ab", "what": "BLEU statistics + ROUGE-L + CIDEr-D of every row",
                       "kernel_timer": "HIP events around %d back-to-back launches, per launch, median of %d" % (a.inner, a.runs),
                       "host_timer": "wall clock: device-to-host copy of the ids, cut at eos, plain-Python float64 scorers; median of %d" % a.host_runs,
                       "reward_40x5": measure(40, 5, a), "validation_4096": measure(4096, 1, a), "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
