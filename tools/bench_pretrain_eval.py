#!/usr/bin/env python3
"""A/B of the per-batch scoring of pre-training validation: hero_amd.pretrain_eval.ce_eval / feat_eval (one pass over the head's
own output, counters on the device, nothing read on the host) against the reference formulation of pretrain.py:462-608 on the
SAME bf16 logits:
    scores = logits[:, :ncols].float();  F.cross_entropy(scores, labels, reduction='sum').item();
    (scores.max(dim=-1)[1] == labels).sum().item()
and, for the feature terms, F.mse_loss(none).sum(1).sqrt().sum().item() + F.cosine_similarity(...).sum().item() on fp32 rows.

Shapes: the MLM rows of a D3 batch (32 videos x 15 subtitles x 19 maskable tokens at 15 %: 1368 rows) x 50 265 columns (ld 50 272);
one FOM shape (32 x 60 frames = 1920 rows x 100 clip positions, 15 % of the rows with a target); 288 masked frames x 4352.

Timer: host clock around `--inner` back-to-back scorings of one batch, closed by a device synchronise (the reference's .item()
calls synchronise by themselves; the device path is synchronised once, as a validator reads its counters once), per scoring;
the two sides alternate, median of `--runs` windows after warm-up.  The achieved GB/s is the bytes of the logits' real columns
over the device path's time.  Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MLM = (1368, 50265, 50272)
FOM = (1920, 100, 100)
FEAT = (288, 4352)


def window_us(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / inner


def ab(dev_fn, ref_fn, a):
    for _ in range(3):
        dev_fn()
        ref_fn()
    d, r = [], []
    for _ in range(a.runs):
        d.append(window_us(dev_fn, a.inner))
        r.append(window_us(ref_fn, a.inner))
    return d, r


def ce_pair(shape, ignore_index, valid_share, g):
    from hero_amd import pretrain_eval as E
    rows, cols, ld = shape
    logits = torch.randn(rows, ld, generator=g, device="cuda").to(torch.bfloat16)
    labels = torch.randint(0, cols, (rows,), generator=g, device="cuda")
    if valid_share < 1:
        labels[torch.rand(rows, generator=g, device="cuda") >= valid_share] = ignore_index
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")

    def dev_fn():
        E.ce_eval(logits, labels, ncols=cols, ignore_index=ignore_index, acc=acc)

    ref = [0.0, 0]

    def ref_fn():
        scores = logits[:, :cols].float()
        y = labels
        if valid_share < 1:                                       # validate_fom: the rows with a target
            loc = (labels != ignore_index).nonzero().squeeze()
            scores, y = scores[loc, :], labels[loc]
        ref[0] += F.cross_entropy(scores, y, reduction="sum").item()
        ref[1] += (scores.max(dim=-1)[1] == y).sum().item()

    acc.zero_()
    dev_fn()
    ref[:] = [0.0, 0]
    ref_fn()
    got = acc.tolist()
    same = got[1] == ref[1]                                       # random bf16 logits tie now and then: max() may pick another column
    assert abs(got[0] - ref[0]) <= 1e-4 * got[2] + 1e-4 * abs(ref[0]), (got, ref)
    return dev_fn, ref_fn, {"loss_sum": got[0], "reference_loss_sum": ref[0], "correct": got[1], "reference_correct": ref[1],
                            "counts_equal": bool(same), "valid_rows": got[2]}


def feat_pair(shape, g):
    from hero_amd import pretrain_eval as E
    rows, cols = shape
    p = torch.randn(rows, cols, generator=g, device="cuda")
    t = torch.randn(rows, cols, generator=g, device="cuda")
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")

    def dev_fn():
        E.feat_eval(p, t, acc=acc)

    ref = [0.0, 0.0]

    def ref_fn():
        ref[0] += torch.sqrt(F.mse_loss(p, t, reduction="none").sum(dim=1)).sum().item()
        ref[1] += F.cosine_similarity(p, t, dim=-1).sum().item()

    acc.zero_()
    dev_fn()
    ref[:] = [0.0, 0.0]
    ref_fn()
    got = acc.tolist()
    assert abs(got[0] - ref[0]) <= 1e-5 * abs(ref[0]) and abs(got[1] - ref[1]) <= 1e-4, (got, ref)
    return dev_fn, ref_fn, {"l2_sum": got[0], "reference_l2_sum": ref[0], "cos_sum": got[1], "reference_cos_sum": ref[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain_eval: needs a GPU (nothing is measured without one)")
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {"bench": "pretrain_eval_ab",
           "timer": "host clock around %d back-to-back scorings of one batch + one device synchronise, per scoring; sides alternate; "
                    "median of %d windows" % (a.inner, a.runs)}
    for name, (dev_fn, ref_fn, info), nbytes in (
            ("mlm", ce_pair(MLM, -1, 1.0, g), MLM[0] * MLM[1] * 2),
            ("fom", ce_pair(FOM, -1, 0.15, g), FOM[0] * FOM[1] * 2),
            ("feat", feat_pair(FEAT, g), 2 * FEAT[0] * FEAT[1] * 4)):
        d, r = ab(dev_fn, ref_fn, a)
        md, mr = statistics.median(d), statistics.median(r)
        out[name] = dict(info, shape=list({"mlm": MLM, "fom": FOM, "feat": FEAT}[name]), device_us_median=round(md, 2), device_us_min=round(min(d), 2),
                         device_us_max=round(max(d), 2), reference_us_median=round(mr, 2), reference_us_min=round(min(r), 2),
                         reference_us_max=round(max(r), 2), reference_over_device=round(mr / md, 2),
                         device_gb_per_s=round(nbytes / (md * 1e-6) / 1e9, 1))
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
