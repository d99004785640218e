#!/usr/bin/env python3
"""Same-process A/B/C of a pre-training micro-step with a FRESH mask draw every step, at bench.py's D3 shape - HERO-base, bf16,
32 videos x 60 frames, 15 subtitles x (4 frames + 20 tokens), vocabulary 50265 padded to 50272, accumulation 2, one GPU - for
the three tasks whose masks PretrainMasker draws on the device (mlm, mfm-nce, fom):

  eager   eager launches on mlm_batch() / mfm_batch() / fom_batch(pairs=False) after advance() + draw(): the compact forms
          read the counts on the host and the model takes its row lists with torch.nonzero - the only way a new mask could
          run before the fixed-capacity forms existed;
  fixed   TrainStep(use_graph=True) on static_batch(task): the fixed-capacity step, hipGraph replay, TrainStep draws in front
          of every replay;
  floor   TrainStep(use_graph=True) on compact batches whose masks never change: the replay `bench.py --workload D3` times.

One sample is the wall time of `--windows` accumulation windows of one task between two device synchronisations, divided by
their micro-steps; sides and tasks alternate sample by sample after `--warmup` untimed rounds (captures and the re-records
that follow another side's new weight copies happen there); the figures are medians over `--samples` samples.  Three models
are alive in this process and every optimiser step refreshes the compute copies of ALL cached weights - the same surcharge on
every side, so each absolute figure sits above bench.py's; read the ratios and differences.  fixed - floor is the price of the
draw kernels, the memo refresh and the rows between the count and the capacity (for MLM zero rows of the vocabulary GEMM:
mlm_rows against the mean masked count is reported).  Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402

TASKS = ("mlm", "mfm-nce", "fom")
MASK_TASK = {"mlm": "mlm", "mfm-nce": "mfm", "fom": "fom"}
MIX = {"mlm": 2, "mfm-nce": 2, "fom": 1}                  # config/pretrain-tv-16gpu.json:11-14 without vsm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--windows", type=int, default=4, help="accumulation windows per sample")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds over the tasks and sides")
    ap.add_argument("--prob", type=float, default=0.15)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.samples * a.windows >= 15
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd import synth
    from hero_amd.pretrain_data import PretrainMasker
    from hero_amd.step import TrainStep
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    hero_amd.set_compute_dtype(torch.bfloat16)
    cfg = json.loads(json.dumps(bench.HERO_BASE))
    cfg["f_config"]["vocab_size"] = 50265
    cfg_path = bench.config_file(cfg, "D3")
    sh = synth.SHAPES["D2"]
    subs = [[(list(range(s * sh["fps"], (s + 1) * sh["fps"])), sh["toks"]) for s in range(sh["subs"])] for _ in range(sh["videos"])]
    host = synth.video_batch(subs, [sh["frames"]] * sh["videos"], bench.VFEAT, 50265, torch.Generator().manual_seed(1))
    dev = synth.to_device({k: v for k, v in host.items() if k != "lengths"}, device)
    ln = {k: torch.as_tensor(v, dtype=torch.int32).to(device) for k, v in host["lengths"].items()}
    opts = dict(learning_rate=3e-5, gradient_accumulation_steps=2)          # config/pretrain-tv-16gpu.json:33-34

    sides = {}
    for name, graph in (("eager", False), ("fixed", True), ("floor", True)):
        model = bench.build_model(device, cfg_path, pretraining=True)
        masker = PretrainMasker.for_batch(host, device, synth.MASK_ID, (3, 50265), 0, mlm_prob=a.prob, mfm_prob=a.prob, fom_prob=a.prob,
                                          seed=12345)
        masker.draw(dev, ln)
        side = dict(model=model, masker=masker, trainer=TrainStep(model, opts=opts, task="mlm", use_graph=graph),
                    samples={t: [] for t in TASKS}, counts=[])
        if name == "fixed":
            for which in ("mlm", "mfm", "fom"):
                masker.draw_fixed(dev, ln, which)
            side["batches"] = {t: masker.static_batch(MASK_TASK[t]) for t in TASKS}
        elif name == "floor":                                               # one draw, compact forms, the same objects every step
            side["batches"] = {"mlm": masker.mlm_batch(), "mfm-nce": masker.mfm_batch(), "fom": masker.fom_batch(pairs=False)}
        sides[name] = side
    accum = opts["gradient_accumulation_steps"]
    compact = {"mlm": lambda m: m.mlm_batch(), "mfm-nce": lambda m: m.mfm_batch(), "fom": lambda m: m.fom_batch(pairs=False)}

    def sample(name, side, task, timed):
        tr, m = side["trainer"], side["masker"]
        HF.set_grad_sink(tr.arena)                       # the arena that was built last is installed: every side needs its own
        if name != "eager":
            tr.prepare(side["batches"][task], task)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.windows * accum):
            if name == "eager":                          # the draw, the host read of the counts and nonzero are this side's step
                m.advance().draw(dev, ln, tasks=(MASK_TASK[task],))
                tr.micro_step(compact[task](m), task=task)
            else:
                tr.micro_step(side["batches"][task], task=task)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if timed:
            side["samples"][task].append(dt / (a.windows * accum) * 1e3)
            if name == "fixed" and task != "fom":
                side["counts"].append((task, m.counts.tolist()))            # outside the timed region

    for r in range(a.warmup + a.samples):
        for task in TASKS:
            for name, side in sides.items():
                sample(name, side, task, r >= a.warmup)
    med = {t: {k: statistics.median(v["samples"][t]) for k, v in sides.items()} for t in TASKS}
    fm = sides["fixed"]["masker"]
    mean_tok = statistics.mean(c[0] for t, c in sides["fixed"]["counts"] if t == "mlm")
    mean_frm = statistics.mean(c[1] for t, c in sides["fixed"]["counts"] if t == "mfm-nce")
    mix = {k: sum(MIX[t] * med[t][k] for t in TASKS) / sum(MIX.values()) for k in sides}
    out = {"bench": "pretrain_replay_ab", "shape": "D3 (HERO-base, 32 videos x 60 frames, vocabulary 50272, accumulation %d)" % accum,
           "dtype": "bf16", "mask_prob": a.prob, "timer": "host clock between device synchronisations, sides and tasks alternating",
           "samples": a.samples, "windows_per_sample": a.windows, "live_models": len(sides),
           "ms_per_step": {t: {k: round(v, 3) for k, v in med[t].items()} for t in TASKS},
           "min_ms_per_step": {t: {k: round(min(v["samples"][t]), 3) for k, v in sides.items()} for t in TASKS},
           "max_ms_per_step": {t: {k: round(max(v["samples"][t]), 3) for k, v in sides.items()} for t in TASKS},
           "eager_over_fixed": {t: round(med[t]["eager"] / med[t]["fixed"], 3) for t in TASKS},
           "fixed_minus_floor_ms": {t: round(med[t]["fixed"] - med[t]["floor"], 3) for t in TASKS},
           "mix_2_2_1_ms_per_step": {k: round(v, 3) for k, v in mix.items()},
           "mix_eager_over_fixed": round(mix["eager"] / mix["fixed"], 3), "mix_fixed_minus_floor_ms": round(mix["fixed"] - mix["floor"], 3),
           "fixed_faster_than_eager": {t: med[t]["fixed"] < med[t]["eager"] for t in TASKS},
           "mlm_rows": fm.mlm_rows, "mean_masked_tokens": round(mean_tok, 1), "mlm_zero_row_share": round(fm.mlm_rows / mean_tok - 1.0, 3),
           "mfm_rows": fm.mfm_rows, "mean_masked_frames": round(mean_frm, 1), "overflow": fm.overflow.tolist(),
           "fixed_counts": dict(sides["fixed"]["trainer"].counts), "floor_counts": dict(sides["floor"]["trainer"].counts),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
