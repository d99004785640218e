#!/usr/bin/env python3
"""Same-process A/B/C of the reference's TVR recipe (config/train-tvr-8gpu.json: drop_svmr_prob 0.8) at bench.py's D2 shape -
HERO-base, bf16, 32 videos per micro-step, accumulation 2, one GPU:

  eager   drop_svmr_prob 0.8, eager launches, the model draws on the host: how the recipe ran before the start / end term had a
          device gate (graph mode refused it) - the baseline;
  gated   the same recipe under use_graph=True: hipGraph replay, the term behind hero_amd.head.StEdGate;
  floor   drop_svmr_prob 0 under use_graph=True: the replay bench.py times.

One sample is the wall time of `--windows` accumulation windows between two device synchronisations, divided by their
micro-steps; the three sides alternate sample by sample, after `--warmup` untimed rounds; the figures are medians over `--samples`
samples (>= 15 windows each).  Three models are alive in this process and every optimiser step refreshes the compute copies of
ALL cached weights, the other sides' included - the same surcharge on every side, so each absolute figure sits above bench.py's;
read the differences.  gated - floor is the price of launching the gated-off kernels on 80 % of the steps (they zero dctx, and
the video_query_linear GEMMs run on zeros); a captured step cannot skip them.  Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--windows", type=int, default=4, help="accumulation windows per sample")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds over the three sides")
    ap.add_argument("--drop", type=float, default=0.8)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.samples * a.windows >= 15
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.step import TrainStep
    from hero_amd.synth import make_batch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    hero_amd.set_compute_dtype(torch.bfloat16)
    cfg = bench.config_file(bench.HERO_BASE, "D2")
    batch = make_batch("D2", vfeat_dim=bench.VFEAT, vocab=50272, seed=1, device=device)
    random.seed(0)
    sides = {}
    for name, drop, graph in (("eager", a.drop, False), ("gated", a.drop, True), ("floor", 0.0, True)):
        model = bench.build_model(device, cfg)
        model.drop_svmr_prob = drop
        # the set of used parameters changes from window to window under the eager recipe: no static_usage there
        trainer = TrainStep(model, use_graph=graph, static_usage=drop == 0.0, uniform_shapes=True)
        sides[name] = dict(model=model, trainer=trainer, samples=[])
    accum = sides["floor"]["trainer"].opts.gradient_accumulation_steps

    def sample(side, timed):
        tr = side["trainer"]
        HF.set_grad_sink(tr.arena)                       # the arena that was built last is installed: eager launches need their own
        tr.prepare(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.windows * accum):
            tr.micro_step(batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if timed:
            side["samples"].append(dt / (a.windows * accum) * 1e3)

    for r in range(a.warmup + a.samples):
        for side in sides.values():
            sample(side, r >= a.warmup)
    med = {k: statistics.median(v["samples"]) for k, v in sides.items()}
    gate = sides["gated"]["model"].st_ed_gate
    out = {"bench": "tvr_recipe_ab", "shape": "D2 (HERO-base, 32 videos, accumulation %d)" % accum, "dtype": "bf16",
           "drop_svmr_prob": a.drop, "timer": "host clock between device synchronisations, sides alternating",
           "samples": a.samples, "windows_per_sample": a.windows, "live_models": len(sides),
           "eager_ms_per_step": round(med["eager"], 3), "gated_graph_ms_per_step": round(med["gated"], 3),
           "floor_graph_ms_per_step": round(med["floor"], 3),
           "min_ms_per_step": {k: round(min(v["samples"]), 3) for k, v in sides.items()},
           "max_ms_per_step": {k: round(max(v["samples"]), 3) for k, v in sides.items()},
           "gated_minus_floor_ms": round(med["gated"] - med["floor"], 3),
           "gated_minus_floor_pct_of_step": round(100.0 * (med["gated"] - med["floor"]) / med["floor"], 2),
           "eager_over_gated": round(med["eager"] / med["gated"], 2),
           "gated_counts": dict(sides["gated"]["trainer"].counts), "floor_counts": dict(sides["floor"]["trainer"].counts),
           "gated_has_gate": gate is not None, "floor_has_gate": sides["floor"]["model"].st_ed_gate is not None,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
