#!/usr/bin/env python3
"""A/B of the full-corpus retrieval paths at the TVR-val shape (run on the GPU box):

    python tools/bench_retrieval.py [--videos 2179] [--frames 100] [--dim 768] [--queries 80] [--batches 20] [--warmup 3] [--postprocess]

A synthetic index (seeded frame embeddings of `--videos` clips of different lengths, stored bf16 like the bf16 encoder's
output; HERO-base head weights from a seed) and `--batches` different query batches; `CorpusIndex.search` (HIP kernels) and
`search_torch` (the reference's formulation) are timed in the same process, alternating, one HIP-event pair per batch, after
`--warmup` batches of each; medians are reported.  The query encoder is replaced by given modularised queries - it is the same
call in both paths and not what is compared.  Peak memory is torch's peak allocation above the index during one path's batches.

`--postprocess` adds a second A/B on the fused path's outputs: `postprocess` + `RecallMeter.update` (hero_moment_nms,
hero_first_hit; one HIP-event pair per batch) against `postprocess_host` (the reference's NMS restated in Python; wall clock,
given host copies made before its clock starts, and without any metric work - both choices favour the baseline), alternating,
same warm-up, medians; plus how many candidates survive.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


class Head(torch.nn.Module):
    """The part of HeroForVcmr a search touches, with HERO-base shapes and seeded weights."""

    def __init__(self, dim, gen):
        super().__init__()
        from hero_amd.model.vcmr import HeroForVcmr
        self.lw_neg_ctx = self.lw_neg_q = 8.0
        self.training = False
        self.gather_gpus = False
        self.video_query_linear = torch.nn.Linear(dim, dim)
        self.video_st_predictor = torch.nn.Conv1d(1, 1, 5, padding=2, bias=False)
        self.video_ed_predictor = torch.nn.Conv1d(1, 1, 5, padding=2, bias=False)
        self.q_feat_attn = None
        with torch.no_grad():
            self.video_query_linear.weight.copy_(torch.randn(dim, dim, generator=gen) * dim ** -0.5)
            self.video_query_linear.bias.copy_(torch.randn(dim, generator=gen) * 0.1)
            self.video_st_predictor.weight.copy_(torch.randn(1, 1, 5, generator=gen) * 0.5)
            self.video_ed_predictor.weight.copy_(torch.randn(1, 1, 5, generator=gen) * 0.5)
        for name in ("get_pred_from_raw_query", "get_pred_from_mod_query", "_get_st_ed_prob", "get_video_level_scores"):
            setattr(self, name, getattr(HeroForVcmr, name).__get__(self))
        self._conv5 = HeroForVcmr._conv5
        self.mod_q = None

    def encode_txt_inputs(self, *a, **k):
        return self.mod_q


def postprocess_ab(HR, index, model, ids, queries, gts, args, gen):
    """postprocess + RecallMeter.update (device) against postprocess_host (host) on the outputs of the fused search."""
    meter = HR.RecallMeter(device="cuda")
    times = {"device": [], "host": []}
    survivors = {"vcmr": [], "svmr": []}
    for i, (q, gt) in enumerate(zip(queries, gts)):
        model.mod_q = q
        out = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt)
        start = torch.rand(args.queries, generator=gen) * args.frames
        gt_ts = torch.stack([start, start + 3 + 9 * torch.rand(args.queries, generator=gen)], dim=1).to("cuda")
        desc_type = torch.randint(0, 3, (args.queries,), generator=gen).to("cuda")
        out_host = {k: v.cpu() for k, v in out.items()}
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        post = HR.postprocess(out)
        meter.update(post, gt, gt_ts, desc_type)
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = HR.postprocess_host(out_host)
        t1 = time.perf_counter()
        for task in survivors:
            if not torch.equal(post[task + "_nms_st"].cpu(), host[task + "_nms_st"]):
                raise SystemExit("bench_retrieval: postprocess and postprocess_host disagree on %s of batch %d" % (task, i))
        if i >= args.warmup:
            times["device"].append(e0.elapsed_time(e1))
            times["host"].append((t1 - t0) * 1e3)
            for task in survivors:
                survivors[task].append(float(post[task + "_nms_count"].float().mean()))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"ms_postprocess": {k: round(v, 3) for k, v in med.items()},
            "ms_postprocess_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
            "postprocess_candidates": int(out["vcmr_st"].shape[1]), "nms_thd": 0.5, "max_after_nms": 100,
            "mean_survivors": {k: round(statistics.mean(v), 1) for k, v in survivors.items()},
            "speedup_postprocess_device_over_host": round(med["host"] / med["device"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2179)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=80)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--postprocess", action="store_true", help="also time postprocess + RecallMeter.update against postprocess_host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval: needs a GPU (a CPU run gives no time)")
    from hero_amd import retrieval as HR
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    model = Head(args.dim, gen).to(dev).eval()
    lens = torch.randint(args.frames // 3, args.frames + 1, (args.videos,), generator=gen)
    mask = (torch.arange(args.frames).view(1, -1) < lens.view(-1, 1)).long()
    ctx = (torch.randn(args.videos, args.frames, args.dim, generator=gen) * mask.unsqueeze(-1)).to(torch.bfloat16)
    index = HR.CorpusIndex(ctx.to(dev), mask.to(dev))
    del ctx
    n = args.batches + args.warmup
    queries = [torch.randn(args.queries, args.dim, generator=gen).to(dev) for _ in range(n)]
    gts = [torch.randint(0, args.videos, (args.queries,), generator=gen).to(dev) for _ in range(n)]
    ids = torch.zeros(args.queries, 4, dtype=torch.long, device=dev)
    paths = {"fused": index.search, "torch": index.search_torch}
    times = {k: [] for k in paths}
    peak = {}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i in range(n):
        for name, fn in paths.items():                      # alternating: both see the same clocks and neighbours
            model.mod_q = queries[i]
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(model, ids, None, torch.ones_like(ids), gt_vidx=gts[i])
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            del out
    med = {k: statistics.median(v) for k, v in times.items()}
    extra = postprocess_ab(HR, index, model, ids, queries, gts, args, gen) if args.postprocess else {}
    print(json.dumps({
        "tool": "bench_retrieval", "device": torch.cuda.get_device_name(0), "videos": args.videos, "frames": args.frames, "dim": args.dim,
        "queries_per_batch": args.queries, "timed_batches": args.batches, "warmup_batches": args.warmup, "corpus_dtype": "bfloat16",
        "ms_per_query_batch": {k: round(v, 3) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
        "queries_per_s": {k: round(args.queries / v * 1e3, 1) for k, v in med.items()},
        "peak_mem_mb_above_index": {k: round(v / 2 ** 20, 1) for k, v in peak.items()},
        "index_mb": round(base / 2 ** 20, 1), "speedup_fused_over_torch": round(med["torch"] / med["fused"], 2), **extra}))


if __name__ == "__main__":
    main()
