#!/usr/bin/env python3
"""A/B of the full-corpus retrieval paths at the TVR-val shape (run on the GPU box):

    python tools/bench_retrieval.py [--videos 2179] [--frames 100] [--dim 768] [--queries 80] [--batches 20] [--warmup 3]

A synthetic index (seeded frame embeddings of `--videos` clips of different lengths, stored bf16 like the bf16 encoder's
output; HERO-base head weights from a seed) and `--batches` different query batches; `CorpusIndex.search` (HIP kernels) and
`search_torch` (the reference's formulation) are timed in the same process, alternating, one HIP-event pair per batch, after
`--warmup` batches of each; medians are reported.  The query encoder is replaced by given modularised queries - it is the same
call in both paths and not what is compared.  Peak memory is torch's peak allocation above the index during one path's batches.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2179)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=80)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    print(json.dumps({
        "tool": "bench_retrieval", "device": torch.cuda.get_device_name(0), "videos": args.videos, "frames": args.frames, "dim": args.dim,
        "queries_per_batch": args.queries, "timed_batches": args.batches, "warmup_batches": args.warmup, "corpus_dtype": "bfloat16",
        "ms_per_query_batch": {k: round(v, 3) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
        "queries_per_s": {k: round(args.queries / v * 1e3, 1) for k, v in med.items()},
        "peak_mem_mb_above_index": {k: round(v / 2 ** 20, 1) for k, v in peak.items()},
        "index_mb": round(base / 2 ** 20, 1), "speedup_fused_over_torch": round(med["torch"] / med["fused"], 2)}))


if __name__ == "__main__":
    main()
