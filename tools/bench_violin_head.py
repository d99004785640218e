#!/usr/bin/env python3
"""Same-process A/B of the VIOLIN head: hero_amd.violin.FramePoolFn + BceHeadFn against their PyTorch formulation
(HeroForViolin.get_modularized_video's ops on a sliced copy of the frame rows; linear_2 -> sigmoid -> binary_cross_entropy),
forward + backward, at the recipe's geometry (S, L, Lq, D) = (8, 100, 30, 768) in bf16 (4 videos x 2 statements,
max_clip_len 100; the tail's K is 2 D).  One HIP-event pair per run covers pool and tail, the two sides alternating, medians
over 20 runs after 5 warm-up runs of each.  Prints one JSON line; `--out FILE` also writes it there.

What it does not time: linear_1 + GELU + LayerNorm between pool and tail (the same kernels on both sides), and the
gradient-arena route of TrainStep - the weights are plain tensors here, so both sides return their gradients to autograd."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="8,100,30,768")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    from hero_amd.violin import BceHeadFn, FramePoolFn
    S, L, Lq, D = (int(x) for x in a.shape.split(","))
    K = 2 * D
    g = torch.Generator().manual_seed(0)
    seq = torch.randn(S, L + Lq, D, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    w = (torch.randn(1, D, generator=g) * 2 / D ** 0.5).cuda().requires_grad_(True)
    m = torch.ones(S, L, device="cuda")
    m[-2:, L - L // 4:] = 0
    dpooled = torch.randn(S, D, generator=g).cuda()
    h = torch.randn(S, K, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    w2 = (torch.randn(1, K, generator=g) * 2 / K ** 0.5).cuda().requires_grad_(True)
    b2 = torch.zeros(1, device="cuda", requires_grad=True)
    t = torch.randint(0, 2, (S,), generator=g).cuda()
    one = torch.ones((), device="cuda")

    def fused():
        pooled = FramePoolFn.apply(seq, m, w, L)
        loss, _ = BceHeadFn.apply(h, w2, b2, t)
        torch.autograd.backward([pooled, loss], [dpooled, one])

    def pytorch():
        X = seq[:, :L].float()
        mk = m.unsqueeze(-1)
        att = F.softmax(F.linear(X, w) * mk + (1 - mk) * -1e4, dim=1)
        pooled = torch.einsum("vlm,vld->vmd", att, X).squeeze(1)
        z = F.linear(h.float(), w2, b2)
        loss = F.binary_cross_entropy(torch.sigmoid(z).squeeze(-1), t.float(), reduction="mean")
        torch.autograd.backward([pooled, loss], [dpooled, one])

    def timed(fn):
        for x in (seq, w, h, w2, b2):
            x.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(5):
        timed(fused), timed(pytorch)
    tf, tp = [], []
    for _ in range(a.runs):
        tf.append(timed(fused))
        tp.append(timed(pytorch))
    line = json.dumps({"bench": "violin_head_ab", "shape_S_L_Lq_D": [S, L, Lq, D], "K": K, "dtype": "bf16", "what": "pool + tail, forward + backward",
                       "timer": "HIP events, one pair per run, sides alternating", "runs": a.runs,
                       "fused_us_median": round(statistics.median(tf), 1), "fused_us_min": round(min(tf), 1),
                       "pytorch_us_median": round(statistics.median(tp), 1), "pytorch_us_min": round(min(tp), 1),
                       "pytorch_over_fused": round(statistics.median(tp) / statistics.median(tf), 2),
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
