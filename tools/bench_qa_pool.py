#!/usr/bin/env python3
"""Same-process A/B of the video-QA head: hero_amd.qa.QaPoolFn against the PyTorch formulation
(HeroForVideoQA.get_modularized_video's ops on a sliced copy of the frame rows), forward + backward, at the TVQA recipe's
geometry (Nv, A, L, Lqa, D) = (4, 5, 100, 120, 768) in bf16.  One HIP-event pair per run, the two sides alternating,
medians over 20 runs after 5 warm-up runs of each.  Prints one line; `--out FILE` also writes it there.

What it does not time: the two weight vectors are plain tensors here, so QaPoolFn returns their gradients to autograd (the
fixed-order column sum, then a view) where the training step adds them straight into the gradient arena (HF.SINK) - the
parameter-gradient route of TrainStep is not in this figure.  The PyTorch side pays autograd's accumulation likewise."""
import argparse
import statistics
import sys

import torch
import torch.nn.functional as F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4,5,100,120,768")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    from hero_amd.qa import QaPoolFn
    Nv, A, L, Lqa, D = (int(x) for x in a.shape.split(","))
    g = torch.Generator().manual_seed(0)
    seq = torch.randn(Nv * A, L + Lqa, D, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    wq = (torch.randn(1, D, generator=g) * 2 / D ** 0.5).cuda().requires_grad_(True)
    ws = (torch.randn(1, D, generator=g) * 2 / D ** 0.5).cuda().requires_grad_(True)
    m = torch.ones(Nv * A, L, device="cuda")
    m[-A:, L - L // 4:] = 0
    dqa, dse = torch.randn(Nv, A, D, generator=g).cuda(), torch.randn(Nv, L, D, generator=g).cuda()

    def fused():
        qa, se = QaPoolFn.apply(seq, m, wq, ws, A, L)
        torch.autograd.backward([qa, se], [dqa, dse])

    def pytorch():
        X = seq[:, :L].float().view(Nv, A, L, D)
        mk = m.view(Nv, A, L, 1)
        att_se = F.softmax(F.linear(X, ws) * mk + (1 - mk) * -1e4, dim=1)
        att_qa = F.softmax(F.linear(X, wq) * mk + (1 - mk) * -1e4, dim=2)
        se = torch.einsum("vqlm,vqld->vlmd", att_se, X).squeeze(2)
        qa = torch.einsum("vqlm,vqld->vqmd", att_qa, X).squeeze(2)
        torch.autograd.backward([qa, se], [dqa, dse])

    def timed(fn):
        for t in (seq, wq, ws):
            t.grad = None
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
    line = ("qa_pool A/B (Nv, A, L, Lqa, D) = (%d, %d, %d, %d, %d) bf16, forward + backward, HIP events, median of %d: "
            "QaPoolFn %.1f us (min %.1f)  PyTorch formulation %.1f us (min %.1f)  ratio %.2fx  [%s]"
            % (Nv, A, L, Lqa, D, a.runs, statistics.median(tf), min(tf), statistics.median(tp), min(tp),
               statistics.median(tp) / statistics.median(tf), torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
