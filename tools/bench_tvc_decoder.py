#!/usr/bin/env python3
"""Same-process A/B of the captioning decoder: HeroForTvc.decode on the HIP kernels (hero_dec_attention_*, hero_smooth_ce_*,
the existing GEMM / LayerNorm nodes) against the PyTorch formulation the same module keeps (`fused_decoder = False`), forward +
backward of the mean caption loss, at the recipe's geometry: HERO-base (hidden 768, 12 heads, 2 decoder layers, vocabulary 50272),
4 videos x 10 captions, Lt = 25 caption positions, Lv = 20 segment frames, lsr 0.1.

What is timed: the caption embedding + emb_LayerNorm, the two decoder layers, the tied vocabulary projection and the loss, with
their backward - on encoder outputs that are a leaf tensor, so the hierarchical encoder (the same kernels on both sides) is not in
it.  The fused side computes in bf16 with fp32 accumulation; the PyTorch side runs the module's fp32 formulation under
torch.autocast(bfloat16), which is how a PyTorch user would run it in bf16.  One HIP-event pair per run, the two sides alternating,
medians over `--runs` runs after 5 warm-up runs of each.  Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = dict(attention_probs_dropout_prob=0.1, hidden_act="gelu", hidden_dropout_prob=0.1, hidden_size=768, initializer_range=0.02,
            intermediate_size=3072, max_position_embeddings=514, num_attention_heads=12, type_vocab_size=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="40,25,20", help="captions, Lt, Lv")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import hero_amd
    from hero_amd.model import HeroForTvc
    N, Lt, Lv = (int(x) for x in a.shape.split(","))
    cfg = {"f_config": dict(BASE, num_hidden_layers=1, vocab_size=50272), "c_config": dict(BASE, num_hidden_layers=1),
           "d_config": dict(BASE, num_hidden_layers=2, max_position_embeddings=1024, type_vocab_size=1, vocab_size=50272)}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cfg, f)                                # the encoders are built (one layer each) but never run here
    torch.manual_seed(0)
    hero_amd.set_compute_dtype(torch.bfloat16)
    model = HeroForTvc.from_pretrained(f.name, {}, vfeat_dim=64, max_frm_seq_len=32, lsr=0.1).cuda()
    os.unlink(f.name)
    model.train()                                        # dropout 0.1 on, as in training (each side draws its own masks)
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(N, Lv, 768, generator=g).cuda().requires_grad_(True)
    lens_v = torch.randint(1, Lv + 1, (N,), generator=g)
    lens_v[0] = Lv
    mask = (torch.arange(Lv).unsqueeze(0) < lens_v.unsqueeze(1)).long().cuda()
    lens_t = torch.randint(4, Lt + 1, (N,), generator=g)
    lens_t[0] = Lt
    valid = torch.arange(Lt).unsqueeze(0) < lens_t.unsqueeze(1)
    ids = torch.where(valid, torch.randint(3, 50272, (N, Lt), generator=g), torch.ones((), dtype=torch.long)).cuda()
    labels = torch.where(valid, torch.randint(3, 50272, (N, Lt), generator=g), -torch.ones((), dtype=torch.long)).cuda()
    pos = torch.arange(Lt).unsqueeze(0).cuda()
    batch = {"cap_attn_mask": mask, "cap_input_ids": ids, "cap_pos_ids": pos, "cap_tgt_ids": labels}
    model.encode = lambda b: enc                         # caption_loss on given encoder outputs

    def fused():
        model.fused_decoder = True
        model.caption_loss(batch).backward()

    def pytorch():
        model.fused_decoder = False
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model.caption_loss(batch)
        loss.backward()

    def timed(fn):
        model.zero_grad(set_to_none=True)
        enc.grad = None
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
    line = json.dumps({"bench": "tvc_decoder_ab", "shape_N_Lt_Lv": [N, Lt, Lv], "model": "HERO-base decoder, 2 layers, vocab 50272, lsr 0.1",
                       "dtype": "bf16 (PyTorch side: fp32 formulation under autocast(bfloat16))", "mode": "eager, dropout on",
                       "what": "embedding + 2 decoder layers + vocabulary projection + loss, forward + backward",
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
