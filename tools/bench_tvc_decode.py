#!/usr/bin/env python3
"""Same-process A/B of captioning greedy decode: TvcGenerator.greedy_decode on given encoder outputs, three sides -
    uncached       every step runs the 2-layer decoder over the whole [N, max_step] id buffer (the default)
    cached         kv_cache=True: one row per caption and step on hero_dec_attention_step / _row, cross K|V projected once
    cached_graph   the same step captured once and replayed max_step times
at the recipe's geometry: HERO-base (hidden 768, 12 heads, 2 decoder layers, vocabulary 50272), bf16, 40 captions, Lv = 20 segment
frames, max_step = 30.

What is timed: one whole greedy decode - state set-up, max_step steps, the single host transfer of the ids at its end - on encoder
outputs that are given, so the hierarchical encoder (the same on every side) is not in it.  The model is in eval mode.  One
HIP-event pair per decode, the sides alternating, medians over `--runs` decodes after 3 warm-up decodes of each (the graph side
captures in its first).  The ids of the sides are compared on every run and the counts are part of the line.  The weights are
random, so the bf16 scores over 50272 columns are close to flat and hold near and exact ties: one rounding that differs between
the sides (another GEMM tile route at M = N rows, another summation order in the attention) flips an arg-max, and everything
behind it in that caption.  Equal ids are therefore NOT expected between uncached and cached here (with trained weights they
are what tests/test_gpu_tvc_decode.py pins); what is expected is equal ids between the cached sides, and close scores, which the
tool measures untimed under teacher forcing on random ids.  Prints one JSON line; `--out FILE` also writes it."""
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
    ap.add_argument("--shape", default="40,20,30", help="captions, Lv, max_step")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import hero_amd
    from hero_amd.model import HeroForTvc, TvcGenerator
    N, Lv, max_step = (int(x) for x in a.shape.split(","))
    cfg = {"f_config": dict(BASE, num_hidden_layers=1, vocab_size=50272), "c_config": dict(BASE, num_hidden_layers=1),
           "d_config": dict(BASE, num_hidden_layers=2, max_position_embeddings=1024, type_vocab_size=1, vocab_size=50272)}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cfg, f)                                # the encoders are built (one layer each) but never run here
    torch.manual_seed(0)
    hero_amd.set_compute_dtype(torch.bfloat16)
    model = HeroForTvc.from_pretrained(f.name, {}, vfeat_dim=64, max_frm_seq_len=32, lsr=0.1).cuda()
    os.unlink(f.name)
    model.eval()
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(N, Lv, 768, generator=g).cuda()
    lens_v = torch.randint(1, Lv + 1, (N,), generator=g)
    lens_v[0] = Lv
    batch = {"cap_attn_mask": (torch.arange(Lv).unsqueeze(0) < lens_v.unsqueeze(1)).long().cuda()}
    bos, eos = 0, -1                                     # no id is cut: the sides are compared position by position
    sides = {"uncached": TvcGenerator(model, max_step, bos, eos),
             "cached": TvcGenerator(model, max_step, bos, eos, kv_cache=True),
             "cached_graph": TvcGenerator(model, max_step, bos, eos, kv_cache=True, use_graph=True)}

    def timed(gen):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ids = gen.greedy_decode(batch, encoder_outputs=enc)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, ids

    # untimed: the cached step's scores against the uncached decoder's under teacher forcing on random ids, both bf16
    with torch.no_grad():
        ids = torch.randint(3, 50272, (N, max_step), generator=g).cuda()
        full = model.decode(enc, batch["cap_attn_mask"], ids, torch.arange(max_step).unsqueeze(0).cuda(), None, compute_loss=False)
        state = model.init_decode_state(enc, batch["cap_attn_mask"], max_step)
        steps = torch.stack([model.decode_step(state, ids[:, t]).float() for t in range(max_step)], dim=1)
        score_err = float((steps - full).abs().max() / full.abs().max())
        del full, steps, state

    for _ in range(3):
        for gen in sides.values():
            timed(gen)
    times = {k: [] for k in sides}
    same = {k: 0 for k in sides if k != "uncached"}
    graph_same, pos_same = 0, []
    for _ in range(a.runs):
        got = {}
        for k, gen in sides.items():
            us, got[k] = timed(gen)
            times[k].append(us)
        for k in same:
            same[k] += int(got[k] == got["uncached"])
        graph_same += int(got["cached_graph"] == got["cached"])
        pos_same.append(sum(x == y for r, s in zip(got["cached"], got["uncached"]) for x, y in zip(r, s)) / float(N * max_step))
    med = {k: statistics.median(v) for k, v in times.items()}
    line = json.dumps({"bench": "tvc_decode_ab", "shape_N_Lv_maxstep": [N, Lv, max_step],
                       "model": "HERO-base decoder, 2 layers, vocab 50272", "dtype": "bf16", "mode": "eval, greedy, no early exit",
                       "what": "one greedy decode on given encoder outputs: state set-up + max_step steps + id transfer",
                       "timer": "HIP events, one pair per decode, sides alternating", "runs": a.runs,
                       "uncached_us_median": round(med["uncached"], 1), "uncached_us_min": round(min(times["uncached"]), 1),
                       "cached_us_median": round(med["cached"], 1), "cached_us_min": round(min(times["cached"]), 1),
                       "cached_graph_us_median": round(med["cached_graph"], 1), "cached_graph_us_min": round(min(times["cached_graph"]), 1),
                       "uncached_over_cached": round(med["uncached"] / med["cached"], 2),
                       "uncached_over_cached_graph": round(med["uncached"] / med["cached_graph"], 2),
                       "runs_with_ids_equal_to_uncached": same, "runs_with_graph_ids_equal_to_cached": graph_same,
                       "cached_positions_equal_to_uncached": round(statistics.median(pos_same), 4),
                       "teacher_forced_scores_cached_vs_uncached_rel_err": float("%.3e" % score_err),
                       "graphs_captured": sides["cached_graph"].counts["captures"],
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
