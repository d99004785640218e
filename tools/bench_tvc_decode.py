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
tool measures untimed under teacher forcing on random ids.  Prints one JSON line; `--out FILE` also writes it.

`--beam B` measures beam search instead, on the same model, inputs and timer, five sides alternating -
    greedy_cached[_graph]   the cached greedy decode above, for scale
    beam_fused[_graph]      TvcGenerator.beam_decode on the kernels' route: N * B rows, hero_beam_select, attention through the
                            ancestry table - no cache copy, the encoder K|V projected once for N captions
    beam_torch              the formulation in PyTorch ops around the SAME cached step (class TorchBeam below): the encoder rows
                            replicated B times, log_softmax + topk over [N, B * 50272], index_select of every layer's cache by
                            parent in every step.  Eager only: torch.topk over slices this long zeroes its counters with
                            memset nodes, which a captured hipGraph does not order like the kernels around them on this stack
                            (tests/test_cpu_boundary.py::test_no_memset_nodes_in_the_kernel_library) - replayed, it can hand
                            index_select indices that were never written.  Graph replay is "not available" for this side.
(eos = 2 here: the selection needs a real id; with random weights it is rarely chosen).  What is timed is again one whole
decode on given encoder outputs.  The sides' ids are compared; with random weights equal ids are not expected between the
fused and the PyTorch side (near ties, see above), between the fused side and its own graph replay they are.

`--sample S [--top-k K --top-p P --temperature T]` measures sampled decoding instead, four sides alternating -
    greedy_cached           the cached greedy decode above, for scale
    sample_fused[_graph]    TvcGenerator.sample_decode on the kernels' route: N * S rows on the beam state, one hero_sample_select
                            per step, the seed a device word
    sample_torch            the same draw in PyTorch ops (hero_amd.model.tvc.sample_select_torch: sort of the whole vocabulary,
                            cumulative sum, hash and arg-max as tensor ops, the per-row hash keys made on the host) around the
                            SAME cached step and the same shared encoder keys.  Eager only: its keys are host values.
Every run draws with a new seed, the same on all sampling sides.  The fused sides must agree with each other on every run; the
fused and the PyTorch side draw the same tokens wherever fp32 decides them, which the line reports as a share of captions."""
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


class TorchBeam(object):
    """Beam search written in PyTorch ops around the cached decode step, as it can be written without hero_beam_select and the
    beam entry points of the attention kernel: a decode state over N * B replicated encoder rows, and per step log_softmax,
    topk over the caption's B * V candidates and an index_select of every layer's cache by parent.  Same rules as
    TvcGenerator.beam_decode (a finished beam offers only eos at its score; length-normalised pick), ties as topk leaves them."""

    def __init__(self, model, max_step, B, bos, eos):
        self.model, self.max_step, self.B, self.bos, self.eos = model, max_step, B, bos, eos
        self.state = None

    def _setup(self, enc, mask):
        B, dev = self.B, enc.device
        N, V = enc.shape[0], self.model.config.f_config.vocab_size
        R = N * B
        self.state = self.model.init_decode_state(enc.repeat_interleave(B, 0), mask.repeat_interleave(B, 0), self.max_step)
        self.cum = torch.empty(R, dtype=torch.float32, device=dev)
        self.fin = torch.empty(R, dtype=torch.bool, device=dev)
        self.len, self.last = (torch.empty(R, dtype=torch.long, device=dev) for _ in range(2))
        self.ids = torch.empty((R, self.max_step), dtype=torch.long, device=dev)
        self.base = (torch.arange(N, device=dev) * B).unsqueeze(1)
        self.cum0 = torch.full((N, B), -1.0e30, device=dev)
        self.cum0[:, 0] = 0.0
        self.eos_only = torch.full((1, V), float("-inf"), device=dev)
        self.eos_only[0, self.eos] = 0.0

    def _reset(self, enc, mask):
        self.model.refill_decode_state(self.state, enc.repeat_interleave(self.B, 0), mask.repeat_interleave(self.B, 0))
        self.cum.copy_(self.cum0.view(-1))
        self.fin.zero_()
        self.len.zero_()
        self.ids.zero_()
        self.last.fill_(self.bos)

    def _step(self):
        st, B = self.state, self.B
        scores = self.model.decode_step(st, self.last)
        R, V = scores.shape
        lp = torch.where(self.fin.unsqueeze(1), self.eos_only, torch.log_softmax(scores.float(), dim=-1))
        val, idx = (self.cum.unsqueeze(1) + lp).view(R // B, B * V).topk(B, dim=1)
        idx = idx.clamp(0, B * V - 1)                            # the gathers below have no bounds check of their own
        rows, v = (self.base + idx // V).view(-1), (idx % V).view(-1)
        for c in st.cache:
            c.copy_(c.index_select(0, rows))
        ids = self.ids.index_select(0, rows)
        ids.scatter_(1, (st.pos - 1).long().view(1, 1).expand(R, 1), v.unsqueeze(1))
        self.ids.copy_(ids)
        was = self.fin.index_select(0, rows)
        self.len.copy_(self.len.index_select(0, rows) + (~was).long())
        self.fin.copy_(was | (v == self.eos))
        self.cum.copy_(val.view(-1))
        self.last.copy_(v)

    @torch.no_grad()
    def decode(self, batch, enc, length_penalty=1.0):
        mask = batch["cap_attn_mask"]
        if self.state is None:
            self._setup(enc, mask)
        self._reset(enc, mask)
        for _ in range(self.max_step):
            self._step()
        N, B = enc.shape[0], self.B
        norm = self.cum.view(N, B) / self.len.view(N, B).clamp(min=1).float() ** length_penalty
        rows = self.base.view(-1) + norm.argmax(dim=1)
        return self.ids[rows].tolist()


class TorchSample(object):
    """Sampled decoding written around the cached decode step with hero_amd.model.tvc.sample_select_torch in place of
    hero_sample_select: the same N * S-row state over N blocks of encoder keys, int64 tables, the pick of
    TvcGenerator.sample_decode."""

    def __init__(self, model, max_step, S, bos, eos, params):
        self.model, self.max_step, self.S, self.bos, self.eos, self.params = model, max_step, S, bos, eos, params
        self.state = None

    @torch.no_grad()
    def decode(self, batch, enc, seed, length_penalty=1.0):
        from hero_amd.model.tvc import BeamTables, sample_select_torch
        mask, S = batch["cap_attn_mask"], self.S
        N = enc.shape[0]
        if self.state is None:
            self.state = self.model.init_decode_state(enc, mask, self.max_step, S, beam_tables=True)
            self.tb = BeamTables(N, S, self.max_step, enc.device, False)
        self.model.refill_decode_state(self.state, enc, mask)
        tb = self.tb.reset_sampling()
        last = torch.full((N * S,), self.bos, dtype=torch.long, device=enc.device)
        for t in range(self.max_step):
            last, _ = sample_select_torch(self.model.decode_step(self.state, last), tb, t, self.eos, seed, *self.params)
        norm = tb.cum.view(N, S) / tb.len.view(N, S).clamp(min=1).float() ** length_penalty
        best = torch.sort(norm, dim=1, descending=True, stable=True).indices[:, 0]
        return tb.ids[torch.arange(N, device=enc.device) * S + best].tolist()


def main_sample(a, model, batch, enc, N, Lv, max_step):
    from hero_amd.model import TvcGenerator
    S, bos, eos = a.sample, 0, 2
    params = (a.temperature, a.top_k, a.top_p)
    greedy = TvcGenerator(model, max_step, bos, eos, kv_cache=True)
    fused = {"sample_fused": TvcGenerator(model, max_step, bos, eos, kv_cache=True),
             "sample_fused_graph": TvcGenerator(model, max_step, bos, eos, kv_cache=True, use_graph=True)}
    plain = TorchSample(model, max_step, S, bos, eos, params)
    run = {"greedy_cached": lambda seed: greedy.greedy_decode(batch, encoder_outputs=enc)}
    run.update({k: (lambda seed, g=g: g.sample_decode(batch, S, *params, seed=seed, encoder_outputs=enc)) for k, g in fused.items()})
    run["sample_torch"] = lambda seed: [greedy.cut_eos(r) for r in plain.decode(batch, enc, seed)]

    def timed(fn, seed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ids = fn(seed)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, ids

    for i in range(3):
        for fn in run.values():
            timed(fn, 1000 + i)
    times = {k: [] for k in run}
    same = {"sample_fused_graph_vs_sample_fused": 0, "sample_fused_vs_sample_torch": 0}
    cap_same = []
    for i in range(a.runs):
        got = {}
        for k, fn in run.items():
            us, got[k] = timed(fn, i)
            times[k].append(us)
        same["sample_fused_graph_vs_sample_fused"] += int(got["sample_fused_graph"] == got["sample_fused"])
        same["sample_fused_vs_sample_torch"] += int(got["sample_fused"] == got["sample_torch"])
        cap_same.append(sum(x == y for x, y in zip(got["sample_fused"], got["sample_torch"])) / float(N))
    out = {"bench": "tvc_sample_ab", "shape_N_Lv_maxstep": [N, Lv, max_step], "samples": S, "temperature": a.temperature,
           "top_k": a.top_k, "top_p": a.top_p, "model": "HERO-base decoder, 2 layers, vocab 50272", "dtype": "bf16",
           "mode": "eval, no early exit, length_penalty 1, a new seed every run",
           "what": "one whole decode on given encoder outputs: state set-up + max_step steps + pick + id transfer",
           "timer": "HIP events, one pair per decode, sides alternating", "runs": a.runs,
           "sample_torch_graph": "not available: the hash keys of sample_select_torch are host values"}
    for k, v in times.items():
        out[k + "_us_median"], out[k + "_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    out.update({"sample_torch_over_sample_fused": round(statistics.median(times["sample_torch"]) / statistics.median(times["sample_fused"]), 2),
                "runs_with_equal_ids": same, "captions_equal_fused_vs_torch": round(statistics.median(cap_same), 4),
                "graphs_captured": {k: g.counts["captures"] for k, g in fused.items()},
                "device": torch.cuda.get_device_name(0)})
    return json.dumps(out)


def main_beam(a, model, batch, enc, N, Lv, max_step):
    from hero_amd.model import TvcGenerator
    B, bos, eos = a.beam, 0, 2
    greedy = {"greedy_cached": TvcGenerator(model, max_step, bos, eos, kv_cache=True),
              "greedy_cached_graph": TvcGenerator(model, max_step, bos, eos, kv_cache=True, use_graph=True)}
    fused = {"beam_fused": TvcGenerator(model, max_step, bos, eos, kv_cache=True),
             "beam_fused_graph": TvcGenerator(model, max_step, bos, eos, kv_cache=True, use_graph=True)}
    plain = {"beam_torch": TorchBeam(model, max_step, B, bos, eos)}
    run = {k: (lambda g=g: g.greedy_decode(batch, encoder_outputs=enc)) for k, g in greedy.items()}
    run.update({k: (lambda g=g: g.beam_decode(batch, B, encoder_outputs=enc)) for k, g in fused.items()})
    run.update({k: (lambda g=g: [g.cut_eos(r) for r in g.decode(batch, enc)]) for k, g in plain.items()})
    for g in plain.values():
        g.cut_eos = fused["beam_fused"].cut_eos

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ids = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, ids

    for _ in range(3):
        for fn in run.values():
            timed(fn)
    times = {k: [] for k in run}
    same = {"beam_fused_graph_vs_beam_fused": 0, "beam_fused_vs_beam_torch": 0}
    cap_same = []
    for _ in range(a.runs):
        got = {}
        for k, fn in run.items():
            us, got[k] = timed(fn)
            times[k].append(us)
        same["beam_fused_graph_vs_beam_fused"] += int(got["beam_fused_graph"] == got["beam_fused"])
        same["beam_fused_vs_beam_torch"] += int(got["beam_fused"] == got["beam_torch"])
        cap_same.append(sum(x == y for x, y in zip(got["beam_fused"], got["beam_torch"])) / float(N))
    out = {"bench": "tvc_beam_ab", "shape_N_Lv_maxstep": [N, Lv, max_step], "beam": B,
           "model": "HERO-base decoder, 2 layers, vocab 50272", "dtype": "bf16", "mode": "eval, no early exit, length_penalty 1",
           "what": "one whole decode on given encoder outputs: state set-up + max_step steps + pick + id transfer",
           "timer": "HIP events, one pair per decode, sides alternating", "runs": a.runs,
           "beam_torch_graph": "not available: torch.topk puts memset nodes into a captured step"}
    for k, v in times.items():
        out[k + "_us_median"], out[k + "_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    out.update({"runs_with_equal_ids": same, "captions_equal_fused_vs_torch": round(statistics.median(cap_same), 4),
                "graphs_captured": {k: g.counts["captures"] for k, g in list(greedy.items()) + list(fused.items())},
                "device": torch.cuda.get_device_name(0)})
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="40,20,30", help="captions, Lv, max_step")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--beam", type=int, default=0, help="beam size: measure beam search (fused, PyTorch formulation) beside the cached greedy decode")
    ap.add_argument("--sample", type=int, default=0, help="samples per caption: measure sampled decoding (fused, PyTorch formulation) beside the cached greedy decode")
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--temperature", type=float, default=1.0)
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
    if a.beam or a.sample:
        line = (main_sample if a.sample else main_beam)(a, model, batch, enc, N, Lv, max_step)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0
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
