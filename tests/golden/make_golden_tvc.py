#!/usr/bin/env python3
"""Golden vectors for video captioning (TVC) by importing the *reference* HERO code: its datasets and collates (data/tvc.py) on
in-memory stand-ins for the LMDB readers, and its model (model/tvc.py) with the tiny weights of tests/golden/tiny_model.npz plus
a seeded tiny decoder (d_config: hidden 128, 2 heads, 2 layers, intermediate 256, 64 positions, vocabulary 160).

Container-only (needs /root/reference), like its siblings whose stubs it reuses; never imported by a test.
Writes tests/golden/case_tvc.npz:

  desc                 JSON: per video the subtitle tokens, the captions (tokens, time stamps), the clips; the d_config
  feat.<vid>           the video's frame features
  out.*                EVERY tensor / list of the reference's training batch (TvcTrainDataset + its collate)
  val.* / eval.*       the reference's validation and submission batches (TvcValDataset / TvcEvalDataset + their collates)
  param.<name>         the seeded parameters outside v_encoder (position_embeddings, emb_LayerNorm, decoder.*; not the tri_mask):
                       multiples of 1/64, stored exactly as float16
  enc_out              what HeroForTvc.encode returns for the training batch (Ncap, Lv, D)
  scores               prediction_scores (Ncap, Lt, vocab) at dropout 0
  loss_lsr, loss_ce    the loss VECTORS for lsr = 0.1 (valid positions only) and lsr = 0 (all positions, zeros at ignored ones),
                       mean_lsr, mean_ce their `.mean()`
  grad.<param>         gradients of loss_lsr.mean() for six parameters (the reference code run in float64, rounded to fp32);
                       grad32_err.<param>: max-normalised error of the reference's fp32 run against them.  gradce.<param>: the
                       same for loss_ce.mean() (float64 run)
  greedy               JSON: the token lists TvcGenerator.greedy_decode gives for max_step = 8 (its loop, model/tvc.py:301-338,
                       restated without the .cuda() calls), bos 0 and eos = greedy_eos (a token the decode emits; the captions' own
                       eos never comes out of a random tiny model); greedy_raw: the ids before cut_eos; greedy_margin: the
                       smallest lead of a step's top-1 logit over the runner-up, relative to the row's largest magnitude
  state_keys           JSON list: the model's state-dict keys

3 videos of 9 / 6 / 10 frames with 3 / 1 / 2 captions of different lengths: one segment has a single frame, one is clamped at
the video's end, one end stamp lands on x.5 frames (3.75 s / 1.5 = 2.5 -> 2, half to even).  The maker asserts that the case is
not vacuous.

Run:  python tests/golden/make_golden_tvc.py
"""
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                                   # noqa: E402  (apex / horovod stubs)
from make_golden_collate import install_data_stubs        # noqa: E402  (lmdb, lz4, msgpack, toolz stubs)

D_CONFIG = dict(G.TINY["f_config"], max_position_embeddings=64)
BOS, EOS, MAX_STEP = 0, 2, 8
GRADS = ["decoder.layer.0.self_attention.key.weight", "decoder.layer.1.dec_enc_attention.key.weight", "position_embeddings.weight",
         "v_encoder.f_encoder.embeddings.word_embeddings.weight", "v_encoder.c_encoder.encoder.layer.0.attention.self.key.weight",
         "emb_LayerNorm.weight"]
VIDEOS = [  # (frames in the db, [(sub_idx, [frames], n_words)])
    (9, [(0, [0, 1, 2], 5), (1, [3, 4], 4), (2, [], 3), (3, [6, 7], 6)]),
    (6, [(0, [0, 1], 3), (1, [2, 3, 4], 6)]),
    (10, [(0, [1, 2, 3, 4], 4), (1, [5], 2), (2, [7, 8], 5)]),
]
CAPTIONS = [  # per video: (words, [start s, end s]) -> the segment at 1.5 s per frame
    [(5, [0.0, 4.0]),       # (0, 3)
     (3, [3.2, 3.9]),       # (2, 3): a single frame
     (7, [0.0, 3.75])],     # 2.5 frames -> round half to even -> (0, 2)
    [(4, [6.0, 20.0])],     # (4, 6): clamped at the video's end
    [(6, [1.0, 8.0]),       # (0, 5)
     (2, [12.0, 14.0])],    # (8, 9)
]
WANT_RANGES = (((0, 3), (2, 3), (0, 2)), ((4, 6),), ((0, 5), (8, 9)))


def build_batches(seed, vocab=160, frame_interval=1.5, max_clip_len=16):
    from data.data import SubTokLmdb, VideoFeatLmdb, VideoFeatSubTokDataset
    from data.tvc import CaptionTokLmdb, TvcEvalDataset, TvcTrainDataset, TvcValDataset
    g = torch.Generator().manual_seed(seed)

    class FeatDb(VideoFeatLmdb):                           # the LMDB reader replaced by a dict of tensors
        def __init__(self, feats):
            self.feats, self.max_clip_len, self.frame_interval = feats, max_clip_len, frame_interval
            self.name2nframe = {k: v.shape[0] for k, v in feats.items()}

        def __getitem__(self, name):
            return self.feats[name][:min(self.name2nframe[name], self.max_clip_len)].float()

        def __del__(self):
            pass

    class SubDb(SubTokLmdb):                               # keeps the real compute_sub2frames
        def __init__(self, db):
            self.db, self.max_clip_len = db, max_clip_len
            self.sep, self.cls_ = 2, 0
            self.id2len = {k: v["nframe"] for k, v in db.items()}
            self.vid2dur, self.vid2idx = {}, {}
            self.vid_sub2frame, self.vid2vonly_frames = self.compute_sub2frames()

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    class CapDb(CaptionTokLmdb):                           # keeps the real get_caption (bos / eos, truncation)
        def __init__(self, caps, clips, v2caps, v2clips):
            self.cap_db, self.clip_db, self._v2caps, self._v2clips = caps, clips, v2caps, v2clips
            self.pad, self.bos, self.eos, self.max_txt_len = 1, BOS, EOS, -1

        vid2caps = property(lambda self: self._v2caps)
        vid2clips = property(lambda self: self._v2clips)

    words = lambda n: torch.randint(3, vocab, (n,), generator=g).tolist()      # noqa: E731
    feats, subdb, caps, clips, v2caps, v2clips, desc, lines = {}, {}, {}, {}, {}, {}, [], []
    cid = 0
    for v, ((nf, subs), vcaps) in enumerate(zip(VIDEOS, CAPTIONS)):
        vid = "v%02d" % v
        feats[vid] = torch.randn(nf, G.VFEAT, generator=g)
        toks = [words(nw) for _, _, nw in subs]
        subdb[vid] = {"input_ids": toks, "unique_sub2frames": [(si, list(fr)) for si, fr, _ in subs],
                      "unmatched_frames": [], "nframe": nf}
        v2caps[vid], v2clips[vid], dcaps = [], [], []
        for nw, ts in vcaps:
            cid += 1
            ids = words(nw)
            caps[str(cid)] = {"input_ids": ids, "ts": ts}
            clips[str(cid)] = {"ts": ts, "captions": [{"text": "caption %d" % cid}]}
            v2caps[vid].append(str(cid))
            v2clips[vid].append(str(cid))
            lines.append(json.dumps({"vid_name": vid, "clip_id": cid, "ts": ts}))
            dcaps.append({"id": cid, "tokens": ids, "ts": ts})
        desc.append({"vid": vid, "sub_tokens": toks, "captions": dcaps})
    video_db = VideoFeatSubTokDataset(SubDb(subdb), FeatDb(feats), max_txt_len=-1, sub_ctx_len=0)
    capdb = CapDb(caps, clips, v2caps, v2clips)
    train = TvcTrainDataset(video_db, capdb)
    batch = TvcTrainDataset.collate([train[i] for i in range(len(train))])
    val = TvcValDataset(video_db, capdb)
    vbatch = TvcValDataset.collate([val[i] for i in range(len(val))])
    with tempfile.NamedTemporaryFile("w", suffix=".jsonl", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    ev = TvcEvalDataset(video_db, f.name)
    ebatch = TvcEvalDataset.collate([ev[i] for i in range(len(ev))])
    os.unlink(f.name)
    return batch, vbatch, ebatch, {"videos": desc, "d_config": D_CONFIG, "bos": BOS, "eos": EOS, "frame_interval": frame_interval}, feats


def greedy(model, batch):
    """TvcGenerator.greedy_decode (model/tvc.py:301-338) without its .cuda() calls; also the smallest top-1 lead."""
    with torch.no_grad():
        enc = model.encode(batch)
        mask = batch["cap_attn_mask"]
        n = mask.size(0)
        input_ids = torch.zeros(n, MAX_STEP, dtype=torch.long)
        pos_ids = torch.arange(0, MAX_STEP + 1).unsqueeze(0)
        last, margin = torch.full((n,), BOS, dtype=torch.long), float("inf")
        for step in range(MAX_STEP):
            input_ids[:, step] = last
            score = model.decode(enc, mask, input_ids[:, :step + 1], pos_ids[:, :step + 1], None, compute_loss=False)
            output_ids = score.max(dim=-1)[1]
            last = output_ids[:, -1]
            top2 = score[:, -1].topk(2, dim=-1)[0]
            margin = min(margin, float(((top2[:, 0] - top2[:, 1]) / score[:, -1].abs().max(dim=-1)[0]).min()))
    return output_ids.tolist(), margin


def run(model, batch, out):
    params = dict(model.named_parameters())
    model.zero_grad()
    loss = model(batch, "train", compute_loss=True)
    loss.mean().backward()
    with torch.no_grad():
        scores = model(batch, "train", compute_loss=False)
        enc = model.encode(batch)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")      # what HeroForTvc builds for lsr = 0
    smooth, model.loss_func = model.loss_func, ce
    with torch.no_grad():
        loss_ce = model(batch, "train", compute_loss=True)
    model.loss_func = smooth
    out.update({"scores": scores.numpy(), "enc_out": enc.numpy(), "loss_lsr": loss.detach().numpy(), "loss_ce": loss_ce.numpy(),
                "mean_lsr": loss.detach().mean().numpy(), "mean_ce": loss_ce.mean().numpy()})

    m64 = copy.deepcopy(model).double()
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    p64 = dict(m64.named_parameters())
    m64.zero_grad()
    l64 = m64(b64, "train", compute_loss=True).mean()
    l64.backward()
    assert abs(float(l64.detach()) - float(loss.detach().mean())) < 1e-5
    for n_ in GRADS:
        g64 = p64[n_].grad.detach()
        out["grad." + n_] = g64.float().numpy().copy()
        e32 = float((params[n_].grad.double() - g64).abs().max() / g64.abs().max())
        out["grad32_err." + n_] = np.array(e32)
        print("fp32 run vs float64 run, rel_err of grad", n_, "%.3e" % e32)
    m64.zero_grad()
    m64.loss_func = ce
    m64(b64, "train", compute_loss=True).mean().backward()
    for n_ in GRADS:
        out["gradce." + n_] = p64[n_].grad.detach().float().numpy().copy()

    raw_ids, margin = greedy(model, batch)
    # a random tiny model never emits the captions' own eos (2) within 8 steps: the generator's `eos` is a token that the decode
    # does emit at a later step of some caption, so that cut_eos (model/tvc.py:332-338) shortens some rows and not others
    late = sorted({t for row in raw_ids for t in row[2:]} - {row[0] for row in raw_ids})
    assert late, "no token to serve as eos"
    gen_eos = late[0]
    cut = lambda ids: ids[:ids.index(gen_eos)] if gen_eos in ids else ids   # noqa: E731  (cut_eos)
    ids = [cut(row) for row in raw_ids]
    out["greedy"], out["greedy_raw"], out["greedy_margin"] = np.array(json.dumps(ids)), np.array(json.dumps(raw_ids)), np.array(margin)
    out["greedy_eos"] = np.array(gen_eos)

    # ---- the case must not be vacuous --------------------------------------------------------------------------------------
    assert batch["clip_ranges"] == WANT_RANGES, batch["clip_ranges"]
    tgt = batch["cap_tgt_ids"]
    n_valid = int((tgt != -1).sum())
    assert loss.shape == (n_valid,) and loss_ce.shape == (tgt.numel(),) and n_valid < tgt.numel()
    assert float(loss_ce[(tgt == -1).reshape(-1)].abs().max()) == 0.0
    assert abs(float(loss.mean()) - float(loss_ce.mean())) > 0.1, "the two denominators do not show"
    assert len(set((tgt != -1).sum(1).tolist())) > 3, "caption lengths do not differ"
    assert margin >= 1e-3, "an arg-max of the greedy decode is decided by rounding: reseed (margin %.3e)" % margin
    assert len(set(map(tuple, ids))) > 1, "every caption decodes to the same tokens"
    assert any(len(i) < MAX_STEP for i in ids) and any(len(i) > 0 for i in ids), "eos is never / always first"
    m = batch["cap_attn_mask"]
    assert int(m.sum(1).min()) == 1 and int(m.sum(1).max()) == m.shape[1] and float(enc[m == 0].abs().max()) == 0.0
    print("batch", {k: tuple(v.shape) for k, v in batch.items() if torch.is_tensor(v)})
    print("mean_lsr", float(loss.mean()), "mean_ce", float(loss_ce.mean()), "greedy", ids, "margin %.3e" % margin)


def main():
    G.install_stubs()
    install_data_stubs()
    sys.path.insert(0, G.REF)
    from model.tvc import HeroForTvc                        # noqa: reference import

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    cfg = dict(json.load(open(os.path.join(HERE, "tiny_config.json"))), d_config=D_CONFIG)
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cfg, f)
    batch, vbatch, ebatch, raw, feats = build_batches(43)
    for seed in range(31, 41):                              # reseed until no arg-max of the decode is a near tie
        model = HeroForTvc.from_pretrained(f.name, state_dict=dict(sd), vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM, lsr=0.1)
        g = torch.Generator().manual_seed(seed)
        out = {}
        with torch.no_grad():
            for n_, p in model.named_parameters():
                if not n_.startswith("v_encoder"):
                    # multiples of 1/64: exact in float16, which is how they are stored (the file stays below 1 MiB)
                    p.copy_((1.0 if n_.endswith("LayerNorm.weight") else 0.0) + torch.round(0.08 * 64 * torch.randn(p.shape, generator=g)) / 64)
                    out["param." + n_] = p.detach().numpy().astype(np.float16)
                    assert (out["param." + n_].astype(np.float32) == p.detach().numpy()).all()
        model.train()
        for m_ in model.modules():
            if isinstance(m_, torch.nn.Dropout):
                m_.p = 0.0
        if greedy(model, batch)[1] >= 1e-3:
            break
    os.unlink(f.name)
    out["state_keys"] = np.array(json.dumps(sorted(model.state_dict().keys())))
    out["desc"] = np.array(json.dumps(raw))
    for k, v in feats.items():
        out["feat." + k] = v.numpy()
    for name, b in (("out.", batch), ("val.", vbatch), ("eval.", ebatch)):
        for k, v in b.items():
            out[name + k] = v.numpy() if torch.is_tensor(v) else np.array(json.dumps(v))
    run(model, batch, out)
    path = os.path.join(HERE, "case_tvc.npz")
    np.savez_compressed(path, **out)
    print("wrote case_tvc.npz", os.path.getsize(path), "bytes (decoder seed %d)" % seed)


if __name__ == "__main__":
    main()
