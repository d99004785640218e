#!/usr/bin/env python3
"""Golden vectors for video-and-language inference (VIOLIN) by importing the *reference* HERO code: its datasets and collates
(data/violin.py) on in-memory stand-ins for the LMDB readers, and its model (model/violin.py) with the tiny weights of
tests/golden/tiny_model.npz plus seeded values for the two parameter groups the task adds.

Container-only (needs /root/reference), like its siblings whose stubs it reuses; never imported by a test.
Writes tests/golden/case_violin.npz:

  desc                 JSON: per video the subtitle tokens, the two statements and their truth values, the qids; sub_ctx_len
  feat.<vid>           the video's frame features
  out.*                EVERY tensor / list of the reference's training batch (ViolinDataset sampled by statement + violin_collate:
                       every item is a statement and its paired one, 3 items -> S = 6)
  eval.*               the reference's evaluation batch (ViolinEvalDataset + violin_eval_collate over all six statements), `qids` included
  logits, violin_loss  the reference forward on the training batch, dropout 0
  val.loss, val.acc, val.results     what eval_violin.py:validate_violin computes from the evaluation batch (sum of
                       binary_cross_entropy(sigmoid(z), t) over the examples / their number, share of sigmoid(z) > 0.5 == t, qid -> 0 | 1)
  grad.<param>         gradients of violin_loss for five parameters (the reference code run in float64, rounded to fp32);
                       grad32_err.<param>: max-normalised error of the reference's fp32 run against them
  pool.*               the head in isolation: its inputs X (S, L, D) and mask as the model saw them, pooled, and for a seeded
                       upstream gradient dpooled the reference's dX, dw (fp32 autograd)
  h                    the output of violin_pred_head.LayerNorm (S, 2 D): the classifier tail's input
  param.<name>         the seeded parameters of violin_pool and violin_pred_head
  state_keys           JSON list: the model's state-dict keys

3 videos of 9 / 6 / 10 frames (so the two shorter ones have masked frames), sub_ctx_len = 2 as in config/train-violin-8gpu.json,
statement lengths that differ.  The maker asserts that the case is not vacuous.

Run:  python tests/golden/make_golden_violin.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                                   # noqa: E402  (apex / horovod stubs)
from make_golden_collate import install_data_stubs        # noqa: E402  (lmdb, lz4, msgpack, toolz stubs)

SUB_CTX_LEN = 2
GRADS = ["violin_pool.weight", "violin_pred_head.linear_2.weight", "violin_pred_head.linear_2.bias",
         "v_encoder.c_encoder.encoder.layer.0.attention.self.key.weight",
         "v_encoder.f_encoder.encoder.layer.1.attention.self.key.weight"]
VIDEOS = [  # (frames in the db, [(sub_idx, [frames], n_words)])
    (9, [(0, [0, 1, 2], 5), (1, [3, 4], 4), (2, [], 3), (3, [6, 7], 6)]),
    (6, [(0, [0, 1], 3), (1, [2, 3, 4], 6)]),
    (10, [(0, [1, 2, 3, 4], 4), (1, [5], 2), (2, [7, 8], 5)]),
]
STATEMENTS = [  # per video: (words of statement -0, words of statement -1, which of the pair the training set samples, truth of -0)
    (4, 9, 0, True), (7, 2, 1, False), (3, 11, 0, True),
]


def build_batches(seed, vocab=160, frame_interval=1.5, max_clip_len=16):
    from data.data import QaQueryTokLmdb, SubTokLmdb, VideoFeatLmdb, VideoFeatSubTokDataset
    from data.violin import ViolinDataset, ViolinEvalDataset, violin_collate, violin_eval_collate
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

    class QaDb(QaQueryTokLmdb):                            # `listed`: the ids the dataset iterates over (id2len)
        def __init__(self, db, q2v, listed):
            self.db, self.query2video, self.sep, self.cls_ = db, q2v, 2, 0
            self.video2query = {}
            for k, v in q2v.items():
                self.video2query.setdefault(v, []).append(k)
            self.id2len = {k: len(db[k]["input_ids"]) for k in listed}

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    words = lambda n: torch.randint(3, vocab, (n,), generator=g).tolist()      # noqa: E731
    feats, subdb, qdb, q2v, desc, sampled = {}, {}, {}, {}, [], []
    for v, ((nf, subs), (n0, n1, pick, truth0)) in enumerate(zip(VIDEOS, STATEMENTS)):
        vid = "v%02d" % v
        feats[vid] = torch.randn(nf, G.VFEAT, generator=g)
        toks = [words(nw) for _, _, nw in subs]
        subdb[vid] = {"input_ids": toks, "unique_sub2frames": [(si, list(fr)) for si, fr, _ in subs],
                      "unmatched_frames": [], "nframe": nf}
        stmts = [words(n0), words(n1)]
        for i in (0, 1):
            qid = "s%02d-%d" % (v, i)
            qdb[qid] = {"input_ids": stmts[i], "target": truth0 if i == 0 else not truth0}
            q2v[qid] = vid
        sampled.append("s%02d-%d" % (v, pick))
        desc.append({"vid": vid, "sub_tokens": toks, "statements": stmts, "targets": [truth0, not truth0], "sampled": pick})
    video_db = VideoFeatSubTokDataset(SubDb(subdb), FeatDb(feats), max_txt_len=-1, sub_ctx_len=SUB_CTX_LEN)
    ds = ViolinDataset(sorted(feats), video_db, QaDb(qdb, q2v, sampled), sampled_by_q=True)
    assert ds.qids == sampled
    batch = violin_collate([ds[i] for i in range(len(ds))])
    eds = ViolinEvalDataset(sorted(feats), video_db, QaDb(qdb, q2v, sorted(qdb)), sampled_by_q=True)
    ebatch = violin_eval_collate([eds[i] for i in range(len(eds))])
    assert ebatch["qids"] == sorted(qdb)
    return batch, ebatch, {"videos": desc, "sub_ctx_len": SUB_CTX_LEN, "sep": 2}, feats


def run(model, batch, ebatch, out):
    from model.modeling_utils import mask_logits
    params = dict(model.named_parameters())
    seen = {}
    pool = model.get_modularized_video

    def spy(frame_embeddings, frame_mask):                 # the head's inputs and output as the model saw them
        pooled = pool(frame_embeddings, frame_mask)
        seen.update(X=frame_embeddings.detach().clone(), mask=frame_mask.detach().clone(), pooled=pooled.detach().clone())
        return pooled
    model.get_modularized_video = spy
    hook = model.violin_pred_head.LayerNorm.register_forward_hook(lambda m_, i_, o_: seen.update(h=o_.detach().clone()))
    model.zero_grad()
    loss = model(batch, task="violin", compute_loss=True)
    loss.backward()
    with torch.no_grad():
        logits = model(batch, task="violin", compute_loss=False)
    hook.remove()
    model.get_modularized_video = pool
    out.update({"logits": logits.numpy(), "violin_loss": loss.detach().numpy(), "h": seen["h"].numpy()})

    # the stored gradients come from the SAME reference code run in float64 and are rounded to fp32 once
    m64 = copy.deepcopy(model).double()
    m64.get_modularized_video = type(model).get_modularized_video.__get__(m64)
    m64.zero_grad()
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    l64 = m64(b64, task="violin", compute_loss=True)
    l64.backward()
    assert abs(float(l64) - float(loss)) < 1e-5
    p64 = dict(m64.named_parameters())
    for n_ in GRADS:
        g64 = p64[n_].grad.detach()
        out["grad." + n_] = g64.float().numpy().copy()
        e32 = float((params[n_].grad.double() - g64).abs().max() / g64.abs().max())
        out["grad32_err." + n_] = np.array(e32)
        print("fp32 run vs float64 run, rel_err of grad", n_, "%.3e" % e32)

    # the evaluation batch: the sums of the validation loop
    model.eval()
    eb = {k: v for k, v in ebatch.items() if k != "qids"}
    with torch.no_grad():
        z = model(eb, "violin", compute_loss=False)
    model.train()
    t = ebatch["targets"]
    pred = (torch.sigmoid(z) > 0.5).long()
    val_loss = float(torch.nn.functional.binary_cross_entropy(torch.sigmoid(z), t.to(z.dtype), reduction="sum")) / len(ebatch["qids"])
    val_acc = int((pred.squeeze() == t.squeeze()).sum()) / len(ebatch["qids"])
    results = {str(q): int(a) for q, a in zip(ebatch["qids"], pred.squeeze().tolist())}
    out.update({"val.loss": np.array(val_loss), "val.acc": np.array(val_acc), "val.results": np.array(json.dumps(results)),
                "val.logits": z.numpy()})

    # the head in isolation, with a seeded upstream gradient
    g = torch.Generator().manual_seed(99)
    X = seen["X"].clone().requires_grad_(True)
    model.zero_grad()
    pooled = pool(X, seen["mask"])
    dpooled = torch.randn(pooled.shape, generator=g)
    (pooled * dpooled).sum().backward()
    out.update({"pool.X": seen["X"].numpy(), "pool.mask": seen["mask"].numpy(), "pool.pooled": seen["pooled"].numpy(),
                "pool.dpooled": dpooled.numpy(), "pool.dX": X.grad.numpy().copy(),
                "pool.dw": model.violin_pool.weight.grad.numpy().copy()})

    # ---- the case must not be vacuous --------------------------------------------------------------------------------------
    m = seen["mask"]
    assert m.shape[0] == 6 and float(m.min()) == 0.0, "no masked frame"
    with torch.no_grad():
        att = mask_logits(model.violin_pool(seen["X"]), m.unsqueeze(-1)).softmax(1).squeeze(-1)
    n_valid = m.sum(1, keepdim=True).expand_as(m)
    assert float((att - 1.0 / n_valid)[m.bool()].abs().max()) > 0.05, "the attention is uniform on the valid frames"
    for tg in (batch["targets"], t):
        assert set(tg.reshape(-1).tolist()) == {0, 1}, tg
    assert len(set(batch["q_attn_masks"].sum(1).tolist())) > 2, "statement lengths do not differ"
    assert 0.0 < val_acc < 1.0, val_acc
    right = ((logits > 0).long().reshape(-1) == batch["targets"].reshape(-1))
    assert bool(right.any()) and not bool(right.all()), right
    assert float(logits.abs().max()) < 8 and float(z.abs().max()) < 8
    print("batch", {k: tuple(v.shape) for k, v in batch.items() if torch.is_tensor(v)})
    print("violin_loss", float(loss), "logits", logits.reshape(-1).numpy().round(3).tolist(), "targets", batch["targets"].reshape(-1).tolist())
    print("val loss", val_loss, "acc", val_acc, results)


def main():
    G.install_stubs()
    install_data_stubs()
    sys.path.insert(0, G.REF)
    from model.violin import HeroForViolin                 # noqa: reference import

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    model = HeroForViolin.from_pretrained(os.path.join(HERE, "tiny_config.json"), state_dict=sd,
                                          vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM)
    g = torch.Generator().manual_seed(29)
    out = {}
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.split(".")[0] in ("violin_pool", "violin_pred_head"):
                # violin_pool: frame scores a few units apart, so the attention leaves the uniform
                scale = {"violin_pool": 0.3}.get(n_.split(".")[0], 0.05)
                p.copy_((1.0 if n_.endswith("LayerNorm.weight") else 0.0) + scale * torch.randn(p.shape, generator=g))
                out["param." + n_] = p.detach().numpy().copy()
    model.train()
    for m_ in model.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    out["state_keys"] = np.array(json.dumps(sorted(model.state_dict().keys())))
    batch, ebatch, raw, feats = build_batches(41)
    out["desc"] = np.array(json.dumps(raw))
    for k, v in feats.items():
        out["feat." + k] = v.numpy()
    for name, b in (("out.", batch), ("eval.", ebatch)):
        for k, v in b.items():
            out[name + k] = v.numpy() if torch.is_tensor(v) else np.array(json.dumps(v))
    run(model, batch, ebatch, out)
    path = os.path.join(HERE, "case_violin.npz")
    np.savez_compressed(path, **out)
    print("wrote case_violin.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
