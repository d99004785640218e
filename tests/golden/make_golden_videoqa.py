#!/usr/bin/env python3
"""Golden vectors for multiple-choice video QA (TVQA / How2QA) by importing the *reference* HERO code: its dataset and
collate (data/videoQA.py:62-183) on in-memory stand-ins for the LMDB readers, and its model (model/videoQA.py) with the
tiny weights of tests/golden/tiny_model.npz plus seeded values for the four parameter groups the task adds.

Container-only (needs /root/reference), like its siblings whose stubs it reuses; never imported by a test.
Writes tests/golden/case_videoqa.npz.  Per case `<c>` in ("a5", "a4") - 5 answers (TVQA) and 4 (How2QA):

  <c>.desc            JSON: per video the subtitle tokens, question, answers, target, time stamp; frame interval
  <c>.feat.<vid>      the video's frame features
  <c>.out.*           EVERY tensor / list of the reference batch (video_qa_collate)
  <c>.logits, <c>.qa_loss, <c>.temporal_loss, <c>.st_prob, <c>.ed_prob     the reference forward, dropout 0
  <c>.grad.<param>    gradients of qa_loss + 0.4 * temporal_loss for five parameters (the reference code run in float64, rounded
                      to fp32); <c>.grad32_err.<param>: max-normalised error of the reference's fp32 run against them
  a5.pool.*           the head in isolation: its inputs X (Nv, A, L, D) and mask as the model saw them, both pooled outputs,
                      and for seeded upstream gradients dqa / dse the reference's dX, dw_qa, dw_se (fp32 autograd)
  param.<name>        the seeded parameters of qa_pool, qa_pred_head, st_ed_pool, st_ed_pred_head
  state_keys          JSON list: the model's state-dict keys

3 videos of 9 / 6 / 10 frames (so the two shorter ones have masked frames), QA lengths that differ, one question without
a time stamp (-> (-1, -1)), one without a target (-> -1).  The maker asserts that the case is not vacuous.

Run:  python tests/golden/make_golden_videoqa.py
"""
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

LW_ST_ED = 0.4
GRADS = ["qa_pool.weight", "st_ed_pool.weight", "qa_pred_head.linear_2.weight",          # small ones: the file stays under 1 MiB
         "v_encoder.c_encoder.encoder.layer.0.attention.self.key.weight",
         "v_encoder.f_encoder.encoder.layer.1.attention.self.key.weight"]
VIDEOS = [  # (frames in the db, [(sub_idx, [frames], n_words)])
    (9, [(0, [0, 1, 2], 5), (1, [3, 4], 4), (2, [], 3), (3, [6, 7], 6)]),
    (6, [(0, [0, 1], 3), (1, [2, 3, 4], 6)]),
    (10, [(0, [1, 2, 3, 4], 4), (1, [5], 2), (2, [7, 8], 5)]),
]
QUESTIONS = {  # per case: (question words, answer words per answer, target, ts)
    "a5": [(2, [1, 12, 3, 9, 6], 2, "1.6-7.4"), (1, [10, 2, 7, 14, 1], None, "0.0-3.1"), (3, [4, 13, 1, 8, 2], 4, None)],
    "a4": [(1, [2, 11, 5, 14], 1, "3.0-6.2"), (3, [12, 1, 8, 3], 3, None), (2, [6, 13, 1, 9], None, "4.4-13.0")],
}


def build_batch(case, seed, vocab=160, frame_interval=1.5, max_clip_len=16):
    from data.data import QaQueryTokLmdb, SubTokLmdb, VideoFeatLmdb, VideoFeatSubTokDataset
    from data.videoQA import VideoQaDataset, video_qa_collate
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

    class QaDb(QaQueryTokLmdb):
        def __init__(self, db, q2v):
            self.db, self.query2video, self.sep, self.cls_ = db, q2v, 2, 0
            self.video2query = {v: [k] for k, v in q2v.items()}
            self.id2len = {k: len(v["input_ids"][0]) for k, v in db.items()}

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    words = lambda n: torch.randint(3, vocab, (n,), generator=g).tolist()      # noqa: E731
    feats, subdb, qdb, q2v, desc = {}, {}, {}, {}, []
    for v, ((nf, subs), (nq, nas, target, ts)) in enumerate(zip(VIDEOS, QUESTIONS[case])):
        vid, qid = "v%02d" % v, "q%02d" % v
        feats[vid] = torch.randn(nf, G.VFEAT, generator=g)
        toks = [words(nw) for _, _, nw in subs]
        subdb[vid] = {"input_ids": toks, "unique_sub2frames": [(si, list(fr)) for si, fr, _ in subs],
                      "unmatched_frames": [], "nframe": nf}
        question, answers = words(nq), [words(n) for n in nas]
        qdb[qid] = {"input_ids": [question] + answers, "target": target, "ts": ts}
        q2v[qid] = vid
        desc.append({"vid": vid, "sub_tokens": toks, "question": question, "answers": answers, "target": target, "ts": ts})
    video_db = VideoFeatSubTokDataset(SubDb(subdb), FeatDb(feats), max_txt_len=-1, sub_ctx_len=0)
    ds = VideoQaDataset(sorted(feats), video_db, QaDb(qdb, q2v), sampled_by_q=True)
    assert ds.qids == sorted(qdb)
    batch = video_qa_collate([ds[i] for i in range(len(ds))])
    return batch, {"videos": desc, "frame_interval": frame_interval, "sep": 2}, feats


def run_case(case, model, batch, out):
    from model.modeling_utils import mask_logits
    params = dict(model.named_parameters())
    seen = {}
    pool = model.get_modularized_video

    def spy(frame_embeddings, frame_mask):                 # the head's inputs and outputs as the model saw them
        se, qa = pool(frame_embeddings, frame_mask)
        seen.update(X=frame_embeddings.detach().clone(), mask=frame_mask.detach().clone(), se=se.detach().clone(), qa=qa.detach().clone())
        return se, qa
    model.get_modularized_video = spy
    hook = model.st_ed_pred_head.register_forward_hook(lambda m_, i_, o_: seen.update(pred=o_.detach().clone()))
    model.zero_grad()
    qa_loss, temporal_loss = model(batch, task="tvqa" if case == "a5" else "how2qa", compute_loss=True)
    (qa_loss + LW_ST_ED * temporal_loss).backward()
    with torch.no_grad():
        logits = model(batch, task="tvqa", compute_loss=False)
    hook.remove()
    model.get_modularized_video = pool
    first = seen["mask"][:, 0]
    out.update({case + ".logits": logits.numpy(), case + ".qa_loss": qa_loss.detach().numpy(),
                case + ".temporal_loss": temporal_loss.detach().numpy(),
                case + ".st_prob": mask_logits(seen["pred"][:, :, 0], first).numpy(),
                case + ".ed_prob": mask_logits(seen["pred"][:, :, 1], first).numpy()})
    # The stored gradients come from the SAME reference code run in float64 and are rounded to fp32 once: the gradient of
    # st_ed_pool.weight is a sum that cancels twice (ds sums to zero over the answers, and the answer copies of a frame are
    # close to each other), so the reference's own fp32 run is only good to ~3e-4 of its largest element there - a third
    # of the bound the parity tests hold gradients to.  `grad32.*` keeps that fp32 run's figures for the record.
    import copy
    m64 = copy.deepcopy(model).double()
    m64.get_modularized_video = type(model).get_modularized_video.__get__(m64)
    m64.zero_grad()
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    q64, t64 = m64(b64, task="tvqa", compute_loss=True)
    (q64 + LW_ST_ED * t64).backward()
    assert abs(float(q64) - float(qa_loss)) < 1e-5 and abs(float(t64) - float(temporal_loss)) < 1e-5
    p64 = dict(m64.named_parameters())
    for n_ in GRADS:
        g64 = p64[n_].grad.detach()
        out["%s.grad.%s" % (case, n_)] = g64.float().numpy().copy()
        e32 = float((params[n_].grad.double() - g64).abs().max() / g64.abs().max())
        out["%s.grad32_err.%s" % (case, n_)] = np.array(e32)
        print(case, "fp32 run vs float64 run, rel_err of grad", n_, "%.3e" % e32)

    # the head in isolation, with seeded upstream gradients
    g = torch.Generator().manual_seed(99)
    X = seen["X"].clone().requires_grad_(True)
    model.zero_grad()
    se, qa = pool(X, seen["mask"])
    dqa, dse = torch.randn(qa.shape, generator=g), torch.randn(se.shape, generator=g)
    ((qa * dqa).sum() + (se * dse).sum()).backward()
    if case == "a5":                                         # one case carries the head's own tensors (file size)
        out.update({"a5.pool.X": seen["X"].numpy(), "a5.pool.mask": seen["mask"].numpy(),
                    "a5.pool.qa_pooled": seen["qa"].numpy(), "a5.pool.se_pooled": seen["se"].numpy(),
                    "a5.pool.dqa": dqa.numpy(), "a5.pool.dse": dse.numpy(), "a5.pool.dX": X.grad.numpy().copy(),
                    "a5.pool.dw_qa": model.qa_pool.weight.grad.numpy().copy(),
                    "a5.pool.dw_se": model.st_ed_pool.weight.grad.numpy().copy()})

    # ---- the case must not be vacuous --------------------------------------------------------------------------------------
    tg, ts = batch["targets"].squeeze(-1), batch["ts_targets"]
    assert int((tg != -1).sum()) >= 2 and int((tg == -1).sum()) >= 1, tg
    assert int((ts[:, 0] != -1).sum()) >= 2 and int((ts[:, 1] != -1).sum()) >= 2 and int((ts[:, 0] == -1).sum()) >= 1, ts
    m = seen["mask"]
    assert float(m.min()) == 0.0, "no masked frame"
    A = m.shape[1]
    assert seen["qa"].shape != seen["se"].shape or not torch.equal(seen["qa"], seen["se"])
    with torch.no_grad():
        s_qa = mask_logits(model.qa_pool(seen["X"]), m.unsqueeze(-1)).softmax(2).squeeze(-1)
        s_se = mask_logits(model.st_ed_pool(seen["X"]), m.unsqueeze(-1)).softmax(1).squeeze(-1)
    valid = m.bool()
    n_valid = m.sum(2, keepdim=True).expand_as(m)
    assert float((s_qa - 1.0 / n_valid)[valid].abs().max()) > 0.05, "att_qa is uniform on the valid frames"
    assert float((s_se - 1.0 / A)[valid].abs().max()) > 0.05, "att_se is uniform on the valid frames"
    assert float((s_se - 1.0 / A)[~valid].abs().max()) < 1e-6                     # masked frames: uniform over the answers
    assert float((seen["qa"].mean(1) - seen["se"].mean(1)).abs().max()) > 1e-3, "the two pools give the same thing"
    print(case, "batch", {k: tuple(v.shape) for k, v in batch.items() if torch.is_tensor(v)})
    print(case, "qa_loss", float(qa_loss), "temporal_loss", float(temporal_loss), "logits", logits.numpy().round(3).tolist())


def main():
    G.install_stubs()
    install_data_stubs()
    sys.path.insert(0, G.REF)
    from model.videoQA import HeroForVideoQA              # noqa: reference import

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    model = HeroForVideoQA.from_pretrained(os.path.join(HERE, "tiny_config.json"), state_dict=sd,
                                           vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM)
    g = torch.Generator().manual_seed(23)
    out = {}
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.split(".")[0] in ("qa_pool", "qa_pred_head", "st_ed_pool", "st_ed_pred_head"):
                # qa_pool: frame scores a few units apart.  st_ed_pool: the answer copies of a frame differ little in a tiny,
                # randomly initialised model, so its softmax over the answers needs large weights to leave the uniform
                scale = {"qa_pool": 0.3, "st_ed_pool": 6.0}.get(n_.split(".")[0], 0.05)
                p.copy_((1.0 if n_.endswith("LayerNorm.weight") else 0.0) + scale * torch.randn(p.shape, generator=g))
                out["param." + n_] = p.detach().numpy().copy()
    model.train()
    for m_ in model.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    out["state_keys"] = np.array(json.dumps(sorted(model.state_dict().keys())))
    for case, seed in (("a5", 31), ("a4", 32)):
        batch, raw, feats = build_batch(case, seed)
        out[case + ".desc"] = np.array(json.dumps(raw))
        for k, v in feats.items():
            out["%s.feat.%s" % (case, k)] = v.numpy()
        for k, v in batch.items():
            out["%s.out.%s" % (case, k)] = v.numpy() if torch.is_tensor(v) else np.array(json.dumps(v))
        run_case(case, model, batch, out)
    out["__cases__"] = np.array(json.dumps(["a5", "a4"]))
    path = os.path.join(HERE, "case_videoqa.npz")
    np.savez_compressed(path, **out)
    print("wrote case_videoqa.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
