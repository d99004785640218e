#!/usr/bin/env python3
"""Golden vectors for video retrieval (MSR-VTT), video-only corpora and DiDeMo recall by importing the *reference* HERO code: its
datasets and collates (data/vr.py, data/vr_video_only.py, data/vcmr_video_only.py) on in-memory stand-ins for the LMDB readers,
its model (model/vr.py) with the tiny weights of tests/golden/tiny_model.npz, its validators (train_vr.py, train_vcmr.py,
eval_vr.py) and its metric code (utils/tvr_standalone_eval.py).

Container-only (needs the reference checkout), like its siblings whose stubs it reuses (make_golden.py: apex / horovod;
make_golden_collate.py: lmdb, lz4, msgpack, toolz; make_golden_postproc.py's numpy shim for eval_by_task_type); never imported by
a test.  Writes tests/golden/case_vr.npz:

  desc                       JSON: per video its subtitles (sub_idx, frames, tokens); the queries (qid, tokens, video, ts); cls / sep
  feat.<vid>                 the video's frame features (3 videos of 9 / 6 / 10 frames)
  batch.<name>.<key>         EVERY tensor / list of five reference batches over the five queries (two of them on one video):
                               vr_vonly       VrVideoOnlyDataset + vr_collate
                               vr_vonly_eval  VrVideoOnlyEvalDataset + vr_eval_collate
                               vr_vonly_full  VrVideoOnlyFullEvalDataset + vr_full_eval_collate
                               vr_sub         VrDataset (video + subtitles) + vr_collate
                               vcmr_vonly     VcmrVideoOnlyDataset + vcmr_collate (DiDeMo-style: one [st, ed] per query)
  vr.<name>.train_neg_ctx / train_neg_q      HeroForVr (margin 0.1, lw_neg_ctx = lw_neg_q = 10, use_all_neg) in training mode at
                                             dropout 0 on vr_vonly / vr_sub
  vr.<name>.eval_neg_ctx / eval_neg_q        its eval-mode loss vectors;  vr.<name>.scores: q2video_scores
  vr.<name>.grad.<param>     gradients of loss_neg_ctx + loss_neg_q for five parameters (the reference code run in float64, rounded to
                             fp32); vr.<name>.grad32_err.<param>: max-normalised error of the reference's fp32 run against them
  state_keys                 JSON list: the state-dict keys of the reference HeroForVr
  val.vr.<i>.neg_ctx / neg_q            per batch of the two-batch loader (3 + 2 items of vr_vonly_eval), what validate_vr scored
  val.vcmr.<i>.st_ed / neg_ctx / neg_q  the same for validate_vcmr (HeroForVcmr, lw_st_ed 0.01, lw_neg 8) on vcmr_vonly items
  val.vr.log / val.vcmr.log  JSON: the returned dictionaries without valid/ex_per_s;  val.*.opts: JSON of the loss weights
  full.<corpus>.val_log / .submission   JSON: validate_full_vr (eval_vr.py:137-305) on the video-only and the video + sub corpus,
                             max_vr_video 2, video batches of 2, query batches of 3 + 2; val_log without its *_ex_per_s key
  full.<corpus>.scores       the [5, 3] q2video scores behind it;  full.score_tol: the tolerance the gaps were asserted against
  didemo.<case>.video / st / ed         int32 [Nq, P] prediction rows (frame indices);  gt_vidx int32 [Nq]
  didemo.<case>.gt_ts / gt_n            the ragged ground truth (4, 4, 5 and 7 annotators, twice; 5 s grid) padded with zeros
  didemo.<case>.ts_list      JSON: the same as the reference's JSON holds it;  cfg: JSON vfeat_interval (i15: 1.5, i20: 2)
  didemo.<case>.metrics      JSON of eval_retrieval's dictionary for VCMR and SVMR, predictions = those rows in seconds

Asserted here: the batches are what the descriptions say; the two queries of one video make q_vidx differ from arange; every
score gap among the videos of a query exceeds ten times full.score_tol; no DiDeMo IoU is within 1e-5 of a threshold other than
exactly on it; and on at least one DiDeMo case the metrics change when `need` is forced to 1 and when only annotator 0 is read.

Run:  python tests/golden/make_golden_vr.py
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

np.bool = bool                # the reference's metric code predates numpy 1.24

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                                   # noqa: E402  (apex / horovod stubs)
from make_golden_collate import install_data_stubs        # noqa: E402  (lmdb, lz4, msgpack, toolz stubs)

VIDEOS = [  # (frames in the db, [(sub_idx, [frames], n_words)])
    (9, [(0, [0, 1, 2], 5), (1, [3, 4], 4), (2, [], 3), (3, [6, 7], 6)]),
    (6, [(0, [0, 1], 3), (1, [2, 3, 4], 6)]),
    (10, [(0, [1, 2, 3, 4], 4), (1, [5], 2), (2, [7, 8], 5)]),
]
QUERIES = [(4, 0, [1.0, 6.2]), (7, 1, [0.0, 4.4]), (2, 1, [3.1, 8.0]), (9, 2, [4.6, 12.5]), (5, 2, [7.4, 13.0])]     # words, video, ts
GRADS = ["q_feat_attn.modular_vector_mapping.weight", "q_feat_attn.query_input_proj.net.1.weight",
         "v_encoder.f_encoder.img_embeddings.img_linear.weight",
         "v_encoder.c_encoder.encoder.layer.0.attention.self.key.weight",
         "v_encoder.f_encoder.encoder.layer.1.attention.self.key.weight"]
SCORE_TOL = 1e-3              # ten times the fp32 parity bound of these cosine scores (tests/test_gpu_parity.py holds 2e-4 relative)
SEED = 62                     # of the videos, subtitles and queries: one whose score gaps pass the assertion in main()
VR_OPTS = types.SimpleNamespace(lw_neg_ctx=10.0, lw_neg_q=10.0, task="msrvtt_video_only")
VCMR_OPTS = types.SimpleNamespace(lw_st_ed=0.01, lw_neg_ctx=8.0, lw_neg_q=8.0, task="didemo_video_only")
IOU_THDS = (0.5, 0.7)


def build(seed, vocab=160, frame_interval=1.5, max_clip_len=16):
    from data.data import QueryTokLmdb, SubTokLmdb, VideoFeatLmdb, VideoFeatSubTokDataset
    from data.vr import MsrvttQueryTokLmdb
    from data.vr_video_only import VideoFeatDataset
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

    def fill(self, db, q2v):
        self.db, self.query2video, self.cls_, self.sep = db, q2v, 0, 2
        self.video2query = {}
        for k, v in q2v.items():
            self.video2query.setdefault(v, []).append(k)
        self.id2len = {k: len(v["input_ids"]) for k, v in db.items()}

    class VrQDb(MsrvttQueryTokLmdb):                       # keeps the real query_data property
        def __init__(self, db, q2v):
            fill(self, db, q2v)
            self.query_data_f = [{"sen_id": int(k), "clip_name": v, "desc": ""} for k, v in q2v.items()]

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    class VcmrQDb(QueryTokLmdb):
        def __init__(self, db, q2v):
            fill(self, db, q2v)
            self.query_data = {}

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    words = lambda n: torch.randint(3, vocab, (n,), generator=g).tolist()      # noqa: E731
    feats, subdb, desc = {}, {}, []
    for v, (nf, subs) in enumerate(VIDEOS):
        vid = "v%02d" % v
        feats[vid] = torch.randn(nf, G.VFEAT, generator=g)
        toks = [words(nw) for _, _, nw in subs]
        subdb[vid] = {"input_ids": toks, "unique_sub2frames": [(si, list(fr)) for si, fr, _ in subs], "unmatched_frames": [], "nframe": nf}
        desc.append({"vid": vid, "subs": [(si, list(fr)) for si, fr, _ in subs], "sub_tokens": toks})
    qdb, q2v, qdesc = {}, {}, []
    for q, (nw, v, ts) in enumerate(QUERIES):
        qid = str(q)
        qdb[qid] = {"input_ids": words(nw), "target": list(ts)}
        q2v[qid] = "v%02d" % v
        qdesc.append({"qid": qid, "tokens": qdb[qid]["input_ids"], "vid": q2v[qid], "ts": list(ts)})
    img_db = FeatDb(feats)
    vonly = VideoFeatDataset({"CLS": 0, "SEP": 2}, img_db)
    vsub = VideoFeatSubTokDataset(SubDb(subdb), img_db, max_txt_len=-1, sub_ctx_len=0)
    raw = {"videos": desc, "queries": qdesc, "cls": 0, "sep": 2, "frame_interval": frame_interval}
    return feats, vonly, vsub, VrQDb(qdb, q2v), VcmrQDb(qdb, q2v), raw


def pack(out, prefix, batch):
    for k, v in batch.items():
        out[prefix + k] = v.numpy() if torch.is_tensor(v) else np.array(json.dumps(v))


def model_case(model, batch, out, pre):
    params = dict(model.named_parameters())
    model.train()
    model.zero_grad()
    lc, lq = model(batch, task="msrvtt_video_only", compute_loss=True)
    (lc + lq).backward()
    out[pre + "train_neg_ctx"], out[pre + "train_neg_q"] = lc.detach().numpy(), lq.detach().numpy()
    m64 = copy.deepcopy(model).double()
    m64.zero_grad()
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    c64, q64 = m64(b64, task="msrvtt_video_only", compute_loss=True)
    (c64 + q64).backward()
    assert abs(float(c64 + q64) - float(lc + lq)) < 1e-4
    p64 = dict(m64.named_parameters())
    for n_ in GRADS:
        g64 = p64[n_].grad.detach()
        assert float(g64.abs().max()) > 1e-6, ("no gradient reaches", n_)
        out[pre + "grad." + n_] = g64.float().numpy().copy()
        e32 = float((params[n_].grad.double() - g64).abs().max() / g64.abs().max())
        out[pre + "grad32_err." + n_] = np.array(e32)
        print(pre, "fp32 vs float64 grad", n_, "%.3e" % e32)
    model.eval()
    with torch.no_grad():
        ec, eq = model(batch, task="msrvtt_video_only", compute_loss=True)
        scores = model(batch, task="msrvtt_video_only", compute_loss=False)
    model.train()
    out[pre + "eval_neg_ctx"], out[pre + "eval_neg_q"], out[pre + "scores"] = ec.numpy(), eq.numpy(), scores.numpy()
    assert float(lc) > 0 and float(lq) > 0, "a ranking term is zero: the case is vacuous"
    print(pre, "train", float(lc), float(lq), "eval", ec.numpy().round(3).tolist(), eq.numpy().round(3).tolist())


class Tap:
    """The model as a validator sees it, recording what it scored."""

    def __init__(self, model):
        self.model, self.outs = model, []

    def __call__(self, batch, task, compute_loss=True):
        self.outs.append(self.model(batch, task, compute_loss=compute_loss))
        return self.outs[-1]


def didemo_case(rng, S, interval, nq=8, p=24, nv=3, length=40):
    """prediction rows over three videos near the annotated moment; ground truth of 4, 4, 5, 7 annotators on a 5 s grid who
    mostly agree, with one or two who do not"""
    counts = [4, 4, 5, 7] * (nq // 4)
    gt_vidx = rng.integers(0, nv, size=nq).astype(np.int32)
    ts_list, video, st, ed = [], [], [], []
    for q in range(nq):
        a = int(rng.integers(0, 5))
        base = [5.0 * a, 5.0 * (a + int(rng.integers(1, 3)))]
        ts = []
        for g in range(counts[q]):
            if g >= 2 and rng.uniform() < 0.5:             # a dissenting annotator
                b = int(rng.integers(0, 6))
                ts.append([5.0 * b, 5.0 * (b + 1)])
            else:
                ts.append(list(base))
        if q % 4 == 1:                                      # annotator 0 alone somewhere else: reading only annotator 0 goes wrong
            ts[0] = [5.0 * ((a + 3) % 6), 5.0 * ((a + 3) % 6 + 1)]
        if q % 4 == 2:                                      # only ONE annotator at `base`: need = 1 would count it
            ts = [list(base)] + [[50.0 + 5 * g, 55.0 + 5 * g] for g in range(1, counts[q])]
        ts_list.append(ts)
        v = np.where(rng.uniform(size=p) < 0.5, gt_vidx[q], rng.integers(0, nv, size=p)).astype(np.int32)
        c = base[0] / interval
        s = np.clip(np.round(c + rng.integers(-4, 5, size=p)), 0, length - 2).astype(np.int32)
        e = np.minimum(s + rng.integers(1, 8, size=p), length - 1).astype(np.int32)
        first_own = int(rng.integers(1, 6))                 # the best predictions are in other videos or far off
        v[:first_own] = (gt_vidx[q] + 1) % nv
        video.append(v), st.append(s), ed.append(e)
    video, st, ed = np.stack(video), np.stack(st), np.stack(ed)
    preds = [dict(desc_id=q, desc="", predictions=[[int(video[q, i]), float(st[q, i] * interval), float((ed[q, i] + 1) * interval), 1.0 - 0.01 * i]
                                                    for i in range(p)]) for q in range(nq)]
    sub = {"VCMR": preds, "SVMR": copy.deepcopy(preds), "video2idx": {"vid%d" % v: v for v in range(nv)}}
    gts = [dict(desc_id=q, desc="", vid_name="vid%d" % gt_vidx[q], ts=ts_list[q]) for q in range(nq)]
    metrics = json.loads(json.dumps(S.eval_retrieval(sub, gts, iou_thds=IOU_THDS, match_number=True, verbose=False, use_desc_type=False)))
    for q in range(nq):                                     # an IoU is exactly a threshold or well away from it
        p0, p1 = st[q] * float(interval), (ed[q] + 1) * float(interval)
        for g0, g1 in ts_list[q]:
            hull = np.maximum(p1, g1) - np.minimum(p0, g0)
            iou = np.maximum(0, np.minimum(p1, g1) - np.maximum(p0, g0)) / hull
            for thd in IOU_THDS:
                near = np.abs(iou - thd) < 1e-5
                assert (np.abs(iou - thd)[near] < 1e-12).all(), "a metric IoU is too close to a threshold"
    G_ = max(counts)
    gt_ts = np.zeros((nq, G_, 2), dtype=np.float32)
    for q, ts in enumerate(ts_list):
        gt_ts[q, :len(ts)] = np.asarray(ts, dtype=np.float32)
    return dict(video=video, st=st, ed=ed, gt_vidx=gt_vidx, gt_ts=gt_ts, gt_n=np.asarray(counts, dtype=np.int32),
                ts_list=np.array(json.dumps(ts_list)), cfg=np.array(json.dumps(dict(vfeat_interval=interval))),
                metrics=np.array(json.dumps(metrics))), metrics


def main():
    G.install_stubs()
    install_data_stubs()
    tbx = types.ModuleType("tensorboardX")
    tbx.SummaryWriter = object
    sys.modules["tensorboardX"] = tbx
    sys.path.insert(0, G.REF)
    import eval_vr as EV                                   # noqa: reference import
    import train_vcmr as TC                                # noqa: reference import
    import train_vr as TV                                  # noqa: reference import
    from data.vcmr import vcmr_collate                     # noqa: reference import
    from data.vcmr_video_only import VcmrVideoOnlyDataset
    from data.vr import VrDataset, VrFullEvalDataset, vr_collate, vr_eval_collate, vr_full_eval_collate
    from data.vr_video_only import VrVideoOnlyDataset, VrVideoOnlyEvalDataset, VrVideoOnlyFullEvalDataset
    from model.vcmr import HeroForVcmr
    from model.vr import HeroForVr
    from utils import tvr_standalone_eval as S
    TV.all_gather_list = TC.all_gather_list = lambda x: [x]              # one rank
    EV.move_to_cuda = lambda b: b                                          # the reference code runs on the CPU here

    feats, vonly, vsub, vr_qdb, vcmr_qdb, raw = build(SEED)
    vids = sorted(feats)
    out = {"desc": np.array(json.dumps(raw))}
    for k, v in feats.items():
        out["feat." + k] = v.numpy()
    everything = lambda ds: [ds[i] for i in range(len(ds))]               # noqa: E731
    ds_vonly = VrVideoOnlyDataset(vids, vonly, vr_qdb)
    ds_eval = VrVideoOnlyEvalDataset(vids, vonly, vr_qdb)
    ds_full = VrVideoOnlyFullEvalDataset(vids, vonly, vr_qdb)
    ds_sub = VrDataset(vids, vsub, vr_qdb)
    ds_sub_full = VrFullEvalDataset(vids, vsub, vr_qdb)
    ds_vcmr = VcmrVideoOnlyDataset(vids, vonly, vcmr_qdb)
    batches = {"vr_vonly": vr_collate(everything(ds_vonly)), "vr_vonly_eval": vr_eval_collate(everything(ds_eval)),
               "vr_vonly_full": vr_full_eval_collate(everything(ds_full)), "vr_sub": vr_collate(everything(ds_sub)),
               "vcmr_vonly": vcmr_collate(everything(ds_vcmr))}
    for name, b in batches.items():
        pack(out, "batch.%s." % name, b)
    b = batches["vr_vonly"]
    assert b["f_sub_input_ids"].tolist() == [[0]] * 5 and b["f_attn_masks"].shape == (5, 11) and b["num_subs"] == [1] * 5
    assert b["q_vidx"].tolist() != list(range(5)) and (b["targets"] == -1).all() and batches["vr_vonly_eval"]["qids"] == [str(i) for i in range(5)]
    assert (batches["vcmr_vonly"]["targets"] >= 0).all() and len(set(b["query_attn_masks"].sum(1).tolist())) == 5

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    cfg = os.path.join(HERE, "tiny_config.json")

    def no_dropout(m):
        for m_ in m.modules():
            if isinstance(m_, torch.nn.Dropout):
                m_.p = 0.0
        return m
    model = no_dropout(HeroForVr.from_pretrained(cfg, state_dict=copy.deepcopy(sd), vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM, margin=0.1,
                                                 lw_neg_ctx=10.0, lw_neg_q=10.0, use_all_neg=True))
    out["state_keys"] = np.array(json.dumps(sorted(model.state_dict().keys())))
    for name in ("vr_vonly", "vr_sub"):
        model_case(model, batches[name], out, "vr.%s." % name)

    # ---- the in-training validators over a two-batch loader ----------------------------------------------------------------
    items = everything(ds_eval)
    tap = Tap(model)
    model.eval()
    log = TV.validate_vr(tap, [vr_eval_collate(items[:3]), vr_eval_collate(items[3:])], VR_OPTS)
    for i, (c, q) in enumerate(tap.outs):
        out["val.vr.%d.neg_ctx" % i], out["val.vr.%d.neg_q" % i] = c.numpy(), q.numpy()
    out["val.vr.log"] = np.array(json.dumps({k: float(v) for k, v in log.items() if k != "valid/ex_per_s"}))
    out["val.vr.opts"] = np.array(json.dumps({k: v for k, v in vars(VR_OPTS).items()}))
    print("validate_vr", log)
    vcmr = no_dropout(HeroForVcmr.from_pretrained(cfg, state_dict=copy.deepcopy(sd), vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM, margin=0.1,
                                                  lw_neg_ctx=8.0, lw_neg_q=8.0, lw_st_ed=0.01, ranking_loss_type="hinge", use_hard_negative=False,
                                                  hard_pool_size=20, use_all_neg=True, drop_svmr_prob=0.0))
    vcmr.eval()
    tap = Tap(vcmr)
    items = everything(ds_vcmr)
    log = TC.validate_vcmr(tap, [vcmr_collate(items[:3]), vcmr_collate(items[3:])], VCMR_OPTS)
    for i, (s, c, q) in enumerate(tap.outs):
        out["val.vcmr.%d.st_ed" % i], out["val.vcmr.%d.neg_ctx" % i], out["val.vcmr.%d.neg_q" % i] = s.numpy(), c.numpy(), q.numpy()
    out["val.vcmr.log"] = np.array(json.dumps({k: float(v) for k, v in log.items() if k != "valid/ex_per_s"}))
    out["val.vcmr.opts"] = np.array(json.dumps({k: v for k, v in vars(VCMR_OPTS).items()}))
    print("validate_vcmr", log)

    # ---- the full driver ---------------------------------------------------------------------------------------------------
    class Loader:
        def __init__(self, dataset):
            self.dataset = dataset

        def __iter__(self):
            items = everything(self.dataset)
            return iter([vr_full_eval_collate(items[:3]), vr_full_eval_collate(items[3:])])

    model_opts = types.SimpleNamespace(max_clip_len=16, max_vr_video=2, distributed_eval=False)
    for corpus, ds, task in (("vonly", ds_full, "msrvtt_video_only"), ("sub", ds_sub_full, "msrvtt_video_sub")):
        opts = types.SimpleNamespace(task=task, vr_eval_video_batch_size=2)
        val_log, submission = EV.validate_full_vr(model, Loader(ds), "val", opts, model_opts)
        model.eval()
        with torch.no_grad():
            from data.data import video_collate
            emb = [model.v_encoder(video_collate([ds.video_db[v]]), "repr") for v in vids]
            total = torch.zeros(3, 10, emb[0].shape[-1])
            masks = torch.zeros(3, 10, dtype=torch.long)
            for i, e in enumerate(emb):
                total[i, :e.shape[1]], masks[i, :e.shape[1]] = e[0], 1
            qb = {k: v for k, v in batches["vr_vonly_full"].items() if k.startswith("query_")}
            scores = model.get_pred_from_raw_query(total, masks, **qb, cross=True, val_gather_gpus=False).float()
        gaps = scores.sort(dim=1, descending=True).values
        gaps = (gaps[:, :-1] - gaps[:, 1:]).min()
        assert float(gaps) > 10 * SCORE_TOL, ("two videos of a query score within %g" % (10 * SCORE_TOL), corpus, float(gaps), scores)
        for e, row in zip(submission["VR"], scores.topk(2, dim=1).indices.tolist()):
            assert [p[0] for p in e["predictions"]] == row
        out["full.%s.val_log" % corpus] = np.array(json.dumps({k: float(v) for k, v in val_log.items() if not k.endswith("_ex_per_s")}))
        out["full.%s.submission" % corpus] = np.array(json.dumps(submission))
        out["full.%s.scores" % corpus] = scores.numpy()
        print("validate_full_vr", corpus, {k: v for k, v in val_log.items() if not k.endswith("_ex_per_s")}, "min gap %.4f" % float(gaps))
    out["full.score_tol"] = np.array(SCORE_TOL)

    # ---- DiDeMo recall -----------------------------------------------------------------------------------------------------
    sys.path.append(os.path.dirname(os.path.dirname(HERE)))              # the repository root: tests.didemo_reference
    from hero_amd.retrieval import RecallMeter
    from tests import didemo_reference as DR
    rng = np.random.default_rng(31)
    told_need = told_first = False
    for name, interval in (("i15", 1.5), ("i20", 2.0)):
        case, metrics = didemo_case(rng, S, interval)
        for k, v in case.items():
            out["didemo.%s.%s" % (name, k)] = v
        loaded = {"didemo.%s.%s" % (name, k): (json.loads(str(v)) if v.dtype.kind == "U" else v) for k, v in case.items()}
        c = DR._didemo_case(loaded, name)
        got = DR.meter_from_rows(RecallMeter(vfeat_interval=interval), c).compute()
        assert got["VCMR"] == metrics["VCMR"] and got["SVMR"] == metrics["SVMR"], (got, metrics)
        told_need |= DR.meter_from_rows(RecallMeter(vfeat_interval=interval), c, need=1).compute() != got
        told_first |= DR.meter_from_rows(RecallMeter(vfeat_interval=interval), c, only_first=True).compute() != got
        assert any(0 < x < 100 for x in metrics["VCMR"].values()) and any(0 < x < 100 for x in metrics["SVMR"].values()), metrics
        print("didemo", name, metrics)
    assert told_need and told_first, "the DiDeMo cases do not tell the rules apart"
    path = os.path.join(HERE, "case_vr.npz")
    np.savez_compressed(path, **out)
    print("wrote case_vr.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
