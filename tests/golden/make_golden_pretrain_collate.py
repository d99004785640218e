#!/usr/bin/env python3
"""Golden vectors for the PRE-TRAINING batch boundary, produced by the reference's own data code.

Container-only (needs the reference checkout, HERO_REFERENCE or /root/reference).  The reference's four pre-training
datasets and collates
    VideoMlmDataset.__getitem__ / mlm_collate        data/mlm.py:21-176
    MfmDataset.__getitem__ / mfm_collate             data/mfm.py:19-97
    FomDataset.__getitem__ / fom_collate             data/fom.py:18-115
    VsmDataset.__getitem__ / vsm_collate             data/vsm.py:20-145
are IMPORTED and RUN here over in-memory stand-ins for the two LMDB readers, with the stubs of make_golden_collate.py
(install_data_stubs) and stand-ins built the way its build_case builds them.  Each of the four batches of a case is
made right after random.seed(case seed), videos in sorted order.

Writes tests/golden/case_pretrain_collate.npz.  Per case `<c>`:
    <c>.desc               JSON: per video the frame count, sub2frames as compute_sub2frames left them, the token ids per
                           subtitle; the Python seed, sub_ctx_len, max_txt_len, the probabilities, query_per_video, the
                           special ids and v_range
    <c>.feat.<vid>         the (clipped) frame features
    <c>.<task>.<key>       every tensor (array) / list (JSON) of the reference batch, task in mlm, mfm, fom, vsm
Cases: `narrow` (the spec of make_golden_collate.py: a zero-frame subtitle, frames no subtitle covers, a subtitle cut by
max_clip_len), `ctx1` (sub_ctx_len = 1, max_txt_len = 6), `atleast1` (a seed that leaves a subtitle without a drawn token:
asserted), `oneframe` (a one-frame video), rand0 .. rand3 (small random ragged batches).

Run:  python tests/golden/make_golden_pretrain_collate.py
"""
import json
import os
import random
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("HERO_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs  # noqa: E402  (apex + horovod stubs)
from make_golden_collate import install_data_stubs  # noqa: E402

MASK, CLS, SEP, V_RANGE = 4, 0, 2, (5, 160)
FIRED = []          # one entry per sentence of the last case that the at-least-one rule of random_word masked

# the `narrow` spec of make_golden_collate.py (queries dropped: the pre-training tasks have none)
NARROW = [
    dict(nframe_db=12, unmatched=[9, 10], subs=[(0, [0, 1, 2, 3, 4], 2), (1, [], 4), (2, [5], 5), (3, [6, 7, 8], 3)]),
    dict(nframe_db=20, subs=[(0, [0, 1], 4), (1, [2, 3, 4], 1), (2, [12, 13, 14, 15], 3), (3, [16, 17], 2)]),
    dict(nframe_db=5, subs=[(0, [1, 2, 3], 3)]),
]


def build_dbs(spec, vfeat, max_clip_len, max_txt_len, sub_ctx_len, seed, vocab=160):
    """The stand-ins of make_golden_collate.build_case (dicts behind the two LMDB readers, the real compute_sub2frames)."""
    from data.data import SubTokLmdb, VideoFeatLmdb, VideoFeatSubTokDataset
    g = torch.Generator().manual_seed(seed)

    class FeatDb(VideoFeatLmdb):
        def __init__(self, feats):
            self.feats, self.max_clip_len, self.frame_interval = feats, max_clip_len, 1.5
            self.name2nframe = {k: v.shape[0] for k, v in feats.items()}

        def __getitem__(self, name):                   # data/data.py:107-119 without the lmdb read
            return self.feats[name][:min(self.name2nframe[name], self.max_clip_len)].float()

        def __del__(self):
            pass

    class SubDb(SubTokLmdb):                           # keeps the real compute_sub2frames
        def __init__(self, db):
            self.db, self.max_clip_len = db, max_clip_len
            self.sep, self.cls_, self.mask, self.v_range = SEP, CLS, MASK, list(V_RANGE)
            self.id2len = {k: v["nframe"] for k, v in db.items()}
            self.vid2dur, self.vid2idx = {}, {}
            self.vid_sub2frame, self.vid2vonly_frames = self.compute_sub2frames()

        def __getitem__(self, k):
            return self.db[k]

        def __del__(self):
            pass

    feats, subdb = {}, {}
    for v, s in enumerate(spec):
        vid = "v%02d" % v
        feats[vid] = torch.randn(s["nframe_db"], vfeat, generator=g)
        toks = {si: torch.randint(V_RANGE[0], vocab, (nw,), generator=g).tolist() for si, _, nw in s["subs"]}
        subdb[vid] = {"input_ids": [toks.get(i, []) for i in range(max(toks) + 1)],
                      "unique_sub2frames": [(si, list(fr)) for si, fr, _ in s["subs"]],
                      "unmatched_frames": list(s.get("unmatched", [])), "nframe": s["nframe_db"]}
    txt_db = SubDb(subdb)
    video_db = VideoFeatSubTokDataset(txt_db, FeatDb(feats), max_txt_len=max_txt_len, sub_ctx_len=sub_ctx_len)
    return video_db, feats, subdb


def build_case(spec, vfeat, max_clip_len, seed, py_seed, sub_ctx_len=0, max_txt_len=-1, mask_prob=0.15, reorder_p=0.15,
               query_per_video=2):
    from data.fom import FomDataset, fom_collate
    from data.mfm import MfmDataset, mfm_collate
    from data.mlm import VideoMlmDataset, mlm_collate
    from data.vsm import VsmDataset, vsm_collate
    video_db, feats, subdb = build_dbs(spec, vfeat, max_clip_len, max_txt_len, sub_ctx_len, seed)
    vids = sorted(feats)
    sets = {"mlm": (VideoMlmDataset(vids, video_db, mask_prob, sub_ctx_len), mlm_collate),
            "mfm": (MfmDataset(vids, video_db, mask_prob), mfm_collate),
            "fom": (FomDataset(vids, video_db, reorder_p), fom_collate),
            "vsm": (VsmDataset(vids, video_db, query_per_video, sub_ctx_len), vsm_collate)}
    # count the sentences that the at-least-one rule masks: no draw of the sentence falls under mask_prob (then random_word
    # calls nothing but random.random(), once per token, so the draws can be replayed from the saved state)
    import data.mlm as ref_mlm
    ref_random_word = ref_mlm.random_word

    def counting_random_word(tokens, vocab_range, mask, mask_prob=0.15):
        before = random.getstate()
        res = ref_random_word(tokens, vocab_range, mask, mask_prob)
        after = random.getstate()
        random.setstate(before)
        if tokens and all(random.random() >= mask_prob for _ in tokens):
            FIRED.append(1)
        random.setstate(after)
        return res
    del FIRED[:]
    ref_mlm.random_word = counting_random_word
    batches, items = {}, {}
    for task, (ds, collate) in sets.items():
        random.seed(py_seed)
        items[task] = [ds[i] for i in range(len(ds))]
        batches[task] = collate(items[task])
    ref_mlm.random_word = ref_random_word
    raw ={"videos": [{"vid": v, "nframes": min(subdb[v]["nframe"], max_clip_len),
                       "sub2frames": [(si, list(fr)) for si, fr in video_db.vid_sub2frame[v]],
                       "sub_tokens": subdb[v]["input_ids"]} for v in vids],
           "py_seed": py_seed, "sub_ctx_len": sub_ctx_len, "max_txt_len": max_txt_len, "mask_prob": mask_prob,
           "reorder_p": reorder_p, "query_per_video": query_per_video, "mask": MASK, "cls": CLS, "sep": SEP, "v_range": list(V_RANGE)}
    return batches, raw, {v: video_db.img_db[v] for v in vids}, items


def pack(prefix, batches, raw, feats):
    out = {prefix + ".desc": np.array(json.dumps(raw))}
    for k, v in feats.items():
        out["%s.feat.%s" % (prefix, k)] = v.numpy()
    for task, batch in batches.items():
        for k, v in batch.items():
            out["%s.%s.%s" % (prefix, task, k)] = v.numpy() if torch.is_tensor(v) else np.array(json.dumps(v))
    return out


def random_spec(g, n_videos):
    """Small ragged videos whose frame lists stay inside the video (the pre-training datasets index the features with the
    unfiltered lists) and where every video has a subtitle with frames (VSM needs a query)."""
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))     # noqa: E731
    spec = []
    for _ in range(n_videos):
        nf = ri(4, 24)
        subs, f0 = [], 0
        for si in range(ri(2, 6)):
            k = min(ri(0, 5) if si else ri(1, 5), nf - f0)
            if f0 < nf and ri(0, 4) == 0:
                f0 += 1                            # a frame no subtitle covers
                k = min(k, nf - f0)
            subs.append((si, list(range(f0, f0 + k)), ri(1, 12)))
            f0 += k
        spec.append(dict(nframe_db=nf, subs=subs))
    return spec


def main():
    install_stubs()
    install_data_stubs()
    sys.path.insert(0, REF)
    out, names = {}, []

    def add(name, *a, **kw):
        batches, raw, feats, items = build_case(*a, **kw)
        out.update(pack(name, batches, raw, feats))
        names.append(name)
        return batches, items

    add("narrow", NARROW, 8, 14, seed=11, py_seed=101)
    add("ctx1", NARROW, 8, 14, seed=12, py_seed=102, sub_ctx_len=1, max_txt_len=6)
    # a seed that leaves at least one subtitle without a drawn token, so that the "at least one" rule fires: such a row's
    # only label is its first token, which then reads MASK
    add("atleast1", NARROW, 8, 14, seed=13, py_seed=103, mask_prob=0.05)
    assert len(FIRED) >= 1, "pick another py_seed: the at-least-one rule did not fire"
    print("atleast1: subtitles masked by the at-least-one rule:", len(FIRED))
    one = [dict(nframe_db=1, subs=[(0, [0], 3), (1, [], 2)]), dict(nframe_db=7, subs=[(0, [0, 1], 4), (1, [3, 4, 5], 2)])]
    b, _ = add("oneframe", one, 6, 14, seed=14, py_seed=104)
    assert int(b["mfm"]["c_v_masks"][0].sum()) == 1 and b["mfm"]["c_attn_masks"][0].sum() == 1
    g = torch.Generator().manual_seed(7)
    for i in range(4):
        add("rand%d" % i, random_spec(g, 2 + i % 3), 6, 24, seed=30 + i, py_seed=200 + i, sub_ctx_len=i % 2,
            query_per_video=1 + i)
    out["__cases__"] = np.array(json.dumps(names))
    path = os.path.join(HERE, "case_pretrain_collate.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
